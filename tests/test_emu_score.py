"""Teacher-forced scoring of given sequences (ntts_backbone_score / _read_score_logits, ntts_k_head_score_probe) on the CPU SIMT emulator: the
target-capture epilogue (csrc/kernels/gemm.h EPI_ARGMAX_LSE_TGT) and the merge kernel (csrc/kernels/score.h) through the kernel-level probe against
tests/score_spec.py, the engine's values against the spec on the tapped rows, against the CPU oracle and against what the decoder records, the
chunking, the isolation from running requests and the refusals.
tests/test_gpu_score.py runs the same bodies on libneutts_hip.so."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import backbone_ref as br
from neutts import _hip
from common import bf16_ulp, make_engine
import score_spec as spec
import test_emu_logprobs as lcases
import test_emu_variants as vcases
from test_emu_logprobs import LSE_TOL
from test_emu_repetition import device_of


@pytest.fixture(scope="module")
def lib(emu_lib):
    return emu_lib


model = lcases.model
model3000 = lcases.model3000


# ---------------------------------------------------------------------------------------------- 2. the epilogue and the merge through the probe
EDGES = [63, 64, 95, 96, 255, 256, 287, 288]          # both sides of every tile and partial-group edge
SCORE_PROBE_CASES = [("64x64", 5, 200, 64, False), ("128x128", 129, 3000, 64, False), ("256x256", 257, 600, 128, False),
                     ("256x256", 257, 600, 128, True), ("256x288", 70, 3000, 64, False)]


def probe_targets(M, N, argmax, rng, launch):
    """Row m of launch `launch`: column 0, N - 1 (in the part-padded last tile), the edges below N, the row's own argmax column, then random columns."""
    pattern = [0, N - 1] + [c for c in EDGES if c < N] + ["argmax"]
    tg = np.empty(M, dtype=np.int32)
    for m in range(M):
        k = launch * M + m
        c = pattern[k] if k < len(pattern) else int(rng.integers(0, N))
        tg[m] = argmax[m] if c == "argmax" else c
    return tg, len(pattern)


def check_score_probe(lib_path, variant, M, N, K, fp8=False, seed=0, scale=1.0, min_peak=4.0):
    """Logits and the three partial arrays are bit for bit those of ntts_k_head_logprob_probe on the same inputs; target_val is the returned row's
    entry at the target, exactly; nothing is left NaN; the merged outputs are the spec's on the returned row."""
    lib = _hip.load_library(lib_path)
    rng = np.random.default_rng(300 + seed + M)
    x, w = lcases.probe_inputs(lib_path, M, N, K, seed, scale)
    v = _hip.HEAD_VARIANTS[variant]
    kw = dict(fp8=fp8, xscale=4.0 * scale / 448.0)
    want = _hip.head_logprob_probe(lib, x.data_ptr(), w.data_ptr(), M, N, K, v, **kw)
    argmax = want[0].argmax(axis=1)
    launch, worst = 0, 0.0
    while True:
        tg, n_special = probe_targets(M, N, argmax, rng, launch)
        got = _hip.head_score_probe(lib, x.data_ptr(), w.data_ptr(), M, N, K, v, tg, **kw)
        for a, b, name in ((want[0], got["logits"], "logits"), (want[2], got["part_val"], "part_val"), (want[3], got["part_idx"], "part_idx"),
                           (want[5], got["part_sum"], "part_sum")):
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), (variant, name, launch)
        assert got["width"] == want[4]
        rows = got["logits"]
        assert np.array_equal(got["target_val"].view(np.uint32), rows[np.arange(M), tg].view(np.uint32)), (variant, launch)
        for name in ("target_val", "logprob", "argmax_logprob"):
            assert not np.isnan(got[name]).any(), (variant, name)
        assert (got["argmax"] >= 0).all() and np.array_equal(got["argmax"], rows.argmax(axis=1)), (variant, launch)
        lp, am, alp = spec.score_rows(rows, tg)
        worst = max(worst, float(np.abs(got["logprob"] - lp).max()), float(np.abs(got["argmax_logprob"] - alp).max()))
        assert (got["logprob"] <= got["argmax_logprob"]).all() and (got["argmax_logprob"] <= 0).all()
        assert np.array_equal(got["logprob"][tg == argmax].view(np.uint32), got["argmax_logprob"][tg == argmax].view(np.uint32))
        launch += 1
        if launch * M >= n_special:
            break
    peak = float(np.abs(rows).max())
    print(f"[score] probe {variant} fp8={fp8} M={M} N={N}: {launch} launches, max |value - spec| = {worst:.3e} (bound {LSE_TOL:.0e}), peak logit {peak:.1f}")
    assert worst <= LSE_TOL, (variant, worst)
    assert peak >= min_peak, peak
    return peak


@pytest.mark.parametrize("variant,M,N,K,fp8", SCORE_PROBE_CASES)
def test_target_epilogue_and_merge_equal_the_specification(lib, variant, M, N, K, fp8):
    check_score_probe(lib, variant, M, N, K, fp8)


def test_target_epilogue_with_large_logits(lib):
    """X scaled until |logits| reach ~80: most terms of every sum underflow to 0; everything stays finite and within the bound."""
    peak = check_score_probe(lib, "128x128", 129, 3000, 64, False, seed=3, scale=2.5, min_peak=70.0)
    assert peak < 200.0


def test_score_probe_refuses_bad_arguments(lib):
    h = _hip.load_library(lib)
    dev = device_of(lib)
    x = torch.zeros(4, 64, dtype=torch.bfloat16, device=dev)
    w = torch.zeros(64, 64, dtype=torch.bfloat16, device=dev)
    for kw in (dict(variant=3), dict(variant=8), dict(variant=4, fp8=True), dict(target=[0, 1, 2, 64]), dict(target=[0, -1, 2, 3])):
        a = dict(variant=0, fp8=False, target=[0, 1, 2, 3])
        a.update(kw)
        with pytest.raises(_hip.NeuTTSHipError) as ei:
            _hip.head_score_probe(h, x.data_ptr(), w.data_ptr(), 4, 64, 64, a["variant"], a["target"], fp8=a["fp8"])
        assert ei.value.code == -1, kw
    out = _hip.head_score_probe(h, x.data_ptr(), w.data_ptr(), 4, 64, 64, 0, [0, 1, 2, 63])      # rows of zeros: every logit 0, S = N exactly
    assert np.allclose(out["logprob"], -np.log(64.0), atol=1e-6) and out["argmax"].tolist() == [0, 0, 0, 0]


# ---------------------------------------------------------------------------------------------- 3. the engine on the tapped rows
LENS = (33, 47, 70)                                    # straddle the 32- and 64-token page edges


def seqs_for(cfg, lens=LENS, seed=160):
    return [br.synthetic_prompt(cfg, seed + i, n) for i, n in enumerate(lens)]


def froms_for(lens=LENS):
    return [1, lens[1] // 2, lens[2] - 1]              # everything, from a middle position, exactly one value


def tapped_check(eng, seqs, froms, slots, chunk_rows=0, tag=""):
    """One score call with the tap on: n_out, the packing, every value against the spec on its tapped row, argmax exact.  Returns the packed outputs."""
    eng.set_debug(True)
    try:
        lp, am, alp = eng.score_call(seqs, slots, froms, chunk_rows)
        counts = [len(q) - f for q, f in zip(seqs, froms)]
        assert len(lp) == len(am) == len(alp) == sum(counts)
        assert lp.dtype == np.float32 and am.dtype == np.int32 and alp.dtype == np.float32
        targets = [t for q, f in zip(seqs, froms) for t in q[f:]]
        rows = [eng.read_score_logits(r) for r in range(sum(counts))]
        assert all(np.isfinite(r).all() for r in rows)                                         # no processor: no masked column
        wlp, wam, walp = spec.score_rows(rows, targets)
        worst = max(float(np.abs(lp - wlp).max()), float(np.abs(alp - walp).max()))
        print(f"[score] engine {tag}: {sum(counts)} values, max |value - spec on the tapped row| = {worst:.3e} (bound {LSE_TOL:.0e})")
        assert worst <= LSE_TOL, worst
        assert np.array_equal(am, wam)
        assert (lp <= alp).all() and (alp <= 0).all()
        with pytest.raises(_hip.NeuTTSHipError) as ei:
            eng.read_score_logits(sum(counts))
        assert ei.value.code == -1
    finally:
        eng.set_debug(False)
    return lp, am, alp


def check_engine_on_tapped_rows(lib, cfg, w, max_batch, froms=None, **kw):
    eng = make_engine(cfg, w, lib, max_batch=max_batch, **kw)
    seqs = seqs_for(cfg)
    froms = froms or froms_for()
    try:
        free0 = eng.kv_stats()["free_pages"]
        packed = tapped_check(eng, seqs, froms, [0, 1, 2], tag=f"max_batch={max_batch} V={cfg.vocab_size} head_dim={cfg.head_dim}")
        assert eng.kv_stats()["free_pages"] == free0 and eng.free_slots() == max_batch
        per = eng.score(seqs, froms)                                                           # the list form: the same bits, split per sequence
        assert [len(t[0]) for t in per] == [len(q) - f for q, f in zip(seqs, froms)]
        for k in range(3):
            assert np.array_equal(np.concatenate([t[k] for t in per]).view(np.uint32), packed[k].view(np.uint32))
        with pytest.raises(_hip.NeuTTSHipError) as ei:                                        # the tap is off again
            eng.read_score_logits(0)
        assert ei.value.code == -4
    finally:
        eng.close()


@pytest.mark.parametrize("max_batch", [3, 16])                      # a small-batch engine (its decode lm_head is the GEMV) / a tile-path engine
def test_engine_on_the_tapped_rows(lib, model, max_batch):
    check_engine_on_tapped_rows(lib, *model, max_batch)


def test_engine_on_the_tapped_rows_vocabulary_3000(lib, model3000):
    check_engine_on_tapped_rows(lib, *model3000, 5)


QWEN3 = dict(vocab_size=512, hidden_size=256, intermediate_size=384, num_layers=2, num_heads=2, num_kv_heads=1, head_dim=128, attention_bias=False,
             qk_norm=True)


def test_engine_on_the_tapped_rows_general_attention(lib):
    """head_dim 128 with per-head q / k RMSNorm (the general attention path), 98 scored rows."""
    cfg = br.BackboneConfig(**QWEN3)
    check_engine_on_tapped_rows(lib, cfg, br.make_weights(cfg, 41), 4, froms=[1, 1, 50])


# ---------------------------------------------------------------------------------------------- 4. chunking
def check_chunking(eng, cfg):
    seqs = seqs_for(cfg, (34, 48, 71), seed=170)                                              # 33 + 47 + 70 = 150 scored rows
    outs = [eng.score_call(seqs, [0, 1, 2], [1, 1, 1], chunk) for chunk in (64, 100, 0)]
    assert len(outs[0][0]) == 150
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    alone = eng.score_call(seqs[:1], [2], [1])                                                # ... nor does what a sequence is packed with
    for a, b in zip(outs[0], alone):
        assert len(b) == 33 and np.array_equal(a[:33].view(np.uint32), b.view(np.uint32))
    return outs[0]


def test_chunking_and_packing_do_not_change_a_bit(lib, model):
    cfg, w = model
    eng = make_engine(cfg, w, lib, max_batch=4)
    try:
        check_chunking(eng, cfg)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- 5. against the oracle
def oracle_bar(row):
    """Per value: two logits enter it, the target's and the row's dominant terms, each within the 4-ulp band common.teacher_forced_compare grants."""
    return 2.0 * 4.0 * bf16_ulp(float(np.abs(row).max()))


def oracle_scores(cfg, w, seqs, froms):
    wd = br.cast_weights(w, torch.bfloat16)
    out = []
    for q, f in zip(seqs, froms):
        rows = spec.oracle_rows(cfg, wd, q)
        lp, am, alp = spec.score(rows, q, f)
        out.append((lp, am, alp, [oracle_bar(rows[j - 1]) for j in range(f, len(q))]))
    return out


def check_against_oracle(lib, cfg, w, max_batch, tag):
    seqs, froms = seqs_for(cfg), froms_for()
    want = oracle_scores(cfg, w, seqs, froms)
    eng = make_engine(cfg, w, lib, max_batch=max_batch)
    try:
        got = eng.score(seqs, froms)
    finally:
        eng.close()
    worst = 0.0
    for (lp, am, alp), (wlp, wam, walp, bars) in zip(got, want):
        for k in range(len(lp)):
            for g, o in ((lp[k], wlp[k]), (alp[k], walp[k])):
                worst = max(worst, abs(float(g) - o) / bars[k])
    print(f"[score] {tag} vs the oracle: max |value - oracle| = {worst:.3f} of the bar (2 x 4 bf16 ulps of the row's largest logit)")
    assert worst <= 1.0, worst
    return worst


def test_against_the_oracle(lib, model, model3000):
    """Measured (profiles/score_parity.txt): 0.128 / 0.124 of the bar on the emulator, 0.127 / 0.125 on an MI355X (V = 512 / 3000)."""
    check_against_oracle(lib, *model, 3, "V=512")
    check_against_oracle(lib, *model3000, 5, "V=3000")


# ---------------------------------------------------------------------------------------------- 6. against generation
def check_against_generation(lib, cfg, w, max_batch):
    """A greedy request with the record on and min_new_tokens = 0, six tokens; then prompt + output scored from len(prompt): the decoder's record and
    the score are the same quantity up to the arithmetic of the decode step against the prompt pass -- each within the oracle bar of the oracle,
    so within twice the bar of each other -- and the score's argmax is the generated id wherever the step's top-2 gap is clear."""
    eng = make_engine(cfg, w, lib, max_batch=max_batch)
    N, eos = 6, cfg.vocab_size - 1
    p = br.synthetic_prompt(cfg, 181, 39)
    eng.set_logprobs(True)
    eng.set_debug(True)
    try:
        eng.prefill([p], [0], [_hip.Sampling(max_length=len(p) + N, min_new_tokens=0, eos_token_id=eos, do_sample=False)])
        taps = []
        for step in range(N):
            if step:
                eng.decode(1)
            taps.append(eng.read_logits(0))
        ids, rec = eng.read(0)[0], eng.read_logprobs(0)
        assert len(ids) == N == len(rec) and eos not in ids[:-1]
        eng.release(0)
        lp, am, alp = eng.score_call([p + ids], [1], [len(p)])
        worst, clear = 0.0, 0
        for k in range(N):
            bar = 2.0 * oracle_bar(taps[k])
            worst = max(worst, abs(float(lp[k]) - float(rec[k])) / bar)
            top2 = np.sort(taps[k])[-2:]
            if top2[1] - top2[0] > 4.0 * bf16_ulp(float(top2[1])):
                clear += 1
                assert am[k] == ids[k], (k, am[k], ids[k])
        print(f"[score] vs the decoder's record (max_batch={max_batch}): max |score - record| = {worst:.3f} of twice the oracle bar; {clear} of {N} steps clear")
        assert worst <= 1.0, worst
    finally:
        eng.set_debug(False)
        eng.close()


@pytest.mark.parametrize("max_batch", [3, 16])
def test_against_generation(lib, model, max_batch):
    check_against_generation(lib, *model, max_batch)


# ---------------------------------------------------------------------------------------------- 7. isolation and life cycle
def test_running_requests_do_not_notice(lib, model):
    """A greedy + penalised request and a sampled one, decoded step by step, without and with score calls between the steps (on the free slots):
    the same ids and the same recorded log-probabilities, bit for bit.  The pages come back, the slots can be filled at once, and a second score
    call gives the first one's bits."""
    cfg, w = model
    eng = make_engine(cfg, w, lib, max_batch=4)
    N, eos = 6, cfg.vocab_size - 1
    ps = [br.synthetic_prompt(cfg, 190 + i, 21 + 13 * i) for i in range(2)]
    sts = [dict(repetition_penalty=1.3), dict(lcases.WARPED, seed=31)]
    seqs, froms = seqs_for(cfg)[:2], [1, 20]

    def sp(p, st):
        return _hip.Sampling(**dict(dict(max_length=len(p) + N, min_new_tokens=N, eos_token_id=eos, do_sample=False), **st))

    def run(with_score):
        scores = []
        eng.prefill(ps, [0, 2], [sp(p, st) for p, st in zip(ps, sts)])
        for _ in range(N - 1):
            if with_score:
                free = eng.kv_stats()["free_pages"]
                scores.append(eng.score_call(seqs, [3, 1], froms))
                assert eng.kv_stats()["free_pages"] == free
            eng.decode(1)
        out = [(eng.read(s)[0], eng.read_logprobs(s)) for s in (0, 2)]
        eng.release(0)
        eng.release(2)
        return out, scores

    eng.set_logprobs(True)
    try:
        alone = eng.score_call(seqs, [3, 1], froms)
        plain, _ = run(False)
        mixed, scores = run(True)
        for (ia, la), (ib, lb) in zip(plain, mixed):
            assert ia == ib and len(ia) == N and np.array_equal(la.view(np.uint32), lb.view(np.uint32))
        for sc in scores:                                                                      # ... and the scores do not notice the requests
            assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(sc, alone))
        st = eng.kv_stats()
        assert st["free_pages"] == st["total_pages"] and eng.free_slots() == 4
        eng.prefill([seqs[0]], [3], [sp(seqs[0], {})])                                        # a slot a score call used: filled again at once
        eng.decode(2)
        assert len(eng.read(3)[0]) == 3
        eng.release(3)
        again = eng.score_call(seqs, [3, 1], froms)
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(again, alone))
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- 8. refusals
def raw_score(eng, seqs, slots, froms, cap, chunk_rows=0):
    """The C call with a caller-chosen `cap`: (return code, n_out)."""
    lens = np.asarray([len(q) for q in seqs], dtype=np.int32)
    ids = np.ascontiguousarray(np.concatenate([np.asarray(q, dtype=np.int32) for q in seqs]))
    sl, sf = np.asarray(slots, dtype=np.int32), np.asarray(froms, dtype=np.int32)
    lp, alp, am = np.zeros(max(cap, 1), dtype=np.float32), np.zeros(max(cap, 1), dtype=np.float32), np.zeros(max(cap, 1), dtype=np.int32)
    n = C.c_int64(-7)
    i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    rc = eng.lib.ntts_backbone_score(eng.h, len(lens), ids.ctypes.data_as(i32p), lens.ctypes.data_as(i32p), sl.ctypes.data_as(i32p),
                                     sf.ctypes.data_as(i32p), chunk_rows, lp.ctypes.data_as(f32p), am.ctypes.data_as(i32p), alp.ctypes.data_as(f32p),
                                     cap, C.byref(n))
    return rc, n.value


def test_refusals_leave_the_engine_as_it_was(lib, model):
    cfg, w = model
    V = cfg.vocab_size
    seqs, froms = seqs_for(cfg), froms_for()
    kw = dict(max_batch=4, max_context=128, max_prefill_tokens=256)
    fresh = make_engine(cfg, w, lib, **kw)
    try:
        want = fresh.score_call(seqs, [0, 1, 2], froms)
    finally:
        fresh.close()
    eng = make_engine(cfg, w, lib, **kw)

    def still_fresh():
        st = eng.kv_stats()
        assert st["free_pages"] == st["total_pages"]
        got = eng.score_call(seqs, [0, 1, 2], froms)
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, want))

    def refused(code, match, seqs_, slots, froms_):
        with pytest.raises(_hip.NeuTTSHipError, match=match) as ei:
            eng.score_call(seqs_, slots, froms_)
        assert ei.value.code == code, (ei.value.code, str(ei.value))
        still_fresh()

    a, b = seqs[0], seqs[1]
    try:
        still_fresh()
        refused(-1, "sequence 1", [a, b], [0, 0], [1, 1])                                     # a repeated slot
        refused(-1, "sequence 1", [a, b], [0, 1], [1, 0])                                     # score_from outside [1, len)
        refused(-1, "sequence 0", [a, b], [0, 1], [len(a), 1])
        refused(-1, "sequence 1", [a, list(range(129))], [0, 1], [1, 1])                      # len > max_context
        refused(-1, "sequence 0", [a[:5] + [V] + a[6:], b], [0, 1], [1, 1])                   # an id outside [0, V)
        refused(-1, "sequence 1", [a[:5] + [V - 1] + a[6:], b[:-1] + [-1]], [0, 1], [1, 1])
        refused(-1, "max_prefill_tokens", [list(range(100))] * 3, [0, 1, 2], [1, 1, 1])       # 300 tokens > 256
        refused(-1, "sequence 0", [a], [4], [1])                                              # no such slot
        eng.prefill([b], [1], [_hip.Sampling(max_length=len(b) + 4, min_new_tokens=4, eos_token_id=V - 1, do_sample=False)])
        with pytest.raises(_hip.NeuTTSHipError, match="sequence 1.*busy") as ei:              # a busy slot
            eng.score_call([a, b], [0, 1], [1, 1])
        assert ei.value.code == -1
        eng.decode(1)
        busy_ids = eng.read(1)[0]
        eng.release(1)
        assert len(busy_ids) == 2
        still_fresh()
        total = sum(len(q) - f for q, f in zip(seqs, froms))                                  # 32 + 24 + 1
        rc, n = raw_score(eng, seqs, [0, 1, 2], froms, cap=total - 1)                         # room for one value too few: the needed count, nothing run
        assert rc == -1 and n == total == 57
        still_fresh()
        rc, n = raw_score(eng, seqs, [0, 1, 2], froms, cap=total)
        assert rc == 0 and n == total
        eng.set_logits_range(100, 400, V - 1)                                                 # a restricted head
        with pytest.raises(_hip.NeuTTSHipError) as ei:
            eng.score_call([a], [0], [1])
        assert ei.value.code == -4
        eng.set_logits_range(None)
        still_fresh()
        eng.calibrate(True)                                                                   # calibration mode
        with pytest.raises(_hip.NeuTTSHipError) as ei:
            eng.score_call([a], [0], [1])
        assert ei.value.code == -4
        eng.calibrate(False)
        still_fresh()
    finally:
        eng.close()


def test_pages_that_do_not_fit_and_a_tap_that_would_not(lib, model3000):
    cfg, w = model3000
    seqs = seqs_for(cfg)
    q = (br.synthetic_prompt(cfg, 5, 100) * 21)[:2048]
    fresh = make_engine(cfg, w, lib, max_batch=2, max_context=128, max_prefill_tokens=256)
    try:
        want = fresh.score_call(seqs[:2], [0, 1], [1, 1])
        want_q = fresh.score_call([q[:40]], [0], [32])
    finally:
        fresh.close()
    same = lambda got, ref: all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, ref))
    eng = make_engine(cfg, w, lib, max_batch=2, max_context=128, max_prefill_tokens=256, num_pages=4)
    try:
        assert eng.kv_stats()["total_pages"] == 4
        with pytest.raises(_hip.NeuTTSHipError) as ei:
            eng.score_call(seqs[1:], [0, 1], [1, 1])                                          # 2 + 3 pages
        assert ei.value.code == -3 and eng.kv_stats()["free_pages"] == 4
        got = eng.score_call(seqs[:2], [0, 1], [1, 1])                                        # 2 + 2 pages: fits, and gives a fresh engine's bits
        assert len(got[0]) == 32 + 46 and same(got, want) and eng.kv_stats()["free_pages"] == 4
    finally:
        eng.close()
    # 64 MB of tapped rows = 5 592 rows of 3 000 logits: more scored positions are refused while the tap is on (before anything runs)
    big = make_engine(cfg, w, lib, max_batch=3, max_context=2048, max_prefill_tokens=6144)
    try:
        big.set_debug(True)
        with pytest.raises(_hip.NeuTTSHipError, match="64 MB") as ei:
            big.score_call([q, q, q], [0, 1, 2], [1, 1, 1])                                   # 6 141 rows
        assert ei.value.code == -1
        st = big.kv_stats()
        assert st["free_pages"] == st["total_pages"]
        lp = big.score_call([q[:40]], [0], [32])[0]                                           # a stretch that fits is served, tap on
        assert len(lp) == 8 and np.isfinite(big.read_score_logits(7)).all()
        big.set_debug(False)
        assert same(big.score_call([q[:40]], [0], [32]), want_q)                              # ... and after the refusal the engine gives a fresh one's bits
    finally:
        big.set_debug(False)
        big.close()


# ---------------------------------------------------------------------------------------------- 9. the fp8 engine
def test_fp8_engine_on_the_tapped_rows(lib):
    """weight_dtype = fp8 (e4m3 lm_head input rows at the head's static scale): the values on the tapped rows of 57 and of 150 scored positions (the
    256 x 256 tile), the latter in one chunk and in chunks of 64."""
    cfg = vcases.fp8_cfg()
    w = br.make_weights(cfg, 23, peak_sigma=0.5)
    scales = br.default_fp8_input_scales(cfg)
    eng = vcases._engine(cfg, w, lib, max_batch=3, input_scales=scales, weight_dtype="fp8", max_prefill_tokens=512)
    try:
        tapped_check(eng, seqs_for(cfg), froms_for(), [0, 1, 2], tag="fp8, 57 rows")
        seqs = seqs_for(cfg, (34, 48, 71), seed=170)
        bits = eng.score_call(seqs, [0, 1, 2], [1, 1, 1])
        tapped = tapped_check(eng, seqs, [1, 1, 1], [2, 0, 1], chunk_rows=64, tag="fp8, 150 rows")
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(bits, tapped))   # the tap, the slots and the chunking change nothing
    finally:
        eng.close()
