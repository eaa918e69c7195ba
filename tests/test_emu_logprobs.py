"""Per-token log-probabilities (ntts_backbone_set_logprobs / _read_logprobs / _read_finished_logprobs, ntts_k_head_logprob_probe) on the CPU SIMT
emulator: the log-sum-exp epilogues (csrc/kernels/gemm.h gemm_epilogue / gemm_epilogue_nat, gemv.h) and the sampling kernel's merge through the
kernel-level probe against tests/logprob_spec.py, the engine's record against the spec on every step's tapped row and against the CPU oracle,
and the record's way through slots, parking rows, prefix sharing and the restricted head.
tests/test_gpu_logprobs.py runs the same bodies on libneutts_hip.so."""
import numpy as np
import pytest
import torch

from oracle import backbone_ref as br
from neutts import _hip
from common import make_engine
import logprob_spec as spec
import test_emu_repetition as rcases
from test_emu_repetition import EMU_PROBE_CASES, PENALTIES, FIXED_COLS, device_of

LSE_TOL = 1e-4        # absolute, on M + log S and on a log-probability: ~2 ulp per expf, fp32 sums of <= 96 terms per partial and <= 3 400 partials
                      # per row, one logf -- ~1e-5 relative on S -- plus the fp32 ulp of a value <= 64: 1e-4 leaves 10 x
SUM_TOL = 1e-5        # relative, on one partial's sum


@pytest.fixture(scope="module")
def lib(emu_lib):
    return emu_lib


model = rcases.model
model3000 = rcases.model3000


# ---------------------------------------------------------------------------------------------- 2. the epilogues through the probe
def probe_inputs(lib_path, M, N, K, seed, scale=1.0):
    dev = device_of(lib_path)
    gen = torch.Generator(device=dev).manual_seed(100 + seed + M)
    x = (torch.randn((M, K), generator=gen, device=dev, dtype=torch.float32) * scale).to(torch.bfloat16).contiguous()
    w = torch.randn((N, K), generator=gen, device=dev, dtype=torch.float32).to(torch.bfloat16).contiguous()
    return x, w


def check_lse_outputs(out, M, N, variant):
    """What every run of the probe must satisfy, on its OWN returned row: partial sums, zero padding groups, no NaN, (M, log S)."""
    logits, row16, pv, pi, width, ps, rmax, rlogs = out
    assert width == {"gemv": 16, "256x288": 96}.get(variant, 64) and ps.shape == pv.shape
    assert not np.isnan(logits).any() and not np.isnan(ps).any() and not np.isnan(rmax).any() and not np.isnan(rlogs).any()
    n_groups = (N + width - 1) // width
    worst = 0.0
    for m in range(M):
        gmax, gsum = spec.group_sums(logits[m], width)
        assert np.array_equal(pv[m, :n_groups].astype(np.float64), gmax), (variant, m)
        rel = np.abs(ps[m, :n_groups].astype(np.float64) - gsum) / np.maximum(gsum, 1e-300)
        assert rel.max() <= SUM_TOL, (variant, m, int(rel.argmax()), rel.max())
        assert (ps[m, :n_groups][~np.isfinite(gmax)] == 0).all()
        assert rmax[m] == logits[m].max(), (variant, m)
        worst = max(worst, abs(float(rmax[m]) + float(rlogs[m]) - spec.logsumexp(logits[m])))
    assert (pv[:, n_groups:] == -np.inf).all() and (ps[:, n_groups:] == 0).all()          # groups made of padding columns only: exactly 0
    print(f"[logprobs] probe {variant} M={M} N={N}: max |M + log S - logsumexp| = {worst:.3e} (bound {LSE_TOL:.0e})")
    assert worst <= LSE_TOL, (variant, worst)
    return worst


def check_logprob_probe(lib_path, variant, M, N, K, fp8=False, seed=0, scale=1.0, min_peak=4.0):
    """Every tile variant, without and with the penalty, two rows of three masking their EOS column: logits, bf16 row, part_val and part_idx are
    bit for bit those of ntts_k_head_penalty_probe on the same inputs, and the log-sum-exp outputs hold on the returned row."""
    lib = _hip.load_library(lib_path)
    rng = np.random.default_rng(100 + seed + M)
    x, w = probe_inputs(lib_path, M, N, K, seed, scale)
    v = _hip.HEAD_VARIANTS[variant]
    eos = N - 1
    mask = np.array([eos + 1 if m % 3 != 2 else 0 for m in range(M)], dtype=np.int32)
    kw = dict(fp8=fp8, xscale=4.0 * scale / 448.0)
    pen = np.array([PENALTIES[m % 4] for m in range(M)], dtype=np.float32)
    seen = rng.random((M, N)) < 0.05
    for c in FIXED_COLS:
        if c < N:
            seen[:, c] = True
    seen[:, eos] = True                                                                   # the masked EOS is also seen
    peak = 0.0
    for extra in (dict(), dict(mask_eos=mask), dict(seen=seen, rep_pen=pen, mask_eos=mask)):
        want = _hip.head_penalty_probe(lib, x.data_ptr(), w.data_ptr(), M, N, K, v, **extra, **kw)
        got = _hip.head_logprob_probe(lib, x.data_ptr(), w.data_ptr(), M, N, K, v, **extra, **kw)
        for a, b, name in zip(want[:4], got[:4], ("logits", "bf16 row", "part_val", "part_idx")):
            assert a.dtype == b.dtype and np.array_equal(a.view(np.uint32 if a.itemsize == 4 else np.uint16),
                                                         b.view(np.uint32 if b.itemsize == 4 else np.uint16)), (variant, name, sorted(extra))
        assert want[4] == got[4]
        if "mask_eos" in extra:
            assert (got[0][mask > 0, eos] == -np.inf).all()
        check_lse_outputs(got, M, N, variant)
        peak = max(peak, float(np.abs(got[0][np.isfinite(got[0])]).max()))
    assert peak >= min_peak, peak
    return peak


@pytest.mark.parametrize("variant,M,N,K,fp8", EMU_PROBE_CASES)
def test_lse_epilogue_equals_the_specification(lib, variant, M, N, K, fp8):
    check_logprob_probe(lib, variant, M, N, K, fp8)


def test_lse_epilogue_with_large_logits(lib):
    """X scaled until |logits| reach ~80: most terms of every sum underflow to 0; everything stays finite and within the bound."""
    peak = check_logprob_probe(lib, "128x128", 129, 3000, 64, False, seed=3, scale=2.5, min_peak=70.0)
    assert peak < 200.0


def test_logprob_probe_refuses_bad_arguments(lib):
    h = _hip.load_library(lib)
    dev = device_of(lib)
    x = torch.zeros(4, 64, dtype=torch.bfloat16, device=dev)
    w = torch.zeros(64, 64, dtype=torch.bfloat16, device=dev)
    for kw in (dict(variant=3), dict(variant=4, fp8=True), dict(rep_pen=0.0), dict(variant=8, M=17)):
        a = dict(variant=0, M=4, rep_pen=1.3, fp8=False)
        a.update(kw)
        with pytest.raises(_hip.NeuTTSHipError) as ei:
            _hip.head_logprob_probe(h, x.data_ptr(), w.data_ptr(), a["M"], 64, 64, a["variant"], seen=np.zeros((a["M"], 64), dtype=bool),
                                    rep_pen=a["rep_pen"], fp8=a["fp8"])
        assert ei.value.code == -1, kw
    # a row of zeros: every logit 0, S = N exactly
    out = _hip.head_logprob_probe(h, x.data_ptr(), w.data_ptr(), 4, 64, 64, 0)
    assert (out[6] == 0).all() and np.allclose(out[7], np.log(64.0), atol=1e-6)


# ---------------------------------------------------------------------------------------------- 4. the engine's record on the tapped rows
WARPED = dict(do_sample=True, top_k=50, top_p=0.95, min_p=0.05, temperature=0.7, seed=977)      # none of these enters a log-probability


def samp(cfg, n_new, plen=0, **kw):
    """n_new tokens exactly: EOS stays masked (min_new_tokens live) until max_length stops the request."""
    d = dict(max_length=(plen + n_new) if plen else 64, min_new_tokens=n_new, eos_token_id=cfg.vocab_size - 1, do_sample=False)
    d.update(kw)
    return _hip.Sampling(**d)


def check_record_on_tapped_rows(lib, model, max_batch, N=6):
    """Slots 0 / 1 / 2: a greedy, a sampled (every warper on) and a penalised request, filled by ONE prompt pass (so that every tap shows the row
    its slot's token was chosen from).  First token and N - 1 decode steps: entry i == spec.logprob(tapped row, id i) within 1e-4, earlier entries
    stay, every value <= 0; then the greedy slot against the CPU oracle's logits for the same ids."""
    cfg, w = model
    eng = make_engine(cfg, w, lib, max_batch=max_batch)
    eos = cfg.vocab_size - 1
    ps = [br.synthetic_prompt(cfg, 60 + i, 14 + 5 * i) for i in range(3)]
    sts = [dict(), WARPED, dict(repetition_penalty=1.3)]
    eng.set_logprobs(True)
    eng.set_debug(True)
    try:
        eng.prefill(ps, [0, 1, 2], [samp(cfg, N, len(p), **st) for p, st in zip(ps, sts)])
        prev = [np.zeros(0, dtype=np.float32)] * 3
        taps, worst = [], 0.0
        for step in range(N):
            if step:
                eng.decode(1)
            for s in range(3):
                ids, lp, row = eng.read(s)[0], eng.read_logprobs(s), eng.read_logits(s)
                assert len(ids) == step + 1 and lp.shape == (step + 1,) and lp.dtype == np.float32
                assert np.array_equal(lp[:step], prev[s])                                  # what was recorded stays
                assert row[eos] == -np.inf                                                  # the masked EOS column contributes 0 (spec: exp(-inf))
                want = spec.logprob(row, ids[step])
                worst = max(worst, abs(float(lp[step]) - want))
                assert abs(float(lp[step]) - want) <= LSE_TOL, (s, step, float(lp[step]), want)
                assert lp[step] <= 0.0
                if s == 0:
                    assert ids[step] == int(np.argmax(row))
                    taps.append(row)
                prev[s] = lp
        print(f"[logprobs] engine max_batch={max_batch} V={cfg.vocab_size}: max |logprob - spec| = {worst:.3e} (bound {LSE_TOL:.0e})")
        st, nn = eng.poll()
        assert st[:3].tolist() == [2, 2, 2] and nn[:3].tolist() == [N, N, N]               # finished by max_length: exactly n_new entries each
        assert prev[1].max() < 0.0                                                         # (a sampled token is not certain)
        # the oracle's logits, teacher-forced along the engine's greedy ids
        ids0 = eng.read(0)[0]
        ref = br.generate(cfg, br.cast_weights(w, torch.bfloat16), ps[0], len(ps[0]) + N, eos, min_new_tokens=N, keep_logits=True, force_ids=ids0)
        for i, (tap, orow) in enumerate(zip(taps, ref.logits)):
            orow = orow.numpy()
            fin = np.isfinite(orow)
            assert np.array_equal(fin, np.isfinite(tap))
            bound = 2.0 * float(np.abs(tap[fin] - orow[fin]).max()) + LSE_TOL              # both terms of the definition move by at most that
            assert abs(float(prev[0][i]) - spec.logprob(orow, ids0[i])) <= bound, (i, float(prev[0][i]), spec.logprob(orow, ids0[i]), bound)
    finally:
        eng.set_debug(False)
        eng.close()


@pytest.mark.parametrize("max_batch", [3, 16])                      # GEMV path / 64 x 64 tile path
def test_record_on_the_tapped_rows(lib, model, max_batch):
    check_record_on_tapped_rows(lib, model, max_batch)


def test_record_on_the_tapped_rows_vocabulary_3000(lib, model3000):
    check_record_on_tapped_rows(lib, model3000, 5)


def test_eos_token_has_an_entry(lib, model):
    """A request that stops on its EOS id: the EOS token's log-probability is the last entry, the count is n_new; while the EOS column is masked
    (min_new_tokens) it contributes nothing to the sum."""
    cfg, w = model
    eng = make_engine(cfg, w, lib, max_batch=3)
    p = br.synthetic_prompt(cfg, 81, 17)
    eng.set_logprobs(True)
    eng.set_debug(True)
    try:
        eng.prefill([p], [0], [samp(cfg, 8, len(p))])
        eng.decode(7)
        free = eng.read(0)[0]
        free_lp = eng.read_logprobs(0)
        eng.release(0)
        k = next(i for i in range(2, 8) if free[i] not in free[:i])                       # the id greedy decoding reaches at step k for the first time
        eos = free[k]
        eng.prefill([p], [0], [_hip.Sampling(max_length=len(p) + 8, min_new_tokens=2, eos_token_id=eos, do_sample=False)])
        row0 = eng.read_logits(0)
        assert row0[eos] == -np.inf and abs(float(eng.read_logprobs(0)[0]) - spec.logprob(row0, eng.read(0)[0][0])) <= LSE_TOL
        for step in range(1, k + 1):
            eng.decode(1)
        ids, fin = eng.read(0)
        lp = eng.read_logprobs(0)
        assert fin and ids == free[: k + 1] and ids[-1] == eos and len(lp) == k + 1
        row = eng.read_logits(0)
        assert np.isfinite(row[eos]) and abs(float(lp[-1]) - spec.logprob(row, eos)) <= LSE_TOL
        assert len(free_lp) == 8 and (lp <= 0).all()
        eng.decode(2)                                                                      # a finished row records nothing more
        assert np.array_equal(eng.read_logprobs(0), lp)
    finally:
        eng.set_debug(False)
        eng.close()


# ---------------------------------------------------------------------------------------------- 5. slot life cycle
def test_record_follows_the_request(lib, model):
    """One request -- sampled, penalised, a prompt of two shared pages and a tail -- under one engine configuration: bit-identical ids and
    log-probabilities alone, in a full ragged batch, in another slot, in a recycled slot, through a parking row, and as a prefix-sharing
    follower."""
    cfg, w = model
    eng = make_engine(cfg, w, lib, max_batch=4, park_slots=2, max_context=256, max_prefill_tokens=1024)
    N = 6
    head = br.synthetic_prompt(cfg, 7, 70)
    a, b = head + br.synthetic_prompt(cfg, 8, 9), head + br.synthetic_prompt(cfg, 9, 13)
    st = dict(WARPED, repetition_penalty=1.2)
    sa = samp(cfg, N, len(a), **st)
    eng.set_logprobs(True)

    def finish(slot, steps=N - 1):
        eng.decode(steps)
        out = eng.read(slot)[0], eng.read_logprobs(slot)
        return out

    def same(got, tag):
        assert got[0] == want[0] and got[1].shape == (N,) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), (tag, got, want)

    try:
        eng.prefill([a], [0], [sa])                                                        # alone
        want = finish(0)
        eng.release(0)
        assert len(want[0]) == N and (want[1] < 0).all()
        fill = [br.synthetic_prompt(cfg, 90 + i, 11 + 7 * i) for i in range(3)]            # a full ragged batch, the request in another slot;
        eng.prefill(fill + [a], [0, 1, 3, 2], [samp(cfg, N + 4, len(q), do_sample=bool(i % 2), seed=i) for i, q in enumerate(fill)] + [sa])
        same(finish(2), "ragged batch")
        eng.decode(4)                                                                      # the neighbours run on to N + 4 tokens
        assert len(eng.read_logprobs(3)) == N + 4 and np.array_equal(eng.read_logprobs(2), want[1])
        for s in range(4):
            eng.release(s)
        eng.prefill([a], [3], [sa])                                                        # a recycled slot whose last occupant recorded N + 4 values
        got = finish(3)
        same(got, "recycled slot")
        assert len(eng.read_logprobs(3)) == N
        eng.release(3)
        eng.prefill([fill[0]], [1], [samp(cfg, N + 4, len(fill[0]))])                      # through a parking row, while slot 1 decodes
        eng.prefill([a], [5], [sa])
        eng.decode(2)
        assert np.array_equal(eng.read_logprobs(5), want[1][:1])                           # the first token's value waits in the parking row
        eng._mark_busy([0])
        eng.activate([5], [0])
        assert np.array_equal(eng.read_logprobs(0), want[1][:1])
        same(finish(0), "parking row")
        eng.release(0)
        eng.release(1)
        sb = samp(cfg, N, len(b), **dict(st, seed=5))                                      # as a prefix-sharing follower of b
        eng.prefill([b, a], [0, 1], [sb, sa], donors=[None, (0, 70)])
        assert eng.kv_stats()["prompt_tokens_shared"] == 64
        same(finish(1), "prefix-sharing follower")
        shared_b = eng.read(0)[0], eng.read_logprobs(0)
        eng.release(0)
        eng.release(1)
        eng.prefill([b], [0], [sb])
        plain_b = finish(0)
        assert plain_b[0] == shared_b[0] and np.array_equal(plain_b[1], shared_b[1])
        eng.release(0)
    finally:
        eng.close()


def test_restricted_head_values_follow_the_compacted_row(lib, model):
    cfg, w = model
    eng = make_engine(cfg, w, lib, max_batch=2)
    lo, hi, eos = 100, 400, cfg.vocab_size - 1
    eng.set_logits_range(lo, hi, eos)
    eng.set_logprobs(True)
    eng.set_debug(True)
    p = br.synthetic_prompt(cfg, 10, 24)
    try:
        eng.prefill([p, p], [0, 1], [samp(cfg, 4, len(p)), samp(cfg, 4, len(p), **WARPED)])
        for step in range(4):
            if step:
                eng.decode(1)
            for s in (0, 1):
                row, ids, lp = eng.read_logits(s), eng.read(s)[0], eng.read_logprobs(s)
                assert np.isfinite(row).sum() == hi - lo and lo <= ids[step] < hi          # [range | masked EOS]; -inf everywhere else
                assert abs(float(lp[step]) - spec.logprob(row, ids[step])) <= LSE_TOL
    finally:
        eng.set_debug(False)
        eng.close()
    full = make_engine(cfg, w, lib, max_batch=2)                                           # the same request on the full head: a larger sum
    try:
        full.set_logprobs(True)
        full.prefill([p], [0], [samp(cfg, 4, len(p))])
        assert full.read_logprobs(0)[0] < lp[0] or full.read(0)[0] != ids[:1]
    finally:
        full.close()


def test_read_finished_equals_read_and_state_errors(lib, model):
    cfg, w = model
    eng = make_engine(cfg, w, lib, max_batch=3)
    p = br.synthetic_prompt(cfg, 3, 12)
    try:
        for call in (lambda: eng.read_logprobs(0), lambda: eng.read_finished_logprobs(0)):  # the switch is off
            with pytest.raises(_hip.NeuTTSHipError) as ei:
                call()
            assert ei.value.code == -4
        with pytest.raises(_hip.NeuTTSHipError) as ei:
            eng.generate([p], [samp(cfg, 4, len(p))], return_logprobs=True)
        assert ei.value.code == -4 and eng.free_slots() == 3
        eng.prefill([p], [1], [samp(cfg, 5, len(p))])
        with pytest.raises(_hip.NeuTTSHipError) as ei:
            eng.set_logprobs(True)                                                         # a slot is in use
        assert ei.value.code == -4 and not eng.logprobs
        eng.release(1)
        eng.set_logprobs(True)
        eng.set_logprobs(True)                                                             # (idempotent)
        eng.prefill([p], [1], [samp(cfg, 5, len(p), **WARPED)])
        with pytest.raises(_hip.NeuTTSHipError) as ei:
            eng.set_logprobs(False)
        assert ei.value.code == -4 and eng.logprobs
        eng.decode(4)
        eng.poll_begin()                                                                   # a run-ahead snapshot, more steps queued behind it
        eng.decode(2)
        st, nn = eng.poll_end()
        assert st[1] == 2 and nn[1] == 5
        fin = eng.read_finished_logprobs(1)
        assert fin.dtype == np.float32 and np.array_equal(fin, eng.read_logprobs(1)) and len(fin) == 5
        with pytest.raises(_hip.NeuTTSHipError) as ei:
            eng.read_finished_logprobs(0)                                                  # not finished in that snapshot
        assert ei.value.code == -4
        eng.release(1)
        assert len(eng.read_logprobs(1)) == 0                                              # a free slot shows nothing of its last occupant
        # generate(): one array per prompt, read before the slot is released -- also through on_finished
        ps = [br.synthetic_prompt(cfg, 20 + i, 9 + 4 * i) for i in range(5)]
        sp = [samp(cfg, 3 + i, len(q), **(WARPED if i % 2 else {})) for i, q in enumerate(ps)]
        ids, lps = eng.generate(ps, sp, return_logprobs=True)
        assert [len(x) for x in ids] == [3, 4, 5, 6, 7] == [len(x) for x in lps]
        seen = []
        ids2, lps2 = eng.generate(ps, sp, return_logprobs=True, run_ahead=False, on_finished=lambda i, s, n: seen.append((i, n)))
        assert sorted(seen) == [(i, 3 + i) for i in range(5)] and ids2 == [[]] * 5
        assert all(np.array_equal(x, y) for x, y in zip(lps, lps2))
        assert eng.generate(ps, sp) == ids                                                 # without the flag: the plain list
        eng.set_logprobs(False)
        assert eng.generate(ps, sp) == ids
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- 6. off means unchanged
def check_off_means_unchanged(lib, model, max_batch, calls=(3, 4)):
    """A mixed greedy / sampled / penalised batch draws the same ids with the switch off, on, off and on again; every toggle is followed by at
    least two decode calls (on the GPU: a captured step graph and a replay of it)."""
    cfg, w = model
    eng = make_engine(cfg, w, lib, max_batch=max_batch)
    N = 1 + sum(calls)
    ps = [br.synthetic_prompt(cfg, 40 + i, 10 + 3 * i) for i in range(4)]
    sts = [dict(), dict(do_sample=True, top_k=8, temperature=1.5, seed=5), dict(repetition_penalty=1.4),
           dict(do_sample=True, top_k=20, temperature=0.9, top_p=0.9, seed=6, repetition_penalty=1.2)]

    def run():
        eng.prefill(ps, [0, 1, 2, 3], [samp(cfg, N, len(p), **st) for p, st in zip(ps, sts)])
        for n in calls:
            eng.decode(n)
        out = [eng.read(s)[0] for s in range(4)]
        lps = [eng.read_logprobs(s) for s in range(4)] if eng.logprobs else None
        for s in range(4):
            eng.release(s)
        assert all(len(x) == N for x in out)
        return out, lps

    try:
        off, _ = run()
        eng.set_logprobs(True)
        on, lps = run()
        eng.set_logprobs(False)
        off2, _ = run()
        eng.set_logprobs(True)
        on2, lps2 = run()
        assert off == on == off2 == on2
        assert all(np.array_equal(a, b) and (a <= 0).all() and len(a) == N for a, b in zip(lps, lps2))
    finally:
        eng.close()


@pytest.mark.parametrize("max_batch", [4, 16])
def test_off_means_unchanged(lib, model, max_batch):
    check_off_means_unchanged(lib, model, max_batch)
