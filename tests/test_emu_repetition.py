"""Repetition penalty (ntts_sampling.repetition_penalty / .prompt_ignore_length, ABI 11) on the CPU SIMT emulator: the lm_head epilogues
(csrc/kernels/gemm.h gemm_epilogue / gemm_epilogue_nat, gemv.h) through the kernel-level probe against tests/repetition_spec.py, the
per-slot seen bitmap through ntts_backbone_read_seen, and the engine's token choice on every step's tapped logits.
tests/test_gpu_repetition.py runs the same bodies on libneutts_hip.so."""
import numpy as np
import pytest
import torch

from oracle import backbone_ref as br
from neutts import _hip
from common import make_engine
import repetition_spec as rspec
import sampling_spec as sspec

MARGIN = 1e-5      # tests/test_emu_sampling_nucleus.py MARGIN: a draw / a cut this close to a boundary may fall either way
PENALTIES = [1.0, 1.3, 0.8, 2.0]
FIXED_COLS = [0, 15, 16, 31, 32, 63, 64, 255, 256, 2975, 2976, 2998, 2999]
NO_INDEX = 0x7FFFFFFF


@pytest.fixture(scope="module")
def lib(emu_lib):
    return emu_lib


@pytest.fixture(scope="module")
def model():
    cfg = br.BackboneConfig.tiny(vocab_size=512, num_layers=1)
    w = br.make_weights(cfg, 23, peak_sigma=0.3)
    return cfg, w


def device_of(lib):
    return "cuda" if "emu" not in lib else "cpu"


# ---------------------------------------------------------------------------------------------- 1. the epilogues through the probe
def check_head_probe(lib_path, variant, M, N, K, fp8=False, seed=0):
    """Every tile variant: processed logits == penalise(plain run's logits) bit for bit, rows with penalty 1 == the plain run, bf16 row ==
    fp32 dump, every partial == (max, first index) of its group of the PENALISED row; a row whose plain argmax is seen (the argmax must
    move) and a masked-EOS column that is seen (stays -inf, no NaN)."""
    lib = _hip.load_library(lib_path)
    rng = np.random.default_rng(100 + seed + M)
    dev = device_of(lib_path)
    gen = torch.Generator(device=dev).manual_seed(100 + seed + M)
    x = torch.randn((M, K), generator=gen, device=dev, dtype=torch.float32).to(torch.bfloat16).contiguous()
    w = torch.randn((N, K), generator=gen, device=dev, dtype=torch.float32).to(torch.bfloat16).contiguous()
    v = _hip.HEAD_VARIANTS[variant]
    eos = N - 1
    mask = np.array([eos + 1 if m % 3 != 2 else 0 for m in range(M)], dtype=np.int32)      # two rows of three mask their EOS column
    kw = dict(fp8=fp8, xscale=4.0 / 448.0)
    plain, plain16, pv0, pi0, width = _hip.head_penalty_probe(lib, x.data_ptr(), w.data_ptr(), M, N, K, v, mask_eos=mask, **kw)
    assert np.isfinite(plain[:, : N - 1]).all() and np.abs(plain).max() > 4
    assert (plain[mask > 0, eos] == -np.inf).all() and np.isfinite(plain[mask == 0, eos]).all()

    pen = np.array([PENALTIES[m % 4] for m in range(M)], dtype=np.float32)
    seen = rng.random((M, N)) < 0.05                                                      # bitmaps differ from row to row
    for c in FIXED_COLS:
        if c < N:
            seen[:, c] = True
    seen[:, eos] = True                                                                   # the masked EOS is also seen
    moved = [m for m in range(M) if m % 4 == 3][:3]                                       # penalty 2.0: the plain argmax is seen -> it must move
    for m in moved:
        seen[m, int(np.argmax(plain[m]))] = True
    got, got16, pv, pi, width2 = _hip.head_penalty_probe(lib, x.data_ptr(), w.data_ptr(), M, N, K, v, seen=seen, rep_pen=pen, mask_eos=mask, **kw)
    assert width2 == width and pv.shape == pv0.shape and width == {"gemv": 16, "256x288": 96}.get(variant, 64)
    assert not np.isnan(got).any()
    for m in range(M):
        want = rspec.penalise(plain[m], np.flatnonzero(seen[m]), pen[m])
        assert np.array_equal(got[m].view(np.uint32), want.view(np.uint32)), (variant, m, pen[m], np.flatnonzero(got[m] != want)[:8])
        if pen[m] == 1.0:
            assert np.array_equal(got[m].view(np.uint32), plain[m].view(np.uint32)) and np.array_equal(pv[m], pv0[m]) and np.array_equal(pi[m], pi0[m])
        else:
            assert (got[m] != plain[m]).sum() >= 0.03 * N
        if mask[m]:
            assert got[m, eos] == -np.inf
    for m in moved:
        assert int(np.argmax(got[m])) != int(np.argmax(plain[m])), m
    # the row the sampler reads is the dump, value for value
    assert np.array_equal(got16.astype(np.uint32) << 16, got.view(np.uint32))
    # the partials: maximum and FIRST index of every group of `width` columns of the penalised row
    n_groups = (N + width - 1) // width
    assert pv.shape[1] >= n_groups
    padded = np.full((M, n_groups * width), -np.inf, dtype=np.float32)
    padded[:, :N] = got
    grp = padded.reshape(M, n_groups, width)
    gmax, garg = grp.max(axis=2), grp.argmax(axis=2) + np.arange(n_groups)[None, :] * width
    assert np.array_equal(pv[:, :n_groups], gmax), (variant, np.argwhere(pv[:, :n_groups] != gmax)[:4])
    want_idx = np.where(gmax > -np.inf, garg, NO_INDEX)
    assert np.array_equal(pi[:, :n_groups], want_idx), (variant, np.argwhere(pi[:, :n_groups] != want_idx)[:4])
    assert (pv[:, n_groups:] == -np.inf).all()                                            # groups made of padding columns only
    # and the global argmax the sampling kernel would reduce them to: the first maximum of the penalised row
    for m in range(M):
        best = pv[m].max()
        assert int(pi[m][pv[m] == best].min()) == rspec.first_argmax(got[m])


# (variant, M = the smallest that spans two m-blocks of the tile, N, K); the gemv form has no m-blocks and needs N % 16 == 0
EMU_PROBE_CASES = [("64x64", 65, 3000, 64, False), ("128x128", 129, 3000, 64, False), ("256x256", 257, 3000, 64, False),
                   ("256x288", 257, 3000, 64, False), ("gemv", 5, 2992, 64, False), ("64x64", 65, 3000, 128, True), ("128x128", 129, 3000, 128, True), ("256x256", 257, 3000, 128, True),
                   ("gemv", 3, 2992, 128, True)]


@pytest.mark.parametrize("variant,M,N,K,fp8", EMU_PROBE_CASES)
def test_epilogue_equals_the_specification(lib, variant, M, N, K, fp8):
    check_head_probe(lib, variant, M, N, K, fp8)


def test_probe_refuses_bad_arguments(lib):
    h = _hip.load_library(lib)
    dev = device_of(lib)
    x = torch.zeros(4, 64, dtype=torch.bfloat16, device=dev)
    w = torch.zeros(64, 64, dtype=torch.bfloat16, device=dev)
    for kw in (dict(variant=3), dict(variant=4, fp8=True), dict(rep_pen=0.0), dict(rep_pen=float("nan")), dict(rep_pen=float("inf")), dict(rep_pen=-1.0),
               dict(variant=8, M=17)):
        a = dict(variant=0, M=4, rep_pen=1.3, fp8=False)
        a.update(kw)
        with pytest.raises(_hip.NeuTTSHipError) as ei:
            _hip.head_penalty_probe(h, x.data_ptr(), w.data_ptr(), a["M"], 64, 64, a["variant"], seen=np.zeros((a["M"], 64), dtype=bool),
                                    rep_pen=a["rep_pen"], fp8=a["fp8"])
        assert ei.value.code == -1, kw


# ---------------------------------------------------------------------------------------------- 2. slot state through read_seen
def samp(cfg, n_new, plen=0, **kw):
    """n_new tokens exactly: EOS stays masked (min_new_tokens live) until max_length stops the request."""
    d = dict(max_length=(plen + n_new) if plen else 64, min_new_tokens=n_new, eos_token_id=cfg.vocab_size - 1, do_sample=False)
    d.update(kw)
    return _hip.Sampling(**d)


def seen_of(eng, slot):
    return set(eng.read_seen(slot).tolist())


def test_bitmap_follows_prompt_and_generated_tokens(lib, model):
    cfg, w = model
    eng = make_engine(cfg, w, lib, max_batch=4)
    p = br.synthetic_prompt(cfg, 3, 20)
    p[7] = p[2]                                                    # duplicates are the norm
    with pytest.raises(_hip.NeuTTSHipError) as ei:                 # no bitmap before the first penalised request
        eng.read_seen(0)
    assert ei.value.code == -4
    for ignore in (0, 5, len(p), len(p) + 9):
        eng.prefill([p, p], [1, 2], [samp(cfg, 8, repetition_penalty=1.3, prompt_ignore_length=ignore), samp(cfg, 8)])
        first = eng.read(1)[0]
        assert seen_of(eng, 1) == rspec.seen_set(p, first, ignore) and len(first) == 1
        assert seen_of(eng, 2) == set() and seen_of(eng, 0) == set() and seen_of(eng, 3) == set()    # penalty 1.0 / untouched neighbours
        eng.decode(6)
        ids = eng.read(1)[0]
        assert len(ids) == 7 and seen_of(eng, 1) == rspec.seen_set(p, ids, ignore)
        assert seen_of(eng, 2) == set()
        eng.release(1)
        eng.release(2)
    # a slot reused by a shorter, different prompt: no stale bits; and by an unpenalised one: cleared
    q = br.synthetic_prompt(cfg, 4, 9)
    eng.prefill([q], [1], [samp(cfg, 4, repetition_penalty=0.8)])
    assert seen_of(eng, 1) == rspec.seen_set(q, eng.read(1)[0])
    eng.release(1)
    eng.prefill([q], [1], [samp(cfg, 4)])
    eng.decode(2)
    assert seen_of(eng, 1) == set()
    eng.release(1)


def test_bitmap_moves_with_a_parked_request(lib, model):
    cfg, w = model
    eng = make_engine(cfg, w, lib, max_batch=2, park_slots=2)
    p, q = br.synthetic_prompt(cfg, 5, 14), br.synthetic_prompt(cfg, 6, 11)
    N = 6
    # the reference run: straight into decode slot 0
    eng.prefill([p], [0], [samp(cfg, N, repetition_penalty=2.0, prompt_ignore_length=3)])
    eng.decode(N - 1)
    want = eng.read(0)[0]
    want_seen = seen_of(eng, 0)
    eng.release(0)
    assert want_seen == rspec.seen_set(p, want, 3)
    # parked in row 3 while slot 1 decodes something else, then activated into slot 0 (whose old bits must not survive)
    eng.prefill([q], [1], [samp(cfg, N + 2, repetition_penalty=1.3)])
    eng.prefill([p], [3], [samp(cfg, N, repetition_penalty=2.0, prompt_ignore_length=3)])
    eng.decode(2)                                                  # the parked request does not decode
    assert seen_of(eng, 3) == rspec.seen_set(p, want[:1], 3)
    eng._mark_busy([0])
    eng.activate([3], [0])
    assert seen_of(eng, 0) == rspec.seen_set(p, want[:1], 3)
    eng.decode(N - 1)
    assert eng.read(0)[0] == want and seen_of(eng, 0) == want_seen
    assert seen_of(eng, 1) == rspec.seen_set(q, eng.read(1)[0])
    eng.release(0)
    eng.release(1)
    # without the penalty the same request generates something else: the penalty did travel with it
    eng.prefill([p], [0], [samp(cfg, N)])
    eng.decode(N - 1)
    assert eng.read(0)[0] != want
    eng.release(0)
    # an unpenalised request activated into a slot whose last penalised occupant left bits behind: the row arrives empty
    eng.prefill([p], [0], [samp(cfg, N, repetition_penalty=1.3)])
    eng.release(0)
    assert seen_of(eng, 0) != set()
    eng.prefill([q], [2], [samp(cfg, N)])
    eng._mark_busy([0])
    eng.activate([2], [0])
    eng.decode(2)
    assert seen_of(eng, 0) == set() and len(eng.read(0)[0]) == 3
    eng.release(0)


def test_shared_prefix_prompt_marks_the_full_prompt(lib, model):
    cfg, w = model
    eng = make_engine(cfg, w, lib, max_batch=3, max_context=256)
    head = br.synthetic_prompt(cfg, 7, 70)                          # two whole pages are shared
    a, b = head + br.synthetic_prompt(cfg, 8, 9), head + br.synthetic_prompt(cfg, 9, 13)
    sp = [samp(cfg, 5, len(a), repetition_penalty=1.3), samp(cfg, 5, len(b), repetition_penalty=1.3, prompt_ignore_length=4)]
    eng.prefill([a, b], [0, 1], sp, donors=[None, (0, 70)])
    assert eng.kv_stats()["prompt_tokens_shared"] == 64
    eng.decode(4)
    shared = [eng.read(s)[0] for s in (0, 1)]
    shared_seen = [seen_of(eng, s) for s in (0, 1)]
    eng.release(0)
    eng.release(1)
    eng.prefill([a, b], [0, 1], sp)
    eng.decode(4)
    assert [eng.read(s)[0] for s in (0, 1)] == shared and [seen_of(eng, s) for s in (0, 1)] == shared_seen
    assert shared_seen[1] == rspec.seen_set(b, shared[1], 4)
    eng.release(0)
    eng.release(1)


def test_restricted_head_bitmap_is_column_indexed(lib, model):
    cfg, w = model
    eng = make_engine(cfg, w, lib, max_batch=2)
    lo, hi, eos = 100, 400, cfg.vocab_size - 1
    eng.set_logits_range(lo, hi, eos)
    p = br.synthetic_prompt(cfg, 10, 24) + [eos, lo, hi - 1, hi, lo - 1]
    eng.set_debug(True)
    try:
        eng.prefill([p, p], [0, 1], [samp(cfg, 6, repetition_penalty=1.3), samp(cfg, 6)])
        plain = eng.read_logits(1)
        row = eng.read_logits(0)
        cols = {t - lo for t in p if lo <= t < hi} | {hi - lo}        # [range | EOS]; ids outside are dropped
        first = eng.read(0)[0]
        col_of = lambda t: t - lo if t != eos else hi - lo
        assert seen_of(eng, 0) == cols | {col_of(first[0])}
        seen_ids = {t for t in p if lo <= t < hi or t == eos}
        assert np.array_equal(row.view(np.uint32), rspec.penalise(plain, seen_ids, 1.3).view(np.uint32))
        assert first[0] == rspec.first_argmax(row)
        eng.decode(3)
        ids = eng.read(0)[0]
        assert seen_of(eng, 0) == cols | {col_of(t) for t in ids} and all(lo <= t < hi for t in ids)
    finally:
        eng.set_debug(False)
        eng.release(0)
        eng.release(1)
        eng.set_logits_range(None)


# ---------------------------------------------------------------------------------------------- 3. / 4. first token and every decode step, exact
SAMPLED = dict(do_sample=True, top_k=12, temperature=1.2, top_p=0.9, min_p=0.02, seed=4711)


def check_choice(row, tok, st, step):
    """greedy: the first argmax of the row; do_sample: tests/sampling_spec.sample on it, under the MARGIN rule.  Returns 1 if compared."""
    if not st.get("do_sample"):
        assert tok == rspec.first_argmax(row), (step, tok, rspec.first_argmax(row))
        return 1
    d = sspec.sample(row, st["top_k"], st["temperature"], st["seed"], step, st["top_p"], st["min_p"])
    assert tok in d.ids
    if d.margin > MARGIN and d.cut_margin > MARGIN:
        assert tok == d.token, (step, tok, d.token, d.margin, d.cut_margin)
        return 1
    return 0


@pytest.mark.parametrize("max_batch", [3, 16])                      # GEMV path / 64 x 64 tile path
@pytest.mark.parametrize("st", [dict(do_sample=False), SAMPLED], ids=["greedy", "sampled"])
def test_first_token_and_every_step_on_the_tapped_row(lib, model, max_batch, st):
    check_first_token_and_steps(lib, model, max_batch, st)


@pytest.fixture(scope="module")
def model3000():
    cfg = br.BackboneConfig.tiny(vocab_size=3000, num_layers=1)      # no multiple of 16 / 32 / 64: the last column group of every tile is part empty
    return cfg, br.make_weights(cfg, 29, peak_sigma=0.3)


@pytest.mark.parametrize("st", [dict(do_sample=False), SAMPLED], ids=["greedy", "sampled"])
def test_first_token_and_every_step_vocabulary_3000(lib, model3000, st):
    check_first_token_and_steps(lib, model3000, 5, st)


def check_first_token_and_steps(lib, model, max_batch, st):
    """Slots 0 and 1 get the same prompt with penalty 1.0 and 1.3.  First token: read_logits(pen) == penalise(read_logits(plain), set(prompt), 1.3)
    bit for bit and the id is the choice the specification makes on that row.  Then 8 steps: the penalised slot's row equals penalise of the
    row an UNPENALISED twin computes when it is teacher-forced along the same ids, and every id is the specification's choice on its row."""
    cfg, w = model
    eng = make_engine(cfg, w, lib, max_batch=max_batch)
    p = br.synthetic_prompt(cfg, 30, 18)
    N = 9
    eng.set_debug(True)
    try:
        eng.prefill([p, p], [0, 1], [samp(cfg, N, **st), samp(cfg, N, repetition_penalty=1.3, **st)])
        checked = 0
        for step in range(N):
            if step:
                eng.decode(1)
            ids = eng.read(1)[0]
            assert len(ids) == step + 1
            plain, row = eng.read_logits(0), eng.read_logits(1)
            assert plain[cfg.vocab_size - 1] == -np.inf and row[cfg.vocab_size - 1] == -np.inf
            want = rspec.penalise(plain, rspec.seen_set(p, ids[:step]), 1.3)
            assert np.array_equal(row.view(np.uint32), want.view(np.uint32)), (step, np.flatnonzero(row != want)[:8])
            assert (row != plain).sum() >= len(set(p)) - 1
            checked += check_choice(row, ids[step], st, step)
            check_choice(plain, eng.read(0)[0][step], st, step)
            eng.debug_force(0, ids[step])                          # the twin follows the penalised slot's ids: same context next step
        assert checked >= N - 1
        assert seen_of(eng, 1) == rspec.seen_set(p, eng.read(1)[0]) and seen_of(eng, 0) == set()
    finally:
        eng.set_debug(False)
        eng.release(0)
        eng.release(1)


# ---------------------------------------------------------------------------------------------- 5. defaults
def test_unpenalised_batches_do_not_change(lib, model):
    """The ids of a batch without a penalised request: before any penalised request touched the engine == with Sampling's explicit defaults ==
    with a zeroed penalty field == afterwards, once the bitmap is allocated (penalised neighbour in flight, and none)."""
    cfg, w = model
    eng = make_engine(cfg, w, lib, max_batch=4)
    N = 8
    ps = [br.synthetic_prompt(cfg, 40 + i, 10 + 3 * i) for i in range(3)]
    sts = [dict(do_sample=False), dict(do_sample=True, top_k=8, temperature=1.5, seed=5), dict(do_sample=True, top_k=20, temperature=0.9, top_p=0.9, seed=6)]

    def run(extra, penalised_neighbour=False):
        sp = [samp(cfg, N, **st, **extra) for st in sts]
        eng.prefill(ps, [0, 1, 2], sp)
        if penalised_neighbour:
            eng.prefill([ps[0]], [3], [samp(cfg, N, repetition_penalty=1.7)])
        eng.decode(N - 1)
        out = [eng.read(s)[0] for s in range(3 + penalised_neighbour)]
        for s in range(3 + penalised_neighbour):
            eng.release(s)
        return out

    before = run({})
    assert before == run(dict(repetition_penalty=1.0, prompt_ignore_length=0)) == run(dict(repetition_penalty=0.0, prompt_ignore_length=7))
    with pytest.raises(_hip.NeuTTSHipError):
        eng.read_seen(0)                                           # still no bitmap
    mixed = run({}, penalised_neighbour=True)
    assert mixed[:3] == before and mixed[3] != before[0]           # neighbours of a penalised request; the penalty changes ITS ids
    assert run({}) == before                                       # bitmap allocated, nobody penalised
    assert all(len(x) == N for x in before)


# ---------------------------------------------------------------------------------------------- 6. validation
INVALID = [("repetition_penalty", float("nan")), ("repetition_penalty", -1.0), ("repetition_penalty", -0.0001), ("repetition_penalty", float("inf")),
           ("repetition_penalty", float("-inf")), ("prompt_ignore_length", -1)]


def test_invalid_values_are_refused_and_touch_no_slot(lib, model):
    cfg, w = model
    eng = make_engine(cfg, w, lib, max_batch=2)
    p = br.synthetic_prompt(cfg, 3, 12)
    for field, value in INVALID:
        kw = dict(repetition_penalty=1.3)
        kw[field] = value
        for do_sample in (False, True):                            # greedy and sampled requests alike
            with pytest.raises(_hip.NeuTTSHipError) as ei:
                eng._prefill_call(2, np.asarray(p + p, dtype=np.int32), np.asarray([len(p)] * 2, dtype=np.int32), np.asarray([0, 1], dtype=np.int32),
                                  [samp(cfg, 4), samp(cfg, 4, do_sample=do_sample, **kw)], None)
            assert ei.value.code == -1 and "prompt 1" in str(ei.value) and field in str(ei.value), (field, value, str(ei.value))
            st, _ = eng.poll()
            assert st.tolist() == [0, 0] and eng.kv_stats()["free_pages"] == eng.kv_stats()["total_pages"]
    # a penalty that is off ignores the ignore length; 0 (a zeroed field) is off
    ids = [None, None]
    for i, kw in enumerate((dict(repetition_penalty=0.0, prompt_ignore_length=-5), dict())):
        eng.prefill([p], [i], [samp(cfg, 4, **kw)])
    eng.decode(3)
    ids = [eng.read(s)[0] for s in (0, 1)]
    assert ids[0] == ids[1] and len(ids[0]) == 4
    eng.release(0)
    eng.release(1)
