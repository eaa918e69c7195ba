"""Nucleus (top_p) and min-p sampling behind top-k (ntts_sampling.top_p / .min_p, ABI 10) on the CPU SIMT emulator: the device
function that chooses the token (csrc/kernels/sample.h sample_topk_row) against tests/sampling_spec.py -- through the kernel-level
probe on synthetic rows (both the grouped scan and the full-row fallback), and through the engine, where every draw is checked on
that step's tapped logits.  tests/test_gpu_sampling_nucleus.py runs the same bodies on libneutts_hip.so."""
import numpy as np
import pytest
import torch

from oracle import backbone_ref as br
from neutts import _hip
from common import make_engine
import sampling_spec as spec

MARGIN = 1e-5      # a draw / a cut this close (relative) to a boundary may fall either way on a device whose exp differs in the last bit


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


# ---------------------------------------------------------------------------------------------- the probe on synthetic rows
def synthetic_rows(V, seed, n_random=10, k_max=50):
    """[(row, k, T, top_p, min_p, seed, exact)]: `exact` marks constructed rows whose arithmetic AT the cut is exact in fp32 (sums of
    ones, e = exp(0)), so that a cut margin of 0 is not a coin toss; every other row must keep MARGIN from its cuts (asserted)."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n_random):
        x = spec.bf16_round(rng.standard_normal(V).astype(np.float32) * np.float32([1.0, 2.0, 4.0][i % 3]))
        rows.append((x, [8, k_max, 1, 20][i % 4], [0.7, 1.0, 1.3][i % 3], [0.95, 0.8, 0.5, 1.0][i % 4], [0.0, 0.05, 0.2][(i // 2) % 3], 100 + i, False))
    low = spec.bf16_round(rng.standard_normal(V).astype(np.float32) - 8.0)
    # ties at the top-p cut: six tokens share the maximum, the cut falls inside the group -> the lowest ids survive
    x = low.copy()
    tie_ids = np.sort(rng.choice(V, size=6, replace=False))
    x[tie_ids] = 2.0
    rows.append((x, 20, 1.0, 0.45, 0.0, 7, False))
    # ... and at a lower rank: one clear maximum, then four equal values of which the cut keeps two
    x = low.copy()
    x[tie_ids[0]] = 3.0
    x[tie_ids[1:5]] = 2.5
    rows.append((x, 8, 1.0, 0.7, 0.0, 8, False))
    # all logits equal (more candidates than the list holds: the 512 lowest ids; the cut falls by rank = by id)
    rows.append((np.full(V, 1.5, dtype=np.float32), k_max, 1.0, 0.3, 0.0, 9, True))
    rows.append((np.full(V, 1.5, dtype=np.float32), k_max, 0.7, 1.0, 0.5, 10, True))
    # k = 1: a single maximum; tied maxima (ties at the k-th value are kept, the nucleus then cuts among them)
    x = low.copy()
    x[V // 3] = 4.0
    rows.append((x, 1, 1.0, 0.9, 0.1, 11, True))
    x = low.copy()
    x[tie_ids] = 4.0
    rows.append((x, 1, 1.3, 0.5, 0.0, 12, True))
    # top_p -> 0: the greedy token, first maximum
    rows.append((x.copy(), k_max, 1.0, 1e-6, 0.0, 13, True))
    rows.append((rows[0][0], k_max, 1.0, 1e-6, 0.0, 14, True))
    # min_p = 1: exactly the maximal tokens
    rows.append((x.copy(), k_max, 0.7, 1.0, 1.0, 15, True))
    rows.append((rows[1][0], 20, 1.0, 1.0, 1.0, 16, True))
    # a masked EOS (-inf) that would have been the maximum's neighbour; and -inf INSIDE the candidate list (fewer finite logits than k:
    # the k-th largest is -inf, every token qualifies, the 512 lowest ids are kept, e = 0 for the masked ones)
    x = rows[2][0].copy()
    x[V - 1] = -np.inf
    rows.append((x, k_max, 1.0, 0.9, 0.02, 17, False))
    x = np.full(V, -np.inf, dtype=np.float32)
    x[np.sort(rng.choice(min(V, 400), size=5, replace=False))] = spec.bf16_round(rng.standard_normal(5).astype(np.float32))
    rows.append((x, 8, 1.0, 0.9, 0.0, 18, False))
    # k at the list's capacity on a random row: bf16 ties at the k-th value push the count past 512 by a few -- the lowest tie ids stay
    rows.append((rows[0][0], 512, 1.0, 0.9, 0.0, 19, False))
    rows.append((rows[1][0], 512, 1.3, 1.0, 0.001, 20, False))
    return rows


def check_probe(lib_path, V, ld, group_width, rows, step=3):
    lib = _hip.load_library(lib_path)
    buf = torch.full((len(rows), ld), float("-inf"), dtype=torch.float32)       # (the padding columns must never be looked at)
    buf[:, V:] = 1e30
    for r, row in enumerate(rows):
        buf[r, :V] = torch.from_numpy(row[0])
    dev = buf.to(torch.bfloat16).to(device_of(lib_path)).contiguous()
    tok, ids = _hip.sample_probe(lib, dev.data_ptr(), ld, len(rows), V, group_width, [r[1] for r in rows], [r[2] for r in rows],
                                 [r[3] for r in rows], [r[4] for r in rows], [r[5] for r in rows], step)
    cut = checked = 0
    for r, (x, k, T, top_p, min_p, seed, exact) in enumerate(rows):
        d = spec.sample(x, k, T, seed, step, top_p, min_p)
        assert exact or d.cut_margin > MARGIN, (r, d.cut_margin)                  # (a property of the row, not of the kernel: pick another row)
        assert np.array_equal(ids[r], d.ids), (V, group_width, r, k, T, top_p, min_p, ids[r].tolist(), d.ids.tolist())
        cut += len(d.ids) < len(spec.candidates(x, k, T)[0])
        if d.margin > MARGIN:
            assert int(tok[r]) == d.token, (V, group_width, r, int(tok[r]), d.token, d.margin)
            checked += 1
    assert cut >= len(rows) // 2 and checked >= len(rows) - 2
    return rows


@pytest.mark.parametrize("V,ld,group_width", [
    (4096, 4096, 64),     # grouped scan: 64 groups >= k
    (4096, 4096, 0),      # full row
    (1003, 1008, 16),     # a vocabulary that is no multiple of the 16-byte vectors nor of the group: the scalar tails of both scans
    (1003, 1008, 0),
    (512, 512, 16),       # fewer groups (32) than k = 50: the grouped entry falls back to the full row by itself
])
def test_probe_survivors_and_draw_equal_the_specification(lib, V, ld, group_width):
    rows = synthetic_rows(V, 5 + V)
    check_probe(lib, V, ld, group_width, rows)
    assert any(spec.sample(x, k, T, s, 3, tp, mp).straddle for x, k, T, tp, mp, s, _ in rows)      # the tie rule is exercised


def test_probe_refuses_invalid_parameters(lib):
    h = _hip.load_library(lib)
    dev = torch.zeros(1, 64, dtype=torch.bfloat16, device=device_of(lib))
    for kw in (dict(top_p=0.0), dict(top_p=1.5), dict(top_p=float("nan")), dict(min_p=-0.1), dict(min_p=1.01), dict(min_p=float("nan")),
               dict(top_k=0), dict(temperature=0.0)):
        a = dict(top_k=5, temperature=1.0, top_p=1.0, min_p=0.0)
        a.update(kw)
        with pytest.raises(_hip.NeuTTSHipError) as ei:
            _hip.sample_probe(h, dev.data_ptr(), 64, 1, 64, 0, a["top_k"], a["temperature"], a["top_p"], a["min_p"], 1, 0)
        assert ei.value.code == -1, kw


# ---------------------------------------------------------------------------------------------- through the engine
def samp(cfg, n_new, plen=0, **kw):
    """n_new tokens exactly: EOS stays masked (min_new_tokens live) until max_length stops the request."""
    d = dict(max_length=(plen + n_new) if plen else 64, min_new_tokens=n_new, eos_token_id=cfg.vocab_size - 1, do_sample=True)
    d.update(kw)
    return _hip.Sampling(**d)


def run(eng, prompts, slots, sampling, n_new):
    eng.prefill(prompts, slots, sampling)
    eng.decode(n_new - 1)
    out = [eng.read(s)[0] for s in slots]
    for s in slots:
        eng.release(s)
    return out


SETTINGS = [dict(top_k=8, temperature=1.5, top_p=0.8, min_p=0.0, seed=77),                      # top_p alone
            dict(top_k=50, temperature=1.0, top_p=1.0, min_p=0.05, seed=(5 << 32) | 12345),      # min_p alone
            dict(top_k=20, temperature=0.9, top_p=0.9, min_p=0.1, seed=4242)]                    # both


@pytest.mark.parametrize("max_batch", [2, 16])     # GEMV path (16-column groups) / tile path (64-column groups)
def test_every_draw_equals_the_specification(lib, model, max_batch):
    """Token for token over 10 steps: the engine's draw equals tests/sampling_spec.sample on that step's processed logits (debug tap), with
    min_new_tokens live (the EOS column is -inf in every row).  A step within MARGIN of a draw or cut boundary is not compared: at most
    one of a request's ten."""
    cfg, w = model
    eng = make_engine(cfg, w, lib, max_batch=max_batch)
    N = 10
    eng.set_debug(True)
    try:
        cut = 0
        for slot, st in zip([0, 1] if max_batch == 2 else [1, 7, 15], SETTINGS):
            p = br.synthetic_prompt(cfg, 30 + slot, 18)
            eng.prefill([p], [slot], [samp(cfg, N, **st)])
            checked = 0
            for step in range(N):
                if step:
                    eng.decode(1)
                ids, _ = eng.read(slot)
                row = eng.read_logits(slot)
                assert row[cfg.vocab_size - 1] == -np.inf
                d = spec.sample(row, st["top_k"], st["temperature"], st["seed"], step, st["top_p"], st["min_p"])
                cut += len(d.ids) < len(spec.candidates(row, st["top_k"], st["temperature"])[0])
                if d.margin > MARGIN and d.cut_margin > MARGIN:
                    assert ids[step] == d.token, (slot, step, ids[step], d.token, d.margin, d.cut_margin)
                    assert ids[step] in d.ids
                    checked += 1
            assert checked >= N - 1
            eng.release(slot)
        assert cut >= N            # the two stages did cut candidates away
    finally:
        eng.set_debug(False)


def test_defaults_are_the_topk_sampler_and_ids_do_not_depend_on_placement(lib, model):
    """Sampling() == Sampling(top_p=1.0, min_p=0.0) id for id; a request's ids depend on its own settings and seed only -- not on its
    slot, its neighbours or THEIR settings, nor on being admitted through parking rows in waves of min_admit by generate()."""
    cfg, w = model
    eng = make_engine(cfg, w, lib, max_batch=4, park_slots=2)
    N = 10
    p, q, r = (br.synthetic_prompt(cfg, 3, 20), br.synthetic_prompt(cfg, 4, 9), br.synthetic_prompt(cfg, 5, 13))
    base = dict(top_k=8, temperature=1.5, seed=5)
    a = run(eng, [p, p], [0, 1], [samp(cfg, N, **base), samp(cfg, N, top_p=1.0, min_p=0.0, **base)], N)
    assert a[0] == a[1]
    nuc = dict(top_k=20, temperature=1.2, top_p=0.7, min_p=0.05, seed=6)
    alone = run(eng, [p], [2], [samp(cfg, N, **nuc)], N)[0]
    assert alone != a[0]
    b = run(eng, [q, p, r, p], [0, 3, 1, 2], [samp(cfg, N, **base), samp(cfg, N, **nuc), samp(cfg, N, top_k=50, temperature=0.8, top_p=0.5, seed=9),
                                             samp(cfg, N, **base)], N)
    assert b[1] == alone and b[3] == a[0]
    # generate(): 7 requests over 4 decode slots + 2 parking rows, admitted two at a time; the nucleus request is parked at least once
    prompts = [q, r, p, q, p, r, p]
    sps = [samp(cfg, N, len(pp), top_k=50, temperature=1.0, top_p=[1.0, 0.9, 0.6][i % 3], min_p=[0.0, 0.1][i % 2], seed=50 + i)
           for i, pp in enumerate(prompts)]
    sps[4] = samp(cfg, N, len(p), **nuc)
    sps[6] = samp(cfg, N, len(p), **nuc)
    sps[2] = samp(cfg, N, len(p), **base)
    got = eng.generate(prompts, sps, steps_per_poll=4, min_admit=2)
    assert got[4] == alone and got[6] == alone and got[2] == a[0]
    assert all(len(g) == N for g in got)


def test_first_token_distribution_over_the_surviving_set(lib, model):
    """640 first-token draws follow the renormalised softmax over the specification's survivors (count and bound of
    tests/test_emu_sampling.py::test_first_token_distribution)."""
    cfg, w = model
    B, K, T, TOP_P, MIN_P = 16, 12, 0.8, 0.85, 0.04
    eng = make_engine(cfg, w, lib, max_batch=B)
    p = br.synthetic_prompt(cfg, 11, 16)
    eng.set_debug(True)
    eng.prefill([p], [0], [samp(cfg, 1, len(p), top_k=K, temperature=T, top_p=TOP_P, min_p=MIN_P, seed=1)])
    eng.sync()
    row = eng.read_logits(0)
    eng.release(0)
    eng.set_debug(False)
    ids, e, cut_margin, _ = spec.survivors(row, K, T, TOP_P, MIN_P)
    assert cut_margin > MARGIN and 2 <= len(ids) < len(spec.candidates(row, K, T)[0])
    want = e.astype(np.float64) / e.astype(np.float64).sum()
    counts = {int(i): 0 for i in ids}
    n = 0
    for rep in range(40):
        sp = [samp(cfg, 1, len(p), top_k=K, temperature=T, top_p=TOP_P, min_p=MIN_P, seed=1000 * rep + s) for s in range(B)]
        eng.prefill([p] * B, list(range(B)), sp)
        out, _ = eng.read_all()
        for s in range(B):
            assert out[s][0] in counts, (out[s][0], counts)
            counts[out[s][0]] += 1
            eng.release(s)
        n += B
    got = np.array([counts[int(i)] for i in ids]) / n
    assert n == 640 and np.abs(got - want).max() < 0.07, (got, want)


INVALID = [("top_p", 0.0), ("top_p", -0.5), ("top_p", 1.0001), ("top_p", float("nan")), ("min_p", -1e-3), ("min_p", 1.5), ("min_p", float("nan"))]


def test_invalid_values_are_refused_and_touch_no_slot(lib, model):
    cfg, w = model
    eng = make_engine(cfg, w, lib, max_batch=2)
    p = br.synthetic_prompt(cfg, 3, 12)
    good = samp(cfg, 4, top_k=5, temperature=1.0, seed=1)
    for field, value in INVALID:
        with pytest.raises(_hip.NeuTTSHipError) as ei:
            eng._prefill_call(2, np.asarray(p + p, dtype=np.int32), np.asarray([len(p)] * 2, dtype=np.int32), np.asarray([0, 1], dtype=np.int32),
                              [good, samp(cfg, 4, top_k=5, temperature=1.0, seed=1, **{field: value})], None)
        assert ei.value.code == -1 and "prompt 1" in str(ei.value) and field in str(ei.value), (field, value, str(ei.value))
        st, _ = eng.poll()
        assert st.tolist() == [0, 0] and eng.kv_stats()["free_pages"] == eng.kv_stats()["total_pages"]
    # greedy requests ignore both fields
    bad = samp(cfg, 4, top_p=float("nan"), min_p=7.0)
    bad.do_sample = False
    ids = run(eng, [p, p], [0, 1], [bad, samp(cfg, 4, do_sample=False)], 4)
    assert ids[0] == ids[1] and len(ids[0]) == 4
