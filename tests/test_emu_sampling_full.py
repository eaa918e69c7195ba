"""Sampling over the whole vocabulary (ntts_sampling.top_k = -1) on the CPU SIMT emulator: the device function that chooses the token
(csrc/kernels/sample.h sample_full_row) against tests/sampling_full_spec.py -- through the kernel-level probe on synthetic rows, and
through the engine, where every draw is checked on that step's tapped logits.  tests/test_gpu_sampling_full.py runs the same bodies on
libneutts_hip.so.

A device's exp differs from numpy's in the last bits, so the comparison is the specification's own window (delta = 1e-5, the project's
MARGIN): strict survivors <= device survivors <= loose survivors, and the drawn token's interval of cumulative mass meets target +- delta * S.
Rows whose arithmetic at the cut is exact must match exactly, and of all rows of a parametrisation at most 10 % may differ from the
specification's survivors and token at all."""
import numpy as np
import pytest
import torch

from oracle import backbone_ref as br
from neutts import _hip
from common import make_engine
import sampling_full_spec as full
import sampling_spec as spec

MARGIN = full.MARGIN


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
def tie_ids(V):
    """six columns spread over the first 2048-column tile, the last one and column V - 1"""
    ids = sorted({3, 700, V // 2, ((V - 1) // 2048) * 2048 + 5, V - 2, V - 1})
    assert len(ids) == 6
    return np.asarray(ids)


def synthetic_rows(V, seed, n_random=10):
    """[(row, T, top_p, min_p, seed, exact)]: `exact` marks constructed rows whose survivors, token and total mass involve e = exp(0) = 1 only
    (and integer arithmetic on 2^32), so that they must match the specification bit for bit."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n_random):      # (row 0: top_p = 1 and min_p = 0 -- all V columns survive)
        x = spec.bf16_round(rng.standard_normal(V).astype(np.float32) * np.float32([1.0, 2.0, 4.0][i % 3]))
        rows.append((x, [0.7, 1.0, 1.3][i % 3], [1.0, 0.95, 0.8, 0.5][i % 4], [0.0, 0.05, 0.2][(i // 2) % 3], 100 + i, False))
    low = spec.bf16_round(rng.standard_normal(V).astype(np.float32) - 20.0)     # background of ~1e-9 of the maximum each, whatever V
    ties = tie_ids(V)
    # six tied maxima, the cut inside the group: the 3 / the 5 lowest ids stay (Q = 6 * 2^32 + a little: lim / 2^32 = 2.7.. / 4.8..)
    x = low.copy()
    x[ties] = 2.0
    rows.append((x, 1.0, 0.45, 0.0, 7, True))
    rows.append((x, 1.3, 0.8, 0.0, 8, True))
    # one maximum, then four equal values of which two stay (e = exp(-0.5): masses 1, 1.61, 2.21 before ranks 1, 2, 3; lim = 0.6 * 3.43 = 2.06)
    x = low.copy()
    x[ties[0]] = 3.0
    x[ties[1:5]] = 2.5
    rows.append((x, 1.0, 0.6, 0.0, 9, False))
    # constant rows: every e = 1; the nucleus cuts by id alone
    const = np.full(V, 1.5, dtype=np.float32)
    rows.append((const, 1.0, 1.0, 0.0, 10, True))
    rows.append((const, 1.0, 0.3, 0.0, 11, True))
    rows.append((const, 0.7, 1.0, 0.5, 12, True))
    # min_p = 1: exactly the maximal tokens
    x = low.copy()
    x[ties] = 4.0
    rows.append((x, 0.7, 1.0, 1.0, 13, True))
    rows.append((rows[1][0], 1.0, 1.0, 1.0, 14, True))
    # top_p -> 0: rank 0 alone, the first maximum
    rows.append((x, 1.0, 1e-6, 0.0, 15, True))
    rows.append((rows[0][0], 1.0, 1e-6, 0.0, 16, True))
    # a masked EOS (-inf) in the last column; a row with five finite values, cut and uncut
    x = rows[2][0].copy()
    x[V - 1] = -np.inf
    rows.append((x, 1.0, 0.9, 0.02, 17, False))
    x = np.full(V, -np.inf, dtype=np.float32)
    x[np.sort(rng.choice(min(V, 400), size=5, replace=False))] = spec.bf16_round(rng.standard_normal(5).astype(np.float32))
    rows.append((x, 1.0, 0.9, 0.0, 18, False))
    rows.append((x, 1.3, 1.0, 0.0, 19, False))
    return rows


def check_token(d, x, T, top_p, min_p, tok):
    """The window on the draw; a token the specification's own survivors do not hold must at least be a loose survivor."""
    if 0 <= tok < x.size and d.keep[tok]:
        assert full.token_in_window(d, tok), (tok, d.token, d.target, d.S)
    else:
        assert 0 <= tok < x.size and full.survivors(x, T, top_p, min_p, delta=+MARGIN, eq=(d.e, d.q))[tok], (tok, d.token)
    return tok == d.token


def check_full_probe(lib_path, V, ld, group_width, rows, step=3):
    lib = _hip.load_library(lib_path)
    buf = torch.full((len(rows), ld), float("-inf"), dtype=torch.float32)
    buf[:, V:] = 1e30                                                             # (the padding columns must never be looked at)
    for r, row in enumerate(rows):
        buf[r, :V] = torch.from_numpy(row[0])
    dev = buf.to(torch.bfloat16).to(device_of(lib_path)).contiguous()
    tok, n, bits, total = _hip.sample_full_probe(lib, dev.data_ptr(), ld, len(rows), V, group_width, [r[1] for r in rows], [r[2] for r in rows],
                                                 [r[3] for r in rows], [r[4] for r in rows], step)
    inexact = cut = 0
    for r, (x, T, top_p, min_p, seed, exact) in enumerate(rows):
        d = full.sample(x, T, seed, step, top_p, min_p)
        got = full.bits_to_mask(bits[r], V)
        where = (V, group_width, r, T, top_p, min_p)
        assert int(n[r]) == int(got.sum()) and not (bits[r][-1] >> np.uint32((V - 1) % 32) >> np.uint32(1)), where     # no bit past column V - 1
        strict = full.survivors(x, T, top_p, min_p, delta=-MARGIN, eq=(d.e, d.q))
        loose = full.survivors(x, T, top_p, min_p, delta=+MARGIN, eq=(d.e, d.q))
        assert not (strict & ~got).any() and not (got & ~loose).any(), (where, np.flatnonzero(strict & ~got)[:8], np.flatnonzero(got & ~loose)[:8])
        same = check_token(d, x, T, top_p, min_p, int(tok[r])) and np.array_equal(got, d.keep)
        assert got[int(tok[r])], where
        print(f"V {V} gw {group_width} row {r}: {int(n[r])} of {V} survive, token {int(tok[r])} (spec {d.token}), S {int(total[r])} (spec {d.S}), same {same}")
        if exact:
            assert same and int(total[r]) == d.S, (where, int(tok[r]), d.token, int(total[r]), d.S)
        elif np.array_equal(got, d.keep):
            assert abs(int(total[r]) - d.S) <= MARGIN * d.S, (where, int(total[r]), d.S)
        inexact += not same
        cut += int(d.keep.sum()) < V
    assert inexact * 10 <= len(rows), (inexact, len(rows))
    assert cut >= len(rows) // 2
    return tok, bits, total


@pytest.mark.parametrize("V,ld", [
    (1003, 1008),         # no multiple of the 16-byte vectors: the scalar tail; one tile
    (4096, 4096),         # two full tiles
    (66001, 66008),       # ids past 65 535, 33 tiles, a tail
])
def test_probe_survivors_draw_and_total_meet_the_specification(lib, V, ld):
    rows = synthetic_rows(V, 5 + V)
    a = check_full_probe(lib, V, ld, 0, rows)                                    # the maximum from a pass over the row
    b = check_full_probe(lib, V, ld, 16 if V < 4096 else 64, rows)              # ... from the maxima of column groups, as in the decode step
    for u, v in zip(a, b):
        assert np.array_equal(u, v)                                              # the results do not depend on group_width
    kept = [int(full.sample(x, T, s, 3, tp, mp).keep.sum()) for x, T, tp, mp, s, _ in rows]
    assert kept[0] == V and 3 in kept and 5 in kept and 1 in kept and 6 in kept  # uncut; the ties cut at 3 and at 5; top_p -> 0; min_p = 1


def test_probe_refuses_invalid_parameters(lib):
    h = _hip.load_library(lib)
    dev = torch.zeros(1, 64, dtype=torch.bfloat16, device=device_of(lib))
    for kw in (dict(top_p=0.0), dict(top_p=1.5), dict(top_p=float("nan")), dict(min_p=-0.1), dict(min_p=1.01), dict(min_p=float("nan")),
               dict(temperature=0.0), dict(temperature=float("nan")), dict(group_width=12), dict(group_width=-8), dict(ld=60), dict(vocab=0),
               dict(step=-1)):
        a = dict(temperature=1.0, top_p=1.0, min_p=0.0, group_width=0, ld=64, vocab=64, step=0)
        a.update(kw)
        with pytest.raises(_hip.NeuTTSHipError) as ei:
            _hip.sample_full_probe(h, dev.data_ptr(), a["ld"], 1, a["vocab"], a["group_width"], a["temperature"], a["top_p"], a["min_p"], 1, a["step"])
        assert ei.value.code == -1, kw
    with pytest.raises(_hip.NeuTTSHipError) as ei:                                # the top-k probe's id list holds 512: it keeps refusing -1
        _hip.sample_probe(h, dev.data_ptr(), 64, 1, 64, 0, -1, 1.0, 1.0, 0.0, 1, 0)
    assert ei.value.code == -1
    tok, n, bits, total = _hip.sample_full_probe(h, dev.data_ptr(), 64, 1, 64, 0, 1.0, 1.0, 0.0, 1, 0)       # a row of zeros: all 64 survive
    assert int(n[0]) == 64 and int(total[0]) == 64 << 32 and bits[0].tolist() == [0xFFFFFFFF] * 2 and 0 <= int(tok[0]) < 64


# ---------------------------------------------------------------------------------------------- through the engine
def samp(cfg, n_new, plen=0, **kw):
    """n_new tokens exactly: EOS stays masked (min_new_tokens live) until max_length stops the request."""
    d = dict(max_length=(plen + n_new) if plen else 64, min_new_tokens=n_new, eos_token_id=cfg.vocab_size - 1, do_sample=True, top_k=_hip.TOP_K_OFF)
    d.update(kw)
    return _hip.Sampling(**d)


def run(eng, prompts, slots, sampling, n_new):
    eng.prefill(prompts, slots, sampling)
    eng.decode(n_new - 1)
    out = [eng.read(s)[0] for s in slots]
    for s in slots:
        eng.release(s)
    return out


SETTINGS = [dict(temperature=1.0, top_p=1.0, min_p=0.0, seed=31),                               # plain ancestral sampling
            dict(temperature=1.5, top_p=0.8, min_p=0.0, seed=77),                               # top_p alone
            dict(temperature=1.3, top_p=1.0, min_p=0.05, seed=(5 << 32) | 12345),               # min_p alone
            dict(temperature=0.9, top_p=0.9, min_p=0.1, seed=4242)]                             # both


@pytest.mark.parametrize("max_batch", [2, 16])     # GEMV path (16-column groups) / tile path (64-column groups)
def test_every_draw_meets_the_specification(lib, model, max_batch):
    """The first token after the prompt pass and 7 decode steps of every setting: the engine's draw against the specification on that step's
    processed logits (debug tap), with min_new_tokens live (the EOS column is -inf in every row)."""
    cfg, w = model
    eng = make_engine(cfg, w, lib, max_batch=max_batch)
    N = 8
    eng.set_debug(True)
    try:
        inexact = wide = 0
        for slot, st in zip([0, 1, 0, 1] if max_batch == 2 else [1, 7, 15, 4], SETTINGS):
            p = br.synthetic_prompt(cfg, 30 + slot, 18)
            eng.prefill([p], [slot], [samp(cfg, N, **st)])
            for step in range(N):
                if step:
                    eng.decode(1)
                ids, _ = eng.read(slot)
                row = eng.read_logits(slot)
                assert row[cfg.vocab_size - 1] == -np.inf and len(ids) == step + 1
                d = full.sample(row, st["temperature"], st["seed"], step, st["top_p"], st["min_p"])
                inexact += not check_token(d, row, st["temperature"], st["top_p"], st["min_p"], ids[step])
                wide += int(d.keep.sum()) > 60          # more survivors than the top-k sampler's default keeps
            eng.release(slot)
        assert inexact * 10 <= N * len(SETTINGS), inexact
        assert wide >= N
    finally:
        eng.set_debug(False)


def test_mixed_step_ids_do_not_depend_on_the_neighbours(lib, model):
    """One greedy, one top_k = 50 and one top_k = -1 slot in the same steps: the first two draw bit for bit what they draw without the third,
    the third what it draws alone in another slot."""
    cfg, w = model
    eng = make_engine(cfg, w, lib, max_batch=4)
    N = 8
    p, q, r = (br.synthetic_prompt(cfg, 3, 20), br.synthetic_prompt(cfg, 4, 9), br.synthetic_prompt(cfg, 5, 13))
    greedy = samp(cfg, N, do_sample=False, top_k=50)
    topk = samp(cfg, N, top_k=50, temperature=1.2, top_p=0.9, seed=6)
    whole = samp(cfg, N, temperature=1.1, top_p=0.95, min_p=0.01, seed=9)
    two = run(eng, [p, q], [0, 1], [greedy, topk], N)
    alone = run(eng, [r], [3], [whole], N)[0]
    three = run(eng, [p, q, r], [0, 1, 2], [greedy, topk, whole], N)
    assert three[:2] == two and three[2] == alone and len(alone) == N
    # generate(): parked and admitted in waves, the whole-vocabulary request keeps its ids
    eng2 = make_engine(cfg, w, lib, max_batch=2, park_slots=2)
    sps = [samp(cfg, N, len(pp), **kw) for pp, kw in ((p, dict(do_sample=False)), (q, dict(top_k=50, temperature=1.2, top_p=0.9, seed=6)),
                                                      (r, dict(temperature=1.1, top_p=0.95, min_p=0.01, seed=9)), (r, dict(temperature=1.1, top_p=0.95, min_p=0.01, seed=9)))]
    got = eng2.generate([p, q, r, r], sps, steps_per_poll=4, min_admit=2)
    assert got[2] == alone and got[3] == alone and got[0] == two[0] and got[1] == two[1]


def test_logprob_of_a_whole_vocabulary_draw_under_a_repetition_penalty(lib, model):
    """repetition_penalty = 1.3 and set_logprobs: the recorded value is log_softmax of the tapped (penalised) row at the drawn token."""
    cfg, w = model
    eng = make_engine(cfg, w, lib, max_batch=2)
    N = 7
    eng.set_logprobs(True)
    eng.set_debug(True)
    try:
        p = br.synthetic_prompt(cfg, 12, 22)
        st = dict(temperature=1.4, top_p=0.97, min_p=0.0, seed=99)
        eng.prefill([p], [1], [samp(cfg, N, repetition_penalty=1.3, **st)])
        for step in range(N):
            if step:
                eng.decode(1)
            ids, _ = eng.read(1)
            row = eng.read_logits(1)
            lp = eng.read_logprobs(1)
            want = torch.log_softmax(torch.from_numpy(row).double(), dim=0)[ids[step]].item()
            assert len(lp) == step + 1 and abs(float(lp[step]) - want) <= 1e-4, (step, float(lp[step]), want)
            d = full.sample(row, st["temperature"], st["seed"], step, st["top_p"], st["min_p"])
            check_token(d, row, st["temperature"], st["top_p"], st["min_p"], ids[step])
        assert set(eng.read_seen(1).tolist()) >= set(eng.read(1)[0])                # every drawn token was marked for the next step's penalty
    finally:
        eng.set_debug(False)
        eng.release(1)
        eng.set_logprobs(False)


def test_compacted_head_maps_the_drawn_column_to_its_id(lib, model):
    cfg, w = model
    eng = make_engine(cfg, w, lib, max_batch=2)
    lo, hi, eos = 100, 400, cfg.vocab_size - 1
    eng.set_logits_range(lo, hi, eos)
    eng.set_debug(True)
    N = 7
    try:
        p = br.synthetic_prompt(cfg, 10, 24)
        st = dict(temperature=1.6, top_p=0.98, min_p=0.0, seed=5150)
        eng.prefill([p], [0], [samp(cfg, N, **st)])
        for step in range(N):
            if step:
                eng.decode(1)
            ids, _ = eng.read(0)
            row = eng.read_logits(0)
            cols = np.concatenate([row[lo:hi], row[eos:eos + 1]])                  # the head's columns: [range | EOS]
            d = full.sample(cols, st["temperature"], st["seed"], step, st["top_p"], st["min_p"])
            assert lo <= ids[step] < hi
            check_token(d, cols, st["temperature"], st["top_p"], st["min_p"], ids[step] - lo)
        assert len(set(eng.read(0)[0])) > 2
    finally:
        eng.set_debug(False)
        eng.release(0)
        eng.set_logits_range(None)


def test_invalid_top_k_is_refused_and_greedy_ignores_the_field(lib, model):
    cfg, w = model
    eng = make_engine(cfg, w, lib, max_batch=2)
    p = br.synthetic_prompt(cfg, 3, 12)
    good = samp(cfg, 4, temperature=1.0, seed=1)
    for k in (0, -2, -100):
        with pytest.raises(_hip.NeuTTSHipError) as ei:
            eng._prefill_call(2, np.asarray(p + p, dtype=np.int32), np.asarray([len(p)] * 2, dtype=np.int32), np.asarray([0, 1], dtype=np.int32),
                              [good, samp(cfg, 4, top_k=k, temperature=1.0, seed=1)], None)
        assert ei.value.code == -1 and "prompt 1" in str(ei.value) and "top_k" in str(ei.value), (k, str(ei.value))
        st, _ = eng.poll()
        assert st.tolist() == [0, 0] and eng.kv_stats()["free_pages"] == eng.kv_stats()["total_pages"]
    ids = run(eng, [p, p], [0, 1], [samp(cfg, 4, do_sample=False, top_k=-1), samp(cfg, 4, do_sample=False, top_k=50)], 4)
    assert ids[0] == ids[1] and len(ids[0]) == 4
    assert _hip.TOP_K_OFF == -1 and _hip.Sampling(top_k=_hip.TOP_K_OFF).to_c().top_k == -1
