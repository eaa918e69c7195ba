"""tests/sampling_spec.py (the numpy statement of temperature -> top-k -> top-p -> min-p -> draw) against its two neighbours: with
top_p = 1 and min_p = 0 it is oracle/sampling_ref.sample_topk token for token, and its surviving set is the one the installed
transformers warpers leave (TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper -> MinPLogitsWarper, the order of
hf:generation/utils.py _get_logits_processor).  CPU only, no library."""
import numpy as np
import torch

import sampling_spec as spec
from oracle.sampling_ref import sample_topk


def test_default_fields_are_the_topk_oracle():
    rng = np.random.default_rng(3)
    for V in (64, 512, 4096):
        for rep in range(40):
            x = spec.bf16_round(rng.standard_normal(V).astype(np.float32) * 3)
            if rep % 5 == 0:
                x[rng.integers(V)] = -np.inf                      # a masked EOS
            k, T, seed, step = int(rng.choice([1, 5, 50, 600])), float(rng.choice([0.7, 1.0, 1.5])), int(rng.integers(1 << 40)), rep
            tok, margin = sample_topk(x, k, T, seed, step)
            d = spec.sample(x, k, T, seed, step, top_p=1.0, min_p=0.0)
            assert (d.token, d.margin) == (tok, margin)
            assert d.cut_margin == float("inf") and not d.straddle
            kth = np.sort(x)[-min(k, V, 512)]
            assert np.array_equal(d.ids, np.flatnonzero(x >= kth)[:512])


def hf_surviving_values(x, k, T, top_p, min_p):
    from transformers.generation.logits_process import (MinPLogitsWarper, TemperatureLogitsWarper, TopKLogitsWarper,
                                                        TopPLogitsWarper)
    procs = [TemperatureLogitsWarper(T), TopKLogitsWarper(k)]     # (built unconditionally: T = 1 divides by one)
    if top_p < 1.0:
        procs.append(TopPLogitsWarper(top_p))
    if min_p > 0.0:
        procs.append(MinPLogitsWarper(min_p))
    scores = torch.from_numpy(x.copy())[None, :]
    ids = torch.zeros(1, 1, dtype=torch.long)
    for p in procs:
        scores = p(ids, scores)
    return np.sort(x[np.isfinite(scores[0].numpy())])


def test_surviving_set_is_transformers():
    """The multiset of surviving logit VALUES equals transformers' on every row (the ids may differ where bf16 values tie at a cut:
    torch.sort orders equal values arbitrarily, the specification takes the lowest id first).  A row whose nearest candidate lies
    within 1e-5 (relative) of a cut boundary may fall either way in fp32 and is skipped; at most 2 % of the rows may be."""
    rows = skipped = straddle = 0
    for x, k, T, top_p, min_p in spec.case_rows(20240607):
        rows += 1
        ids, e, cut_margin, st = spec.survivors(x, k, T, top_p, min_p)
        if cut_margin < 1e-5:
            skipped += 1
            continue
        straddle += st
        want = hf_surviving_values(x, k, T, top_p, min_p)
        got = np.sort(x[ids])
        assert got.shape == want.shape and np.array_equal(got, want), (x.size, k, T, top_p, min_p, got.size, want.size, cut_margin)
    print(f"{rows} rows, {skipped} skipped (cut margin < 1e-5), {straddle} with tied values on both sides of a cut")
    assert rows == 460 and skipped <= 0.02 * rows
    assert straddle >= 1          # the tie rule is exercised


def test_edge_settings():
    x = spec.bf16_round(np.array([0.5, 2.0, -1.0, 2.0, 1.0, 2.0, -np.inf, 0.25], dtype=np.float32))
    # top_p -> 0: the greedy token, first maximum
    assert spec.sample(x, 8, 1.0, 5, 0, top_p=1e-6).ids.tolist() == [1]
    # min_p = 1: exactly the maximal tokens
    assert spec.sample(x, 8, 1.0, 5, 0, min_p=1.0).ids.tolist() == [1, 3, 5]
    # ties at the top-p cut: lowest id first.  e = 1 each for the three maxima, total = 3 + e^-1 + ...: top_p = 0.3 keeps rank 0 and,
    # because the mass before rank 1 (1 / total ~ 0.21) is still < 0.3, rank 1 -- ids 1 and 3, not 5
    d = spec.sample(x, 8, 1.0, 5, 0, top_p=0.3)
    assert d.ids.tolist() == [1, 3] and d.straddle
    # all equal: every rank carries the same mass, the cut falls by rank = by id
    y = np.full(16, 1.5, dtype=np.float32)
    assert spec.sample(y, 16, 1.0, 1, 0, top_p=0.5).ids.tolist() == list(range(8))
    # k = 1 with ties kept at the k-th value, then the nucleus cut
    assert spec.sample(x, 1, 1.0, 1, 0).ids.tolist() == [1, 3, 5]
    assert spec.sample(x, 1, 1.0, 1, 0, top_p=0.5).ids.tolist() == [1, 3]
