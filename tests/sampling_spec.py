"""The device sampler's full contract in numpy (TEST INFRASTRUCTURE): temperature -> top-k -> top-p -> min-p -> draw, the order
of transformers' `_get_logits_processor`.  Stages 1 and 4 are oracle/sampling_ref.sample_topk (with top_p = 1 and min_p = 0 this
function IS that one, token for token: tests/test_sampling_spec.py); stages 2 and 3 restate TopPLogitsWarper / MinPLogitsWarper
(hf:generation/logits_process.py) from the top of the distribution, with the tie rule and the summation order the kernel
(neutts-air_amd/csrc/kernels/sample.h sample_topk_row) is held to:

  1. S0 = every token whose processed bf16 logit is >= the k-th largest (ties kept), in token-id order, capped at 512;
     e_a = fp32 exp((logit_a - max) * (1 / T))
  2. top_p < 1: rank S0 by value descending, ties by token id ascending; c_0 = 0, c_{j+1} = fp32(c_j + e_(j)) in that order,
     total_p = c_n; rank j survives iff j == 0 or c_j < fp32(top_p * total_p)
  3. min_p > 0: a token survives iff e_a >= fp32(min_p)
  4. survivors in token-id order, total = their e summed in that order, u from Philox(seed, step), inverse CDF.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from oracle.sampling_ref import uniform

CAP = 512


class Draw(NamedTuple):
    token: int
    margin: float        # draw margin (oracle/sampling_ref.sample_topk's): distance of u * total from the nearest cumulative sum, relative to total
    ids: np.ndarray      # final survivors, token-id order
    cut_margin: float    # distance of the nearest candidate from a top-p / min-p boundary (relative); inf if neither stage is active
    e: np.ndarray        # their softmax numerators (fp32)
    straddle: bool       # a value sits on both sides of a cut: only the tie rule decides which ids survive


def candidates(logits, k: int, temperature: float):
    """Stage 1: (ids in token order, their values, their e)."""
    x = np.asarray(logits, dtype=np.float32)
    k = min(int(k), x.size, CAP)
    kth = np.partition(x, x.size - k)[x.size - k]
    idx = np.flatnonzero(x >= kth)[:CAP]
    v = x[idx]
    it = np.float32(1.0) / np.float32(temperature)
    e = np.exp(((v - v.max()) * it).astype(np.float32)).astype(np.float32)
    return idx, v, e


def survivors(logits, k: int, temperature: float, top_p: float = 1.0, min_p: float = 0.0):
    """Stages 1-3: (ids, e, cut_margin, straddle)."""
    idx, v, e = candidates(logits, k, temperature)
    keep = np.ones(idx.size, dtype=bool)
    cut_margin = float("inf")
    if top_p < 1.0:
        order = np.lexsort((idx, -v))                                   # value descending, then token id ascending
        cs = np.cumsum(e[order], dtype=np.float32)                      # (accumulate: strictly sequential fp32 additions)
        c = np.concatenate([np.zeros(1, dtype=np.float32), cs[:-1]])    # mass strictly before rank j
        total_p = cs[-1]
        lim = np.float32(np.float32(top_p) * total_p)
        kr = c < lim
        kr[0] = True
        keep[order] = kr
        if idx.size > 1:
            cut_margin = min(cut_margin, float(np.abs(c[1:].astype(np.float64) - float(lim)).min() / max(float(total_p), 1e-30)))
    if min_p > 0.0:
        mp = np.float32(min_p)
        keep &= e >= mp
        cut_margin = min(cut_margin, float(np.abs(e.astype(np.float64) - float(mp)).min() / float(mp)))
    straddle = bool(np.intersect1d(v[keep], v[~keep]).size)
    return idx[keep], e[keep], cut_margin, straddle


def draw(ids, e, seed: int, step: int):
    """Stage 4 on a surviving set: (token, draw margin)."""
    cums = np.cumsum(e, dtype=np.float32)
    total = cums[-1]
    target = np.float32(np.float32(uniform(seed, step)) * total)
    hit = np.flatnonzero(cums.astype(np.float64) > float(target))
    pick = int(ids[hit[0]]) if hit.size else int(ids[-1])
    return pick, float(np.abs(cums.astype(np.float64) - float(target)).min()) / max(float(total), 1e-30)


def sample(logits, k: int, temperature: float, seed: int, step: int, top_p: float = 1.0, min_p: float = 0.0) -> Draw:
    ids, e, cut_margin, straddle = survivors(logits, k, temperature, top_p, min_p)
    pick, margin = draw(ids, e, seed, step)
    return Draw(pick, margin, ids, cut_margin, e, straddle)


def bf16_round(x) -> np.ndarray:
    """fp32 -> the nearest bf16 value (RNE), as fp32."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def case_rows(seed: int, plan=((512, 200), (4096, 200), (217488, 60))):
    """The seeded case generator of the HF comparison: (logits row of bf16 values, k, T, top_p, min_p) over random rows of
    several spreads at three vocabulary sizes, every parameter drawn from the grid below."""
    rng = np.random.default_rng(seed)
    for V, n in plan:
        for _ in range(n):
            x = bf16_round(rng.standard_normal(V).astype(np.float32) * np.float32(rng.choice([1.0, 2.0, 4.0])))
            yield (x, int(rng.choice([1, 8, 50, 200])), float(rng.choice([0.7, 1.0, 1.3])), float(rng.choice([1.0, 0.95, 0.8, 0.5])),
                   float(rng.choice([0.0, 0.05, 0.2])))
