"""Whole-vocabulary sampling (ntts_sampling.top_k = -1) in numpy and Python integers (TEST INFRASTRUCTURE): the contract the device function
neutts-air_amd/csrc/kernels/sample.h sample_full_row is held to.  Temperature -> top-p -> min-p -> draw over ALL V columns of the processed
bf16 row (repetition penalty and EOS mask applied, at least one finite value), with the probability masses as INTEGERS, so that the result is
a function of the row and the parameters alone -- not of the order of any additions:

  1. m = max x, it = fp32(1 / T), e_a = fp32 exp(fp32((x_a - m) * it)) (tests/sampling_spec.candidates' expression; -inf gives 0),
     q_a = floor(e_a * 2^32) as an unsigned 64-bit integer (exact; a maximum has q = 2^32); every sum below is an exact integer sum of q
  2. top_p < 1: rank by value descending, ties by token id ascending; c_j = sum_{i<j} q_(i), Q = sum q, lim = floor(top_p * Q) with top_p
     taken as the exact fp32 value M * 2^-s, i.e. lim = (M * Q) >> s; rank j survives iff j == 0 or c_j < lim
  3. min_p > 0: a token survives iff e_a >= fp32(min_p) (an fp32 compare); stages 2 and 3 are both evaluated on the whole row and ANDed
  4. survivors in token-id order, C_a their running sum of q, S the total; u24 = philox(seed, step)[0] >> 8; target = (u24 * S) >> 24;
     the token is the first survivor with C_a > target (it always exists).

A token whose probability is below 2^-32 of the likeliest token's has q = 0 and is never drawn.

`delta` (tests against a device whose exp differs from numpy's in the last bits): survivors(..., delta=+d) is the LOOSE set (lim * (1 + d),
min_p * (1 - d)), delta=-d the STRICT one; token_in_window() is the matching statement for the draw."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from oracle.sampling_ref import philox4x32_10

MARGIN = 1e-5          # the project's margin for a cut / a draw next to a boundary (tests/test_emu_sampling_nucleus.py)
_DEN = 100_000         # 1 / MARGIN as an integer: lim * (1 +- MARGIN) stays integer arithmetic


class FullDraw(NamedTuple):
    token: int
    keep: np.ndarray     # bool [V]: the survivors
    S: int               # their total mass
    target: int
    q: np.ndarray        # uint64 [V]
    e: np.ndarray        # float32 [V]


def masses(x, temperature: float):
    """Stage 1: (e float32 [V], q uint64 [V])."""
    x = np.asarray(x, dtype=np.float32)
    it = np.float32(1.0) / np.float32(temperature)
    with np.errstate(invalid="ignore"):
        e = np.exp(((x - x.max()) * it).astype(np.float32)).astype(np.float32)
    return e, quantise(e)


def quantise(e) -> np.ndarray:
    """q = floor(e * 2^32), exact: e is fp32 in [0, 1], the product is exact in float64."""
    return np.floor(np.asarray(e, dtype=np.float64) * 4294967296.0).astype(np.uint64)


def top_p_limit(top_p: float, Q: int) -> int:
    """floor(top_p * Q) with top_p the exact fp32 value M * 2^-s."""
    b = int(np.float32(top_p).view(np.uint32))
    ex, frac = (b >> 23) & 0xFF, b & 0x7FFFFF
    M, s = ((frac | 0x800000), 150 - ex) if ex else (frac, 149)
    return (M * int(Q)) >> s if s >= 0 else (M * int(Q)) << -s


def survivors(x, temperature: float, top_p: float = 1.0, min_p: float = 0.0, delta: float = 0.0, eq=None) -> np.ndarray:
    """Stages 1-3: the bool mask of the survivors.  delta = +MARGIN / -MARGIN: the loose / strict set.  eq: (e, q) to use instead of
    masses(x, temperature) (a simulated device exp)."""
    x = np.asarray(x, dtype=np.float32)
    e, q = masses(x, temperature) if eq is None else eq
    keep = np.ones(x.size, dtype=bool)
    sgn = (delta > 0) - (delta < 0)
    if top_p < 1.0:
        order = np.lexsort((np.arange(x.size), -x))                  # value descending, then token id ascending
        qs = q[order]
        c = np.cumsum(qs, dtype=np.uint64) - qs                      # mass strictly before rank j (exact: V * 2^32 fits 64 bits)
        lim = top_p_limit(top_p, int(qs.sum(dtype=np.uint64)))
        lim = lim * (_DEN + sgn) // _DEN
        kr = c < np.uint64(lim)
        kr[0] = True
        keep[order] = kr
    if min_p > 0.0:
        if sgn:
            keep &= e.astype(np.float64) >= float(np.float32(min_p)) * (1.0 - sgn * MARGIN)
        else:
            keep &= e >= np.float32(min_p)
    return keep


def u24_of(seed: int, step: int) -> int:
    return philox4x32_10([step, 0, 0, 0], [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF])[0] >> 8


def draw(keep, q, seed: int, step: int):
    """Stage 4: (token, S, target)."""
    ids = np.flatnonzero(keep)
    C = np.cumsum(q[ids], dtype=np.uint64)
    S = int(C[-1])
    target = (u24_of(seed, step) * S) >> 24
    return int(ids[int(np.searchsorted(C, np.uint64(target), side="right"))]), S, target


def sample(x, temperature: float, seed: int, step: int, top_p: float = 1.0, min_p: float = 0.0, eq=None) -> FullDraw:
    x = np.asarray(x, dtype=np.float32)
    e, q = masses(x, temperature) if eq is None else eq
    keep = survivors(x, temperature, top_p, min_p, eq=(e, q))
    tok, S, target = draw(keep, q, seed, step)
    return FullDraw(tok, keep, S, target, q, e)


def token_in_window(d: FullDraw, token: int) -> bool:
    """`token` is a survivor of the specification whose interval [C_{a-1}, C_a) meets target +- MARGIN * S."""
    if not (0 <= token < d.keep.size) or not d.keep[token]:
        return False
    ids = np.flatnonzero(d.keep)
    C = np.cumsum(d.q[ids], dtype=np.uint64)
    a = int(np.searchsorted(ids, token))
    lo, hi = (int(C[a - 1]) if a else 0), int(C[a])
    w = d.S // _DEN
    return lo <= d.target + w and hi > d.target - w


def bits_to_mask(words, V: int) -> np.ndarray:
    """keep_bits_out row (uint32 words, bit c & 31 of word c >> 5) -> bool [V]."""
    return np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8), bitorder="little")[:V].astype(bool)
