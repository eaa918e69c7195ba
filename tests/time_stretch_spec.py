"""The codec's time-stretch stage in numpy (TEST INFRASTRUCTURE): the contract of include/neutts_hip.h ntts_wav_stretch_len / ntts_codec_stretch /
ntts_codec_decode_speed.  A 24 kHz float32 waveform is made `speed` times faster (speed > 1) or slower (speed < 1) without moving its pitch: WSOLA,
waveform-similarity overlap-add, stated so that the choice of every segment is a function of the row and the speed alone -- integer arithmetic on the
PCM16 rounding of the signal, no order of additions -- and the engine's positions can be held to these with array_equal.

Speed is an integer per mille, pm in [PM_MIN, PM_MAX] (the Python layer: round(speed * 1000)).
  n_out = ceil(n_in * 1000 / pm), K = ceil(n_out / HS) output frames of HS samples.
  pm = 1000: the row is copied (positions k * HS, by definition: out[k * HS + i] = x[k * HS + i]).
  s = pcm16(x) is the search signal; x and s read as zero outside [0, n_in).  pmax = max(0, n_in - L).
  Frame 0: p_0 = 0, out[0 .. HS) = x[0 .. HS).
  Frame k >= 1: t_k = p_{k-1} + HS (the natural continuation), a_k = (k * HS * pm + 500) // 1000 (where the speed wants to be),
    candidates c in [clamp(a_k - DELTA), clamp(a_k + DELTA)], clamp to [0, pmax], D(c) = sum_{i < HS} |s[t_k + i] - s[c + i]| (<= 360 * 65535: int32),
    p_k = the c that minimises the tuple (D, |c - t_k|, c);
    out[k * HS + i] = fma(f[i], x[p_k + i] - x[t_k + i], x[t_k + i]) in fp32, f[i] = 0.5 - 0.5 cos(pi (i + 0.5) / HS) built in double, rounded once.
  Where p_k == t_k the output is the input bit for bit.
Up to the last L samples (30 ms) of an utterance may be compressed or dropped (pmax keeps a whole window inside the signal: with n_in - HS the end
of a slowed signal clicks); rows shorter than L come out as the rule says and mean nothing.
"""
from __future__ import annotations

import numpy as np

from wav_format_spec import pcm16

L = 720          # 30 ms: the window a position must leave inside the signal
HS = 360         # output frame (synthesis hop)
DELTA = 240      # +-10 ms of search: one pitch period down to 50 Hz
PM_MIN, PM_MAX = 500, 2000


def permille(speed) -> int:
    return int(round(float(speed) * 1000))


def out_len(n_in: int, pm: int) -> int:
    if not PM_MIN <= pm <= PM_MAX:
        raise ValueError(f"speed {pm} per mille outside [{PM_MIN}, {PM_MAX}]")
    return -(-int(n_in) * 1000 // int(pm))


def n_frames(n_out: int) -> int:
    return -(-int(n_out) // HS)


def fade() -> np.ndarray:
    """f[i], fp32 [HS]: built in double, rounded once."""
    i = np.arange(HS, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(np.pi * (i + 0.5) / HS)).astype(np.float32)


def _padded(v, lo, n):
    """v[lo .. lo + n) with zeros outside the array (lo >= 0)."""
    out = np.zeros(n, dtype=v.dtype)
    hi = min(len(v), lo + n)
    if hi > lo:
        out[: hi - lo] = v[lo:hi]
    return out


def positions(x, pm: int, through_search: bool = False) -> np.ndarray:
    """p_0 .. p_{K-1}, int32.  pm = 1000 copies (positions k * HS) unless through_search forces the rule itself."""
    x = np.asarray(x, dtype=np.float32)
    n_in = len(x)
    K = n_frames(out_len(n_in, pm))
    if pm == 1000 and not through_search:
        return (np.arange(K, dtype=np.int64) * HS).astype(np.int32)
    s = pcm16(x).astype(np.int64)
    pmax = max(0, n_in - L)
    pos = np.zeros(K, dtype=np.int64)
    for k in range(1, K):
        t = int(pos[k - 1]) + HS
        a = (k * HS * pm + 500) // 1000
        c_lo, c_hi = min(max(a - DELTA, 0), pmax), min(max(a + DELTA, 0), pmax)
        ref = _padded(s, t, HS)
        win = _padded(s, c_lo, c_hi - c_lo + HS)
        cand = np.arange(c_lo, c_hi + 1)
        D = np.abs(np.lib.stride_tricks.sliding_window_view(win, HS) - ref[None, :]).sum(axis=1)
        order = np.lexsort((cand, np.abs(cand - t), D))        # last key first: D, then |c - t|, then c
        pos[k] = cand[order[0]]
    return pos.astype(np.int32)


def stretch(x, pm: int, through_search: bool = False):
    """-> (out float64 [n_out]: the exact value of x[t] + f32(f[i]) * (x[p] - x[t]) on the fp32 samples, positions int32 [K])."""
    x = np.asarray(x, dtype=np.float32)
    n_out = out_len(len(x), pm)
    pos = positions(x, pm, through_search)
    if pm == 1000 and not through_search:
        return x.astype(np.float64), pos
    xd = x.astype(np.float64)
    f = fade().astype(np.float64)
    out = np.zeros(len(pos) * HS, dtype=np.float64)
    for k, p in enumerate(pos):
        t = 0 if k == 0 else int(pos[k - 1]) + HS
        xt, xp = _padded(xd, t, HS), _padded(xd, int(p), HS)
        out[k * HS: (k + 1) * HS] = xt + f * (xp - xt)
    return out[:n_out], pos


def continuation_mask(pos, n_out: int) -> np.ndarray:
    """bool [n_out]: output samples of frames with p_k == t_k (frame 0 included), where the output is an input sample bit for bit."""
    m = np.zeros(len(pos) * HS, dtype=bool)
    for k, p in enumerate(pos):
        if k == 0 or int(p) == int(pos[k - 1]) + HS:
            m[k * HS: (k + 1) * HS] = True
    return m[:n_out]


def source_index(pos, n_out: int) -> np.ndarray:
    """int64 [n_out]: t_k + i of every output sample (the input sample a continuation frame copies)."""
    idx = np.zeros(len(pos) * HS, dtype=np.int64)
    for k in range(len(pos)):
        t = 0 if k == 0 else int(pos[k - 1]) + HS
        idx[k * HS: (k + 1) * HS] = t + np.arange(HS)
    return idx[:n_out]


def error_bound(xmax: float) -> float:
    """An fp32 output against `stretch`: one subtraction, one fp32 fade coefficient (already in the spec's value) and one fma: 4 * 2^-24 * max|x|."""
    return 4 * 2.0 ** -24 * float(xmax)
