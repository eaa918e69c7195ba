"""The codec's output stage in numpy, float64 (TEST INFRASTRUCTURE): the contract of include/neutts_hip.h ntts_wav_format / ntts_codec_decode_fmt /
ntts_codec_convert.  A 24 kHz float32 waveform is resampled to one of RATES, then encoded as float32, PCM16 or G.711 mu-law.

Resampling is the construction torchaudio.functional.resample uses by default (`sinc_interp_hann`, rolloff 0.99, lowpass_filter_width W = 6): a
polyphase FIR of `new` phases x `taps` coefficients.  torchaudio is not a dependency of the tests, so THIS file defines the numbers; equality with
torchaudio is intended, not verified.  tests/test_wav_format_spec.py holds the table to its known constants, to scipy's resample_poly and to analytic
tones, and `mulaw` to audioop.lin2ulaw on all 65 536 inputs.
"""
from __future__ import annotations

import math

import numpy as np

NATIVE_RATE = 24000
RATES = (8000, 16000, 22050, 24000, 32000, 44100, 48000)
ROLLOFF = 0.99
DEFAULT_WIDTH = 6
MAX_WIDTH = 64


def ratio(rate: int):
    """(orig, new): the native and the output rate over their greatest common divisor."""
    if rate not in RATES:
        raise ValueError(f"sample rate {rate!r} is not one of {RATES}")
    g = math.gcd(NATIVE_RATE, rate)
    return NATIVE_RATE // g, rate // g


def geometry(rate: int, W: int = 0):
    """(orig, new, width, taps, base) of the filter; W = 0 means DEFAULT_WIDTH."""
    W = W or DEFAULT_WIDTH
    if not 1 <= W <= MAX_WIDTH:
        raise ValueError(f"filter width {W!r} outside [1, {MAX_WIDTH}]")
    orig, new = ratio(rate)
    base = min(orig, new) * ROLLOFF
    width = int(math.ceil(W * orig / base))
    return orig, new, width, 2 * width + orig, base


def table(rate: int, W: int = 0) -> np.ndarray:
    """h[p][j], float64 [new][taps]: phase p, tap j."""
    W = W or DEFAULT_WIDTH
    orig, new, width, taps, base = geometry(rate, W)
    p = np.arange(new, dtype=np.float64)[:, None]
    j = np.arange(taps, dtype=np.float64)[None, :]
    t = np.clip((-p / new + (j - width) / orig) * base, -W, W)
    window = np.cos(np.pi * t / (2 * W)) ** 2
    return np.sinc(t) * window * (base / orig)          # np.sinc(t) = sin(pi t) / (pi t), 1 at 0


def out_len(n_in: int, rate: int) -> int:
    orig, new = ratio(rate)
    return -(-int(n_in) * new // orig)                  # ceil(n_in * new / orig)


def resample(x, rate: int, W: int = 0, coef_dtype=np.float64) -> np.ndarray:
    """x: one utterance's samples (zero outside itself) -> float64 [out_len].  coef_dtype=np.float32 rounds the table once to fp32, as the
    engine's device table is (the sum itself stays float64)."""
    x = np.asarray(x, dtype=np.float64)
    if rate == NATIVE_RATE:
        return x.copy()
    orig, new, width, taps, _ = geometry(rate, W)
    h = table(rate, W).astype(coef_dtype).astype(np.float64)
    n_out = out_len(len(x), rate)
    nq = -(-n_out // new) if n_out else 0
    xp = np.concatenate([np.zeros(width), x, np.zeros(nq * orig + taps)])
    y = np.empty((nq, new), dtype=np.float64)
    for q in range(nq):
        y[q] = h @ xp[q * orig: q * orig + taps]        # xp[i] = x[i - width]
    return y.reshape(-1)[:n_out]


def error_bound(rate: int, W: int = 0, xmax: float = 1.0) -> float:
    """Per-sample bound of an fp32 dot product of `taps` terms in any order (FMA or not) with coefficients rounded once to fp32, against `resample`
    in float64 with the exact table: (taps + 2) * 2^-24 * max_p sum_j |h[p][j]| * max|x|."""
    if rate == NATIVE_RATE:
        return 0.0
    taps = geometry(rate, W)[3]
    return (taps + 2) * 2.0 ** -24 * float(np.abs(table(rate, W)).sum(axis=1).max()) * xmax


def pcm16(x) -> np.ndarray:
    """clip(rint(float32(x) * 32768), -32768, 32767), ties to even, NaN -> 0."""
    v = np.asarray(x, dtype=np.float32).astype(np.float64) * 32768.0
    v = np.where(np.isnan(v), 0.0, v)
    return np.clip(np.rint(v), -32768, 32767).astype(np.int16)


def mulaw(s) -> np.ndarray:
    """G.711 mu-law bytes of int16 samples, the 14-bit form audioop.lin2ulaw(pcm16, 2) computes."""
    v = np.asarray(s, dtype=np.int16).astype(np.int64) >> 2              # arithmetic shift
    mag = np.minimum(np.abs(v), 8159) + 0x21
    seg = np.frexp(mag.astype(np.float64))[1].astype(np.int64) - 1 - 5   # floor(log2(mag)) - 5, exactly (mag = m * 2^e, m in [0.5, 1))
    code = np.where(seg >= 8, 0x7F, (np.minimum(seg, 7) << 4) | ((mag >> (np.minimum(seg, 7) + 1)) & 15))
    return (code ^ np.where(v >= 0, 0xFF, 0x7F)).astype(np.uint8)


ENCODINGS = {"f32": np.float32, "pcm16": np.int16, "mulaw": np.uint8}


def encode(y, encoding: str) -> np.ndarray:
    """The three encodings of ONE fp32 sample stream."""
    y = np.asarray(y, dtype=np.float32)
    if encoding == "f32":
        return y
    if encoding == "pcm16":
        return pcm16(y)
    if encoding == "mulaw":
        return mulaw(pcm16(y))
    raise ValueError(f"unknown encoding {encoding!r}")
