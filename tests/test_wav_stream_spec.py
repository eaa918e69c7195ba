"""The chunked form of the codec's output stage, tests/wav_stream_spec.py (stream_out_count, resample_chunks: the contract of
ntts_wav_stream_* and ntts_streams_pump_end_fmt) against the one-shot form it restates: a signal cut into chunks gives `resample` of the whole
signal, exactly, for every chunking -- with a history of at most taps - 1 samples (resample_chunks asserts that bound itself)."""
import numpy as np
import pytest

import wav_format_spec as spec
import wav_stream_spec as sspec

N = 700
WIDTHS = (6, 16, 64)
_sig = {}


def signal():
    if "x" not in _sig:
        x = np.random.default_rng(11).uniform(-1.0, 1.0, N)
        x.setflags(write=False)
        _sig["x"] = x
    return _sig["x"]


def cut(x, sizes):
    """x in pieces of `sizes` (the rest, if any, as a final piece)."""
    out, i = [], 0
    for s in sizes:
        out.append(x[i: i + s])
        i += s
    if i < len(x):
        out.append(x[i:])
    return out


def chunkings(rate, W):
    orig, new, width, taps, _ = spec.geometry(rate, W) if rate != spec.NATIVE_RATE else (1, 1, 0, 1, 0)
    rng = np.random.default_rng(rate + W)
    return {
        "whole": [N],
        "one sample per chunk": [1] * N,
        "random, with empty chunks": rng.integers(0, 90, size=24).tolist(),
        "shorter than width": [max(1, width - 1)] * 8,
        "exactly orig": [orig] * 40,
        "a final chunk of nothing": [N, 0],
    }


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("rate", spec.RATES)
def test_resample_chunks_equals_resample_of_the_concatenation(rate, W):
    x = signal()
    want = spec.resample(x, rate, W)
    for name, sizes in chunkings(rate, W).items():
        chunks = cut(x, sizes)
        if sum(len(c) for c in chunks) < N or not chunks:
            continue
        got = sspec.resample_chunks(chunks, rate, W)
        assert len(got) == len(chunks)
        # chunk k holds the outputs [M(N_{k-1}), M(N_k))
        n_in = np.cumsum([len(c) for c in chunks])
        counts = [sspec.stream_out_count(int(n), rate, W, last=(k == len(chunks) - 1)) for k, n in enumerate(n_in)]
        assert [len(g) for g in got] == np.diff([0] + counts).tolist(), name
        assert np.array_equal(np.concatenate(got), want), f"rate {rate} W {W}: {name}"
    # the fp32-rounded table, as the engines hold it
    got32 = np.concatenate(sspec.resample_chunks(cut(x, [37] * 18), rate, W, coef_dtype=np.float32))
    assert np.array_equal(got32, spec.resample(x, rate, W, coef_dtype=np.float32))


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("rate", spec.RATES)
def test_stream_out_count_is_monotone_and_ends_at_out_len(rate, W):
    counts = [sspec.stream_out_count(n, rate, W) for n in range(0, 3000)]
    assert counts[0] == 0 and all(b >= a for a, b in zip(counts, counts[1:]))
    for n in (0, 1, 5, 479, 480, 2999):
        last = sspec.stream_out_count(n, rate, W, last=True)
        assert last == spec.out_len(n, rate) and last >= counts[n]
    if rate == spec.NATIVE_RATE:
        assert counts == list(range(3000))
        return
    orig, new, width, taps, _ = spec.geometry(rate, W)
    # a sample comes out exactly when its last input has arrived, and the output lags the input by at most width + orig input samples
    for n in range(0, 3000, 7):
        m = counts[n]
        assert (m // new) * orig + width + orig > n, "an output whose inputs had all arrived was held back"
        assert m == 0 or (m // new - 1) * orig - width + taps <= n, "an output came out before its last input"
        assert n - m * orig / new <= width + orig
    assert taps - 1 <= 390 and width + orig <= 231          # the largest history and lag of any format: 8 kHz with W = 64
