"""tests/stream_speed_spec.py (the numpy contract of stream_speed=) held to the one-shot rule it must reproduce: a signal pushed chunk by chunk, reading
only the history and the chunk, comes out as time_stretch_spec.stretch of the whole signal -- positions and float64 samples, array_equal -- for every
chunking.  CPU only; the engine is held to this spec in tests/test_emu_stream_speed.py."""
import numpy as np
import pytest

import stream_speed_spec as sspec
import time_stretch_spec as spec

SPEEDS = (500, 501, 667, 800, 999, 1001, 1250, 1500, 1999, 2000)
LENGTHS = (0, 1, 359, 719, 720, 959, 960, 961, 1500, 5000, 12000, 26000)

_sig = {}
_ref = {}


def signal(n):
    """A three-harmonic 137 Hz tone plus seeded noise."""
    if n not in _sig:
        t = np.arange(n, dtype=np.float64) / 24000.0
        tone = 0.4 * np.sin(2 * np.pi * 137 * t) + 0.2 * np.sin(2 * np.pi * 274 * t) + 0.1 * np.sin(2 * np.pi * 411 * t)
        _sig[n] = (tone + 0.05 * np.random.default_rng(n).standard_normal(n)).astype(np.float32)
    return _sig[n]


def one_shot(n, pm):
    if (n, pm) not in _ref:
        _ref[(n, pm)] = spec.stretch(signal(n), pm, through_search=True)
    return _ref[(n, pm)]


def cut(x, kind, seed=0):
    """The signal's chunks; the last one is final."""
    n = len(x)
    if kind == "random":
        rng = np.random.default_rng(seed)
        edges = np.unique(rng.integers(0, n + 1, size=min(12, n + 1))) if n else np.zeros(0, dtype=np.int64)
    else:
        edges = np.arange(int(kind), n, int(kind))
    edges = [0] + [int(e) for e in edges if 0 < e < n] + [n]
    return [x[a:b] for a, b in zip(edges[:-1], edges[1:])]


@pytest.mark.parametrize("pm", SPEEDS)
def test_chunks_are_the_one_shot_stretch_for_every_chunking(pm):
    worst = 0
    for n in LENGTHS:
        x = signal(n)
        ref, ref_pos = one_shot(n, pm)
        for kind in ("random", 480, 12000):
            for flush in (False, True):
                chunks = cut(x, kind, seed=pm + n) + ([x[:0]] if flush else [])
                outs, poss, hist = sspec.stretch_chunks(chunks, pm)
                worst = max(worst, hist)
                assert np.array_equal(np.concatenate(poss), ref_pos), (pm, n, kind, flush)
                assert np.array_equal(np.concatenate(outs), ref), (pm, n, kind, flush)
                total = 0
                for c, o in zip(chunks[:-1], outs[:-1]):
                    total += len(c)
                    assert len(o) % spec.HS == 0 and len(o) <= sspec.chunk_out_max(len(c), pm)
                assert len(outs[-1]) <= sspec.chunk_out_max(len(chunks[-1]), pm)
    print(f"speed {pm}: longest history {worst} samples")
    assert worst <= sspec.HIST_MAX == 1560


@pytest.mark.parametrize("pm", (500, 800, 1250, 2000))
def test_one_sample_per_push(pm):
    n = 1500
    x = signal(n)
    ref, ref_pos = one_shot(n, pm)
    outs, poss, hist = sspec.stretch_chunks([x[i: i + 1] for i in range(n)] + [x[:0]], pm)
    assert np.array_equal(np.concatenate(poss), ref_pos) and np.array_equal(np.concatenate(outs), ref) and hist <= sspec.HIST_MAX


@pytest.mark.parametrize("pm", SPEEDS + (1000,))
def test_out_count_is_monotone_and_ends_at_out_len(pm):
    prev = 0
    for N in range(0, 4000):
        m = sspec.stream_out_count(N, pm)
        assert m >= prev and m <= spec.out_len(N, pm) == sspec.stream_out_count(N, pm, last=True)
        if pm != 1000:      # F(N) against its definition
            k = 0
            while sspec.anchor(k, pm) + sspec.LAG <= N:
                k += 1
            assert m == k * spec.HS
            assert spec.out_len(N, pm) - m <= sspec.chunk_out_max(0, pm)
        else:
            assert m == N
        prev = m
    for bad in (499, 2001):
        with pytest.raises(ValueError, match=str(bad)):
            sspec.stream_out_count(100, bad)


def test_unit_speed_is_the_identity():
    x = signal(5000)
    chunks = cut(x, "random", seed=3) + [x[:0]]
    outs, poss, hist = sspec.stretch_chunks(chunks, 1000)
    assert hist == 0 and all(np.array_equal(o, c.astype(np.float64)) for o, c in zip(outs, chunks))     # chunk by chunk: no lag
    assert np.array_equal(np.concatenate(poss), spec.positions(x, 1000))
    assert sspec.chunk_out_max(12000, 1000) == 12000


def test_a_stream_starts_again_after_its_last_chunk():
    s = sspec.Stream(800)
    x, y = signal(5000), signal(1500)
    a = [s.push(c, last=(i == 2)) for i, c in enumerate((x[:2000], x[2000:4100], x[4100:]))]
    b = [s.push(c, last=(i == 1)) for i, c in enumerate((y[:700], y[700:]))]
    assert np.array_equal(np.concatenate([o for o, _ in a]), one_shot(5000, 800)[0])
    assert np.array_equal(np.concatenate([o for o, _ in b]), one_shot(1500, 800)[0])
