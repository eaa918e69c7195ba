"""tests/time_stretch_spec.py (the numpy contract of speed=) held to its own rules and to what a time stretch must do to a voiced signal: keep the
level, add no clicks, keep the pitch.  These three are conditions on the SPEC, checked here on the CPU; they are not tolerances on the kernel (the
kernel is held to the spec: positions exactly, samples within 4 * 2^-24 * max|x|; tests/test_emu_time_stretch.py)."""
import numpy as np
import pytest

import time_stretch_spec as spec

TONE_SPEEDS = (500, 750, 900, 1100, 1250, 1500, 2000)

_ref = {}


def tone(n=12000):
    t = np.arange(n, dtype=np.float64) / 24000.0
    return (0.4 * np.sin(2 * np.pi * 137 * t) + 0.2 * np.sin(2 * np.pi * 274 * t) + 0.1 * np.sin(2 * np.pi * 411 * t)).astype(np.float32)


def stretched_tone(pm):
    if pm not in _ref:
        _ref[pm] = spec.stretch(tone(), pm)
    return _ref[pm]


def test_length_rule_and_frame_count():
    assert spec.L == 720 and spec.HS == 360 and spec.DELTA == 240
    for n_in, pm, n_out in ((0, 800, 0), (1, 500, 2), (1, 2000, 1), (1001, 800, 1252), (1001, 2000, 501), (720, 1000, 720), (12000, 730, 16439),
                            (12000, 1370, 8760)):
        assert spec.out_len(n_in, pm) == n_out == -(-n_in * 1000 // pm)
    assert [spec.n_frames(v) for v in (0, 1, 360, 361, 720, 16439)] == [0, 1, 1, 2, 2, 46]
    assert spec.permille(0.8) == 800 and spec.permille(1.0004) == 1000 and spec.permille(0.7295) in (729, 730)
    for bad in (499, 2001, 0):
        with pytest.raises(ValueError, match=str(bad)):
            spec.out_len(100, bad)
    f = spec.fade()
    assert f.dtype == np.float32 and len(f) == spec.HS and (np.diff(f) > 0).all() and 0 < f[0] < 1e-4 and 1 - 1e-4 < f[-1] < 1
    assert np.allclose(f.astype(np.float64) + f[::-1].astype(np.float64), 1.0, atol=2.0 ** -23)      # the two halves of a frame's cross-fade sum to 1


@pytest.mark.parametrize("kind", ["tone", "noise", "silence"])
def test_unit_speed_through_the_search_continues_naturally(kind):
    """pm = 1000 forced through the search: a_k = t_k = k * HS and D(t_k) = 0 with |c - t_k| = 0, so p_k = k * HS for every frame whose natural
    position the clamp to pmax = n_in - L leaves alone, and there the output is the input.  (Behind pmax the rule compresses the last 30 ms, as
    stated in the contract; the engine copies rows at 1000 and never gets there.)"""
    n = 5000
    x = {"tone": tone(n), "noise": np.random.default_rng(1).uniform(-1, 1, n).astype(np.float32), "silence": np.zeros(n, np.float32)}[kind]
    out, pos = spec.stretch(x, 1000, through_search=True)
    free = np.arange(len(pos)) * spec.HS <= n - spec.L
    assert free.sum() == 12 and np.array_equal(pos[free], (np.arange(len(pos)) * spec.HS)[free])
    assert (pos[~free] <= n - spec.L).all()
    m = int(free.sum()) * spec.HS
    assert np.array_equal(out[:m], x[:m].astype(np.float64))
    copied, cpos = spec.stretch(x, 1000)
    assert np.array_equal(copied, x.astype(np.float64)) and np.array_equal(cpos, np.arange(len(pos)) * spec.HS)


@pytest.mark.parametrize("pm", TONE_SPEEDS)
def test_continuation_spans_are_the_input_exactly(pm):
    x = tone()
    out, pos = stretched_tone(pm)
    assert len(out) == spec.out_len(len(x), pm) and len(pos) == spec.n_frames(len(out))
    assert pos[0] == 0 and (pos >= 0).all() and (pos <= len(x) - spec.L).all()
    keep = spec.continuation_mask(pos, len(out))
    src = spec.source_index(pos, len(out))
    assert keep[: spec.HS].all() and src.max() < len(x)
    assert np.array_equal(out[keep], x.astype(np.float64)[src[keep]])
    # a tie in D goes to the candidate nearest the continuation, then to the lower one: silence continues wherever it may
    zpos = spec.positions(np.zeros(len(x), np.float32), pm)
    for k in range(1, len(zpos)):
        t, a = int(zpos[k - 1]) + spec.HS, (k * spec.HS * pm + 500) // 1000
        lo, hi = (min(max(v, 0), len(x) - spec.L) for v in (a - spec.DELTA, a + spec.DELTA))
        assert zpos[k] == min(max(t, lo), hi)


@pytest.mark.parametrize("pm", TONE_SPEEDS)
def test_tone_keeps_its_level_its_smoothness_and_its_pitch(pm):
    x = tone().astype(np.float64)
    out, _ = stretched_tone(pm)
    rms = np.sqrt(np.mean(out ** 2)) / np.sqrt(np.mean(x ** 2))
    step = np.abs(np.diff(out)).max() / np.abs(np.diff(x)).max()
    spec_out = np.abs(np.fft.rfft(out * np.hanning(len(out))))
    peak_hz = np.argmax(spec_out) * 24000.0 / len(out)
    bin_hz = 24000.0 / len(out)
    print(f"speed {pm}: rms ratio {rms:.4f}, largest step ratio {step:.4f}, peak {peak_hz:.1f} Hz (bin {bin_hz:.2f} Hz)")
    assert 0.98 <= rms <= 1.02                      # output rms over input rms within +-2 %
    assert step <= 1.05                             # largest sample-to-sample step at most 1.05 x the input's: no clicks
    assert abs(peak_hz - 137.0) <= bin_hz           # spectral peak within one FFT bin of the fundamental
