"""tests/wav_format_spec.py (the contract of the codec's output stage) against what it claims to restate: audioop's G.711 mu-law on every int16
input, the filter geometry and gains written into the issue and the header, scipy's polyphase resampler (a different filter: this catches a
wrong phase or stride, not rounding) and analytic tones."""
import math

import numpy as np
import pytest

import wav_format_spec as spec

FILTERED = [r for r in spec.RATES if r != spec.NATIVE_RATE]


def test_mulaw_equals_audioop_on_every_int16():
    audioop = pytest.importorskip("audioop")
    s = np.arange(-32768, 32768, dtype=np.int16)
    want = np.frombuffer(audioop.lin2ulaw(s.tobytes(), 2), dtype=np.uint8)
    assert np.array_equal(spec.mulaw(s), want)


def test_mulaw_known_values():
    got = spec.mulaw(np.array([0, -1, 4, 1000, -1000, 32767, -32768], dtype=np.int16))
    assert got.tolist() == [0xFF, 0x7E, 0xFE, 0xCE, 0x4E, 0x80, 0x00]


def test_pcm16_rounds_to_even_saturates_and_maps_nan_to_zero():
    x = np.array([0.0, 1.0, -1.0, 1.5, -1.5, 0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -0.5 / 32768, -1.5 / 32768, 1 - 2.0 ** -16,
                  -(1 - 2.0 ** -16), np.nan, np.inf, -np.inf], dtype=np.float32)
    assert spec.pcm16(x).tolist() == [0, 32767, -32768, 32767, -32768, 0, 2, 2, 0, -2, 32767, -32768, 0, 32767, -32768]
    assert spec.pcm16(x).dtype == np.int16


# rate: (orig, new, width, taps) at W = 6
GEOMETRY = {8000: (3, 1, 19, 41), 16000: (3, 2, 10, 23), 22050: (160, 147, 7, 174), 32000: (3, 4, 7, 17), 44100: (80, 147, 7, 94),
            48000: (1, 2, 7, 15)}


@pytest.mark.parametrize("rate", FILTERED)
def test_table_geometry_and_gains(rate):
    orig, new, width, taps, _ = spec.geometry(rate)
    assert (orig, new, width, taps) == GEOMETRY[rate]
    h = spec.table(rate)
    assert h.shape == (new, taps) and h.dtype == np.float64
    l1, dc = np.abs(h).sum(axis=1).max(), h.sum(axis=1)
    print(f"rate {rate}: max sum|h| {l1:.4f}, DC gain {dc.min():.6f} .. {dc.max():.6f}")
    assert 1.52 - 5e-3 <= l1 <= 1.87 + 5e-3                    # the largest sum |h| over one phase: 1.52 .. 1.87 over the six rates
    assert 1.00004 - 1e-5 <= dc.min() and dc.max() <= 1.0009 + 1e-5   # torchaudio's own small non-normalisation, kept
    assert spec.geometry(rate, 0) == spec.geometry(rate, 6)


def test_gains_span_the_documented_range():
    l1 = [np.abs(spec.table(r)).sum(axis=1).max() for r in FILTERED]
    assert abs(min(l1) - 1.52) < 5e-3 and abs(max(l1) - 1.87) < 5e-3, l1


def test_rates_and_width_are_validated():
    for bad in (0, 11025, 24001, 96000):
        with pytest.raises(ValueError):
            spec.ratio(bad)
    for bad in (-1, 65):
        with pytest.raises(ValueError):
            spec.geometry(8000, bad)
    assert spec.geometry(8000, 64)[2] == math.ceil(64 * 3 / 0.99)


@pytest.mark.parametrize("rate", spec.RATES)
@pytest.mark.parametrize("n_in", [0, 1, 2, 3, 159, 160, 161])
def test_length_rule(rate, n_in):
    orig, new = spec.ratio(rate)
    want = math.ceil(n_in * new / orig)
    assert spec.out_len(n_in, rate) == want
    x = np.linspace(-1, 1, n_in)
    assert len(spec.resample(x, rate)) == want


def test_native_rate_is_the_identity():
    x = np.random.default_rng(0).uniform(-1, 1, 100)
    assert np.array_equal(spec.resample(x, 24000), x)


def _lowpassed_noise(n=960, seed=5):
    """White noise limited to a fifth of the native Nyquist frequency (2.4 kHz: inside every output rate's pass band)."""
    rng = np.random.default_rng(seed)
    f = np.fft.rfft(rng.standard_normal(n))
    f[len(f) // 5:] = 0
    x = np.fft.irfft(f, n)
    return x / np.abs(x).max()


@pytest.mark.parametrize("rate", FILTERED)
def test_against_scipy_resample_poly(rate):
    from scipy.signal import resample_poly
    x = _lowpassed_noise()
    orig, new = spec.ratio(rate)
    got, want = spec.resample(x, rate), resample_poly(x, new, orig)
    assert len(got) == len(want)
    d = np.abs(got - want).max()
    print(f"rate {rate}: max |spec - scipy.resample_poly| {d:.2e}")
    assert d < 0.01


@pytest.mark.parametrize("rate", FILTERED)
def test_1khz_tone_matches_the_analytic_tone(rate):
    n = 2400                                                 # 0.1 s
    x = np.sin(2 * np.pi * 1000.0 * np.arange(n) / 24000.0)
    y = spec.resample(x, rate)
    m = np.arange(len(y))
    want = np.sin(2 * np.pi * 1000.0 * m / rate)
    mid = slice(len(y) // 4, 3 * len(y) // 4)
    d = np.abs(y[mid] - want[mid]).max()
    print(f"rate {rate}: 1 kHz tone, max error in the middle half {d:.2e}")
    assert d <= 1e-3


def test_encode_applies_the_encodings_to_one_fp32_stream():
    y = np.random.default_rng(1).uniform(-1.2, 1.2, 500)
    assert spec.encode(y, "f32").dtype == np.float32
    assert np.array_equal(spec.encode(y, "pcm16"), spec.pcm16(y.astype(np.float32)))
    assert np.array_equal(spec.encode(y, "mulaw"), spec.mulaw(spec.pcm16(y.astype(np.float32))))
