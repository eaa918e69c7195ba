"""tests/loudness_spec.py against the standard's own numbers (CPU only): the 48 kHz design equals ITU-R BS.1770-4's published table, known signals
read what the standard says they read, the warm-start sub-blocks equal the whole-row filter, and the gain rule branch by branch."""
import numpy as np
import pytest

import loudness_spec as spec


def tone(freq, dbfs, seconds, fs=spec.FS):
    t = np.arange(int(round(seconds * fs)), dtype=np.float64) / fs
    return (10.0 ** (dbfs / 20.0) * np.sin(2 * np.pi * freq * t)).astype(np.float32)


def test_48k_design_equals_the_published_table():
    shelf, hp = spec.k_weighting(48000)
    assert np.abs(np.array(shelf) - np.array(spec.PUBLISHED_48K[0])).max() < 1e-12
    assert np.abs(np.array(hp) - np.array(spec.PUBLISHED_48K[1])).max() < 1e-12


def test_full_scale_997hz_sine_at_48k_reads_minus_3_01():
    L = spec.integrated(tone(997.0, 0.0, 3.0, fs=48000), fs=48000)
    print(f"997 Hz full scale at 48 kHz: {L:.4f} LUFS")
    assert abs(L - (-3.01)) <= 0.01


def test_24k_known_signals():
    L = spec.integrated(tone(1000.0, -20.0, 3.0))
    print(f"1 kHz at -20 dBFS: {L:.4f} LUFS")
    assert abs(L - (-22.98)) <= 0.01
    x = np.concatenate([tone(1000.0, -33.0, 1.0), tone(1000.0, -20.0, 6.0), tone(1000.0, -33.0, 1.0)])
    L, gamma, blocks, past_abs, past_rel = spec.gate(spec.subblock_powers(x))
    print(f"-33 / -20 / -33 dBFS: {L:.4f} LUFS, gamma {gamma:.4f}, {blocks} blocks, {past_abs} past the absolute gate, {past_rel} past both")
    assert abs(L - (-23.18)) <= 0.01
    assert blocks == 77 and past_abs == 77 and blocks - past_rel == 14
    # a second of digital silence between two tones: dropped by the absolute gate, so the reading is the tones' (to what the partly silent blocks add)
    y = np.concatenate([tone(1000.0, -20.0, 2.0), np.zeros(spec.FS, dtype=np.float32), tone(1000.0, -20.0, 2.0)])
    Ly, _, blocks, past_abs, _ = spec.gate(spec.subblock_powers(y))
    P, l = spec.block_loudness(spec.subblock_powers(y))
    silent = l <= spec.ABS_GATE
    assert silent.sum() >= 6 and past_abs == blocks - silent.sum()
    assert abs(Ly - spec.integrated(tone(1000.0, -20.0, 3.0))) < 0.5


def test_warm_start_equals_the_whole_row_filter():
    rng = np.random.default_rng(5)
    n = 2 * spec.FS + 777                                  # speech-like: a modulated tone over a noise floor, a trailing partial sub-block
    t = np.arange(n) / spec.FS
    x = (0.3 * np.sin(2 * np.pi * 180 * t) * (0.6 + 0.4 * np.sin(2 * np.pi * 3 * t)) + 0.01 * rng.standard_normal(n)).astype(np.float32)
    za, zb = spec.subblock_powers(x), spec.subblock_powers_whole(x)
    assert len(za) == len(zb) == n // spec.S
    La, Lb = spec.gate(za)[0], spec.gate(zb)[0]
    print(f"warm start {La:.12f}, whole row {Lb:.12f}, difference {abs(La - Lb):.3e} LU")
    assert abs(La - Lb) <= 1e-9
    assert spec.integrated(x, whole=True) == Lb


def test_rows_without_a_measurable_block():
    for n in (0, 1, 9599):
        assert np.isnan(spec.integrated(tone(440.0, -20.0, 1.0)[:n]))
    assert len(spec.block_loudness(spec.subblock_powers(tone(440.0, -20.0, 1.0)[:9600]))[0]) == 1
    assert len(spec.block_loudness(spec.subblock_powers(tone(440.0, -20.0, 1.0)[:11999]))[0]) == 1
    assert len(spec.block_loudness(spec.subblock_powers(tone(440.0, -20.0, 1.0)[:12000]))[0]) == 2
    assert np.isnan(spec.integrated(np.zeros(24000, dtype=np.float32)))              # nothing past the absolute gate
    bad = tone(440.0, -20.0, 1.0).copy()
    bad[100] = np.nan
    assert np.isnan(spec.integrated(bad)) and spec.peak(bad) == np.inf
    assert spec.gate_margin(tone(440.0, -20.0, 0.3)) == np.inf


def test_gain_rule_branch_by_branch():
    # the target binds
    g = spec.gain(-30.0, 0.05, -16.0)
    assert g == np.float32(10.0 ** (14.0 / 20.0))
    # the peak ceiling binds: 14 dB would lift a peak of 0.5 to 2.5
    g = spec.gain(-30.0, 0.5, -16.0)
    assert g == np.float32(10.0 ** (-1.0 / 20.0) / 0.5)
    assert spec.gain(-30.0, 0.5, -16.0, peak_dbfs=-6.0) == np.float32(10.0 ** (-6.0 / 20.0) / 0.5)
    # the maximum gain binds: 34 dB asked for, 20 allowed
    assert spec.gain(-50.0, 0.001, -16.0) == np.float32(10.0)
    assert spec.gain(-50.0, 0.001, -16.0, max_gain_db=30.0) == np.float32(10.0 ** 1.5)
    # attenuation is held by nothing
    assert spec.gain(-10.0, 0.9, -23.0) == np.float32(10.0 ** (-13.0 / 20.0))
    # a silent row has no peak term; an unmeasurable row has gain 1
    assert spec.gain(-30.0, 0.0, -16.0) == np.float32(10.0 ** (14.0 / 20.0))
    assert spec.gain(float("nan"), 0.5, -16.0) == np.float32(1.0)
    x = tone(1000.0, -20.0, 0.3)
    out, L, pk, g = spec.normalize(x, -16.0)
    assert np.isnan(L) and g == 1.0 and np.array_equal(out, x)
    out, L, pk, g = spec.normalize(tone(1000.0, -20.0, 1.0), None)
    assert g == 1.0 and np.array_equal(out, tone(1000.0, -20.0, 1.0))
    out, L, pk, g = spec.normalize(tone(1000.0, -20.0, 1.0), -16.0)
    assert abs(spec.integrated(out) - (-16.0)) < 1e-5 and out.dtype == np.float32
