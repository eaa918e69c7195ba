"""loudness=: the codec's BS.1770 loudness normalisation (include/neutts_hip.h ntts_codec_normalize / ntts_codec_measure_loudness /
ntts_codec_decode_loud; kernels/codec.h wav_loud_measure_kernel / wav_loud_gate_kernel / wav_loud_apply_kernel) on the CPU SIMT emulator against
tests/loudness_spec.py, through the stage alone, the decode entry points and the NeuTTS class.  tests/test_gpu_loudness.py runs the same bodies on
libneutts_hip.so.

Every comparison of a device loudness or gain with the spec first asserts gate_margin >= 1e-3 LU for its input: the spec alone decides every gate,
so the bound of 1e-6 LU on L (fp64 round-off through poles at radius 0.99 is about 1e-11 LU) is a bound on arithmetic, not on a gating decision."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from oracle import codec_ref as cr
from neutts import _hip
from common import load_codec_fixture, make_codec_engine
import test_emu_neutts_class as class_cases
import loudness_spec as spec
import wav_format_spec as fspec

EINVAL, ESTATE = -1, -4
FS, S = spec.FS, spec.S
MAX_FRAMES = 6700                                       # hop 24: up to 160 800 samples per utterance -- 67 sub-blocks, more than one wave / workgroup of 64
MAX_ROWS = 4 * MAX_FRAMES                               # a workspace of 643 200 samples
L_TOL = 1e-6
MARGIN = 1e-3

_ref = {}


def tone(freq, dbfs, n):
    t = np.arange(n, dtype=np.float64) / FS
    return (10.0 ** (dbfs / 20.0) * np.sin(2 * np.pi * freq * t)).astype(np.float32)


def noise(dbfs, n, seed):
    return (10.0 ** (dbfs / 20.0) * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def bursts(n):
    """Tone bursts with pauses of digital silence and of a noise floor at -65 dBFS: both gates have something to drop."""
    x = np.concatenate([tone(300.0, -12.0, 21000), np.zeros(13000, dtype=np.float32), tone(1200.0, -30.0, 24000), noise(-65.0, 15000, 1),
                        tone(500.0, -18.0, 12000), np.zeros(9000, dtype=np.float32)])
    return np.tile(x, -(-n // len(x)))[:n].copy()


def rows():
    """The rows of the stage tests: (name, waveform, target or None).  Lengths 9599 / 9600 / 11999 / 12000 give no block, one, one (the partial
    sub-block is ignored) and two; `long` crosses the measure kernel's partition of 64 sub-blocks per workgroup."""
    if "rows" not in _ref:
        r = [("n9599", tone(440.0, -20.0, 9599), -16.0), ("n9600", tone(440.0, -20.0, 9600), -16.0), ("n11999", tone(440.0, -20.0, 11999), -16.0),
             ("n12000", tone(440.0, -20.0, 12000), -16.0),
             ("bursts", bursts(94000), -16.0),                      # the target binds
             ("loud", bursts(50011) * np.float32(5.0), -30.0),      # attenuated; samples above full scale
             ("peaky", np.concatenate([tone(440.0, -40.0, 30000), np.full(3, 0.9, dtype=np.float32), tone(440.0, -40.0, 7000)]), -16.0),    # the ceiling binds
             ("floor", noise(-62.0, 40000, 2), -16.0),              # a noise floor above the absolute gate: the maximum gain binds
             ("silent", noise(-90.0, 30000, 3), -16.0),             # under the absolute gate: unmeasurable
             ("off", bursts(33333), None),                          # the option off in a mixed batch
             ("tail", np.concatenate([tone(440.0, -30.0, 12000), np.full(7, 0.5, dtype=np.float32)]), -16.0),       # the peak lies in the unmeasured tail
             ("long", (bursts(160100) * (0.5 + 0.4 * np.sin(2 * np.pi * np.arange(160100) / 70000.0))).astype(np.float32), -20.0),
             ("empty", np.zeros(0, dtype=np.float32), -16.0)]
        for _, x, _ in r:
            x.setflags(write=False)
        _ref["rows"] = r
    return _ref["rows"]


def reference(key, wavs):
    """The spec's (L, peak, gate margin) of every waveform, all sub-blocks filtered side by side; computed once per key."""
    if key not in _ref:
        zs = spec.subblock_powers_many(wavs)
        _ref[key] = [(spec.gate(z)[0] if np.isfinite(w).all() else float("nan"), spec.peak(w), spec.gate_margin_z(z)) for w, z in zip(wavs, zs)]
    return _ref[key]


def engine_result(eng):
    """normalize() of rows() with the figures, once per engine."""
    if not hasattr(eng, "_loud_result"):
        r = rows()
        eng._loud_result = eng.normalize([x for _, x, _ in r], [t for _, _, t in r], return_measured=True)
    return eng._loud_result


DECODE_HOP = 120                                        # the codec passes of these tests: codec_tiny with this hop, so that 80 frames hold a gating block


def make_engine(lib, on_gpu, max_frames=MAX_FRAMES, max_rows=MAX_ROWS, hop=None):
    """The test engine: codec_tiny (hop 24) for the stage on waveforms; with `hop`, the same model at another hop for the tests that run the codec
    pass itself -- the stage reads frames x hop samples either way, and 100 frames decode in a moment where 500 do not."""
    z, cfg, w = load_codec_fixture("codec_tiny")
    if hop is not None:
        cfg = dataclasses.replace(cfg, hop_length=hop)
        w = cr.make_weights(cfg, int(z["seed"]))
    e = make_codec_engine(cfg, w, lib, max_frames=max_frames, max_rows=max_rows)
    e._fixture, e._on_gpu, e._lib_path = z, on_gpu, lib
    return e


def build_class(lib, **kw):
    """The class-level fixture: the tiny codec with a hop of 240, so that the 45 frames of a test utterance are long enough to hold a gating block."""
    return class_cases.build_tts(lib, ccfg=dataclasses.replace(cr.CodecConfig.tiny(), hop_length=240), **kw)


@pytest.fixture(scope="module")
def eng(emu_lib):
    return make_engine(emu_lib, False)


@pytest.fixture(scope="module")
def deng(emu_lib):
    return make_engine(emu_lib, False, max_frames=256, max_rows=1024, hop=DECODE_HOP)


@pytest.fixture(scope="module")
def tts(emu_lib):
    return build_class(emu_lib)


def assert_row(name, x, target, got, m, L, pk, margin, **gain_kw):
    """One row of the engine (waveform `got`, figures m = (L, peak, g)) against the spec's L / peak of x."""
    assert got.dtype == np.float32 and len(got) == len(x)
    assert m[1] == pk, f"{name}: peak {m[1]!r} != {pk!r}"
    if np.isnan(L) or target is None:
        assert np.isnan(m[0]) == bool(np.isnan(L)) and m[2] == 1.0
        assert np.array_equal(got, x), f"{name}: a row with gain 1 is not the input"
        if np.isnan(L):
            return
    assert margin >= MARGIN, f"{name}: gate margin {margin:.2e} LU: the input does not leave the gates to the spec"
    assert abs(m[0] - L) <= L_TOL, f"{name}: L {m[0]:.9f} vs {L:.9f}"
    if target is None:
        return
    g = spec.gain(L, pk, target, **gain_kw)
    assert abs(np.float32(m[2]) - g) <= np.spacing(g), f"{name}: g {m[2]!r} vs {g!r}"
    assert np.float32(m[2]) == m[2]                                     # (a float32 value)
    want = (x * g).astype(np.float32)
    assert (np.abs(got.astype(np.float64) - want) <= spec.sample_bound(want)).all(), f"{name}: samples"


# ---------------------------------------------------------------------------------------------- a. the stage against the spec
def test_measure_loudness_equals_the_spec(eng):
    r = rows()
    ref = reference("rows_ref", [x for _, x, _ in r])
    got = eng.measure_loudness([x for _, x, _ in r])
    assert got.shape == (len(r), 3) and got.dtype == np.float64
    blocks = {name: max(0, len(x) // S - 3) for name, x, _ in r}
    assert [blocks[k] for k in ("n9599", "n9600", "n11999", "n12000")] == [0, 1, 1, 2]
    assert len(r[[n for n, _, _ in r].index("long")][1]) // S == 66       # more sub-blocks than one workgroup of the measure kernel takes
    worst = 0.0
    for (name, x, _), (L, pk, margin), m in zip(r, ref, got):
        assert m[1] == pk and m[2] == 1.0, name
        if np.isnan(L):
            assert np.isnan(m[0]), name
            continue
        assert margin >= MARGIN, f"{name}: gate margin {margin:.2e}"
        worst = max(worst, abs(m[0] - L))
        assert abs(m[0] - L) <= L_TOL, f"{name}: L {m[0]:.9f} vs {L:.9f}"
    assert [name for (name, _, _), (L, _, _) in zip(r, ref) if np.isnan(L)] == ["n9599", "silent", "empty"]
    print(f"max |engine - spec| of L over the rows: {worst:.3e} LU")


def test_normalize_equals_the_spec_row_by_row(eng):
    r = rows()
    ref = reference("rows_ref", [x for _, x, _ in r])
    out, measured = engine_result(eng)
    bound = {}
    for (name, x, target), (L, pk, margin), got, m in zip(r, ref, out, measured):
        assert_row(name, x, target, got, m, L, pk, margin)
        if target is not None and not np.isnan(L):
            g = float(m[2])
            bound[name] = ("target" if abs(20 * np.log10(g) - (target - L)) < 1e-4 else "max_gain" if abs(g - 10.0) < 1e-5 else "peak")
    assert bound["bursts"] == "target" and bound["loud"] == "target" and bound["long"] == "target"
    assert bound["peaky"] == "peak" and bound["tail"] == "peak" and bound["floor"] == "max_gain"
    assert float(np.abs(out[[n for n, _, _ in r].index("peaky")]).max()) <= 10.0 ** (-1.0 / 20.0) * (1 + 2.0 ** -22)
    assert measured[[n for n, _, _ in r].index("loud"), 2] < 1.0


def test_rows_with_the_option_off_and_unmeasurable_rows_are_the_input(eng):
    r = rows()
    out, measured = engine_result(eng)
    for name in ("n9599", "silent", "off", "empty"):
        i = [n for n, _, _ in r].index(name)
        assert measured[i, 2] == 1.0 and np.array_equal(out[i], r[i][1]), name
    bad = tone(440.0, -20.0, 24000).copy()
    bad[12345] = np.nan
    inf = tone(440.0, -20.0, 24000).copy()
    inf[23999] = -np.inf
    got, m = eng.normalize([bad, inf, r[4][1]], -16.0, return_measured=True)
    assert np.isnan(m[0, 0]) and m[0, 1] == np.inf and m[0, 2] == 1.0 and np.array_equal(got[0], bad, equal_nan=True)
    assert np.isnan(m[1, 0]) and m[1, 1] == np.inf and m[1, 2] == 1.0 and np.array_equal(got[1], inf)
    assert m[2, 2] != 1.0                                              # (the row next to them is normalised)
    # the option off for every row: the waveforms as they are, in any format as convert gives them; the figures are still there for whoever asks
    wavs = [r[4][1], r[9][1]]
    same, m = eng.normalize(wavs, None, return_measured=True)
    assert all(np.array_equal(a, b) for a, b in zip(same, wavs)) and (m[:, 2] == 1.0).all() and np.isfinite(m[:, 0]).all()
    mu = eng.normalize(wavs, [None, None], sample_rate=8000, encoding="mulaw")
    assert all(np.array_equal(a, b) for a, b in zip(mu, eng.convert(wavs, sample_rate=8000, encoding="mulaw")))
    assert eng.normalize([], -16.0) == [] and eng.measure_loudness([]).shape == (0, 3)


def test_parameters_per_call(eng):
    r = rows()
    ref = reference("rows_ref", [x for _, x, _ in r])
    names = [n for n, _, _ in r]
    for name, kw in (("peaky", dict(loudness_peak=-6.0)), ("floor", dict(loudness_max_gain=35.0)), ("floor", dict(loudness_max_gain=0.0))):
        i = names.index(name)
        got, m = eng.normalize([r[i][1]], -16.0, return_measured=True, **kw)
        L, pk, margin = ref[i]
        assert_row(name, r[i][1], -16.0, got[0], m[0], L, pk, margin, **{dict(loudness_peak="peak_dbfs", loudness_max_gain="max_gain_db")[k]: v
                                                                         for k, v in kw.items()})
    assert m[0, 2] == 1.0                                               # max gain 0 dB on a quiet row: nothing is lifted


def test_normalize_with_a_format_equals_convert_of_the_normalized_f32(eng):
    r = rows()
    out, _ = engine_result(eng)
    pick = [i for i, (name, _, _) in enumerate(r) if name in ("n12000", "bursts", "loud", "off", "silent")]
    wavs, targets = [r[i][1] for i in pick], [r[i][2] for i in pick]
    for rate, enc in ((24000, "pcm16"), (8000, "mulaw"), (16000, "f32")):
        got = eng.normalize(wavs, targets, sample_rate=rate, encoding=enc)
        want = eng.convert([out[i] for i in pick], sample_rate=rate, encoding=enc)
        for g, w, x in zip(got, want, wavs):
            assert g.dtype == fspec.ENCODINGS[enc] and len(g) == fspec.out_len(len(x), rate) and np.array_equal(g, w)


def test_normalize_splits_batches_larger_than_the_workspace(eng):
    """More rows than the waveform workspace holds at once (643 200 samples): two rounds, the same samples and figures as row by row."""
    wavs = [bursts(70000 - 997 * i) * np.float32(0.3 + 0.1 * i) for i in range(12)]     # 12 x ~65 000 > 643 200: nine rows per round
    targets = [-16.0, -23.0, None] * 4
    ref = reference("split", wavs)
    got, m = eng.normalize(wavs, targets, return_measured=True)
    for i, (x, t, (L, pk, margin)) in enumerate(zip(wavs, targets, ref)):
        assert_row(f"row {i}", x, t, got[i], m[i], L, pk, margin)
    for i in (0, 8, 9, 11):                                            # rows of both rounds against a call of their own
        one, m1 = eng.normalize([wavs[i]], targets[i], return_measured=True)
        assert np.array_equal(one[0], got[i]) and np.array_equal(m1[0], m[i], equal_nan=True)
    assert np.array_equal(eng.measure_loudness(wavs)[:, :2], m[:, :2])


# ---------------------------------------------------------------------------------------------- b. behind the codec pass
def _codes():
    rng = np.random.default_rng(3)
    return [rng.integers(0, 4 ** 4, size=t).tolist() for t in (90, 20, 104)]          # 10 800, 2 400 (no block) and 12 480 samples


CODE_SPEEDS = [0.8, 2.0, 1.0]
CODE_TARGETS = [-16.0, -16.0, -30.0]


def test_decode_with_loudness_equals_the_stages_one_by_one(deng):
    eng = deng
    codes = _codes()
    plain = [p.copy() for p in eng.decode(codes)]
    stretched = eng.stretch(plain, CODE_SPEEDS)
    normal, m = eng.normalize(stretched, CODE_TARGETS, return_measured=True)
    assert np.isfinite(m[[0, 2], 0]).all() and np.isnan(m[1, 0]) and (m[[0, 2], 2] != 1.0).all()
    assert np.array_equal(normal[1], stretched[1])
    for kw in (dict(), dict(sample_rate=24000, encoding="pcm16"), dict(sample_rate=8000, encoding="mulaw")):
        got = eng.decode(codes, speed=CODE_SPEEDS, loudness=CODE_TARGETS, **kw)
        want = eng.convert(normal, **kw)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and np.array_equal(g, w)
    # without a speed; a row with the option off; the two further knobs
    got = eng.decode(codes, loudness=[-20.0, -20.0, None], loudness_peak=-3.0, loudness_max_gain=6.0)
    want = eng.normalize(plain, [-20.0, -20.0, None], loudness_peak=-3.0, loudness_max_gain=6.0)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    assert np.array_equal(got[1], plain[1]) and np.array_equal(got[2], plain[2]) and not np.array_equal(got[0], plain[0])


def test_decode_device_with_loudness_equals_decode(deng):
    """ntts_codec_decode_dev_loud: codes on the device, stretched, normalised (and formatted) waveforms into the engine's pinned buffer."""
    eng = deng
    rng = np.random.default_rng(4)
    lens = np.array([120, 86], dtype=np.int32)
    arr = rng.integers(0, 4 ** 4, size=(2, 120)).astype(np.int32)
    codes = [arr[0, :120].tolist(), arr[1, :86].tolist()]
    if eng._on_gpu:
        import torch
        keep = torch.tensor(arr, device="cuda")
        ptr = keep.data_ptr()
        torch.cuda.synchronize()
    else:
        keep, ptr = arr, arr.ctypes.data                # (the emulator's device memory is host memory)
    for kw in (dict(loudness=[-16.0, -25.0]), dict(loudness=[None, -16.0], speed=[0.75, 1.0], sample_rate=16000, encoding="pcm16")):
        want = [w.copy() for w in eng.decode(codes, **kw)]
        wav = eng.decode_device(ptr, 120, lens, **kw)
        eng.sync()
        assert wav.shape == (2, max(len(w) for w in want)) and wav.dtype == want[0].dtype
        for r, w in enumerate(want):
            assert np.array_equal(wav[r, : len(w)], w)
    del keep


def _i32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def test_option_off_in_every_spelling_is_ntts_codec_decode_speed(eng):
    fresh = make_engine(eng._lib_path, eng._on_gpu, max_frames=128, max_rows=512, hop=DECODE_HOP)      # an engine on which no loudness stage has run
    codes = _codes()[1:]
    speeds = np.array([800, 1000], dtype=np.int32)
    lens = np.array([len(c) for c in codes], dtype=np.int32)
    flat = np.ascontiguousarray(np.concatenate([np.asarray(c, dtype=np.int32) for c in codes]))
    stride = DECODE_HOP * 104

    def call(fn, *extra):
        out = np.zeros((2, stride), dtype=np.float32)
        out_lens = np.zeros(2, dtype=np.int32)
        rc = fn(fresh.h, 2, _i32p(flat), _i32p(lens), _i32p(speeds), *extra, None, C.c_void_p(out.ctypes.data), stride, _i32p(out_lens))
        assert rc == 0, (fresh.lib.ntts_codec_last_error(fresh.h) or b"").decode()
        return out, out_lens

    want, want_lens = call(fresh.lib.ntts_codec_decode_speed)
    off = (_hip.WavLoudnessC * 2)(_hip.WavLoudnessC(0, -16.0, -1.0, 20.0), _hip.WavLoudnessC(0, float("nan"), 99.0, -5.0))     # (not looked at)
    for loud in (None, off):
        got, got_lens = call(fresh.lib.ntts_codec_decode_loud, loud)
        assert got_lens.tolist() == want_lens.tolist() and np.array_equal(got, want)
    plain = [p.copy() for p in fresh.decode(codes)]
    for spelling in (None, [None, None]):
        assert all(np.array_equal(a, b) for a, b in zip(fresh.decode(codes, loudness=spelling), plain))
    a, b = C.c_float(), C.c_float()
    assert fresh.lib.ntts_codec_last_loudness_timing(fresh.h, C.byref(a), C.byref(b)) == ESTATE       # nothing of the stage has been launched
    assert "no loudness" in (fresh.lib.ntts_codec_last_error(fresh.h) or b"").decode()
    on = fresh.decode(codes, loudness=[None, -16.0])
    assert np.array_equal(on[0], plain[0]) and not np.array_equal(on[1], plain[1])
    ms = fresh.last_loudness_timing()
    assert len(ms) == 2 and all(v >= 0.0 for v in ms)


# ---------------------------------------------------------------------------------------------- c. refusals
def raw_normalize(eng, x, n_samples, loud, fmt, dtype, out_stride):
    x = np.ascontiguousarray(x, dtype=np.float32)
    n_samples = np.ascontiguousarray(n_samples, dtype=np.int32)
    arr = (_hip.WavLoudnessC * len(loud))(*[_hip.WavLoudnessC(*v) for v in loud])
    out = np.zeros((x.shape[0], max(1, out_stride)), dtype=dtype)
    out_lens = np.full(x.shape[0], -7, dtype=np.int32)
    measured = np.zeros((x.shape[0], 3))
    rc = eng.lib.ntts_codec_normalize(eng.h, x.shape[0], x.ctypes.data_as(C.POINTER(C.c_float)), x.shape[1], _i32p(n_samples), arr,
                                      C.byref(fmt) if fmt is not None else None, C.c_void_p(out.ctypes.data), out_stride, _i32p(out_lens),
                                      measured.ctypes.data_as(C.POINTER(C.c_double)))
    return rc, out, out_lens, measured


def last_error(eng):
    return (eng.lib.ntts_codec_last_error(eng.h) or b"").decode()


def test_refusals_name_the_problem_and_leave_the_engine_usable(deng):
    eng = deng
    codes = _codes()[:1]
    before = eng.decode(codes, loudness=-16.0)[0].copy()
    x = np.zeros((2, 12000), dtype=np.float32)
    x[:] = tone(440.0, -20.0, 12000)
    cap = eng.max_frames * eng.hop_length
    ok = (1, -16.0, -1.0, 20.0)

    def refused(rc, *words):
        msg = last_error(eng)
        assert rc == EINVAL and msg, (rc, msg)
        assert all(w in msg for w in words), msg

    lens = np.array([len(codes[0])], dtype=np.int32)
    flat = np.asarray(codes[0], dtype=np.int32)
    for bad, words in (((1, 0.5, -1.0, 20.0), ("target_lufs 0.5", "[-70, 0]")), ((1, -70.5, -1.0, 20.0), ("target_lufs -70.5",)),
                       ((1, float("nan"), -1.0, 20.0), ("target_lufs", "nan")), ((1, -16.0, 0.25, 20.0), ("peak_dbfs 0.25", "[-20, 0]")),
                       ((1, -16.0, -21.0, 20.0), ("peak_dbfs -21",)), ((1, -16.0, float("nan"), 20.0), ("peak_dbfs", "nan")),
                       ((1, -16.0, -1.0, -0.5), ("max_gain_db -0.5", "[0, 60]")), ((1, -16.0, -1.0, 61.0), ("max_gain_db 61",)),
                       ((1, -16.0, -1.0, float("inf")), ("max_gain_db inf",))):
        refused(raw_normalize(eng, x, [12000, 12000], [ok, bad], None, np.float32, 12000)[0], "utterance 1", *words)
        out = np.zeros(DECODE_HOP * 90, dtype=np.float32)
        ol = np.zeros(1, dtype=np.int32)
        arr = (_hip.WavLoudnessC * 1)(_hip.WavLoudnessC(*bad))
        refused(eng.lib.ntts_codec_decode_loud(eng.h, 1, _i32p(flat), _i32p(lens), None, arr, None, C.c_void_p(out.ctypes.data), len(out), _i32p(ol)),
                "utterance 0", *words)
    # what ntts_codec_stretch refuses
    refused(raw_normalize(eng, x, [12000, 12000], [ok, ok], None, np.float32, 11999)[0], "out_stride", "12000")
    refused(raw_normalize(eng, x, [12000, 12000], [ok, ok], _hip.WavFormatC(8000, 1, 0), np.int16, 3999)[0], "out_stride", "4000")
    refused(raw_normalize(eng, x, [12000, 12000], [ok, ok], _hip.WavFormatC(12345, 0, 0), np.float32, 12000)[0], "12345")
    refused(raw_normalize(eng, x, [12000, -1], [ok, ok], None, np.float32, 12000)[0], "n_samples -1")
    refused(raw_normalize(eng, x, [12001, 1], [ok, ok], None, np.float32, 12001)[0], "n_samples 12001")
    big = np.zeros((1, cap + 8), dtype=np.float32)
    refused(raw_normalize(eng, big, [cap + 1], [ok], None, np.float32, cap + 8)[0], str(cap + 1))
    m = np.zeros((1, 3))
    refused(eng.lib.ntts_codec_measure_loudness(eng.h, 1, big.ctypes.data_as(C.POINTER(C.c_float)), big.shape[1], _i32p(np.array([cap + 1], dtype=np.int32)),
                                                m.ctypes.data_as(C.POINTER(C.c_double))), str(cap + 1))
    refused(eng.lib.ntts_codec_decode_loud(eng.h, 1, _i32p(flat), _i32p(lens), _i32p(np.array([2001], dtype=np.int32)),
                                           (_hip.WavLoudnessC * 1)(_hip.WavLoudnessC(*ok)), None, C.c_void_p(big.ctypes.data), big.shape[1], _i32p(lens.copy())),
            "speed 2001")
    rc, out, out_lens, measured = raw_normalize(eng, x, [12000, 9000], [ok, ok], None, np.float32, 12000)
    assert rc == 0 and out_lens.tolist() == [12000, 9000] and np.isfinite(measured[0, 0]) and np.isnan(measured[1, 0])
    # the Python layer refuses by name before the library is called
    for bad, word in ((0.5, "0.5"), (-71, "-71"), ("loud", "loud"), (True, "True"), (float("nan"), "nan"), ([-16.0, -16.0], "2 values")):
        with pytest.raises(ValueError, match=word):
            eng.decode(codes, loudness=bad)
        with pytest.raises(ValueError, match=word):
            eng.normalize([before], bad)
    for kw, word in ((dict(loudness_peak=0.5), "loudness_peak"), (dict(loudness_peak=-20.5), "loudness_peak"), (dict(loudness_max_gain=-1), "loudness_max_gain"),
                     (dict(loudness_max_gain=61), "loudness_max_gain"), (dict(loudness_max_gain=float("nan")), "loudness_max_gain")):
        with pytest.raises(ValueError, match=word):
            eng.decode(codes, loudness=-16.0, **kw)
    assert np.array_equal(eng.decode(codes, loudness=-16.0)[0], before)


# ---------------------------------------------------------------------------------------------- d. the class
REF_CODES = [3, 77, 200, 5, 18, 9]
TEXTS = ["Testing.", "One more."]


class StubWatermarker:
    """A host library between the codec and the output: must see the 24 kHz float32 waveform, stretched and normalised."""

    def __init__(self):
        self.seen = []

    def apply_watermark(self, wav, sample_rate):
        self.seen.append((wav.dtype, wav.ndim, sample_rate, wav.copy()))
        return (0.5 * wav).astype(np.float32)


def plain_batch(tts):
    if not hasattr(tts, "_plain_batch_loud"):
        tts._plain_batch_loud = [w.copy() for w in tts.infer_batch(TEXTS, REF_CODES, "So I'm live.")]
    return tts._plain_batch_loud


def test_class_infer_batch_with_a_loudness_per_utterance(tts):
    assert tts.loudness is None and tts.loudness_peak == -1.0 and tts.loudness_max_gain == 20.0
    plain = plain_batch(tts)
    eng = tts.codec.engine
    assert all(len(p) >= 4 * S for p in plain), [len(p) for p in plain]                       # (long enough to be measured)
    got = tts.infer_batch(TEXTS, REF_CODES, "So I'm live.", loudness=[-16, None])
    want, m = eng.normalize([plain[0]], -16.0, return_measured=True)
    assert m[0, 2] != 1.0 and got[0].dtype == np.float32 and np.array_equal(got[0], want[0])
    assert np.array_equal(got[1], plain[1])                             # the row with the option off: the call without it, bit for bit
    assert abs(eng.measure_loudness([got[0]])[0, 0] - (m[0, 0] + 20.0 * np.log10(m[0, 2]))) < 1e-4
    one = tts.infer(TEXTS[0], REF_CODES, "So I'm live.", loudness=-16)
    assert np.array_equal(one, want[0])
    both = tts.infer_batch(TEXTS, REF_CODES, "So I'm live.", loudness=-23.0, speed=1.25, sample_rate=8000, encoding="mulaw")
    conv = eng.convert(eng.normalize(eng.stretch(plain, 1.25), -23.0), sample_rate=8000, encoding="mulaw")
    assert all(g.dtype == np.uint8 and np.array_equal(g, w) for g, w in zip(both, conv))


def test_class_instance_loudness_and_decode_codes(tts):
    codes = [list(range(1, 51)), [9, 8, 7, 250] * 15]                   # 12 000 and 14 400 samples
    eng = tts.codec.engine
    native = [w.copy() for w in tts.decode_codes(codes)]
    try:
        tts.loudness, tts.loudness_peak, tts.loudness_max_gain = -18.0, -2.0, 12.0
        a = tts.decode_codes(codes)                                     # the instance's loudness
        b = tts.decode_codes(codes, loudness=[None, -30.0])             # overridden per call, one per utterance
        c = tts.decode_codes(codes, loudness=None)                      # switched off for the call
        wav = tts.infer(TEXTS[0], REF_CODES, "So I'm live.")
    finally:
        tts.loudness, tts.loudness_peak, tts.loudness_max_gain = None, -1.0, 20.0
    assert all(np.array_equal(x, y) for x, y in zip(a, eng.normalize(native, -18.0, loudness_peak=-2.0, loudness_max_gain=12.0)))
    assert not np.array_equal(a[0], native[0])
    assert np.array_equal(b[0], native[0]) and np.array_equal(b[1], eng.normalize([native[1]], -30.0, loudness_peak=-2.0, loudness_max_gain=12.0)[0])
    assert all(np.array_equal(x, y) for x, y in zip(c, native))
    assert np.array_equal(wav, eng.normalize([plain_batch(tts)[0]], -18.0, loudness_peak=-2.0, loudness_max_gain=12.0)[0])
    assert all(np.array_equal(x, y) for x, y in zip(tts.decode_codes(codes), native))
    for bad, word in ((0.3, "0.3"), (-80, "-80"), ("quiet", "quiet"), ([-16, -16, -16], "3 values")):
        with pytest.raises(ValueError, match=word):
            tts.decode_codes(codes, loudness=bad)
        with pytest.raises(ValueError, match=word):
            tts.infer_batch(TEXTS, REF_CODES, "So I'm live.", loudness=bad)
    from neutts import NeuTTS
    for kw in (dict(loudness=3.0), dict(loudness=-16.0, loudness_peak=1.0), dict(loudness_max_gain=70.0)):
        with pytest.raises(ValueError, match="loudness"):               # checked ahead of any loading
            NeuTTS(backbone_repo=None, codec_repo=None, **kw)


def test_class_streams_refuse_a_loudness(tts):
    with pytest.raises(ValueError, match="loudness=-16.*end"):
        tts.infer_stream("Streaming.", REF_CODES, "So I'm live.", loudness=-16)          # at the call, before a generator exists
    with pytest.raises(ValueError, match="loudness=-16.*end"):
        tts.infer_stream_batch(["Streaming."], REF_CODES, "So I'm live.", loudness=-16)
    try:
        tts.loudness = -20.0
        with pytest.raises(ValueError, match="loudness=-20.0 on the instance"):
            tts.infer_stream("Streaming.", REF_CODES, "So I'm live.")
        with pytest.raises(ValueError, match="loudness=-20.0 on the instance"):
            tts.infer_stream_batch(["Streaming."], REF_CODES, "So I'm live.")
    finally:
        tts.loudness = None
    gen = tts.infer_stream("Streaming.", REF_CODES, "So I'm live.", loudness=None)      # off, spelled out
    gen.close()


def test_class_watermarker_sees_the_normalized_24khz_float(tts):
    plain = plain_batch(tts)
    stub = StubWatermarker()
    tts.watermarker = stub
    try:
        got = tts.infer_batch(TEXTS, REF_CODES, "So I'm live.", speed=[0.8, 1.0], loudness=[-16.0, -23.0], sample_rate=16000, encoding="pcm16")
        one = tts.infer(TEXTS[1], REF_CODES, "So I'm live.", loudness=-23.0)
    finally:
        tts.watermarker = None
    eng = tts.codec.engine
    normal = eng.normalize(eng.stretch(plain, [0.8, 1.0]), [-16.0, -23.0])
    assert [(d, nd, sr) for d, nd, sr, _ in stub.seen] == [(np.dtype(np.float32), 1, 24000)] * 3
    assert all(np.array_equal(s[3], w) for s, w in zip(stub.seen, normal + [normal[1]]))
    want = eng.convert([(0.5 * w).astype(np.float32) for w in normal], sample_rate=16000, encoding="pcm16")
    assert all(g.dtype == np.int16 and np.array_equal(g, w) for g, w in zip(got, want))
    assert one.dtype == np.float32 and np.array_equal(one, (0.5 * normal[1]).astype(np.float32))
