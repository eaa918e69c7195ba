"""speed=: the codec's pitch-preserving time stretch (include/neutts_hip.h ntts_codec_stretch / ntts_codec_decode_speed; kernels/codec.h
wav_stretch_search_kernel / wav_stretch_render_kernel) on the CPU SIMT emulator against tests/time_stretch_spec.py, through ntts_codec_stretch (the
stage alone), the decode entry points and the NeuTTS class.  tests/test_gpu_time_stretch.py runs the same bodies on libneutts_hip.so."""
import ctypes as C

import numpy as np
import pytest

from neutts import _hip
from common import load_codec_fixture, make_codec_engine
import test_emu_neutts_class as class_cases
import time_stretch_spec as spec
import wav_format_spec as fspec

EINVAL = -1
LENGTHS = (0, 1, 359, 720, 721, 1443, 4000, 6144)       # empty, one sample, under one frame, L, L + 1, ~4 frames, many frames, the engine's longest
SPEEDS = (500, 730, 1000, 1370, 2000)
KINDS = ("silence", "tiny", "period60", "noise", "tone")
IN_STRIDE = 6144 + 8
SCRATCH = 1e30                                          # what stands behind every utterance's samples: read as signal, it shows

_ref = {}


def signal(kind, n, seed):
    i = np.arange(n, dtype=np.float64)
    if kind == "silence":                               # every D is 0: the tie rule alone decides
        return np.zeros(n, dtype=np.float32)
    if kind == "tiny":                                  # PCM16 values in -3 .. 3: D takes few values, ties everywhere
        return (np.round(3.0 * np.sin(2 * np.pi * i / 97.3)) / 32768.0).astype(np.float32)
    if kind == "period60":                              # exact period 60 on the PCM16 grid: candidates 60 apart tie in D exactly
        tab = np.random.default_rng(60).integers(-12000, 12000, size=60)
        return (tab[np.arange(n) % 60] / 32768.0).astype(np.float32)
    if kind == "noise":
        return np.random.default_rng(seed).uniform(-1.0, 1.0, size=n).astype(np.float32)
    t = i / 24000.0                                     # the three-harmonic tone
    return (0.4 * np.sin(2 * np.pi * 137 * t) + 0.2 * np.sin(2 * np.pi * 274 * t) + 0.1 * np.sin(2 * np.pi * 411 * t)).astype(np.float32)


def cases():
    """40 ragged rows: every length with every kind of signal, the speeds dealt so that every (length, speed) and every (kind, speed) pair occurs.
    -> (x [40][IN_STRIDE] float32 with 1e30 behind each row, n_samples, per-mille speeds, kinds); computed once."""
    if "x" not in _ref:
        rows = [(n, kind, SPEEDS[(li + ki) % len(SPEEDS)]) for li, n in enumerate(LENGTHS) for ki, kind in enumerate(KINDS)]
        x = np.full((len(rows), IN_STRIDE), SCRATCH, dtype=np.float32)
        for r, (n, kind, _) in enumerate(rows):
            x[r, :n] = signal(kind, n, seed=r)
        x.setflags(write=False)
        _ref["x"] = (x, np.array([r[0] for r in rows], dtype=np.int32), np.array([r[2] for r in rows], dtype=np.int32), [r[1] for r in rows])
    return _ref["x"]


def reference():
    """The spec's (float64 output, positions) of every row of cases(); computed once."""
    if "want" not in _ref:
        x, n, pm, _ = cases()
        _ref["want"] = [spec.stretch(x[r, : n[r]], int(pm[r])) for r in range(len(n))]
    return _ref["want"]


def engine_result(eng):
    """ntts_codec_stretch of cases() in the native format, once per engine: 40 rows of up to 6144 samples through a workspace of 12 288, two rows
    per round."""
    if not hasattr(eng, "_stretch_result"):
        x, n, pm, _ = cases()
        eng._stretch_result = eng.stretch_array(x, n, pm / 1000.0)
    return eng._stretch_result


@pytest.fixture(scope="module")
def eng(emu_lib):
    z, cfg, w = load_codec_fixture("codec_tiny")
    e = make_codec_engine(cfg, w, emu_lib, max_frames=256)       # hop 24: up to 6144 samples per utterance, 12 288 in the workspace
    e._fixture, e._on_gpu = z, False
    return e


@pytest.fixture(scope="module")
def tts(emu_lib):
    return class_cases.build_tts(emu_lib)


# ---------------------------------------------------------------------------------------------- a. the stage against the spec
def test_positions_and_lengths_equal_the_spec(eng):
    x, n, pm, kinds = cases()
    out, out_lens, pos, frames = engine_result(eng)
    want = reference()
    assert out.dtype == np.float32 and pos.dtype == np.int32
    assert out_lens.tolist() == [spec.out_len(int(a), int(s)) for a, s in zip(n, pm)] == [len(w[0]) for w in want]
    assert frames.tolist() == [len(w[1]) for w in want]
    moved = 0
    for r, (_, p) in enumerate(want):
        assert np.array_equal(pos[r, : len(p)], p), f"row {r} ({kinds[r]}, {n[r]} samples, speed {pm[r]}): first difference at frame " \
                                                    f"{int(np.nonzero(pos[r, : len(p)] != p)[0][0])}"
        assert (pos[r, len(p):] == -1).all(), f"row {r}: positions written behind its {len(p)} frames"
        moved += int((np.diff(p) != spec.HS).sum())
    assert moved > 50                                   # (the cases do leave the natural continuation: the search is exercised)


def test_f32_output_within_the_derived_bound_and_exact_on_continuations(eng):
    x, n, pm, kinds = cases()
    out, out_lens, _, _ = engine_result(eng)
    worst = 0.0
    for r, (w, p) in enumerate(reference()):
        y = out[r, : len(w)]
        assert np.isfinite(y).all() and (np.abs(y) < 4.0).all(), f"row {r}: scratch behind the utterance was read as signal"
        if not len(w):
            continue
        xr = x[r, : n[r]]
        bound = spec.error_bound(float(np.abs(xr).max()))        # 4 * 2^-24 * max|x|: one subtraction, one fp32 fade coefficient, one fma
        err = float(np.abs(y.astype(np.float64) - w).max())
        worst = max(worst, err / bound if bound else err)
        assert err <= bound, f"row {r} ({kinds[r]}, speed {pm[r]}): {err:.3e} > {bound:.3e}"
        keep = spec.continuation_mask(p, len(w))                 # p_k == t_k: the input bit for bit
        src = spec.source_index(p, len(w))
        xin = np.concatenate([xr, np.zeros(int(src.max()) + 1, dtype=np.float32)])
        assert np.array_equal(y[keep], xin[src[keep]]), f"row {r}: a continuation frame is not the input"
        if pm[r] == 1000:
            assert np.array_equal(y, xr)
    print(f"max |engine - spec| / bound over the rows: {worst:.3f}")


def test_unit_speed_rows_are_the_input_bit_for_bit(eng):
    x, n, pm, _ = cases()
    out, out_lens, pos, frames = engine_result(eng)
    rows = np.nonzero(pm == 1000)[0]
    assert len(rows) == 8
    for r in rows:
        assert out_lens[r] == n[r] and np.array_equal(out[r, : n[r]], x[r, : n[r]])
        assert pos[r, : frames[r]].tolist() == [k * spec.HS for k in range(frames[r])]
    # a call whose rows are all 1000 launches nothing: the waveforms come back as they are, in any format as convert gives them
    sub = x[rows]
    same, lens, p1, f1 = eng.stretch_array(sub, n[rows], 1.0)
    assert all(np.array_equal(same[i, : lens[i]], sub[i, : n[rows][i]]) for i in range(len(rows)))
    assert all(p1[i, : f1[i]].tolist() == [k * spec.HS for k in range(f1[i])] for i in range(len(rows)))
    mu = eng.stretch([sub[i, : n[rows][i]] for i in range(len(rows))], [1.0] * len(rows), sample_rate=8000, encoding="mulaw")
    conv = eng.convert([sub[i, : n[rows][i]] for i in range(len(rows))], sample_rate=8000, encoding="mulaw")
    assert all(np.array_equal(a, b) for a, b in zip(mu, conv))


def test_stretch_with_a_format_equals_convert_of_the_stretched_f32(eng):
    x, n, pm, _ = cases()
    out, out_lens, _, _ = engine_result(eng)
    rows = [r for r in range(len(n)) if n[r] in (721, 1443, 4000) and out_lens[r] <= 6144]      # (convert takes what the engine's longest utterance holds)
    assert len(rows) == 14 and set(pm[rows]) == set(SPEEDS)
    native = [out[r, : out_lens[r]] for r in rows]
    for rate, enc in ((24000, "pcm16"), (8000, "mulaw")):
        got = eng.stretch([x[r, : n[r]] for r in rows], pm[rows] / 1000.0, sample_rate=rate, encoding=enc)
        want = eng.convert(native, sample_rate=rate, encoding=enc)
        for g, w, s in zip(got, want, native):
            assert g.dtype == fspec.ENCODINGS[enc] and len(g) == fspec.out_len(len(s), rate)
            assert np.array_equal(g, w)


def test_stretch_splits_batches_larger_than_the_workspace(eng):
    """More rows than the waveform workspace holds at once (12 288 samples): several rounds, the same samples and positions as row by row."""
    rng = np.random.default_rng(9)
    wavs = [rng.uniform(-1, 1, 3000 - 61 * i).astype(np.float32) for i in range(9)]            # 9 x ~3000 > 12 288 samples: four rows per round
    speeds = [0.5, 0.73, 1.0, 1.37, 2.0, 0.9, 1.1, 1.0, 1.25]
    got = eng.stretch(wavs, speeds)
    for w, s, g in zip(wavs, speeds, got):
        want, _ = spec.stretch(w, spec.permille(s))
        assert len(g) == len(want) and np.abs(g.astype(np.float64) - want).max() <= spec.error_bound(1.0)
        assert np.array_equal(g, eng.stretch([w], s)[0])
    assert eng.stretch([], 0.8) == []
    assert [len(v) for v in eng.stretch([np.zeros(0, np.float32)] * 2, 0.8)] == [0, 0]


# ---------------------------------------------------------------------------------------------- b. behind the codec pass
def _codes(eng):
    rng = np.random.default_rng(3)
    return [rng.integers(0, 4 ** 4, size=t).tolist() for t in (61, 30, 100, 1, 45)]           # 1464, 720, 2400, 24 and 1080 samples


CODE_SPEEDS = [0.8, 1.0, 0.5, 2.0, 1.37]


def test_decode_with_speed_equals_stretch_of_the_plain_decode(eng):
    codes = _codes(eng)
    plain = [p.copy() for p in eng.decode(codes)]
    fast = eng.decode(codes, speed=CODE_SPEEDS)
    want = eng.stretch(plain, CODE_SPEEDS)
    for p, g, w, s in zip(plain, fast, want, CODE_SPEEDS):
        assert g.dtype == np.float32 and len(g) == spec.out_len(len(p), spec.permille(s))
        assert np.array_equal(g, w)
    assert np.array_equal(fast[1], plain[1])                              # the row at 1.0: bit for bit
    for rate, enc in ((16000, "pcm16"), (8000, "mulaw")):                 # with a format: convert of the stretched f32, bit for bit
        got = eng.decode(codes, speed=CODE_SPEEDS, sample_rate=rate, encoding=enc)
        conv = eng.convert(fast, sample_rate=rate, encoding=enc)
        for g, w in zip(got, conv):
            assert g.dtype == fspec.ENCODINGS[enc] and np.array_equal(g, w)
    one = eng.decode(codes, speed=0.8)                                    # one value for the call
    assert all(np.array_equal(a, b) for a, b in zip(one, eng.stretch(plain, 0.8)))
    arr = np.zeros((2, 61), dtype=np.int32)
    arr[0], arr[1, :30] = codes[0], codes[1]
    wide = eng.decode_array(arr, lens=np.array([61, 30]), speed=[0.8, 1.25])
    assert wide.shape == (2, spec.out_len(1464, 800))
    assert np.array_equal(wide[0], fast[0]) and np.array_equal(wide[1, : spec.out_len(720, 1250)], eng.stretch([plain[1]], 1.25)[0])


def test_default_speed_makes_the_same_calls_and_bits(eng):
    codes = _codes(eng)[:2]
    plain = [p.copy() for p in eng.decode(codes)]
    for speed in (None, 1.0, [1.0, 1.0], 1.0004):                         # (round(speed * 1000) == 1000)
        assert all(np.array_equal(a, b) for a, b in zip(eng.decode(codes, speed=speed), plain))
    lens = np.array([len(c) for c in codes], dtype=np.int32)
    flat = np.ascontiguousarray(np.concatenate([np.asarray(c, dtype=np.int32) for c in codes]))
    i32p = C.POINTER(C.c_int32)
    ones = np.full(2, 1000, dtype=np.int32)
    for sp in (None, ones.ctypes.data_as(i32p)):                          # a null array and an array of 1000s: ntts_codec_decode_fmt's result
        out = np.zeros((2, 61 * 24), dtype=np.float32)
        out_lens = np.zeros(2, dtype=np.int32)
        rc = eng.lib.ntts_codec_decode_speed(eng.h, 2, flat.ctypes.data_as(i32p), lens.ctypes.data_as(i32p), sp, None, C.c_void_p(out.ctypes.data),
                                             out.shape[1], out_lens.ctypes.data_as(i32p))
        assert rc == 0 and out_lens.tolist() == [61 * 24, 30 * 24]
        assert all(np.array_equal(out[r, : out_lens[r]], plain[r]) for r in range(2))
    n = C.c_int64()
    assert eng.lib.ntts_wav_stretch_len(800, 1001, C.byref(n)) == 0 and n.value == 1252
    assert eng.lib.ntts_wav_stretch_len(2000, 1001, C.byref(n)) == 0 and n.value == 501
    assert eng.lib.ntts_wav_stretch_len(499, 1001, C.byref(n)) == EINVAL and eng.lib.ntts_wav_stretch_len(2001, 1001, C.byref(n)) == EINVAL


def test_decode_device_with_speed_equals_decode(eng):
    """ntts_codec_decode_dev_speed: codes on the device, stretched (and formatted) waveforms into the engine's pinned buffer."""
    rng = np.random.default_rng(4)
    lens = np.array([40, 17], dtype=np.int32)
    arr = rng.integers(0, 4 ** 4, size=(2, 40)).astype(np.int32)
    codes = [arr[0, :40].tolist(), arr[1, :17].tolist()]
    if eng._on_gpu:
        import torch
        keep = torch.tensor(arr, device="cuda")
        ptr = keep.data_ptr()
        torch.cuda.synchronize()
    else:
        keep, ptr = arr, arr.ctypes.data                # (the emulator's device memory is host memory)
    for kw in (dict(), dict(sample_rate=16000, encoding="pcm16")):
        want = [w.copy() for w in eng.decode(codes, speed=[0.75, 1.6], **kw)]
        wav = eng.decode_device(ptr, 40, lens, speed=[0.75, 1.6], **kw)
        eng.sync()
        assert wav.shape == (2, max(len(w) for w in want)) and wav.dtype == want[0].dtype
        for r, w in enumerate(want):
            assert np.array_equal(wav[r, : len(w)], w)
    del keep


# ---------------------------------------------------------------------------------------------- c. refusals
def _i32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def raw_stretch(eng, x, n_samples, pm, fmt, dtype, out_stride, pos_stride, want_pos=True):
    x = np.ascontiguousarray(x, dtype=np.float32)
    n_samples = np.ascontiguousarray(n_samples, dtype=np.int32)
    pm = np.ascontiguousarray(pm, dtype=np.int32)
    out = np.zeros((x.shape[0], max(1, out_stride)), dtype=dtype)
    out_lens = np.full(x.shape[0], -7, dtype=np.int32)
    pos = np.full((x.shape[0], max(1, pos_stride)), -1, dtype=np.int32)
    rc = eng.lib.ntts_codec_stretch(eng.h, x.shape[0], x.ctypes.data_as(C.POINTER(C.c_float)), x.shape[1], _i32p(n_samples), _i32p(pm),
                                    C.byref(fmt) if fmt is not None else None, C.c_void_p(out.ctypes.data), out_stride, _i32p(out_lens),
                                    _i32p(pos) if want_pos else None, pos_stride)
    return rc, out, out_lens, pos


def last_error(eng):
    return (eng.lib.ntts_codec_last_error(eng.h) or b"").decode()


def test_refusals_name_the_problem_and_leave_the_engine_usable(eng):
    codes = _codes(eng)[1:2]
    before = eng.decode(codes, speed=0.8)[0].copy()
    x = np.zeros((2, 1000), dtype=np.float32)
    cap = eng.max_frames * eng.hop_length

    def refused(rc, *words):
        msg = last_error(eng)
        assert rc == EINVAL and msg, (rc, msg)
        assert all(w in msg for w in words), msg

    for bad in (499, 2001, 0, -1000):
        refused(raw_stretch(eng, x, [700, 1000], [1000, bad], None, np.float32, 4096, 64)[0], f"speed {bad}", "[500, 2000]")
        lens = np.array([len(codes[0])], dtype=np.int32)
        flat = np.asarray(codes[0], dtype=np.int32)
        out = np.zeros(8192, dtype=np.float32)
        ol = np.zeros(1, dtype=np.int32)
        refused(eng.lib.ntts_codec_decode_speed(eng.h, 1, _i32p(flat), _i32p(lens), _i32p(np.array([bad], dtype=np.int32)), None,
                                                C.c_void_p(out.ctypes.data), 8192, _i32p(ol)), f"speed {bad}")
    # 700 samples at 0.5 -> 1400, 1000 at 0.8 -> 1250: four frames at most
    refused(raw_stretch(eng, x, [700, 1000], [500, 800], None, np.float32, 1399, 4)[0], "out_stride", "1400")
    refused(raw_stretch(eng, x, [700, 1000], [500, 800], None, np.float32, 1400, 3)[0], "pos_stride", "4")
    rc, out, out_lens, pos = raw_stretch(eng, x, [700, 1000], [500, 800], None, np.float32, 1400, 4)
    assert rc == 0 and out_lens.tolist() == [1400, 1250] and (pos >= 0).all()
    rc, out, out_lens, pos = raw_stretch(eng, x, [700, 1000], [500, 800], None, np.float32, 1400, 0, want_pos=False)     # no positions asked for
    assert rc == 0 and out_lens.tolist() == [1400, 1250]
    refused(raw_stretch(eng, x, [700, 1000], [500, 800], _hip.WavFormatC(8000, 1, 0), np.int16, 466, 4)[0], "out_stride", "467")
    refused(raw_stretch(eng, x, [700, 1000], [500, 800], _hip.WavFormatC(12345, 0, 0), np.float32, 4096, 4)[0], "12345")
    refused(raw_stretch(eng, x, [700, -1], [500, 800], None, np.float32, 4096, 64)[0], "n_samples -1")
    refused(raw_stretch(eng, x, [1001, 1], [500, 800], None, np.float32, 4096, 64)[0], "n_samples 1001")
    big = np.zeros((1, cap + 8), dtype=np.float32)
    refused(raw_stretch(eng, big, [cap + 1], [800], None, np.float32, 2 * cap + 8, 64)[0], str(cap + 1))
    rc, out, out_lens, pos = raw_stretch(eng, big, [cap], [500], None, np.float32, 2 * cap, spec.n_frames(2 * cap))     # the longest row, doubled
    assert rc == 0 and out_lens.tolist() == [2 * cap]
    # the Python layer refuses by name before the library is called
    for bad, word in ((0.49, "0.49"), (2.01, "2.01"), ("fast", "fast"), (True, "True"), (float("nan"), "nan"), ([0.8, 0.9], "2 values")):
        with pytest.raises(ValueError, match=word):
            eng.decode(codes, speed=bad)
        with pytest.raises(ValueError, match=word):
            eng.stretch([before], bad)
    assert np.array_equal(eng.decode(codes, speed=0.8)[0], before)


# ---------------------------------------------------------------------------------------------- d. the class
REF_CODES = [3, 77, 200, 5, 18, 9]
TEXTS = ["Testing.", "One more."]


class StubWatermarker:
    """A host library between the codec and the output: must see the 24 kHz float32 waveform of the STRETCHED length."""

    def __init__(self):
        self.seen = []

    def apply_watermark(self, wav, sample_rate):
        self.seen.append((wav.dtype, wav.ndim, sample_rate, len(wav)))
        return (0.5 * wav).astype(np.float32)


def plain_batch(tts):
    if not hasattr(tts, "_plain_batch_speed"):
        tts._plain_batch_speed = [w.copy() for w in tts.infer_batch(TEXTS, REF_CODES, "So I'm live.")]
    return tts._plain_batch_speed


def test_class_infer_batch_with_a_speed_per_utterance(tts):
    assert tts.sample_rate == 24000 and tts.speed == 1.0
    plain = plain_batch(tts)
    eng = tts.codec.engine
    got = tts.infer_batch(TEXTS, REF_CODES, "So I'm live.", speed=[1.0, 0.8])
    assert got[0].dtype == np.float32 and np.array_equal(got[0], plain[0])          # the row at 1.0: the call without speed, bit for bit
    want = eng.stretch([plain[1]], 0.8)[0]
    assert len(got[1]) == spec.out_len(len(plain[1]), 800) and np.array_equal(got[1], want)
    one = tts.infer(TEXTS[1], REF_CODES, "So I'm live.", speed=0.8)
    assert np.array_equal(one, want)
    both = tts.infer_batch(TEXTS, REF_CODES, "So I'm live.", speed=1.25, sample_rate=8000, encoding="mulaw")
    conv = eng.convert(eng.stretch(plain, 1.25), sample_rate=8000, encoding="mulaw")
    assert all(g.dtype == np.uint8 and np.array_equal(g, w) for g, w in zip(both, conv))
    assert tts.sample_rate == 24000


def test_class_instance_speed_and_decode_codes(tts):
    codes = [list(range(1, 41)), [9, 8] * 20]
    eng = tts.codec.engine
    native = [w.copy() for w in tts.decode_codes(codes)]
    try:
        tts.speed = 1.5
        a = tts.decode_codes(codes)                         # the instance's speed
        b = tts.decode_codes(codes, speed=[1.0, 0.6])       # overridden per call, one per utterance
        wav = tts.infer(TEXTS[0], REF_CODES, "So I'm live.")
    finally:
        tts.speed = 1.0
    assert all(np.array_equal(x, y) for x, y in zip(a, eng.stretch(native, 1.5)))
    assert np.array_equal(b[0], native[0]) and np.array_equal(b[1], eng.stretch([native[1]], 0.6)[0])
    assert np.array_equal(wav, eng.stretch([plain_batch(tts)[0]], 1.5)[0])
    assert all(np.array_equal(x, y) for x, y in zip(tts.decode_codes(codes), native))
    for bad, word in ((0.3, "0.3"), (2.5, "2.5"), ("slow", "slow"), ([0.8, 0.9, 1.0], "3 values")):
        with pytest.raises(ValueError, match=word):
            tts.decode_codes(codes, speed=bad)
        with pytest.raises(ValueError, match=word):
            tts.infer_batch(TEXTS, REF_CODES, "So I'm live.", speed=bad)
    from neutts import NeuTTS
    with pytest.raises(ValueError, match="speed"):          # checked ahead of any loading
        NeuTTS(backbone_repo=None, codec_repo=None, speed=3.0)


def test_class_streams_refuse_a_speed(tts):
    for kw in (dict(speed=0.8), dict(speed=1.25)):
        with pytest.raises(ValueError, match="speed=.*one-shot"):
            tts.infer_stream("Streaming.", REF_CODES, "So I'm live.", **kw)          # at the call, before a generator exists
        with pytest.raises(ValueError, match="speed=.*one-shot"):
            tts.infer_stream_batch(["Streaming."], REF_CODES, "So I'm live.", **kw)
    try:
        tts.speed = 0.9
        with pytest.raises(ValueError, match="speed=0.9"):
            tts.infer_stream("Streaming.", REF_CODES, "So I'm live.")
        with pytest.raises(ValueError, match="speed=0.9"):
            tts.infer_stream_batch(["Streaming."], REF_CODES, "So I'm live.")
    finally:
        tts.speed = 1.0
    gen = tts.infer_stream("Streaming.", REF_CODES, "So I'm live.", speed=1.0)      # the default, spelled out
    gen.close()


def test_class_watermarker_sees_the_stretched_24khz_float(tts):
    plain = plain_batch(tts)
    stub = StubWatermarker()
    tts.watermarker = stub
    try:
        got = tts.infer_batch(TEXTS, REF_CODES, "So I'm live.", speed=[0.8, 1.25], sample_rate=16000, encoding="pcm16")
        one = tts.infer(TEXTS[1], REF_CODES, "So I'm live.", speed=1.25)
    finally:
        tts.watermarker = None
    n0, n1 = spec.out_len(len(plain[0]), 800), spec.out_len(len(plain[1]), 1250)
    assert stub.seen == [(np.dtype(np.float32), 1, 24000, n0), (np.dtype(np.float32), 1, 24000, n1), (np.dtype(np.float32), 1, 24000, n1)]
    eng = tts.codec.engine
    slow, fast = eng.stretch([plain[0]], 0.8)[0], eng.stretch([plain[1]], 1.25)[0]
    want = eng.convert([(0.5 * slow).astype(np.float32), (0.5 * fast).astype(np.float32)], sample_rate=16000, encoding="pcm16")
    assert all(g.dtype == np.int16 and np.array_equal(g, w) for g, w in zip(got, want))
    assert one.dtype == np.float32 and np.array_equal(one, (0.5 * fast).astype(np.float32))
