"""The codec's device output stage (include/neutts_hip.h ntts_wav_format: resample 24 kHz -> 8 .. 48 kHz, PCM16, G.711 mu-law) on the CPU SIMT
emulator against tests/wav_format_spec.py, through ntts_codec_convert (the stage alone, the direct way to the kernel), ntts_codec_decode_fmt and the
NeuTTS class.  tests/test_gpu_wav_format.py runs the same bodies on libneutts_hip.so."""
import ctypes as C

import numpy as np
import pytest

from neutts import _hip
from common import load_codec_fixture, make_codec_engine
import test_emu_neutts_class as class_cases
import wav_format_spec as spec

EINVAL = -1
CASES = [(r, 6) for r in spec.RATES] + [(8000, 16)]          # every rate at torchaudio's default width, and a telephony-grade filter
N_SAMPLES = (0, 1, 2, 41, 479, 480, 1000)                    # empty, shorter than the filter, around two blocks of 8 kHz output, several blocks
IN_STRIDE = 1024
SCRATCH = 1e30                                               # what stands behind every utterance's samples: read as signal, it shows

_ref = {}


def ragged_input():
    """[7][1024] float32: uniform in [-1, 1] up to each row's length, 1e30 behind it; computed once."""
    if "x" not in _ref:
        rng = np.random.default_rng(2024)
        x = rng.uniform(-1.0, 1.0, size=(len(N_SAMPLES), IN_STRIDE)).astype(np.float32)
        for r, n in enumerate(N_SAMPLES):
            x[r, n:] = SCRATCH
        x.setflags(write=False)
        _ref["x"] = x
    return _ref["x"]


def reference(rate, W):
    """The spec's float64 outputs of ragged_input(), one array per row; computed once per (rate, W)."""
    if (rate, W) not in _ref:
        x = ragged_input()
        _ref[rate, W] = [spec.resample(x[r, :n], rate, W) for r, n in enumerate(N_SAMPLES)]
    return _ref[rate, W]


@pytest.fixture(scope="module")
def eng(emu_lib):
    z, cfg, w = load_codec_fixture("codec_tiny")
    e = make_codec_engine(cfg, w, emu_lib)            # hop 24, max_frames 64: convert takes up to 1536 samples per utterance
    e._fixture, e._on_gpu = z, False
    return e


@pytest.fixture(scope="module")
def tts(emu_lib):
    return class_cases.build_tts(emu_lib)


# ---------------------------------------------------------------------------------------------- a. convert against the spec
@pytest.mark.parametrize("rate,W", CASES)
def test_convert_f32_against_spec(eng, rate, W):
    x = ragged_input()
    got, out_lens = eng.convert_array(x, N_SAMPLES, sample_rate=rate, encoding="f32", filter_width=W)
    want = reference(rate, W)
    assert got.dtype == np.float32
    assert out_lens.tolist() == [spec.out_len(n, rate) for n in N_SAMPLES] == [len(w) for w in want]
    bound = spec.error_bound(rate, W, xmax=1.0)      # (taps + 2) 2^-24 max_p sum_j |h[p][j]| max|x|: an fp32 dot product in any order, fp32 coefficients
    worst = 0.0
    for r, w in enumerate(want):
        y = got[r, : len(w)].astype(np.float64)
        assert np.isfinite(y).all() and (np.abs(y) < 4.0).all(), f"row {r}: scratch behind the utterance was read as signal"
        if len(w):
            worst = max(worst, float(np.abs(y - w).max()))
    print(f"rate {rate} W {W}: max |engine - spec| {worst:.2e}, bound {bound:.2e}")
    assert worst <= bound                            # (0 at the native rate: the identity is a copy)


# ---------------------------------------------------------------------------------------------- b. the encodings are exact
def _edge_input():
    rng = np.random.default_rng(7)
    k = np.arange(-6, 7, dtype=np.float64)
    edge = np.concatenate([[1.0, -1.0, 1 - 2.0 ** -16, -(1 - 2.0 ** -16), 1.5, -1.5, 0.0], (k + 0.5) / 32768.0,
                           (k * 1000 + 0.5) / 32768.0, [32766.5 / 32768, 32767.5 / 32768, -32767.5 / 32768, -32768.5 / 32768]])
    rows = [np.concatenate([edge, rng.uniform(-1, 1, 300)]), rng.uniform(-1.3, 1.3, 777)]     # the second row saturates now and then
    n = np.array([len(r) for r in rows], dtype=np.int32)
    x = np.full((2, 800), SCRATCH, dtype=np.float32)
    for r, row in enumerate(rows):
        x[r, : len(row)] = row
    return x, n


@pytest.mark.parametrize("rate", [24000, 8000])
def test_encodings_are_exact_functions_of_the_f32_output(eng, rate):
    x, n = _edge_input()
    f32, lens = eng.convert_array(x, n, sample_rate=rate, encoding="f32")
    pcm, lens_p = eng.convert_array(x, n, sample_rate=rate, encoding="pcm16")
    mu, lens_m = eng.convert_array(x, n, sample_rate=rate, encoding="mulaw")
    assert pcm.dtype == np.int16 and mu.dtype == np.uint8
    assert lens.tolist() == lens_p.tolist() == lens_m.tolist() == [spec.out_len(v, rate) for v in n]
    for r in range(2):
        y = f32[r, : lens[r]]
        assert np.array_equal(pcm[r, : lens[r]], spec.pcm16(y))
        assert np.array_equal(mu[r, : lens[r]], spec.mulaw(spec.pcm16(y)))
    if rate == 24000:      # the edge values reach the encoders as they are: saturation at both ends, ties to even
        assert np.array_equal(f32[0, : n[0]], x[0, : n[0]])
        assert pcm[0, :7].tolist() == [32767, -32768, 32767, -32768, 32767, -32768, 0]
        assert pcm[0, 7:20].tolist() == [-6, -4, -4, -2, -2, 0, 0, 2, 2, 4, 4, 6, 6]
        assert int(pcm[1].max()) == 32767 and int(pcm[1].min()) == -32768


# ---------------------------------------------------------------------------------------------- raw C-ABI calls
def _i32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def raw_decode_fmt(eng, codes, fmt, dtype, out_stride=None):
    """ntts_codec_decode_fmt as it is (CodecEngine.decode routes the native format to ntts_codec_decode): -> (rc, [n, out_stride], out_lens)."""
    lens = np.array([len(c) for c in codes], dtype=np.int32)
    flat = np.ascontiguousarray(np.concatenate([np.asarray(c, dtype=np.int32) for c in codes]))
    if out_stride is None:
        out_stride = spec.out_len(eng.hop_length * int(lens.max()), fmt.sample_rate or 24000)
    out = np.zeros((len(codes), max(1, out_stride)), dtype=dtype)
    out_lens = np.full(len(codes), -7, dtype=np.int32)
    rc = eng.lib.ntts_codec_decode_fmt(eng.h, len(codes), _i32p(flat), _i32p(lens), C.byref(fmt), C.c_void_p(out.ctypes.data), out_stride,
                                       _i32p(out_lens))
    return rc, out, out_lens


def raw_convert(eng, x, n_samples, fmt, dtype, out_stride):
    x = np.ascontiguousarray(x, dtype=np.float32)
    n_samples = np.ascontiguousarray(n_samples, dtype=np.int32)
    out = np.zeros((x.shape[0], max(1, out_stride)), dtype=dtype)
    out_lens = np.full(x.shape[0], -7, dtype=np.int32)
    rc = eng.lib.ntts_codec_convert(eng.h, x.shape[0], x.ctypes.data_as(C.POINTER(C.c_float)), x.shape[1], _i32p(n_samples), C.byref(fmt),
                                    C.c_void_p(out.ctypes.data), out_stride, _i32p(out_lens))
    return rc, out, out_lens


def last_error(eng):
    return (eng.lib.ntts_codec_last_error(eng.h) or b"").decode()


def fixture_codes(eng):
    z = eng._fixture
    return [z["codes_0"][0, 0].tolist(), z["codes_1"][0, 0].tolist(), z["codes_0"][1, 0].tolist()]      # 37, 5 and 37 frames


# ---------------------------------------------------------------------------------------------- c. the default is untouched
def test_zeroed_format_is_the_plain_decode_bit_for_bit(eng):
    codes = fixture_codes(eng)
    plain = eng.decode(codes)
    for fmt in (_hip.WavFormatC(0, 0, 0), _hip.WavFormatC(24000, 0, 6), _hip.WavFormatC(24000, 0, 16)):
        rc, out, out_lens = raw_decode_fmt(eng, codes, fmt, np.float32)
        assert rc == 0, last_error(eng)
        assert out_lens.tolist() == [eng.hop_length * len(c) for c in codes]
        for r, p in enumerate(plain):
            assert np.array_equal(out[r, : out_lens[r]], p)
    again = eng.decode(codes, sample_rate=24000, encoding="f32", filter_width=9)
    assert all(np.array_equal(a, p) for a, p in zip(again, plain))
    n = C.c_int64()
    assert eng.lib.ntts_wav_out_len(None, 480, C.byref(n)) == 0 and n.value == 480
    assert eng.lib.ntts_wav_out_len(C.byref(_hip.WavFormatC(8000, 2, 0)), 481, C.byref(n)) == 0 and n.value == 161
    assert eng.lib.ntts_wav_out_len(C.byref(_hip.WavFormatC(8001, 0, 0)), 481, C.byref(n)) == EINVAL


# ---------------------------------------------------------------------------------------------- d. plumbing
@pytest.mark.parametrize("rate,encoding", [(16000, "pcm16"), (8000, "mulaw")])
def test_decode_fmt_equals_convert_of_the_plain_decode(eng, rate, encoding):
    rng = np.random.default_rng(3)
    n_codes = 4 ** 4                                     # the tiny codec's FSQ levels
    codes = [rng.integers(0, n_codes, size=t).tolist() for t in (7, 3, 1)]
    plain = eng.decode(codes)
    want = eng.convert(plain, sample_rate=rate, encoding=encoding)
    got = eng.decode(codes, sample_rate=rate, encoding=encoding)
    for g, w, p in zip(got, want, plain):
        assert g.dtype == w.dtype == spec.ENCODINGS[encoding] and len(g) == spec.out_len(len(p), rate)
        assert np.array_equal(g, w)
    arr = np.zeros((3, 7), dtype=np.int32)
    for r, c in enumerate(codes):
        arr[r, : len(c)] = c
    wide = eng.decode_array(arr, lens=np.array([7, 3, 1]), sample_rate=rate, encoding=encoding)
    assert wide.shape == (3, spec.out_len(7 * eng.hop_length, rate))
    assert all(np.array_equal(wide[r, : len(w)], w) for r, w in enumerate(want))
    # a destination wider than needed: a strided hand-over, the same samples, nothing written past a row's stride
    fc, dtype, _ = _hip.wav_format(rate, encoding)
    stride = spec.out_len(7 * eng.hop_length, rate) + 13
    rc, out, out_lens = raw_decode_fmt(eng, codes, fc, dtype, out_stride=stride)
    assert rc == 0, last_error(eng)
    assert out_lens.tolist() == [len(w) for w in want]
    for r, w in enumerate(want):
        assert np.array_equal(out[r, : len(w)], w)
    assert not out[:, stride - 13:].any()


def test_decode_device_with_a_format_equals_decode(eng):
    """ntts_codec_decode_dev_fmt: codes on the device, formatted waveforms into the engine's pinned buffer (sized in bytes)."""
    rng = np.random.default_rng(4)
    lens = np.array([5, 2], dtype=np.int32)
    arr = rng.integers(0, 4 ** 4, size=(2, 5)).astype(np.int32)
    want = eng.decode([arr[0, :5].tolist(), arr[1, :2].tolist()], sample_rate=16000, encoding="pcm16")
    if eng._on_gpu:
        import torch
        keep = torch.tensor(arr, device="cuda")
        ptr = keep.data_ptr()
        torch.cuda.synchronize()
    else:
        keep, ptr = arr, arr.ctypes.data                # (the emulator's device memory is host memory)
    wav = eng.decode_device(ptr, 5, lens, sample_rate=16000, encoding="pcm16")
    eng.sync()
    assert wav.dtype == np.int16 and wav.shape == (2, spec.out_len(5 * eng.hop_length, 16000))
    for r, w in enumerate(want):
        assert np.array_equal(wav[r, : len(w)], w)
    del keep


# ---------------------------------------------------------------------------------------------- e. refusals
def test_refusals_name_the_problem_and_leave_the_engine_usable(eng):
    codes = fixture_codes(eng)[1:2]
    before = eng.decode(codes)[0].copy()
    x = np.zeros((2, 64), dtype=np.float32)
    ok = _hip.WavFormatC(8000, 1, 0)
    cap = eng.max_frames * eng.hop_length

    def refused(rc, *words):
        msg = last_error(eng)
        assert rc == EINVAL and msg, (rc, msg)
        assert all(w in msg for w in words), msg

    for bad, word in ((_hip.WavFormatC(12345, 0, 0), "12345"), (_hip.WavFormatC(-8000, 0, 0), "-8000"), (_hip.WavFormatC(8000, 3, 0), "encoding 3"),
                      (_hip.WavFormatC(8000, -1, 0), "encoding -1"), (_hip.WavFormatC(8000, 0, -1), "filter_width -1"),
                      (_hip.WavFormatC(8000, 0, 65), "filter_width 65")):
        refused(raw_decode_fmt(eng, codes, bad, np.float32, out_stride=4096)[0], word)
        refused(raw_convert(eng, x, [10, 20], bad, np.float32, out_stride=4096)[0], word)
    need = spec.out_len(len(codes[0]) * eng.hop_length, 8000)
    refused(raw_decode_fmt(eng, codes, ok, np.int16, out_stride=need - 1)[0], "wav_stride")
    refused(raw_convert(eng, x, [10, 20], ok, np.int16, out_stride=6)[0], "out_stride")          # ceil(20 / 3) = 7
    rc, out, out_lens = raw_convert(eng, x, [10, 20], ok, np.int16, out_stride=7)
    assert rc == 0 and out_lens.tolist() == [4, 7]
    refused(raw_convert(eng, x, [10, -1], ok, np.int16, out_stride=64)[0], "n_samples -1")
    refused(raw_convert(eng, x, [65, 1], ok, np.int16, out_stride=64)[0], "n_samples 65")
    big = np.zeros((1, cap + 8), dtype=np.float32)
    refused(raw_convert(eng, big, [cap + 1], ok, np.int16, out_stride=cap)[0], str(cap + 1))
    rc, out, out_lens = raw_convert(eng, big, [cap], ok, np.int16, out_stride=cap)               # the longest utterance the engine takes
    assert rc == 0 and out_lens.tolist() == [spec.out_len(cap, 8000)]
    # the Python layer refuses by name before the library is called
    for kw, word in ((dict(sample_rate=11025), "11025"), (dict(encoding="alaw"), "alaw"), (dict(filter_width=0), "filter_width"),
                     (dict(filter_width=65), "65"), (dict(sample_rate=8000.0), "8000.0"), (dict(sample_rate=True), "True")):
        with pytest.raises(ValueError, match=word):
            eng.decode(codes, **kw)
        with pytest.raises(ValueError, match=word):
            eng.convert([before], **kw)
    assert np.array_equal(eng.decode(codes)[0], before)
    assert np.array_equal(eng.decode(codes, sample_rate=8000, encoding="mulaw")[0], eng.convert([before], sample_rate=8000, encoding="mulaw")[0])


def test_convert_splits_batches_larger_than_the_workspace(eng):
    """More rows than the waveform workspace holds at once (512 rows x 24 samples): several rounds, the same samples as row by row."""
    rng = np.random.default_rng(9)
    wavs = [rng.uniform(-1, 1, 1500 - 37 * i).astype(np.float32) for i in range(12)]          # 12 x ~1500 > 12 288 samples
    got = eng.convert(wavs, sample_rate=16000, encoding="pcm16")
    for w, g in zip(wavs, got):
        assert np.array_equal(g, eng.convert([w], sample_rate=16000, encoding="pcm16")[0])
    assert eng.convert([], sample_rate=8000) == []
    assert [len(v) for v in eng.convert([np.zeros(0, np.float32)] * 2, sample_rate=8000)] == [0, 0]


# ---------------------------------------------------------------------------------------------- f. the class
REF_CODES = [3, 77, 200, 5, 18, 9]
TEXTS = ["Testing.", "One more."]


def plain_batch(tts):
    """The default call's waveforms (greedy decoding: the same ids every time); generated once per instance."""
    if not hasattr(tts, "_plain_batch"):
        tts._plain_batch = [w.copy() for w in tts.infer_batch(TEXTS, REF_CODES, "So I'm live.")]
    return tts._plain_batch


class StubWatermarker:
    """A host library between the codec and the output: must see the 24 kHz float32 waveform; what it returns is what gets converted."""

    def __init__(self):
        self.seen = []

    def apply_watermark(self, wav, sample_rate):
        self.seen.append((wav.dtype, wav.ndim, sample_rate, len(wav)))
        return (0.5 * wav).astype(np.float32)


def test_class_infer_batch_in_a_telephony_format(tts):
    assert tts.sample_rate == 24000 and tts.output_sample_rate == 24000 and tts.output_encoding == "f32" and tts.output_filter_width == 6
    plain = plain_batch(tts)
    got = tts.infer_batch(TEXTS, REF_CODES, "So I'm live.", sample_rate=8000, encoding="mulaw")
    want = tts.codec.engine.convert(plain, sample_rate=8000, encoding="mulaw")
    for p, g, w in zip(plain, got, want):
        assert p.dtype == np.float32 and len(p) % tts.hop_length == 0 and len(p) > 0
        assert g.dtype == np.uint8 and len(g) == -(-len(p) // 3)
        assert np.array_equal(g, w)
    one = tts.infer(TEXTS[0], REF_CODES, "So I'm live.", sample_rate=8000, encoding="mulaw")
    assert np.array_equal(one, got[0])


def test_class_defaults_and_per_call_overrides(tts):
    codes = [[1, 2, 3, 4, 5], [9, 8]]
    native = tts.decode_codes(codes)
    try:
        tts.output_sample_rate, tts.output_encoding, tts.output_filter_width = 16000, "pcm16", 16
        a = tts.decode_codes(codes)                                          # the instance's format
        b = tts.decode_codes(codes, sample_rate=48000)                       # the rate overridden, the encoding kept
        c = tts.decode_codes(codes, sample_rate=24000, encoding="f32")       # back to the native format for one call
        wav = tts.infer(TEXTS[0], REF_CODES, "So I'm live.")
    finally:
        tts.output_sample_rate, tts.output_encoding, tts.output_filter_width = 24000, "f32", 6
    eng = tts.codec.engine
    for n, x, y, z, w in zip(native, a, b, c, codes):
        assert np.array_equal(x, eng.convert([n], sample_rate=16000, encoding="pcm16", filter_width=16)[0])
        assert not np.array_equal(x, eng.convert([n], sample_rate=16000, encoding="pcm16", filter_width=6)[0])
        assert y.dtype == np.int16 and len(y) == 2 * len(n)
        assert np.array_equal(y, eng.convert([n], sample_rate=48000, encoding="pcm16", filter_width=16)[0])
        assert z.dtype == np.float32 and np.array_equal(z, n)
    assert wav.dtype == np.int16 and len(wav) > 0
    for kw, word in ((dict(sample_rate=12000), "12000"), (dict(encoding="pcm8"), "pcm8")):
        with pytest.raises(ValueError, match=word):
            tts.decode_codes(codes, **kw)
        with pytest.raises(ValueError, match=word):
            tts.infer(TEXTS[0], REF_CODES, "So I'm live.", **kw)
    from neutts import NeuTTS
    for kw, word in ((dict(output_sample_rate=12000), "12000"), (dict(output_encoding="wav"), "wav"), (dict(output_filter_width=0), "output_filter_width")):
        with pytest.raises(ValueError, match=word):              # checked ahead of any loading
            NeuTTS(backbone_repo=None, codec_repo=None, **kw)


def test_class_streams_take_the_native_format_only(tts):
    for kw, word in ((dict(sample_rate=8000), "sample_rate=8000"), (dict(encoding="pcm16"), "encoding='pcm16'")):
        with pytest.raises(ValueError, match=word):
            tts.infer_stream("Streaming.", REF_CODES, "So I'm live.", **kw)          # at the call, before a generator exists
        with pytest.raises(ValueError, match=word):
            tts.infer_stream_batch(["Streaming."], REF_CODES, "So I'm live.", **kw)
    try:
        tts.output_encoding = "mulaw"
        with pytest.raises(ValueError, match="encoding='mulaw'"):
            tts.infer_stream("Streaming.", REF_CODES, "So I'm live.")
    finally:
        tts.output_encoding = "f32"
    gen = tts.infer_stream("Streaming.", REF_CODES, "So I'm live.", sample_rate=24000, encoding="f32")     # the native format, spelled out
    gen.close()


def test_class_watermarker_sees_24khz_float_and_its_output_is_converted(tts):
    plain = plain_batch(tts)
    stub = StubWatermarker()
    tts.watermarker = stub
    try:
        got = tts.infer_batch(TEXTS, REF_CODES, "So I'm live.", sample_rate=16000, encoding="pcm16")
        one = tts.infer(TEXTS[1], REF_CODES, "So I'm live.", sample_rate=16000, encoding="pcm16")
    finally:
        tts.watermarker = None
    assert stub.seen == [(np.dtype(np.float32), 1, 24000, len(p)) for p in plain] + [(np.dtype(np.float32), 1, 24000, len(plain[1]))]
    want = tts.codec.engine.convert([(0.5 * p).astype(np.float32) for p in plain], sample_rate=16000, encoding="pcm16")
    for g, w in zip(got, want):
        assert g.dtype == np.int16 and np.array_equal(g, w)
    assert np.array_equal(one, want[1])
