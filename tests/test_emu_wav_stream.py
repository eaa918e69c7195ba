"""The codec's output stage on signals that arrive in CHUNKS (include/neutts_hip.h ntts_wav_stream_*, ntts_streams_set_format /
ntts_streams_pump_end_fmt; kernels/codec.h wav_stream_kernel) on the CPU SIMT emulator: the kernel alone through WavStream against the one-shot
stage (bit for bit: the same dot products) and against tests/wav_format_spec.py / tests/wav_stream_spec.py, then the stream set and the NeuTTS class (stream_sample_rate= /
stream_encoding= / stream_filter_width=).  tests/test_gpu_wav_stream.py runs the same bodies on libneutts_hip.so."""
import ctypes as C

import numpy as np
import pytest

from neutts import _hip
from common import load_codec_fixture, make_codec_engine
import test_emu_neutts_class as class_cases
import test_emu_wav_format as fmt_cases
import wav_format_spec as spec
import wav_stream_spec as sspec

EINVAL, ESTATE = -1, -4
CASES = fmt_cases.CASES + [(22050, 64), (8000, 64)]          # ... and the longest histories: 390 samples at 8 kHz, the widest lag at 22.05 kHz
ONE_BY_ONE = [(8000, 6), (44100, 6)]                         # one sample per push: a down- and an up-sampler (bounded: a push is a launch)
ENCODINGS = ("f32", "pcm16", "mulaw")
SCRATCH = fmt_cases.SCRATCH
N_RAND = 1500

_ref = {}


def signals():
    """name -> float32 signal: ~1500 uniform samples in [-1, 1], and the two rows of edge values of the one-shot tests; computed once."""
    if "sig" not in _ref:
        x, n = fmt_cases._edge_input()
        sig = {"random": np.random.default_rng(2025).uniform(-1.0, 1.0, N_RAND).astype(np.float32),
               "edge": x[0, : n[0]].copy(), "saturating": x[1, : n[1]].copy()}
        for v in sig.values():
            v.setflags(write=False)
        _ref["sig"] = sig
    return _ref["sig"]


def one_shot(eng, name, rate, W, enc):
    """ntts_codec_convert of the whole signal: what the concatenated chunks must equal; computed once per engine and case."""
    key = (id(eng), name, rate, W, enc)
    if key not in _ref:
        _ref[key] = eng.convert([signals()[name]], sample_rate=rate, encoding=enc, filter_width=W)[0].copy()
    return _ref[key]


def spec_f64(name, rate, W):
    if (name, rate, W) not in _ref:
        _ref[name, rate, W] = spec.resample(signals()[name], rate, W)
    return _ref[name, rate, W]


def pieces(n, sizes):
    """[(start, stop)] of a signal of n samples cut by `sizes`; what is left over is one more piece."""
    out, i = [], 0
    for s in sizes:
        out.append((i, min(n, i + s)))
        i = min(n, i + s)
    if i < n:
        out.append((i, n))
    return out


def chunkings(n, rate, W):
    orig, new, width, taps, _ = spec.geometry(rate, W) if rate != spec.NATIVE_RATE else (1, 1, 0, 1, 0)
    per_block = -(-256 * orig // new)                        # input samples behind 256 output samples: one workgroup's worth
    return {
        "all in one push": [n],
        "shorter than width": [max(1, width - 1)] * 12,
        "exactly orig": [orig] * 30,
        "a 256-output block boundary inside a chunk": [per_block // 3, per_block + per_block // 2],
        "zero-length pushes in the middle": [n // 5, 0, 0, n // 3, 0],
        "a final push of nothing": [n // 2, n - n // 2, 0],
    }


def stream_count(eng, fc, n, last):
    m = C.c_int64(-1)
    assert eng.lib.ntts_wav_stream_count(C.byref(fc), n, int(last), C.byref(m)) == 0
    return m.value


def run(ws, x, cuts, stream=0):
    """Push the pieces of x one after the other (the final one with `last`) -> the chunks that came back."""
    outs = []
    for k, (a, b) in enumerate(cuts):
        outs.append(ws.push([x[a:b]], [stream], last=(k == len(cuts) - 1))[0])
    return outs


@pytest.fixture(scope="module")
def eng(emu_lib):
    z, cfg, w = load_codec_fixture("codec_tiny")
    e = make_codec_engine(cfg, w, emu_lib)            # hop 24, max_frames 64: the one-shot stage takes up to 1536 samples per utterance
    e._fixture, e._on_gpu = z, False
    return e


@pytest.fixture(scope="module")
def tts(emu_lib):
    return class_cases.build_tts(emu_lib)


# ---------------------------------------------------------------------------------------------- a. the kernel alone, through WavStream
@pytest.mark.parametrize("rate,W", CASES)
def test_chunks_equal_the_one_shot_stage_bit_for_bit(eng, rate, W):
    """Every chunking, every encoding, every signal: np.array_equal with ntts_codec_convert of the whole signal (no tolerance: the same table, the
    same operands, the same fmaf chain); per-push lengths as the spec and ntts_wav_stream_count say; the f32 output inside the project's own
    fp32 bound of the float64 spec; PCM16 and mu-law exact functions of the f32 chunks."""
    for name, x in signals().items():
        n = len(x)
        bound = spec.error_bound(rate, W, float(np.abs(x).max()))        # (taps + 2) 2^-24 max_p sum_j |h[p][j]| max|x|; max|x| <= 1 for the random signal
        for enc in ENCODINGS:
            want = one_shot(eng, name, rate, W, enc)
            fc = _hip.wav_format(rate, enc, W)[0]
            ws = eng.stream_converter(1, rate, enc, W, max_chunk_samples=n)
            for what, sizes in chunkings(n, rate, W).items():
                cuts = pieces(n, sizes)
                outs = run(ws, x, cuts)                      # (the same converter again and again: a stream is empty after `last`)
                got = np.concatenate(outs)
                assert got.dtype == want.dtype == spec.ENCODINGS[enc]
                assert np.array_equal(got, want), f"{name} {enc} {rate} W {W}: {what}"
                ends = [b for _, b in cuts]
                count = [sspec.stream_out_count(b, rate, W, last=(k == len(ends) - 1)) for k, b in enumerate(ends)]
                assert [len(o) for o in outs] == np.diff([0] + count).tolist(), what
                assert count == [stream_count(eng, fc, b, k == len(ends) - 1) for k, b in enumerate(ends)] == \
                       [ws.out_count(b, k == len(ends) - 1) for k, b in enumerate(ends)]
            ws.close()
        f32 = one_shot(eng, name, rate, W, "f32")
        worst = float(np.abs(f32.astype(np.float64) - spec_f64(name, rate, W)).max())
        print(f"{name} rate {rate} W {W}: max |chunks - spec| {worst:.2e}, bound {bound:.2e}")
        assert worst <= bound
        assert np.array_equal(one_shot(eng, name, rate, W, "pcm16"), spec.pcm16(f32))
        assert np.array_equal(one_shot(eng, name, rate, W, "mulaw"), spec.mulaw(spec.pcm16(f32)))


@pytest.mark.parametrize("rate,W", ONE_BY_ONE)
def test_one_sample_per_push(eng, rate, W):
    x = signals()["random"]
    for enc in ENCODINGS:
        ws = eng.stream_converter(1, rate, enc, W, max_chunk_samples=4)
        outs = run(ws, x, [(i, i + 1) for i in range(len(x))])
        assert np.array_equal(np.concatenate(outs), one_shot(eng, "random", rate, W, enc))
        count = [sspec.stream_out_count(i + 1, rate, W, last=(i == len(x) - 1)) for i in range(len(x))]
        assert [len(o) for o in outs] == np.diff([0] + count).tolist()
        ws.close()


@pytest.mark.parametrize("rate,W,enc", [(8000, 16, "mulaw"), (44100, 6, "f32"), (24000, 6, "pcm16"), (22050, 64, "pcm16")])
def test_three_streams_in_one_call_at_different_phases(eng, rate, W, enc):
    """Every push serves three streams that stand at different places of signals of different lengths, in changing row order; behind every row's
    valid samples stands 1e30: read as signal, it shows."""
    sig = signals()
    names = ["random", "edge", "saturating"]
    sizes = [[211, 0, 500, 17, 772], [50, 60, 70, 80, 77], [1, 300, 2, 400, 74]]        # per stream; 1500, 337 and 777 samples
    cuts = [pieces(len(sig[nm]), sz) for nm, sz in zip(names, sizes)]
    assert all(len(c) == 5 for c in cuts)
    ws = eng.stream_converter(3, rate, enc, W, max_chunk_samples=800)
    got = [[], [], []]
    for k in range(5):
        rows = np.full((3, 800), SCRATCH, dtype=np.float32)
        order = [2, 0, 1] if k % 2 else [0, 1, 2]                                          # (row i of a call is not stream i)
        for r, u in enumerate(order):
            a, b = cuts[u][k]
            rows[r, : b - a] = sig[names[u]][a:b]
        out, lens = ws.push_array(order, rows, [cuts[u][k][1] - cuts[u][k][0] for u in order], [k == 4] * 3)
        for r, u in enumerate(order):
            got[u].append(out[r, : lens[r]].copy())
    for u, nm in enumerate(names):
        y = np.concatenate(got[u])
        assert np.isfinite(y.astype(np.float64)).all()
        assert np.array_equal(y, one_shot(eng, nm, rate, W, enc)), f"stream {u}"
    # every stream is empty again: stream 1 takes the signal stream 0 had
    again = run(ws, sig["random"], pieces(N_RAND, [700, 1, 799]), stream=1)
    assert np.array_equal(np.concatenate(again), one_shot(eng, "random", rate, W, enc))
    ws.close()


def _i32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def raw_push(ws, streams, x, n_samples, last, out_stride):
    st, ns, la = (np.ascontiguousarray(v, dtype=np.int32) for v in (streams, n_samples, last))
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.zeros((len(st), max(1, out_stride)), dtype=ws.dtype)
    lens = np.full(len(st), -7, dtype=np.int32)
    rc = ws.lib.ntts_wav_stream_push(ws.h, len(st), _i32p(st), x.ctypes.data_as(C.POINTER(C.c_float)), x.shape[1], _i32p(ns), _i32p(la),
                                     C.c_void_p(out.ctypes.data), out_stride, _i32p(lens))
    return rc, out, lens, (ws.lib.ntts_wav_stream_last_error(ws.h) or b"").decode()


def test_refusals_name_the_problem_and_move_no_stream(eng):
    x = signals()["random"]
    want = one_shot(eng, "random", 8000, 6, "pcm16")
    ws = eng.stream_converter(2, 8000, "pcm16", 6, max_chunk_samples=600)
    first = ws.push([x[:500]], [1])[0]                       # stream 1 is in the middle of its signal while the refusals come
    rows = np.zeros((2, 700), dtype=np.float32)

    def refused(res, *words):
        rc, _, lens, msg = res
        assert rc == EINVAL and msg and lens.tolist() == [-7] * len(lens), (rc, msg)
        assert all(w in msg for w in words), msg

    refused(raw_push(ws, [0, 2], rows, [10, 10], [0, 0], 64), "stream 2")
    refused(raw_push(ws, [-1, 0], rows, [10, 10], [0, 0], 64), "stream -1")
    refused(raw_push(ws, [1, 1], rows, [10, 10], [0, 0], 64), "stream 1", "twice")
    refused(raw_push(ws, [0, 1], rows, [10, -3], [0, 0], 64), "n_samples -3")
    refused(raw_push(ws, [0, 1], rows, [701, 10], [0, 0], 512), "n_samples 701")           # above in_stride
    refused(raw_push(ws, [0, 1], rows, [10, 601], [0, 0], 512), "n_samples 601", "600")    # above max_chunk_samples
    need = sspec.stream_out_count(1000, 8000, 6) - sspec.stream_out_count(500, 8000, 6)      # stream 1 with 500 more samples
    refused(raw_push(ws, [1, 0], rows, [500, 3], [0, 0], need - 1), "out_stride", str(need - 1))
    for bad, word in ((_hip.WavFormatC(12345, 0, 0), "12345"), (_hip.WavFormatC(8000, 3, 0), "encoding 3"), (_hip.WavFormatC(8000, 0, 65), "filter_width 65")):
        h = C.c_void_p()
        assert eng.lib.ntts_wav_stream_create(eng.h, C.byref(bad), 1, 100, C.byref(h)) == EINVAL
        assert word in (eng.lib.ntts_wav_stream_last_error(None) or b"").decode()
        m = C.c_int64()
        assert eng.lib.ntts_wav_stream_count(C.byref(bad), 10, 0, C.byref(m)) == EINVAL
        assert word in (eng.lib.ntts_wav_stream_last_error(None) or b"").decode()
    for kw, word in ((dict(sample_rate=11025), "11025"), (dict(encoding="alaw"), "alaw"), (dict(filter_width=65), "65")):
        with pytest.raises(ValueError, match=word):          # the Python layer refuses by name before the library is called
            eng.stream_converter(1, **kw)
    # nothing moved: stream 1 goes on where it was, to the right bits
    rest = [ws.push([x[500:1000]], [1])[0], ws.push([x[1000:]], [1], last=True)[0]]
    assert np.array_equal(np.concatenate([first] + rest), want)
    ws.close()


def test_the_native_format_is_a_copy_without_history(eng):
    x = signals()["edge"]
    ws = eng.stream_converter(1, 24000, "f32", 9, max_chunk_samples=len(x))
    assert ws.native
    outs = run(ws, x, pieces(len(x), [100, 0, 37]))
    assert [len(o) for o in outs] == [100, 0, 37, len(x) - 137] and np.array_equal(np.concatenate(outs), x)
    ws.close()


# ---------------------------------------------------------------------------------------------- b. the stream set and the class
REF_CODES = [3, 77, 200, 5, 18, 9, 100, 41]
TEXTS = ["Streaming test.", "Another one, a little longer."]
REF_TEXT = "So I'm live."
FORMATS = [(8000, "mulaw", None), (16000, "pcm16", None), (44100, "f32", None), (8000, "pcm16", 16)]


def on_emu(tts):
    return "emu" in str(tts._lib_path)


class stream_params:
    """The parameters of test_infer_stream_batch_equals_single_streams: one full window (30 tokens) plus a final partial one."""

    def __init__(self, tts):
        self.tts = tts

    def __enter__(self):
        self.tts.min_new_tokens, self.tts.max_context = 34, 150

    def __exit__(self, *exc):
        self.tts.min_new_tokens, self.tts.max_context = 5, 120
        self.tts.stream_on_device = True


def batch(tts, texts=TEXTS, **kw):
    got = [[] for _ in texts]
    for i, chunk in tts.infer_stream_batch(texts, REF_CODES, REF_TEXT, **kw):
        assert isinstance(chunk, np.ndarray)
        got[i].append(chunk)
    return got


def native_batch(tts):
    """The plain call's chunks per utterance (greedy decoding: the same ids every time), device path; generated once per instance."""
    if not hasattr(tts, "_native_stream_batch"):
        with stream_params(tts):
            tts._native_stream_batch = batch(tts)
    return tts._native_stream_batch


def one_shot_of(tts, chunks, rate, enc, W):
    """The one-shot stage on an utterance's concatenated native chunks; a WavStream given the whole signal in one `last` push where the signal is
    longer than ntts_codec_convert takes (max_frames x hop_length)."""
    eng = tts.codec.engine
    whole = np.concatenate(chunks)
    if len(whole) <= eng.max_frames * eng.hop_length:
        return eng.convert([whole], sample_rate=rate, encoding=enc, filter_width=W)[0]
    ws = eng.stream_converter(1, rate, enc, W, max_chunk_samples=len(whole))
    try:
        return ws.push([whole], last=True)[0].copy()
    finally:
        ws.close()


def check_against_native(tts, got, native, rate, enc, W):
    for g, p in zip(got, native):
        assert len(g) == len(p) >= 2 and all(c.dtype == spec.ENCODINGS[enc] for c in g)
        want = one_shot_of(tts, p, rate, enc, W)
        assert np.array_equal(np.concatenate(g), want)
        n_in = np.cumsum([len(c) for c in p])
        count = [sspec.stream_out_count(int(n), rate, W, last=(k == len(p) - 1)) for k, n in enumerate(n_in)]
        assert [len(c) for c in g] == np.diff([0] + count).tolist()


def kv_all_free(tts):
    st = tts.backbone.kv_stats()
    assert st["free_pages"] == st["total_pages"]


@pytest.mark.parametrize("rate,enc,W", FORMATS)
def test_stream_batch_in_a_format_equals_the_one_shot_stage_of_the_native_stream(tts, rate, enc, W):
    native = native_batch(tts)
    kw = dict(stream_sample_rate=rate, stream_encoding=enc)
    if W is not None:
        kw["stream_filter_width"] = W
    with stream_params(tts):
        assert tts._stream_on_device([REF_CODES, REF_CODES])
        got = batch(tts, **kw)                                # the device path: StreamSet(fmt=), the stage behind the cross-fade
        kv_all_free(tts)
    check_against_native(tts, got, native, rate, enc, W or tts.output_filter_width)
    if W is not None:                                         # the width matters: the default one gives other samples
        assert not np.array_equal(np.concatenate(got[0]), one_shot_of(tts, native[0], rate, enc, 6))


def same_chunks(a, b):
    return len(a) == len(b) and all(len(x) == len(y) and all(u.dtype == v.dtype and np.array_equal(u, v) for u, v in zip(x, y)) for x, y in zip(a, b))


def test_device_path_equals_host_loop_and_single_streams(tts):
    kw = dict(stream_sample_rate=8000, stream_encoding="mulaw")
    with stream_params(tts):
        dev = batch(tts, **kw)
        tts.stream_on_device = False                          # numpy windows + _StreamBlender, then a WavStream of one row per utterance
        host = batch(tts, **kw) if not on_emu(tts) else None  # (GPU only: time; the single streams below run the host loop on the emulator)
        singles = [list(tts.infer_stream(t, REF_CODES, REF_TEXT, **kw)) for t in TEXTS[: 1 if on_emu(tts) else 2]]
        tts.stream_on_device = True
        if not on_emu(tts):                                   # ... and a set of one stream on the device
            assert same_chunks(singles, [list(tts.infer_stream(t, REF_CODES, REF_TEXT, **kw)) for t in TEXTS])
        kv_all_free(tts)
    assert host is None or same_chunks(host, dev)
    assert same_chunks(singles, dev[: len(singles)])
    check_against_native(tts, dev, native_batch(tts), 8000, "mulaw", 6)


def test_the_native_format_spelled_out_is_the_plain_call(tts):
    native = native_batch(tts)
    kw = dict(stream_sample_rate=24000, stream_encoding="f32", stream_filter_width=16)
    with stream_params(tts):
        assert same_chunks(batch(tts, **kw), native)          # device path: a StreamSet without a format, plain pump_end
        tts.stream_on_device = False
        one = list(tts.infer_stream(TEXTS[0], REF_CODES, REF_TEXT, **kw))          # host loop: no converter
        assert same_chunks([one], native[:1])
        if not on_emu(tts):
            assert same_chunks(batch(tts, **kw), native)
        kv_all_free(tts)


def test_stream_batch_over_a_gang_in_a_format(tts):
    """As test_infer_stream_batch_over_a_gang_with_staggered_admission: groups of one over two engines, one formatted stream set per group."""
    texts = TEXTS + ["Third."]
    kw = dict(stream_sample_rate=16000, stream_encoding="pcm16")
    tts.gang = _hip.EngineGang(tts.backbone, 2)
    tts.stream_admit = 1
    tts.stream_on_gang = True
    try:
        with stream_params(tts):
            got = batch(tts, texts, **kw)
            assert len(tts._gang_codecs) == 2
            for e in tts.gang.engines:
                st = e.kv_stats()
                assert st["free_pages"] == st["total_pages"] and e.free_slots() == e.max_batch
            if not on_emu(tts):
                assert same_chunks(batch(tts, texts, stream_sample_rate=24000, stream_encoding="f32"), batch(tts, texts))
    finally:
        del tts.stream_admit, tts.stream_on_gang
        for k, c in enumerate(tts._gang_codecs or []):
            c.set_stream(None)
            if k:
                c.close()
        tts._gang_codecs = None
        tts.gang.close()
        tts.gang = None
    native = native_batch(tts)                                # (one engine, device path: a window is defined by token counts, not by the engine)
    check_against_native(tts, got[:2], native, 16000, "pcm16", 6)
    with stream_params(tts):
        third = list(tts.infer_stream(texts[2], REF_CODES, REF_TEXT, **kw))
    assert same_chunks([third], got[2:])


def test_watermarker_sees_24khz_float_windows_and_its_output_is_converted(tts):
    stub, plain = fmt_cases.StubWatermarker(), fmt_cases.StubWatermarker()
    try:
        with stream_params(tts):
            tts.watermarker = plain
            marked = [list(tts.infer_stream(TEXTS[0], REF_CODES, REF_TEXT))]           # the stubbed native stream (host loop: a watermarker is a host library)
            tts.watermarker = stub
            got = [list(tts.infer_stream(TEXTS[0], REF_CODES, REF_TEXT, stream_sample_rate=16000, stream_encoding="pcm16"))]
            if not on_emu(tts):
                assert same_chunks(batch(tts, TEXTS[:1], stream_sample_rate=16000, stream_encoding="pcm16"), got)
    finally:
        tts.watermarker = None
    assert stub.seen[: len(plain.seen)] == plain.seen and all(s[0] == np.dtype(np.float32) and s[1] == 1 and s[2] == 24000 for s in stub.seen)
    check_against_native(tts, got, marked, 16000, "pcm16", 6)
    assert not same_chunks(marked, native_batch(tts)[:1])     # (the stub did change the stream)


def test_constructor_defaults_and_per_call_keywords(tts):
    assert (tts.sample_rate, tts.stream_sample_rate, tts.stream_encoding, tts.stream_filter_width) == (24000, 24000, "f32", None)
    native = native_batch(tts)
    try:
        tts.stream_sample_rate, tts.stream_encoding, tts.stream_filter_width = 8000, "mulaw", 16
        tts.output_sample_rate = 24000
        with stream_params(tts):
            a = batch(tts, TEXTS[:1])                                              # the instance's format
            b = batch(tts, TEXTS[:1], stream_encoding="pcm16", stream_filter_width=6)      # two of the three overridden for one call
            c = batch(tts, TEXTS[:1], stream_sample_rate=24000, stream_encoding="f32")     # back to the native format for one call
            assert tts.sample_rate == 24000 and tts.stream_sample_rate == 8000
    finally:
        tts.stream_sample_rate, tts.stream_encoding, tts.stream_filter_width = 24000, "f32", None
    check_against_native(tts, a, native[:1], 8000, "mulaw", 16)
    check_against_native(tts, b, native[:1], 8000, "pcm16", 6)
    assert same_chunks(c, native[:1])
    for kw, word in ((dict(stream_sample_rate=11025), "11025"), (dict(stream_encoding="alaw"), "alaw"), (dict(stream_filter_width=0), "stream_filter_width"),
                     (dict(stream_filter_width=65), "65"), (dict(stream_sample_rate=8000.0), "8000.0")):
        with pytest.raises(ValueError, match=word):
            tts.infer_stream("Streaming.", REF_CODES, REF_TEXT, **kw)              # at the call, before a generator exists
        with pytest.raises(ValueError, match=word):
            tts.infer_stream_batch(["Streaming."], REF_CODES, REF_TEXT, **kw)
    with pytest.raises(ValueError, match="stream_sample_rate="):                    # the one-shot keywords stay refused, and say where to go
        tts.infer_stream("Streaming.", REF_CODES, REF_TEXT, sample_rate=8000)
    from neutts import NeuTTS
    for kw, word in ((dict(stream_sample_rate=12000), "12000"), (dict(stream_encoding="wav"), "wav"), (dict(stream_filter_width=0), "stream_filter_width")):
        with pytest.raises(ValueError, match=word):                                # checked ahead of any loading
            NeuTTS(backbone_repo=None, codec_repo=None, **kw)
    kv_all_free(tts)


def test_a_stream_that_ends_on_a_window_edge_is_flushed(tts):
    """Toy parameters (lookforward 0, overlap 0) and exactly two windows of tokens: no final window exists, so the held-back outputs come as one
    more chunk, `last`, of a few samples -- on the device path, in the batch host loop and in the single-stream host loop alike."""
    prompt = tts._apply_chat_template(REF_CODES, REF_TEXT, TEXTS[0])
    fmt = (8000, "mulaw", 6)
    look_f, ovl = tts.streaming_lookforward, tts.streaming_overlap_frames
    tts.streaming_lookforward = tts.streaming_overlap_frames = 0
    tts.min_new_tokens, tts.max_context = 50, len(prompt) + 50
    try:
        assert tts._stream_on_device([REF_CODES])
        native = [c for _, c in tts._infer_stream_batch_hip([prompt], [REF_CODES], None, None)]
        dev = [c for _, c in tts._infer_stream_batch_hip([prompt], [REF_CODES], None, fmt)]
        tts.stream_on_device = False
        host = [c for _, c in tts._infer_stream_batch_hip([prompt], [REF_CODES], None, fmt)]           # (the batch host loop's only run on the emulator)
        one = list(tts._infer_stream_hip(prompt, REF_CODES, None, fmt))
        kv_all_free(tts)
    finally:
        tts.stream_on_device = True
        tts.streaming_lookforward, tts.streaming_overlap_frames = look_f, ovl
        tts.min_new_tokens, tts.max_context = 5, 120
    stride = tts.streaming_stride_samples
    assert [len(c) for c in native] == [stride, stride]                          # two regular windows, no final one
    count = [sspec.stream_out_count(stride, 8000, 6), sspec.stream_out_count(2 * stride, 8000, 6), spec.out_len(2 * stride, 8000)]
    assert [len(c) for c in dev] == np.diff([0] + count).tolist() and len(dev[2]) > 0
    assert np.array_equal(np.concatenate(dev), one_shot_of(tts, native, *fmt))
    assert same_chunks([host], [dev]) and same_chunks([one], [dev])


def test_stream_set_abi_set_format_and_plain_pump_end(tts):
    """ntts_streams_set_format after a pump has begun and plain ntts_streams_pump_end on a formatted set are NTTS_ESTATE; a bad format is
    NTTS_EINVAL and names its value."""
    eng, cod = tts.backbone, tts.codec.engine
    prompt = tts._apply_chat_template(REF_CODES, REF_TEXT, "Testing.")
    slot = eng.acquire_slot()
    try:
        eng.prefill([prompt], [slot], [tts._sampling(len(prompt), 0)])
        ss = _hip.StreamSet(eng, cod, [slot], [REF_CODES], int(eng.cfg["max_context"]), 25, 5, 50, 1, tts.hop_length, int(tts._speech_base), 65536,
                            fmt=(8000, "mulaw", 6))
        try:
            lib, i32p = ss.lib, C.POINTER(C.c_int32)
            assert lib.ntts_streams_set_format(ss.h, C.byref(_hip.WavFormatC(8001, 0, 0))) == EINVAL
            assert "8001" in (lib.ntts_streams_last_error(ss.h) or b"").decode()
            assert lib.ntts_streams_set_format(ss.h, C.byref(_hip.WavFormatC(16000, 1, 0))) == 0      # still before the first pump
            assert lib.ntts_streams_set_format(ss.h, C.byref(_hip.WavFormatC(8000, 2, 6))) == 0
            ss.pump_begin()
            assert lib.ntts_streams_set_format(ss.h, C.byref(_hip.WavFormatC(16000, 1, 0))) == ESTATE
            assert lib.ntts_streams_set_format(ss.h, None) == ESTATE
            n, run, more = C.c_int32(), C.c_int32(), C.c_int32()
            ptr, stride = C.POINTER(C.c_float)(), C.c_int64()
            rc = lib.ntts_streams_pump_end(ss.h, 2, C.byref(n), ss._cs.ctypes.data_as(i32p), ss._cn.ctypes.data_as(i32p), ss._cl.ctypes.data_as(i32p),
                                           C.byref(ptr), C.byref(stride), C.byref(run), C.byref(more))
            assert rc == ESTATE and "pump_end_fmt" in (lib.ntts_streams_last_error(ss.h) or b"").decode()
            chunks, _, _ = ss.pump_end()                      # the formatted call goes through (nothing is decodable yet)
            assert chunks == []
        finally:
            ss.close()
    finally:
        eng.sync()
        eng.release(slot)
    kv_all_free(tts)
