"""stream_speed=: the codec's time stretch on signals that arrive in CHUNKS (include/neutts_hip.h ntts_speed_stream_*, ntts_streams_set_speed;
kernels/codec.h wav_stretch_stream_kernel) on the CPU SIMT emulator: the kernel alone through SpeedStream against the one-shot stage (bit for bit:
the same operands, the same fma) and against tests/time_stretch_spec.py / tests/stream_speed_spec.py, then the stream set and the NeuTTS class.
tests/test_gpu_stream_speed.py runs the same bodies on libneutts_hip.so."""
import ctypes as C

import numpy as np
import pytest

from neutts import _hip
from common import load_codec_fixture, make_codec_engine
import test_emu_neutts_class as class_cases
import test_emu_wav_format as fmt_cases
import test_emu_wav_stream as wcases
import stream_speed_spec as sspec
import time_stretch_spec as spec

EINVAL, ESTATE = -1, -4
SPEEDS = (0.5, 0.667, 0.8, 0.999, 1.001, 1.25, 2.0)
EDGE_LENGTHS = (0, 1, 359, 719, 720, 959, 960, 961)      # where the emit rule flips: under a frame, under / at L, under / at / over DELTA + L
LENGTHS = EDGE_LENGTHS + (5000, 26000)                   # ... many frames, and three of the stream's own 12 000-sample chunks
MAX_CHUNK = 12000
FORMATS = [(8000, "mulaw", 16), (16000, "pcm16", 6)]

_ref = {}


def signal(n):
    """A three-harmonic 137 Hz tone plus seeded noise; computed once per length."""
    if ("sig", n) not in _ref:
        t = np.arange(n, dtype=np.float64) / 24000.0
        tone = 0.4 * np.sin(2 * np.pi * 137 * t) + 0.2 * np.sin(2 * np.pi * 274 * t) + 0.1 * np.sin(2 * np.pi * 411 * t)
        x = (tone + 0.05 * np.random.default_rng(n).standard_normal(n)).astype(np.float32)
        x.setflags(write=False)
        _ref["sig", n] = x
    return _ref["sig", n]


def one_shot(eng, n, pm, fmt=None):
    """ntts_codec_stretch of the whole signal: (samples, positions) the concatenated chunks must equal; computed once per engine and case."""
    key = (id(eng), n, pm, fmt)
    if key not in _ref:
        kw = {} if fmt is None else dict(sample_rate=fmt[0], encoding=fmt[1], filter_width=fmt[2])
        out, lens, pos, frames = eng.stretch_array(signal(n)[None, :] if n else np.zeros((1, 1), np.float32), [n], pm / 1000.0, **kw)
        _ref[key] = (out[0, : lens[0]].copy(), pos[0, : frames[0]].copy())
    return _ref[key]


def spec_result(n, pm):
    if ("spec", n, pm) not in _ref:
        _ref["spec", n, pm] = spec.stretch(signal(n), pm)
    return _ref["spec", n, pm]


def cuts(n, kind, seed=0):
    """[(start, stop)] of a signal of n samples: chunks of `kind` samples, or seeded random cuts; at least one piece."""
    if kind == "random":
        edges = np.unique(np.random.default_rng(seed).integers(0, n + 1, size=min(10, n + 1))).tolist() if n else []
    else:
        edges = list(range(kind, n, kind))
    edges = [0] + [e for e in edges if 0 < e < n] + [n]
    return list(zip(edges[:-1], edges[1:]))


def run(ss, x, pieces, pm, stream=0, flush=False):
    """Push the pieces of x one after the other (the final one with `last`; with `flush` an empty push behind them is the last) -> (chunks,
    positions) per push."""
    pieces = list(pieces) + ([(len(x), len(x))] if flush else [])
    outs, poss = [], []
    for k, (a, b) in enumerate(pieces):
        row = np.zeros((1, max(1, b - a)), dtype=np.float32)
        row[0, : b - a] = x[a:b]
        out, out_lens, pos, n_pos = ss.push_array([stream], row, [b - a], [k == len(pieces) - 1], [pm])
        outs.append(out[0, : out_lens[0]].copy())
        poss.append(pos[0, : n_pos[0]].copy())
    return outs, poss


def stream_count(eng, pm, n, last):
    m = C.c_int64(-1)
    assert eng.lib.ntts_speed_stream_count(pm, n, int(last), C.byref(m)) == 0
    return m.value


@pytest.fixture(scope="module")
def eng(emu_lib):
    z, cfg, w = load_codec_fixture("codec_tiny")
    e = make_codec_engine(cfg, w, emu_lib, max_frames=1088, max_rows=1152)       # hop 24: the one-shot stage takes the 26 000-sample signal
    e._fixture, e._on_gpu = z, False
    return e


@pytest.fixture(scope="module")
def tts(emu_lib):
    return class_cases.build_tts(emu_lib, max_batch=4)


# ---------------------------------------------------------------------------------------------- a. the kernel alone, through SpeedStream
@pytest.mark.parametrize("speed", SPEEDS)
def test_chunks_equal_the_one_shot_stage_bit_for_bit(eng, speed):
    """Every length, every chunking, with and without an empty last push: the concatenated f32 chunks are np.array_equal to ntts_codec_stretch of the
    whole signal (engine against engine: no tolerance), the positions np.array_equal to time_stretch_spec.positions, the samples inside
    time_stretch_spec.error_bound of the float64 spec and exact on continuation frames; per-push lengths as stream_speed_spec and
    ntts_speed_stream_count say."""
    pm = spec.permille(speed)
    ss = eng.stream_stretcher(1, speed, max_chunk_samples=MAX_CHUNK)
    worst = 0.0
    for n in LENGTHS:
        x = signal(n)
        want, want_pos = one_shot(eng, n, pm)
        ref, ref_pos = spec_result(n, pm)
        assert np.array_equal(want_pos, ref_pos) and len(want) == len(ref) == spec.out_len(n, pm)
        bound = spec.error_bound(float(np.abs(x).max())) if n else 0.0
        for kind in (MAX_CHUNK, 480, "random"):
            for flush in (False, True):
                pieces = cuts(n, kind, seed=pm + n)
                outs, poss = run(ss, x, pieces, pm, flush=flush)          # (the same stretcher again and again: a stream is empty after `last`)
                what = f"speed {pm}, {n} samples, chunks {kind}, flush {flush}"
                got, got_pos = np.concatenate(outs), np.concatenate(poss)
                assert got.dtype == np.float32 and got_pos.dtype == np.int32
                assert np.array_equal(got_pos, ref_pos), what
                assert np.array_equal(got, want), what
                ends = [b for _, b in pieces] + ([n] if flush else [])
                count = [sspec.stream_out_count(b, pm, last=(k == len(ends) - 1)) for k, b in enumerate(ends)]
                assert count == [stream_count(eng, pm, b, k == len(ends) - 1) for k, b in enumerate(ends)]
                assert [len(o) for o in outs] == np.diff([0] + count).tolist(), what
                if n:
                    err = float(np.abs(got.astype(np.float64) - ref).max())
                    worst = max(worst, err / bound)
                    assert err <= bound, f"{what}: {err:.3e} > {bound:.3e}"
                    keep = spec.continuation_mask(ref_pos, len(ref))
                    src = spec.source_index(ref_pos, len(ref))
                    xin = np.concatenate([x, np.zeros(int(src.max()) + 1, dtype=np.float32)])
                    assert np.array_equal(got[keep], xin[src[keep]]), what
    print(f"speed {pm}: max |engine - spec| / bound {worst:.3f}")
    ss.close()


def test_one_sample_per_push(eng):
    n, pm = 1500, 800
    x = signal(n)
    ss = eng.stream_stretcher(1, 0.8, max_chunk_samples=4)
    outs, poss = run(ss, x, [(i, i + 1) for i in range(n)], pm)
    want, want_pos = one_shot(eng, n, pm)
    assert np.array_equal(np.concatenate(outs), want) and np.array_equal(np.concatenate(poss), want_pos)
    assert [len(o) for o in outs[:959]] == [0] * 959 and len(outs[959]) == spec.HS        # frame 0 with the 960th sample
    ss.close()


def test_three_streams_in_one_call_at_different_speeds_and_phases(eng):
    """Three streams pushed together, their chunk edges at different places, one of them at 1.0: that one's chunks are its input bit for bit, with no
    lag; the others equal their one-shot stretch."""
    n, pms = 5000, (800, 1000, 1500)
    x = signal(n)
    ss = eng.stream_stretcher(3, [pm / 1000.0 for pm in pms], max_chunk_samples=2000)
    edges = [[0, 1200, 2400, 3600, n], [0, 700, 2000, 3100, n], [0, 1999, 2001, 4000, n]]
    got = [[] for _ in pms]
    for k in range(4):
        chunks = [x[e[k]: e[k + 1]] for e in edges]
        outs = ss.push(chunks, last=(k == 3))
        for u, o in enumerate(outs):
            got[u].append(o.copy())
        assert np.array_equal(outs[1], chunks[1])                        # the stream at 1.0: the chunk itself
    for u, pm in enumerate(pms):
        assert np.array_equal(np.concatenate(got[u]), one_shot(eng, n, pm)[0]), f"stream {u} at {pm}"
    ss.close()


@pytest.mark.parametrize("rate,enc,W", FORMATS)
def test_with_a_format_behind_the_stretch(eng, rate, enc, W):
    n = 5000
    x = signal(n)
    for speed in (0.8, 1.25, 1.0):
        pm = spec.permille(speed)
        want = one_shot(eng, n, pm, (rate, enc, W))[0]
        ss = eng.stream_stretcher(1, speed, rate, enc, W, max_chunk_samples=MAX_CHUNK)
        for kind, flush in ((480, False), ("random", True)):
            pieces = cuts(n, kind, seed=rate) + ([(n, n)] if flush else [])
            outs = [ss.push([x[a:b]], last=(k == len(pieces) - 1))[0].copy() for k, (a, b) in enumerate(pieces)]
            got = np.concatenate(outs)
            assert got.dtype == want.dtype and np.array_equal(got, want), f"speed {speed}, {rate} Hz {enc}, chunks {kind}"
        ss.close()


def test_refusals_name_the_problem_and_move_no_stream(eng):
    n = 3000
    x = signal(n)
    ss = eng.stream_stretcher(2, 0.8, max_chunk_samples=1600)
    first = ss.push([x[:1500]], [0])[0].copy()
    lib, i32p, f32p = eng.lib, C.POINTER(C.c_int32), C.POINTER(C.c_float)

    def push(streams, pms, lens, out_stride=4000, in_stride=1600):
        st, pm, ns = (np.ascontiguousarray(v, dtype=np.int32) for v in (streams, pms, lens))
        la = np.zeros(len(st), dtype=np.int32)
        wav = np.zeros((len(st), in_stride), dtype=np.float32)
        out = np.zeros((len(st), max(1, out_stride)), dtype=np.float32)
        out_lens = np.zeros(len(st), dtype=np.int32)
        rc = lib.ntts_speed_stream_push(ss.h, len(st), st.ctypes.data_as(i32p), pm.ctypes.data_as(i32p), wav.ctypes.data_as(f32p), in_stride,
                                        ns.ctypes.data_as(i32p), la.ctypes.data_as(i32p), C.c_void_p(out.ctypes.data), out_stride,
                                        out_lens.ctypes.data_as(i32p), None, 0, None)
        return rc, (lib.ntts_speed_stream_last_error(ss.h) or b"").decode()

    for args, word in ((([0], [499], [10]), "499"), (([0], [2001], [10]), "2001"),             # a speed out of range
                       (([0], [1250], [10]), "began at 800"),                                   # a speed changed in the middle of a signal
                       (([1, 1], [800, 800], [10, 10]), "twice"),                               # a stream named twice
                       (([0], [800], [1601], 4000, 1700), "max_chunk_samples"),                 # n_samples above the cap
                       (([0], [800], [1500], 100), "out_stride"),                               # out_stride too small for what the chunk emits
                       (([2], [800], [10]), "stream 2")):
        rc, msg = push(*args)
        assert rc == EINVAL and word in msg, (args, msg)
    m = C.c_int64()
    assert lib.ntts_speed_stream_count(499, 100, 0, C.byref(m)) == EINVAL and "499" in (lib.ntts_speed_stream_last_error(None) or b"").decode()
    rest = ss.push([x[1500:]], [0], last=True)[0]                        # no stream moved: the signal goes on where it was
    assert np.array_equal(np.concatenate([first, rest]), one_shot(eng, n, 800)[0])
    with pytest.raises(ValueError, match="speed"):
        eng.stream_stretcher(1, 2.5)
    ss.close()


def test_after_its_last_chunk_a_stream_starts_a_new_signal_at_another_speed(eng):
    ss = eng.stream_stretcher(1, 0.8, max_chunk_samples=MAX_CHUNK)
    x, y = signal(5000), signal(961)
    a = [ss.push([x[:2600]])[0].copy(), ss.push([x[2600:]], last=True)[0].copy()]
    b = [ss.push([y[:500]], speed=1.5)[0].copy(), ss.push([y[500:]], last=True, speed=1.5)[0].copy()]
    c = [ss.push([x[:100]], speed=1.0)[0].copy(), ss.push([x[100:5000]], last=True, speed=1.0)[0].copy()]
    assert np.array_equal(np.concatenate(a), one_shot(eng, 5000, 800)[0])
    assert np.array_equal(np.concatenate(b), one_shot(eng, 961, 1500)[0])
    assert np.array_equal(np.concatenate(c), x) and len(c[0]) == 100
    ss.close()


# ---------------------------------------------------------------------------------------------- b. the stream set and the class
REF_CODES, TEXTS, REF_TEXT = wcases.REF_CODES, wcases.TEXTS, wcases.REF_TEXT
THREE = TEXTS + ["Third."]
THREE_SPEEDS = [1.0, 0.8, 1.25]
stream_params, batch, same_chunks, kv_all_free, on_emu = wcases.stream_params, wcases.batch, wcases.same_chunks, wcases.kv_all_free, wcases.on_emu


def plain_batch(tts):
    """The plain call's chunks of the three utterances (greedy decoding: the same ids every time), device path; generated once per instance."""
    if not hasattr(tts, "_plain_three"):
        with stream_params(tts):
            tts._plain_three = batch(tts, THREE)
    return tts._plain_three


def check_against_plain(tts, got, plain, speeds, fmt=None):
    """Per utterance: the concatenated chunks are CodecEngine.stretch of the plain stream's concatenated chunks; in the native format the chunk
    lengths are the rule's, and an utterance at 1.0 is the plain stream chunk for chunk."""
    eng = tts.codec.engine
    kw = {} if fmt is None else dict(sample_rate=fmt[0], encoding=fmt[1], filter_width=fmt[2])
    for g, p, speed in zip(got, plain, speeds):
        pm = spec.permille(speed)
        want = eng.stretch([np.concatenate(p)], speed, **kw)[0]
        assert len(g) == len(p) >= 2 and np.concatenate(g).dtype == want.dtype
        assert np.array_equal(np.concatenate(g), want), f"speed {speed}"
        if fmt is None:
            n_in = np.cumsum([len(c) for c in p])
            count = [sspec.stream_out_count(int(n), pm, last=(k == len(p) - 1)) for k, n in enumerate(n_in)]
            assert [len(c) for c in g] == np.diff([0] + count).tolist()
            if pm == 1000:
                assert same_chunks([g], [p])


def test_stream_batch_at_speeds_equals_the_one_shot_stretch_of_the_plain_stream(tts):
    plain = plain_batch(tts)
    with stream_params(tts):
        assert tts._stream_on_device([REF_CODES] * 3)
        got = batch(tts, THREE, stream_speed=THREE_SPEEDS)               # the device path: StreamSet(speed=), the stage behind the cross-fade
        one = batch(tts, THREE[1:], stream_speed=0.8)                    # one value for all
        kv_all_free(tts)
    check_against_plain(tts, got, plain, THREE_SPEEDS)
    assert same_chunks(one[:1], got[1:2])
    check_against_plain(tts, one[1:], plain[2:], [0.8])
    assert [sum(len(c) for c in g) for g in got] == [spec.out_len(sum(len(c) for c in p), spec.permille(s)) for p, s in zip(plain, THREE_SPEEDS)]


def test_device_path_equals_host_loop_and_single_streams(tts):
    with stream_params(tts):
        dev = batch(tts, THREE, stream_speed=THREE_SPEEDS)
        tts.stream_on_device = False                                     # numpy windows + _StreamBlender, then a SpeedStream of one row per utterance
        host = batch(tts, THREE, stream_speed=THREE_SPEEDS)
        singles = [list(tts.infer_stream(t, REF_CODES, REF_TEXT, stream_speed=s)) for t, s in list(zip(THREE, THREE_SPEEDS))[1: 2 if on_emu(tts) else 3]]
        tts.stream_on_device = True
        if not on_emu(tts):                                              # ... and a set of one stream on the device
            assert same_chunks(singles, [list(tts.infer_stream(t, REF_CODES, REF_TEXT, stream_speed=s)) for t, s in list(zip(THREE, THREE_SPEEDS))[1:]])
        kv_all_free(tts)
    assert same_chunks(host, dev)
    assert same_chunks(singles, dev[1: 1 + len(singles)])
    check_against_plain(tts, dev, plain_batch(tts), THREE_SPEEDS)


def test_stream_batch_over_a_gang_at_speeds(tts):
    """Groups of one over two engines, one stream set with its utterance's speed per group."""
    tts.gang = _hip.EngineGang(tts.backbone, 2)
    tts.stream_admit = 1
    tts.stream_on_gang = True
    try:
        with stream_params(tts):
            got = batch(tts, THREE, stream_speed=THREE_SPEEDS)
            assert len(tts._gang_codecs) == 2
            for e in tts.gang.engines:
                st = e.kv_stats()
                assert st["free_pages"] == st["total_pages"] and e.free_slots() == e.max_batch
    finally:
        del tts.stream_admit, tts.stream_on_gang
        for k, c in enumerate(tts._gang_codecs or []):
            c.set_stream(None)
            if k:
                c.close()
        tts._gang_codecs = None
        tts.gang.close()
        tts.gang = None
    check_against_plain(tts, got, plain_batch(tts), THREE_SPEEDS)        # (a window is defined by token counts, not by the engine)


@pytest.mark.parametrize("rate,enc,W", FORMATS)
def test_stream_batch_at_speeds_in_a_format(tts, rate, enc, W):
    with stream_params(tts):
        got = batch(tts, THREE, stream_speed=THREE_SPEEDS, stream_sample_rate=rate, stream_encoding=enc, stream_filter_width=W)
        tts.stream_on_device = False
        one = list(tts.infer_stream(THREE[1], REF_CODES, REF_TEXT, stream_speed=0.8, stream_sample_rate=rate, stream_encoding=enc, stream_filter_width=W))
        kv_all_free(tts)
    check_against_plain(tts, got, plain_batch(tts), THREE_SPEEDS, (rate, enc, W))
    assert same_chunks([one], got[1:2])


def test_watermarker_sees_speed_1_float_windows_and_its_output_is_stretched(tts):
    stub, plain = fmt_cases.StubWatermarker(), fmt_cases.StubWatermarker()
    try:
        with stream_params(tts):
            tts.watermarker = plain
            marked = [list(tts.infer_stream(TEXTS[0], REF_CODES, REF_TEXT))]           # the stubbed plain stream (host loop: a watermarker is a host library)
            tts.watermarker = stub
            got = [list(tts.infer_stream(TEXTS[0], REF_CODES, REF_TEXT, stream_speed=0.8))]
            if not on_emu(tts):
                assert same_chunks(batch(tts, TEXTS[:1], stream_speed=0.8), got)
    finally:
        tts.watermarker = None
    assert stub.seen[: len(plain.seen)] == plain.seen and all(s[0] == np.dtype(np.float32) and s[1] == 1 and s[2] == 24000 for s in stub.seen)
    check_against_plain(tts, got, marked, [0.8])
    assert not same_chunks(marked, plain_batch(tts)[:1])                 # (the stub did change the stream)


def test_constructor_default_and_per_call_override(tts):
    assert tts.stream_speed == 1.0 and tts.speed == 1.0
    plain = plain_batch(tts)
    try:
        tts.stream_speed = 0.8
        with stream_params(tts):
            a = batch(tts, TEXTS[:1])                                    # the instance's speed
            b = batch(tts, TEXTS[:1], stream_speed=1.25)                 # overridden for one call
            c = batch(tts, TEXTS[:1], stream_speed=1.0)                  # back to 1.0 for one call
            assert tts.speed == 1.0                                      # (the one-shot entry points' speed is another attribute)
    finally:
        tts.stream_speed = 1.0
    check_against_plain(tts, a, plain[:1], [0.8])
    check_against_plain(tts, b, plain[:1], [1.25])
    assert same_chunks(c, plain[:1])
    for kw, word in ((dict(stream_speed=0.4), "0.4"), (dict(stream_speed=2.5), "2.5"), (dict(stream_speed="fast"), "fast"), (dict(stream_speed=True), "True")):
        with pytest.raises(ValueError, match="stream_speed.*" + word):
            tts.infer_stream("Streaming.", REF_CODES, REF_TEXT, **kw)    # at the call, before a generator exists
        with pytest.raises(ValueError, match="stream_speed.*" + word):
            tts.infer_stream_batch(["Streaming."], REF_CODES, REF_TEXT, **kw)
    with pytest.raises(ValueError, match="2 values for 1"):
        tts.infer_stream_batch(["Streaming."], REF_CODES, REF_TEXT, stream_speed=[0.8, 0.9])
    with pytest.raises(ValueError, match="speed=.*one-shot stage.*stream_speed="):      # the one-shot keyword stays refused, and says where to go
        tts.infer_stream("Streaming.", REF_CODES, REF_TEXT, speed=0.8)
    from neutts import NeuTTS
    with pytest.raises(ValueError, match="stream_speed.*3.0"):                         # checked ahead of any loading
        NeuTTS(backbone_repo=None, codec_repo=None, stream_speed=3.0)
    kv_all_free(tts)


def test_a_stream_that_ends_on_a_window_edge_is_flushed(tts):
    """Toy parameters (lookforward 0, overlap 0) and exactly two windows of tokens: no final window exists, so what the stretch holds back comes as
    one more chunk, `last` -- without a format too, on the device path, in the batch host loop and in the single-stream host loop alike; a stream at
    1.0 holds nothing back and gets no such chunk."""
    prompt = tts._apply_chat_template(REF_CODES, REF_TEXT, TEXTS[0])
    look_f, ovl = tts.streaming_lookforward, tts.streaming_overlap_frames
    tts.streaming_lookforward = tts.streaming_overlap_frames = 0
    tts.min_new_tokens, tts.max_context = 50, len(prompt) + 50
    try:
        assert tts._stream_on_device([REF_CODES])
        plain = [c for _, c in tts._infer_stream_batch_hip([prompt], [REF_CODES], None, None)]
        dev = [c for _, c in tts._infer_stream_batch_hip([prompt], [REF_CODES], None, None, [0.8])]
        both = [[], []]
        for i, c in tts._infer_stream_batch_hip([prompt, prompt], [REF_CODES, REF_CODES], None, None, [1.0, 0.8]):
            both[i].append(c)
        tts.stream_on_device = False
        host = [c for _, c in tts._infer_stream_batch_hip([prompt], [REF_CODES], None, None, [0.8])]        # (the batch host loop's only run on the emulator)
        one = list(tts._infer_stream_hip(prompt, REF_CODES, None, None, [0.8]))
        kv_all_free(tts)
    finally:
        tts.stream_on_device = True
        tts.streaming_lookforward, tts.streaming_overlap_frames = look_f, ovl
        tts.min_new_tokens, tts.max_context = 5, 120
    stride = tts.streaming_stride_samples
    assert [len(c) for c in plain] == [stride, stride]                   # two regular windows, no final one
    count = [sspec.stream_out_count(stride, 800), sspec.stream_out_count(2 * stride, 800), spec.out_len(2 * stride, 800)]
    assert [len(c) for c in dev] == np.diff([0] + count).tolist() and len(dev[2]) > 0
    assert np.array_equal(np.concatenate(dev), tts.codec.engine.stretch([np.concatenate(plain)], 0.8)[0])
    assert same_chunks([host], [dev]) and same_chunks([one], [dev])
    assert same_chunks(both, [plain, dev])


class LibCalls:
    """A stand-in for an engine's library handle that records the name of every ntts_streams_* / ntts_speed_stream_* function called through it."""

    def __init__(self, lib, log):
        self._lib, self._log = lib, log

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name.startswith(("ntts_streams_", "ntts_speed_stream_")):
            def call(*a):
                self._log.append(name)
                return fn(*a)
            return call
        return fn


def test_a_set_all_at_unit_speed_makes_the_calls_it_made_before(tts):
    """stream_speed 1.0 -- by default, or spelled out per utterance as 1.0 and 1.0004 -- is the plain call: the same ntts_streams_* calls in the same order
    (no set_speed among them, no speed stream) and the same chunks."""
    eng = tts.backbone
    lib = eng.lib
    logs = []
    plain = plain_batch(tts)[:2]
    try:
        with stream_params(tts):
            for kw in (dict(), dict(stream_speed=[1.0, 1.0004]), dict(stream_speed=[1.0, 0.8])):
                logs.append([])
                eng.lib = LibCalls(lib, logs[-1])
                got = batch(tts, **kw)
                assert same_chunks(got[:1], plain[:1]) and (same_chunks(got, plain) or len(logs) == 3)
    finally:
        eng.lib = lib
    assert logs[0] and "ntts_streams_pump_end" in logs[0] and logs[1] == logs[0]
    assert not any("speed" in name for name in logs[0]) and "ntts_streams_set_speed" in logs[2]
    kv_all_free(tts)


def test_set_speed_all_1000_through_the_abi_is_the_plain_set(tts):
    """ntts_streams_set_speed with every stream at 1000 (and with NULL) builds no stage on the C side: the set hands out the chunks, the chunk
    counts and the row_stride of a set that was never told a speed; a set with one stream at 800 has longer rows."""
    eng, cod = tts.backbone, tts.codec.engine
    i32p = C.POINTER(C.c_int32)
    prompts = [tts._apply_chat_template(REF_CODES, REF_TEXT, t) for t in TEXTS]
    chunk, look_f = tts.streaming_frames_per_chunk, tts.streaming_lookforward

    def drive(speeds):
        slots = [eng.acquire_slot() for _ in prompts]
        out, strides = [[] for _ in prompts], set()
        try:
            eng.prefill(prompts, slots, [tts._sampling(len(p), i) for i, p in enumerate(prompts)])
            ss = _hip.StreamSet(eng, cod, slots, [REF_CODES] * 2, int(eng.cfg["max_context"]), chunk, look_f, tts.streaming_lookback,
                                tts.streaming_overlap_frames, tts.hop_length, int(tts._speech_base), 65536)
            try:
                for pm in speeds:                                        # (several calls before the first pump: the last one holds)
                    arr = None if pm is None else np.ascontiguousarray(pm, dtype=np.int32)
                    assert ss.lib.ntts_streams_set_speed(ss.h, arr.ctypes.data_as(i32p) if arr is not None else None) == 0
                steps = chunk + look_f - 1
                while True:
                    ss.pump_begin()
                    running = ss.pump_wait()
                    if running:
                        eng.decode(steps)
                    more = True
                    while more:
                        n, run, mo = C.c_int32(), C.c_int32(), C.c_int32()
                        ptr, stride = C.POINTER(C.c_float)(), C.c_int64()
                        assert ss.lib.ntts_streams_pump_end(ss.h, len(ss._cs), C.byref(n), ss._cs.ctypes.data_as(i32p), ss._cn.ctypes.data_as(i32p),
                                                            ss._cl.ctypes.data_as(i32p), C.byref(ptr), C.byref(stride), C.byref(run), C.byref(mo)) == 0
                        more = bool(mo.value)
                        strides.add(stride.value)
                        if n.value:
                            buf = np.ctypeslib.as_array(ptr, shape=(n.value, stride.value))
                            for k in range(n.value):
                                out[int(ss._cs[k])].append((np.array(buf[k, : int(ss._cn[k])]), bool(ss._cl[k])))
                    if not running:
                        break
                    steps = chunk
            finally:
                ss.close()
        finally:
            eng.sync()
            for sl in slots:
                eng.release(sl)
        return out, strides

    def same(a, b):
        return same_chunks([[c for c, _ in u] for u in a], [[c for c, _ in u] for u in b]) and [[f for _, f in u] for u in a] == [[f for _, f in u] for u in b]

    with stream_params(tts):
        tts._seed += 1
        plain, plain_strides = drive([])
        ones, ones_strides = drive([[800, 1250], [1000, 1000]])          # a stage was built, then taken away again
        null, null_strides = drive([[800, 800], None])
        slow, slow_strides = drive([[1000, 800]])
    assert len(plain[0]) >= 2 and plain_strides == {(chunk + look_f + tts.streaming_overlap_frames) * tts.hop_length}
    assert same(ones, plain) and ones_strides == plain_strides
    assert same(null, plain) and null_strides == plain_strides
    assert same(slow[:1], plain[:1]) and not same(slow[1:], plain[1:]) and min(slow_strides) > max(plain_strides)
    kv_all_free(tts)


def test_stream_set_abi_set_speed(tts):
    """ntts_streams_set_speed: a speed out of range is NTTS_EINVAL and names it; legal, in either order with set_format, until the first pump_begin
    and NTTS_ESTATE after; both pump_end variants serve a set with speeds in the native format, plain pump_end on a non-native one stays
    NTTS_ESTATE."""
    eng, cod = tts.backbone, tts.codec.engine
    prompt = tts._apply_chat_template(REF_CODES, REF_TEXT, "Testing.")
    i32p = C.POINTER(C.c_int32)

    def pm(v):
        return np.array([v], dtype=np.int32).ctypes.data_as(i32p)

    for fmt, plain_rc in ((None, 0), ((8000, "mulaw", 6), ESTATE)):
        slot = eng.acquire_slot()
        try:
            eng.prefill([prompt], [slot], [tts._sampling(len(prompt), 0)])
            ss = _hip.StreamSet(eng, cod, [slot], [REF_CODES], int(eng.cfg["max_context"]), 25, 5, 50, 1, tts.hop_length, int(tts._speech_base), 65536,
                                fmt=fmt, speed=0.8)
            try:
                lib = ss.lib
                assert lib.ntts_streams_set_speed(ss.h, pm(2001)) == EINVAL and "2001" in (lib.ntts_streams_last_error(ss.h) or b"").decode()
                assert lib.ntts_streams_set_speed(ss.h, pm(499)) == EINVAL
                assert lib.ntts_streams_set_speed(ss.h, None) == 0 and lib.ntts_streams_set_speed(ss.h, pm(1000)) == 0      # still before the first pump
                assert lib.ntts_streams_set_speed(ss.h, pm(1250)) == 0
                ss.pump_begin()
                assert lib.ntts_streams_set_speed(ss.h, pm(800)) == ESTATE and "fixed" in (lib.ntts_streams_last_error(ss.h) or b"").decode()
                assert lib.ntts_streams_set_speed(ss.h, None) == ESTATE
                n, run, more = C.c_int32(), C.c_int32(), C.c_int32()
                ptr, stride = C.POINTER(C.c_float)(), C.c_int64()
                rc = lib.ntts_streams_pump_end(ss.h, 2, C.byref(n), ss._cs.ctypes.data_as(i32p), ss._cn.ctypes.data_as(i32p), ss._cl.ctypes.data_as(i32p),
                                               C.byref(ptr), C.byref(stride), C.byref(run), C.byref(more))
                assert rc == plain_rc and n.value == 0                   # (nothing is decodable yet)
                if rc != 0:
                    chunks, _, _ = ss.pump_end()
                    assert chunks == []
            finally:
                ss.close()
        finally:
            eng.sync()
            eng.release(slot)
    kv_all_free(tts)
