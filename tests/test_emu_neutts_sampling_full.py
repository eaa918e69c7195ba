"""`top_k=-1` (sample over the whole vocabulary) on the class surface: it reaches the engine from the constructor, per call, in per-utterance
lists, on both stream paths and with best_of -- and every other value below 1 is refused before the engine is touched.  On the SIMT emulator;
tests/test_gpu_sampling_full.py runs the same bodies on libneutts_hip.so."""
import numpy as np
import pytest

from neutts import _hip
import test_emu_neutts_sampling as base
from test_emu_neutts_sampling import CTOR, REF, TEXTS, Spy, build_sampling_tts, check_requests

OFF = _hip.TOP_K_OFF


@pytest.fixture(scope="module")
def tts(emu_lib):
    return build_sampling_tts(emu_lib, max_batch=3)


def build_off_tts(lib, **kw):
    """build_sampling_tts with `top_k=-1` among the constructor's arguments."""
    import functools
    import neutts
    real = neutts.NeuTTS
    neutts.NeuTTS = functools.partial(real, **dict(CTOR, top_k=OFF))
    try:
        t = base.cases.build_tts(lib, **kw)
    finally:
        neutts.NeuTTS = real
    t.do_sample = True
    t.max_context = max(len(t._apply_chat_template(REF, "So I'm live.", x)) for x in TEXTS) + 12
    return t


@pytest.fixture(scope="module")
def tts_off(emu_lib):
    return build_off_tts(emu_lib, max_batch=3)


def test_constructor_value_reaches_the_engine(tts_off):
    from neutts import NeuTTS
    tts = tts_off
    assert OFF == -1 and tts.top_k == OFF
    prompt = tts._apply_chat_template(REF, "So I'm live.", "Testing.")
    with Spy(tts.backbone) as spy:
        got = tts.generate_codes([prompt])[0]
    check_requests(tts, spy, [(OFF, 0.7, 0.8, 0.03)])
    assert spy.requests[0][2] == got
    with Spy(tts.backbone) as spy:
        audio = tts.infer("Testing.", REF, "So I'm live.")
    check_requests(tts, spy, [(OFF, 0.7, 0.8, 0.03)])
    assert np.array_equal(audio, tts._decode_ids(spy.requests[0][2]))
    with Spy(tts.backbone) as spy:
        tts.generate_codes([prompt], top_k=40)            # ... and a per-call top-k overrides it
    check_requests(tts, spy, [(40, 0.7, 0.8, 0.03)])
    for bad in (0, -2, 2.5, True):                        # (checked before anything is loaded)
        with pytest.raises(ValueError, match="-1"):
            NeuTTS(backbone_repo=None, top_k=bad)


def test_per_call_and_per_utterance_values_reach_the_engine(tts):
    prompt = tts._apply_chat_template(REF, "So I'm live.", "Testing.")
    with Spy(tts.backbone) as spy:
        tts.generate_codes([prompt], top_k=OFF, top_p=0.95)
    check_requests(tts, spy, [(OFF, 0.7, 0.95, 0.03)])
    with Spy(tts.backbone) as spy:
        tts.infer("Testing.", REF, "So I'm live.", temperature=1.2, top_k=OFF, top_p=1.0, min_p=0.0)      # plain ancestral sampling
    check_requests(tts, spy, [(OFF, 1.2, 1.0, 0.0)])
    assert tts.top_k == CTOR["top_k"]                     # an override does not stick
    texts = TEXTS[1:4]
    want = [(50, 0.7, 0.8, 0.03), (OFF, 0.7, 0.8, 0.03), (12, 0.7, 0.8, 0.03)]
    kw = dict(top_k=[50, OFF, None])
    with Spy(tts.backbone) as spy:
        wavs = tts.infer_batch(texts, REF, "So I'm live.", **kw)
    check_requests(tts, spy, want)
    assert len(wavs) == 3
    prompts = [tts._apply_chat_template(REF, "So I'm live.", t) for t in texts]
    with Spy(tts.backbone) as spy:
        tts.generate_codes(prompts, **kw)
    check_requests(tts, spy, want)
    with Spy(tts.backbone) as spy:
        chunks = list(tts.infer_stream_batch(texts, REF, "So I'm live.", **kw))
    check_requests(tts, spy, want)
    assert {i for i, _ in chunks} == {0, 1, 2}


def test_both_stream_paths(tts):
    for on_device in (True, False):                       # the device-side stream set / the host loop
        tts.stream_on_device = on_device
        try:
            with Spy(tts.backbone) as spy:
                chunks = list(tts.infer_stream("Streaming.", REF, "So I'm live.", top_k=OFF, top_p=0.9, min_p=0.05))
        finally:
            del tts.stream_on_device
        check_requests(tts, spy, [(OFF, 0.7, 0.9, 0.05)])
        assert len(chunks) >= 1 and all(np.isfinite(c).all() and len(c) % tts.hop_length == 0 for c in chunks)


def test_best_of_and_logprobs(tts):
    prompt = tts._apply_chat_template(REF, "So I'm live.", "Testing.")
    with Spy(tts.backbone) as spy:
        ids, lps = tts.generate_codes([prompt], top_k=OFF, top_p=0.95, best_of=2, return_logprobs=True)
    assert len(spy.requests) == 2 and all(sp.top_k == OFF and sp.do_sample for _, sp, _ in spy.requests)
    assert len({sp.seed for _, sp, _ in spy.requests}) == 2
    assert ids[0] in [r[2] for r in spy.requests] and len(lps[0]) == len(ids[0])
    assert np.isfinite(lps[0]).all() and (np.asarray(lps[0]) <= 0).all()


def test_bad_values_raise_before_the_engine_is_touched(tts):
    prompt = tts._apply_chat_template(REF, "So I'm live.", "Testing.")
    seed, calls = tts._seed, dict(tts.backbone.counters)
    for bad in (0, -2, 2.5, True):
        kw = dict(top_k=bad)
        with pytest.raises(ValueError, match="-1"):       # the message names the value that does mean "no top-k"
            tts.generate_codes([prompt], **kw)
        with pytest.raises(ValueError):
            tts.infer("Testing.", REF, "So I'm live.", **kw)
        with pytest.raises(ValueError):
            tts.infer_batch(["a", "b"], REF, "So I'm live.", top_k=[OFF, bad])
        with pytest.raises(ValueError):
            tts.infer_stream("Testing.", REF, "So I'm live.", **kw)              # at the call, not at the first next()
        with pytest.raises(ValueError):
            tts.infer_stream_batch(["a", "b"], REF, "So I'm live.", top_k=[bad, OFF])
    assert tts._seed == seed and tts.backbone.counters == calls and tts.backbone.free_slots() == tts.backbone.max_batch
    assert base.BAD                                       # (the older list of bad values, top_k = 0 among them, stays refused: tests/test_emu_neutts_sampling.py)
