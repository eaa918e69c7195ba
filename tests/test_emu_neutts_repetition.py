"""The repetition penalty on the class surface: `NeuTTS(repetition_penalty=, repetition_ignore_prompt=)` and the per-call keywords of
infer / infer_batch / infer_stream / infer_stream_batch / generate_codes reach the engine's `Sampling` (repetition_ignore_prompt=True as
that utterance's own prompt length), bad values raise before the engine is touched, and the reference positionals of every signature
stay as they are.  On the SIMT emulator; tests/test_gpu_repetition.py runs the same bodies on libneutts_hip.so."""
import functools
import inspect

import numpy as np
import pytest

import test_emu_neutts_class as class_cases
import test_emu_neutts_sampling as sampling_cases
from test_emu_neutts_sampling import REF, TEXTS, Spy, want_index

CTOR = dict(repetition_penalty=1.4, repetition_ignore_prompt=True)
ENTRY_POINTS = (("infer", ["text", "ref_codes", "ref_text"]), ("infer_batch", ["texts", "ref_codes", "ref_texts"]),
                ("infer_stream", ["text", "ref_codes", "ref_text"]), ("infer_stream_batch", ["texts", "ref_codes", "ref_texts"]),
                ("generate_codes", ["prompts"]))


def build_repetition_tts(lib, **kw):
    """test_emu_neutts_class.build_tts with the two constructor arguments (it builds `neutts.NeuTTS(...)` by name); greedy, short runs."""
    import neutts
    real = neutts.NeuTTS
    neutts.NeuTTS = functools.partial(real, **CTOR)
    try:
        t = class_cases.build_tts(lib, **kw)
    finally:
        neutts.NeuTTS = real
    t.max_context = max(len(t._apply_chat_template(REF, "So I'm live.", x)) for x in TEXTS) + 12
    return t


@pytest.fixture(scope="module")
def rtts(emu_lib):
    return build_repetition_tts(emu_lib, max_batch=3)


def check_requests(tts, spy, want):
    """want: one (repetition_penalty, ignore the prompt?) per request, in the order of the call's utterances."""
    assert len(spy.requests) == len(want)
    reqs = sorted(spy.requests, key=lambda r: want_index(tts, r[1]))
    for (prompt, sp, ids), (pen, ign) in zip(reqs, want):
        assert (sp.repetition_penalty, sp.prompt_ignore_length) == (pen, len(prompt) if ign else 0), (sp, pen, ign, len(prompt))
        assert len(ids) >= tts.min_new_tokens
    again = tts.backbone.generate([r[0] for r in reqs], [r[1] for r in reqs])       # engine level: the same Sampling objects
    assert again == [r[2] for r in reqs]
    return reqs


def test_signatures_keep_the_reference_positionals(rtts):
    for name, pos in ENTRY_POINTS:
        ps = inspect.signature(getattr(rtts, name)).parameters
        assert [n for n, p in ps.items() if p.kind == p.POSITIONAL_OR_KEYWORD] == pos
        assert not [n for n, p in ps.items() if p.kind == p.VAR_POSITIONAL]             # the new keywords cannot be given by position
        assert list(ps)[len(pos):len(pos) + 4] == ["temperature", "top_k", "top_p", "min_p"]      # ... and come behind min_p
    from neutts import NeuTTS
    ps = inspect.signature(NeuTTS.__init__).parameters
    assert all(ps[n].kind == ps[n].KEYWORD_ONLY for n in CTOR)
    assert {n: ps[n].default for n in CTOR} == dict(repetition_penalty=1.0, repetition_ignore_prompt=False)      # the reference's call: off
    prompt = rtts._apply_chat_template(REF, "So I'm live.", "Testing.")
    with pytest.raises(TypeError):
        rtts.generate_codes([prompt], None, None, None, None, 1.3)
    with pytest.raises(TypeError, match="repetition_penalti"):
        rtts.generate_codes([prompt], repetition_penalti=1.3)                            # an unknown keyword is still an error


def test_constructor_arguments_reach_the_engine(rtts):
    assert {n: getattr(rtts, n) for n in CTOR} == CTOR
    prompt = rtts._apply_chat_template(REF, "So I'm live.", "Testing.")
    with Spy(rtts.backbone) as spy:
        got = rtts.generate_codes([prompt])[0]
    check_requests(rtts, spy, [(1.4, True)])
    assert spy.requests[0][2] == got
    with Spy(rtts.backbone) as spy:
        audio = rtts.infer("Testing.", REF, "So I'm live.")
    check_requests(rtts, spy, [(1.4, True)])
    assert np.array_equal(audio, rtts._decode_ids(spy.requests[0][2]))


def test_per_call_overrides_and_per_utterance_lists(rtts):
    prompt = rtts._apply_chat_template(REF, "So I'm live.", "Testing.")
    with Spy(rtts.backbone) as spy:
        rtts.generate_codes([prompt], repetition_penalty=1.0)
    check_requests(rtts, spy, [(1.0, True)])
    with Spy(rtts.backbone) as spy:
        rtts.generate_codes([prompt], repetition_penalty=3.0, repetition_ignore_prompt=False)
    check_requests(rtts, spy, [(3.0, False)])
    assert {n: getattr(rtts, n) for n in CTOR} == CTOR               # an override does not stick
    texts = TEXTS[1:4]
    want = [(1.4, True), (2.0, False), (1.1, True)]                  # (a None entry: the attribute)
    kw = dict(repetition_penalty=[None, 2.0, 1.1], repetition_ignore_prompt=[True, False, None])
    with Spy(rtts.backbone) as spy:
        wavs = rtts.infer_batch(texts, REF, "So I'm live.", **kw)
    reqs = check_requests(rtts, spy, want)
    assert len(wavs) == 3 and len({len(r[0]) for r in reqs}) > 1     # each utterance's OWN prompt length
    prompts = [rtts._apply_chat_template(REF, "So I'm live.", t) for t in texts]
    with Spy(rtts.backbone) as spy:
        rtts.generate_codes(prompts, top_k=[5, 6, 7], **kw)
    check_requests(rtts, spy, want)
    with Spy(rtts.backbone) as spy:
        chunks = list(rtts.infer_stream_batch(texts, REF, "So I'm live.", **kw))
    check_requests(rtts, spy, want)
    assert {i for i, _ in chunks} == {0, 1, 2}


def test_stream_entry_points(rtts):
    for on_device in (True, False):                     # the device-side stream set / the host loop
        rtts.stream_on_device = on_device
        try:
            with Spy(rtts.backbone) as spy:
                chunks = list(rtts.infer_stream("Streaming.", REF, "So I'm live.", repetition_penalty=1.2, repetition_ignore_prompt=False, top_k=20))
        finally:
            del rtts.stream_on_device
        check_requests(rtts, spy, [(1.2, False)])
        assert len(chunks) >= 1 and all(np.isfinite(c).all() and len(c) % rtts.hop_length == 0 for c in chunks)


BAD = [dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(repetition_penalty=float("nan")), dict(repetition_penalty=float("inf")),
       dict(repetition_penalty="1.3"), dict(repetition_penalty=True), dict(repetition_ignore_prompt=1), dict(repetition_ignore_prompt="yes")]


def test_bad_values_raise_before_the_engine_is_touched(rtts):
    from neutts import NeuTTS
    prompt = rtts._apply_chat_template(REF, "So I'm live.", "Testing.")
    seed, calls = rtts._seed, dict(rtts.backbone.counters)
    for kw in BAD:
        with pytest.raises(ValueError):
            NeuTTS(backbone_repo=None, **kw)            # (checked before anything is loaded)
        with pytest.raises(ValueError):
            rtts.generate_codes([prompt], **kw)
        with pytest.raises(ValueError):
            rtts.infer("Testing.", REF, "So I'm live.", **kw)
        with pytest.raises(ValueError):
            rtts.infer_batch(["a", "b"], REF, "So I'm live.", **{k: [CTOR[k], v] for k, v in kw.items()})
        with pytest.raises(ValueError):
            rtts.infer_stream("Testing.", REF, "So I'm live.", **kw)          # at the call, not at the first next()
        with pytest.raises(ValueError):
            rtts.infer_stream_batch(["a", "b"], REF, "So I'm live.", **kw)
    with pytest.raises(ValueError):
        rtts.infer_batch(["a", "b"], REF, "So I'm live.", repetition_penalty=[1.3])        # one value per utterance, or one for all
    assert rtts._seed == seed and rtts.backbone.counters == calls and rtts.backbone.free_slots() == rtts.backbone.max_batch


def test_the_sampling_suite_is_untouched_by_the_defaults(rtts):
    """An instance built without the two arguments hands the engine penalty 1.0 / ignore 0 (Sampling's defaults)."""
    from neutts import _hip
    sp = _hip.Sampling()
    assert (sp.repetition_penalty, sp.prompt_ignore_length) == (1.0, 0)
    c = sp.to_c()
    assert (c.repetition_penalty, c.prompt_ignore_length, c.top_p, c.min_p) == (1.0, 0, 1.0, 0.0)
    assert [f[0] for f in _hip.SamplingC._fields_][-2:] == ["repetition_penalty", "prompt_ignore_length"] and _hip.ABI_VERSION == 11
    assert sampling_cases.CTOR.keys().isdisjoint(CTOR)
