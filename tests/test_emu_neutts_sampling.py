"""The sampling arguments of the class surface: `NeuTTS(top_k=, temperature=, top_p=, min_p=)` and the keyword-only per-call
overrides of infer / infer_batch / infer_stream / infer_stream_batch / generate_codes reach the engine -- the request the engine is
handed carries them, and the ids it generates are those of an engine-level run with that `Sampling` and seed.  On the SIMT emulator;
tests/test_gpu_sampling_nucleus.py runs the same bodies on libneutts_hip.so."""
import functools
import inspect

import numpy as np
import pytest

from neutts import _hip
import test_emu_neutts_class as cases

CTOR = dict(top_k=12, temperature=0.7, top_p=0.8, min_p=0.03)
REF = [3, 77, 200, 5, 18, 9]
TEXTS = ["Testing.", "One.", "Two two.", "Three.", "Streaming."]


def build_sampling_tts(lib, **kw):
    """cases.build_tts with constructor sampling arguments (it builds `neutts.NeuTTS(...)` by name), sampling switched on."""
    import neutts
    real = neutts.NeuTTS
    neutts.NeuTTS = functools.partial(real, **CTOR)
    try:
        t = cases.build_tts(lib, **kw)
    finally:
        neutts.NeuTTS = real
    t.do_sample = True
    # short runs: every request stops (max_length) a dozen tokens behind the longest prompt the tests below build
    t.max_context = max(len(t._apply_chat_template(REF, "So I'm live.", x)) for x in TEXTS) + 12
    return t


@pytest.fixture(scope="module")
def tts(emu_lib):
    return build_sampling_tts(emu_lib, max_batch=3)


class Spy:
    """Records, per request of the calls made while it is installed, the Sampling handed to the engine's prompt pass and the ids the slot
    held when it was released."""

    def __init__(self, eng):
        self.eng, self.samp, self.ids, self.requests = eng, {}, {}, []
        self._prefill, self._release, self._release_many = eng.prefill, eng.release, eng.release_many

    def __enter__(self):
        eng = self.eng

        def prefill(prompts, slots, sampling, donors=None):
            self._prefill(prompts, slots, sampling, donors)
            for p, s, sp in zip(prompts, slots, sampling):
                self.samp[s] = (list(p), sp)

        def flush(slot):
            if slot in self.samp:
                p, sp = self.samp.pop(slot)
                self.requests.append((p, sp, eng.read(slot)[0]))

        def release(slot):
            flush(slot)
            self._release(slot)

        def release_many(slots):
            for s in slots:
                flush(s)
            self._release_many(slots)

        eng.prefill, eng.release, eng.release_many = prefill, release, release_many
        return self

    def __exit__(self, *exc):
        del self.eng.prefill, self.eng.release, self.eng.release_many       # (instance attributes shadowing the methods)


def check_requests(tts, spy, want):
    """want: one (top_k, temperature, top_p, min_p) per request, in the order of the call's utterances (= ascending seed index)."""
    assert len(spy.requests) == len(want)
    reqs = sorted(spy.requests, key=lambda r: want_index(tts, r[1]))
    for (prompt, sp, ids), (k, t, tp, mp) in zip(reqs, want):
        assert (sp.top_k, sp.temperature, sp.top_p, sp.min_p, sp.do_sample) == (k, t, tp, mp, True)
        assert len(ids) >= tts.min_new_tokens
    assert len({sp.seed for _, sp, _ in reqs}) == len(want)
    again = tts.backbone.generate([r[0] for r in reqs], [r[1] for r in reqs])       # engine level: the same Sampling objects, the same seeds
    assert again == [r[2] for r in reqs]


def want_index(tts, sp):
    """index of a request within its call, from its seed (NeuTTS._sampling: seed = call * A + index * B + 1 mod 2^64)."""
    for i in range(64):
        if sp.seed == (tts._seed * 0x9E3779B97F4A7C15 + i * 0xD1B54A32D192ED03 + 1) & 0xFFFFFFFFFFFFFFFF:
            return i
    raise AssertionError("seed not of this call")


def test_signatures_keep_the_reference_positionals(tts):
    for name, pos in (("infer", ["text", "ref_codes", "ref_text"]), ("infer_batch", ["texts", "ref_codes", "ref_texts"]),
                      ("infer_stream", ["text", "ref_codes", "ref_text"]), ("infer_stream_batch", ["texts", "ref_codes", "ref_texts"]),
                      ("generate_codes", ["prompts"])):
        ps = inspect.signature(getattr(tts, name)).parameters
        assert [n for n, p in ps.items() if p.kind == p.POSITIONAL_OR_KEYWORD] == pos
        assert {n: p.default for n, p in ps.items() if p.kind == p.KEYWORD_ONLY} == dict(temperature=None, top_k=None, top_p=None, min_p=None)
    from neutts import NeuTTS
    ps = inspect.signature(NeuTTS.__init__).parameters
    assert all(ps[n].kind == ps[n].KEYWORD_ONLY for n in CTOR)
    assert {n: ps[n].default for n in CTOR} == dict(top_k=50, temperature=1.0, top_p=1.0, min_p=0.0)     # the reference's call
    import neuttsair
    assert issubclass(neuttsair.NeuTTSAir, NeuTTS)


def test_constructor_arguments_reach_the_engine(tts):
    assert {n: getattr(tts, n) for n in CTOR} == CTOR
    prompt = tts._apply_chat_template(REF, "So I'm live.", "Testing.")
    with Spy(tts.backbone) as spy:
        got = tts.generate_codes([prompt])[0]
    check_requests(tts, spy, [tuple(CTOR.values())])
    assert spy.requests[0][2] == got
    with Spy(tts.backbone) as spy:
        audio = tts.infer("Testing.", REF, "So I'm live.")
    check_requests(tts, spy, [tuple(CTOR.values())])
    assert np.array_equal(audio, tts._decode_ids(spy.requests[0][2]))


def test_per_call_overrides_reach_the_engine(tts):
    prompt = tts._apply_chat_template(REF, "So I'm live.", "Testing.")
    with Spy(tts.backbone) as spy:
        tts.generate_codes([prompt], top_p=0.5, min_p=0.1)
    check_requests(tts, spy, [(12, 0.7, 0.5, 0.1)])
    with Spy(tts.backbone) as spy:
        tts.infer("Testing.", REF, "So I'm live.", temperature=0.9, top_k=5, top_p=0.95, min_p=0.0)
    check_requests(tts, spy, [(5, 0.9, 0.95, 0.0)])
    assert {n: getattr(tts, n) for n in CTOR} == CTOR               # an override does not stick


def test_per_utterance_lists_in_the_batch_entry_points(tts):
    texts = TEXTS[1:4]
    want = [(12, 0.7, 1.0, 0.2), (4, 0.7, 0.6, 0.2), (30, 0.7, 0.8, 0.2)]          # (temperature: the attribute; a None entry: the attribute)
    kw = dict(top_k=[12, 4, 30], top_p=[1.0, 0.6, None], min_p=0.2)
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


def test_stream_entry_points(tts):
    for on_device in (True, False):                     # the device-side stream set / the host loop
        tts.stream_on_device = on_device
        try:
            with Spy(tts.backbone) as spy:
                chunks = list(tts.infer_stream("Streaming.", REF, "So I'm live.", top_p=0.6, min_p=0.05, top_k=20))
        finally:
            del tts.stream_on_device
        check_requests(tts, spy, [(20, 0.7, 0.6, 0.05)])
        assert len(chunks) >= 1 and all(np.isfinite(c).all() and len(c) % tts.hop_length == 0 for c in chunks)


BAD = [dict(top_p=0.0), dict(top_p=1.2), dict(top_p=float("nan")), dict(top_p="0.9"), dict(min_p=-0.1), dict(min_p=1.1), dict(min_p=float("nan")),
       dict(top_k=0), dict(top_k=2.5), dict(temperature=0.0), dict(temperature=float("inf")), dict(temperature=-1.0)]


def test_bad_values_raise_before_the_engine_is_touched(tts):
    from neutts import NeuTTS
    prompt = tts._apply_chat_template(REF, "So I'm live.", "Testing.")
    seed, calls = tts._seed, dict(tts.backbone.counters)
    for kw in BAD:
        with pytest.raises(ValueError):
            NeuTTS(backbone_repo=None, **kw)            # (checked before anything is loaded)
        with pytest.raises(ValueError):
            tts.generate_codes([prompt], **kw)
        with pytest.raises(ValueError):
            tts.infer("Testing.", REF, "So I'm live.", **kw)
        with pytest.raises(ValueError):
            tts.infer_batch(["a", "b"], REF, "So I'm live.", **{k: [CTOR.get(k, 0.5), v] for k, v in kw.items()})
        with pytest.raises(ValueError):
            tts.infer_stream("Testing.", REF, "So I'm live.", **kw)          # at the call, not at the first next()
        with pytest.raises(ValueError):
            tts.infer_stream_batch(["a", "b"], REF, "So I'm live.", **kw)
    with pytest.raises(ValueError):
        tts.infer_batch(["a", "b"], REF, "So I'm live.", top_p=[0.9])        # one value per utterance, or one for all
    assert tts._seed == seed and tts.backbone.counters == calls and tts.backbone.free_slots() == tts.backbone.max_batch
