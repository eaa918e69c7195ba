"""Log-probabilities and best-of-N on the class surface: `NeuTTS(logprobs=, best_of=)`, `generate_codes(return_logprobs=)`,
`infer / infer_batch(return_scores=)` and `best_of=` on all three.  Values equal an engine-level rerun with the same `Sampling` objects, the
winner of best_of is the candidate with the highest mean log-probability, bad values raise before the engine is touched, the stream entry
points reject the keywords, and an instance built without logprobs=True leaves its engine's switch off.
On the SIMT emulator; tests/test_gpu_logprobs.py runs the same bodies on libneutts_hip.so."""
import functools
import inspect

import numpy as np
import pytest

import logprob_spec as spec
import test_emu_neutts_sampling as sampling_cases
from test_emu_neutts_sampling import REF, TEXTS, Spy, want_index

# the synthetic "walk" weights put all but ~1e-9 of the mass on one token: at temperature 1 every candidate would be the greedy run with
# log-probabilities of exactly 0.  A hot draw among the 12 largest logits makes the candidates differ and their scores telling (the temperature
# does not enter a log-probability)
HOT = dict(temperature=200.0, top_p=1.0, min_p=0.0)
ENTRY_POINTS = ("infer", "infer_batch", "infer_stream", "infer_stream_batch", "generate_codes")


def build_logprob_tts(lib, **kw):
    return sampling_cases.build_sampling_tts(lib, **kw)          # do_sample=True, short runs


@pytest.fixture(scope="module")
def ltts(emu_lib):
    return build_logprob_tts(emu_lib, max_batch=3)


def rerun(tts, reqs):
    """Engine level: the same prompts and Sampling objects, with the record on -> (ids, logprobs)."""
    eng = tts.backbone
    was = eng.logprobs
    eng.set_logprobs(True)
    try:
        return eng.generate([r[0] for r in reqs], [r[1] for r in reqs], return_logprobs=True)
    finally:
        eng.set_logprobs(was)


def by_index(tts, spy):
    return sorted(spy.requests, key=lambda r: want_index(tts, r[1]))


def test_signatures_and_defaults(ltts):
    from neutts import NeuTTS
    ps = inspect.signature(NeuTTS.__init__).parameters
    assert all(ps[n].kind == ps[n].KEYWORD_ONLY for n in ("logprobs", "best_of"))
    assert (ps["logprobs"].default, ps["best_of"].default) == (False, 1)
    for name in ENTRY_POINTS:                                    # the named keyword-only parameters stay the four sampling ones
        q = inspect.signature(getattr(ltts, name)).parameters
        assert {n for n, p in q.items() if p.kind == p.KEYWORD_ONLY} == {"temperature", "top_k", "top_p", "min_p"}
    assert (ltts.logprobs, ltts.best_of) == (False, 1) and not ltts.backbone.logprobs


def test_generate_codes_returns_the_engines_logprobs(ltts):
    prompts = [ltts._apply_chat_template(REF, "So I'm live.", t) for t in TEXTS[1:4]]
    with Spy(ltts.backbone) as spy:
        ids, lps = ltts.generate_codes(prompts, return_logprobs=True, top_k=[12, 4, 30], **HOT)
    assert not ltts.backbone.logprobs                            # switched on for the call only
    reqs = by_index(ltts, spy)
    assert [r[2] for r in reqs] == ids and len(lps) == 3
    assert all(lp.dtype == np.float32 and len(lp) == len(x) >= ltts.min_new_tokens and (lp <= 0).all() for x, lp in zip(ids, lps))
    again_ids, again_lps = rerun(ltts, reqs)
    assert again_ids == ids and all(np.array_equal(a, b) for a, b in zip(again_lps, lps))
    plain = ltts.generate_codes(prompts[:1])
    assert isinstance(plain, list) and isinstance(plain[0], list)                         # without the flag: the ids alone, as before


def test_scores_are_the_mean_logprob(ltts):
    texts = TEXTS[1:4]
    with Spy(ltts.backbone) as spy:
        wavs, scores = ltts.infer_batch(texts, REF, "So I'm live.", return_scores=True, **HOT)
    reqs = by_index(ltts, spy)
    _, lps = rerun(ltts, reqs)
    assert len(wavs) == 3 and len(scores) == 3
    for r, lp, sc, wv in zip(reqs, lps, scores, wavs):
        assert sc == spec.sequence_score(lp) and sc < 0
        assert np.array_equal(wv, ltts._decode_ids(r[2]))
    with Spy(ltts.backbone) as spy:
        wav, score = ltts.infer("Testing.", REF, "So I'm live.", return_scores=True, **HOT)
    _, lps = rerun(ltts, spy.requests)
    assert score == spec.sequence_score(lps[0]) and np.array_equal(wav, ltts._decode_ids(spy.requests[0][2]))
    assert isinstance(ltts.infer("Testing.", REF, "So I'm live."), np.ndarray)
    assert not ltts.backbone.logprobs


def test_best_of_three_picks_the_highest_mean(ltts):
    shared0 = ltts.backbone.kv_stats()["prompt_tokens_shared"]
    with Spy(ltts.backbone) as spy:
        wav, score = ltts.infer("Testing.", REF, "So I'm live.", best_of=3, return_scores=True, **HOT)
    reqs = by_index(ltts, spy)
    assert len(reqs) == 3 and len({r[1].seed for r in reqs}) == 3 and len({tuple(r[0]) for r in reqs}) == 1
    assert [want_index(ltts, r[1]) for r in reqs] == [0, 1, 2]                            # request index i * N + j
    assert ltts.backbone.kv_stats()["prompt_tokens_shared"] > shared0                      # the candidates share the prompt's pages
    ids, lps = rerun(ltts, reqs)
    assert ids == [r[2] for r in reqs] and len({tuple(x) for x in ids}) > 1                # the candidates differ
    means = [spec.sequence_score(lp) for lp in lps]
    win = int(np.argmax(means))                                                            # (argmax: ties to the lowest j)
    assert score == means[win] and np.array_equal(wav, ltts._decode_ids(ids[win]))
    with Spy(ltts.backbone) as spy:
        got = ltts.generate_codes([reqs[0][0]], best_of=3, **HOT)
    ids, lps = rerun(ltts, by_index(ltts, spy))
    assert got == [ids[int(np.argmax([spec.sequence_score(lp) for lp in lps]))]]
    assert not ltts.backbone.logprobs


def test_best_of_per_utterance(ltts):
    texts = TEXTS[1:3]
    with Spy(ltts.backbone) as spy:
        wavs, scores = ltts.infer_batch(texts, REF, "So I'm live.", best_of=[1, 2], return_scores=True, **HOT)
    reqs = by_index(ltts, spy)
    assert [want_index(ltts, r[1]) for r in reqs] == [0, 2, 3] and reqs[1][0] == reqs[2][0] != reqs[0][0]      # i * N + j with N = 2
    ids, lps = rerun(ltts, reqs)
    means = [spec.sequence_score(lp) for lp in lps]
    win = 1 + int(np.argmax(means[1:]))
    assert scores == [means[0], means[win]]
    assert np.array_equal(wavs[0], ltts._decode_ids(ids[0])) and np.array_equal(wavs[1], ltts._decode_ids(ids[win]))
    with Spy(ltts.backbone) as spy:                                                        # without scores: the same selection, waveforms only
        wavs2 = ltts.infer_batch(texts, REF, "So I'm live.", best_of=2)
    assert len(spy.requests) == 4 and isinstance(wavs2, list) and len(wavs2) == 2


def test_a_candidate_without_speech_tokens_cannot_win(ltts):
    """The winner needs at least one speech token: with every candidate but the last made to look empty, the last wins whatever its score."""
    real = ltts._ids_to_codes
    prompt = ltts._apply_chat_template(REF, "So I'm live.", "Testing.")
    with Spy(ltts.backbone) as spy:
        ltts.generate_codes([prompt], best_of=3, **HOT)
    cands = [r[2] for r in by_index(ltts, spy)]
    ltts._seed -= 1                                                                        # the same call again: the same three candidates
    ltts._ids_to_codes = lambda ids: real(ids) if list(ids) == cands[2] else []
    try:
        assert ltts.generate_codes([prompt], best_of=3, **HOT) == [cands[2]]
    finally:
        del ltts._ids_to_codes


def test_bad_values_raise_before_the_engine_is_touched(ltts):
    from neutts import NeuTTS
    prompt = ltts._apply_chat_template(REF, "So I'm live.", "Testing.")
    seed, calls = ltts._seed, dict(ltts.backbone.counters)
    for bad in (0, -1, 2.0, "2", True):
        with pytest.raises(ValueError):
            NeuTTS(backbone_repo=None, best_of=bad)                                        # (checked before anything is loaded)
        with pytest.raises(ValueError):
            ltts.generate_codes([prompt], best_of=bad)
        with pytest.raises(ValueError):
            ltts.infer("Testing.", REF, "So I'm live.", best_of=bad)
        with pytest.raises(ValueError):
            ltts.infer_batch(["a", "b"], REF, "So I'm live.", best_of=[1, bad])
    with pytest.raises(ValueError):
        NeuTTS(backbone_repo=None, logprobs="yes")
    with pytest.raises(ValueError):
        NeuTTS(backbone_repo=None, do_sample=False, best_of=2)
    with pytest.raises(ValueError):
        ltts.infer_batch(["a", "b"], REF, "So I'm live.", best_of=[2])                     # one value per utterance, or one for all
    with pytest.raises(ValueError):
        ltts.generate_codes([prompt], return_logprobs=1)
    with pytest.raises(ValueError):
        ltts.infer("Testing.", REF, "So I'm live.", return_scores="yes")
    with pytest.raises(TypeError):
        ltts.generate_codes([prompt], return_scores=True)                                  # infer's flag, not generate_codes'
    ltts.do_sample = False                                                                 # a greedy instance: identical candidates
    try:
        with pytest.raises(ValueError, match="do_sample"):
            ltts.generate_codes([prompt], best_of=2)
        with pytest.raises(ValueError, match="do_sample"):
            ltts.infer_batch(["a", "b"], REF, "So I'm live.", best_of=[1, 3])
    finally:
        ltts.do_sample = True
    assert ltts._seed == seed and ltts.backbone.counters == calls and ltts.backbone.free_slots() == ltts.backbone.max_batch
    assert not ltts.backbone.logprobs


def test_stream_entry_points_reject_the_keywords(ltts):
    seed = ltts._seed
    for kw in (dict(best_of=2), dict(return_scores=True), dict(return_logprobs=True)):
        with pytest.raises(TypeError, match=next(iter(kw))):
            ltts.infer_stream("Streaming.", REF, "So I'm live.", **kw)
        with pytest.raises(TypeError, match=next(iter(kw))):
            ltts.infer_stream_batch(["a", "b"], REF, "So I'm live.", **kw)
    assert ltts._seed == seed and ltts.backbone.free_slots() == ltts.backbone.max_batch


def test_a_suspended_stream_blocks_the_temporary_switch(ltts):
    ltts.stream_on_device = False
    try:
        gen = ltts.infer_stream("Streaming.", REF, "So I'm live.")
        next(gen)                                                                          # suspended: it holds a decode slot
        assert ltts.backbone.free_slots() < ltts.backbone.max_batch
        with pytest.raises(RuntimeError, match="stream"):
            ltts.infer("Testing.", REF, "So I'm live.", return_scores=True)
        assert not ltts.backbone.logprobs
        assert isinstance(ltts.infer("Testing.", REF, "So I'm live."), np.ndarray)         # a call that needs no scores still runs beside it
        list(gen)
    finally:
        del ltts.stream_on_device
    assert ltts.backbone.free_slots() == ltts.backbone.max_batch
    assert ltts.infer("Testing.", REF, "So I'm live.", return_scores=True)[1] <= 0        # the stream is done: the switch can be borrowed again


def test_constructor_switch_stays_on(emu_lib):
    check_constructor_switch(emu_lib)


def check_constructor_switch(lib):
    import neutts
    real = neutts.NeuTTS
    neutts.NeuTTS = functools.partial(real, logprobs=True)
    try:
        t = build_logprob_tts(lib, max_batch=2)
    finally:
        neutts.NeuTTS = real
    t.best_of = 2                                                                          # (build_tts constructs a greedy instance: best_of follows do_sample)
    try:
        assert t.backbone.logprobs and (t.logprobs, t.best_of) == (True, 2)
        prompt = t._apply_chat_template(REF, "So I'm live.", "Testing.")
        with Spy(t.backbone) as spy:
            ids, lps = t.generate_codes([prompt], return_logprobs=True, **HOT)            # the instance's best_of
        assert len(spy.requests) == 2 and t.backbone.logprobs
        cand = by_index(t, spy)
        again_ids, again_lps = t.backbone.generate([r[0] for r in cand], [r[1] for r in cand], return_logprobs=True)
        win = int(np.argmax([spec.sequence_score(lp) for lp in again_lps]))
        assert ids == [again_ids[win]] and np.array_equal(lps[0], again_lps[win])
        with Spy(t.backbone) as spy:
            t.generate_codes([prompt], best_of=1)                                         # a per-call override
        assert len(spy.requests) == 1 and t.backbone.logprobs
        gen = t.infer_stream("Streaming.", REF, "So I'm live.")                            # the streams run with the record on, untouched by it
        assert len(list(gen)) >= 1
    finally:
        t.close()
