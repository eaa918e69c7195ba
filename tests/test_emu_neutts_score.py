"""Teacher-forced scoring on the class surface: `NeuTTS.score` / `score_batch` assemble prompt + speech-token ids (+ the end token) and hand them to
`BackboneEngine.score`; the values are the engine's on the same ids, `score` is their mean, `top1_agreement` the share of positions where the
model's argmax is the given token; bad arguments raise ValueError before the engine is touched.
On the SIMT emulator; tests/test_gpu_score.py runs the same bodies on libneutts_hip.so."""
import inspect

import numpy as np
import pytest

import logprob_spec as spec
import test_emu_neutts_logprobs as class_cases
from test_emu_neutts_sampling import REF, TEXTS

REF_TEXT = "So I'm live."


@pytest.fixture(scope="module")
def ltts(emu_lib):
    return class_cases.build_logprob_tts(emu_lib, max_batch=3)


def some_codes(tts, n, seed):
    n_codes = tts._oracle[4].vocab_size - tts._speech_base
    return np.random.default_rng(seed).integers(0, min(n_codes, 65536), n).tolist()


def test_score_signatures(ltts):
    from neutts import NeuTTS
    for name in ("score", "score_batch"):
        q = inspect.signature(getattr(NeuTTS, name)).parameters
        assert list(q)[-1] == "include_eos" and q["include_eos"].default is True
    assert list(inspect.signature(NeuTTS.score).parameters) == ["self", "text", "codes", "ref_codes", "ref_text", "include_eos"]
    assert list(inspect.signature(NeuTTS.score_batch).parameters) == ["self", "texts", "codes", "ref_codes", "ref_texts", "include_eos"]
    q = inspect.signature(ltts.backbone.score).parameters
    assert list(q) == ["seqs", "score_from", "chunk_rows"] and q["score_from"].default is None and q["chunk_rows"].default == 0
    assert not ltts.logprobs and not ltts.backbone.logprobs                                # no constructor switch is needed


def test_score_equals_the_engine_on_the_assembled_ids(ltts):
    codes = some_codes(ltts, 9, 1)
    prompt = ltts._apply_chat_template(REF, REF_TEXT, TEXTS[1])
    ids = prompt + [ltts._speech_base + c for c in codes] + [ltts._eos_id]
    assert ltts._ids_to_codes(ids[len(prompt):]) == codes                                  # the inverse of _ids_to_codes
    (lp, am, alp), = ltts.backbone.score([ids], len(prompt))
    free0 = ltts.backbone.kv_stats()["free_pages"]
    got = ltts.score(TEXTS[1], codes, REF, REF_TEXT)
    assert sorted(got) == ["logprobs", "score", "top1_agreement"]
    assert got["logprobs"].dtype == np.float32 and np.array_equal(got["logprobs"].view(np.uint32), lp.view(np.uint32)) and len(lp) == 10
    assert got["score"] == spec.sequence_score(lp) and got["score"] < 0
    assert got["top1_agreement"] == float(np.mean(am == np.asarray(ids[len(prompt):])))
    assert ltts.backbone.kv_stats()["free_pages"] == free0 and ltts.backbone.free_slots() == ltts.backbone.max_batch
    short = ltts.score(TEXTS[1], codes, REF, REF_TEXT, include_eos=False)                  # exactly one entry fewer, the others unchanged
    assert len(short["logprobs"]) == 9 and np.array_equal(short["logprobs"].view(np.uint32), lp[:9].view(np.uint32))
    assert not ltts.backbone.logprobs


def test_top1_agreement_of_the_models_own_greedy_run(ltts):
    """What greedy decoding emits is the argmax everywhere: agreement 1 on its own output, less on a sequence with some codes replaced."""
    was = ltts.do_sample
    ltts.do_sample = False
    try:
        prompt = ltts._apply_chat_template(REF, REF_TEXT, TEXTS[2])
        own = ltts._ids_to_codes(ltts.generate_codes([prompt])[0])
    finally:
        ltts.do_sample = was
    assert len(own) >= 5
    assert ltts.score(TEXTS[2], own, REF, REF_TEXT, include_eos=False)["top1_agreement"] == 1.0
    n_codes = ltts._oracle[4].vocab_size - ltts._speech_base
    other = list(own)
    other[2] = (other[2] + 1) % n_codes
    got = ltts.score(TEXTS[2], other, REF, REF_TEXT, include_eos=False)
    assert got["top1_agreement"] <= 1.0 - 1.0 / len(own) and got["score"] < ltts.score(TEXTS[2], own, REF, REF_TEXT, include_eos=False)["score"]


def test_score_batch_equals_single_calls(ltts):
    texts = TEXTS[1:5]                                                                     # more utterances than decode slots: two engine calls
    codes = [some_codes(ltts, 5 + 3 * i, 10 + i) for i in range(len(texts))]
    many = ltts.score_batch(texts, codes, REF, REF_TEXT)
    assert len(many) == len(texts)
    for t, c, m in zip(texts, codes, many):
        one = ltts.score(t, c, REF, REF_TEXT)
        assert np.array_equal(one["logprobs"].view(np.uint32), m["logprobs"].view(np.uint32)) and len(m["logprobs"]) == len(c) + 1
        assert one["score"] == m["score"] and one["top1_agreement"] == m["top1_agreement"]
    per_ref = ltts.score_batch(texts[:2], codes[:2], [REF, REF], [REF_TEXT, REF_TEXT], include_eos=False)
    assert all(np.array_equal(a["logprobs"], b["logprobs"][:-1]) for a, b in zip(per_ref, many))


def test_bad_arguments_raise_before_the_engine_is_touched(ltts):
    eng = ltts.backbone
    calls = []
    real = eng.score
    eng.score = lambda *a, **k: calls.append(a) or real(*a, **k)
    n_codes = ltts._oracle[4].vocab_size - ltts._speech_base
    try:
        for kw in (dict(codes=[]), dict(codes=[1, -1]), dict(codes=[1, 65536]), dict(codes=[1, 2.5]), dict(codes=[True, 2]), dict(include_eos=1),
                   dict(include_eos=None), dict(codes=[n_codes + 5] if n_codes < 65536 else [-3]), dict(codes=[1] * 4096)):
            a = dict(codes=[1, 2, 3], include_eos=True)
            a.update(kw)
            with pytest.raises(ValueError):
                ltts.score(TEXTS[1], a["codes"], REF, REF_TEXT, a["include_eos"])
        with pytest.raises(ValueError):
            ltts.score_batch(TEXTS[1:3], [[1, 2]], REF, REF_TEXT)                          # one code sequence for two utterances
        with pytest.raises(ValueError):
            ltts.score_batch(TEXTS[1:3], [[1, 2], [3]], [REF], [REF_TEXT])
        eng.logits_range = (ltts._speech_base, ltts._speech_base + 8, ltts._eos_id)      # what set_logits_range records: the restricted head
        try:
            with pytest.raises(RuntimeError, match="whole vocabulary"):
                ltts.score(TEXTS[1], [1, 2, 3], REF, REF_TEXT)
        finally:
            eng.logits_range = None
        assert calls == []
    finally:
        del eng.score
