"""Per-token log-probabilities and best-of-N on a real MI355X through libneutts_hip.so: the bodies of tests/test_emu_logprobs.py and
tests/test_emu_neutts_logprobs.py re-bound to the product library (captured step graphs included: the emulator has none), the lm_head probe at
NeuTTS-Air's real width on the tiles the 256-slot engines run, the wide lock-step shape (640 slots) with recorded rows in its first and its last
m-block, and one NeuTTS-Air-geometry engine checked against the specification on six slots' tapped rows."""
import numpy as np
import pytest
import torch

from oracle import backbone_ref as br
from neutts import _hip
from common import load_fixture, make_engine
import logprob_spec as spec
import test_emu_logprobs as cases
import test_emu_neutts_logprobs as class_cases
from test_emu_logprobs import LSE_TOL, WARPED

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(hip_lib):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _hip.load_library(hip_lib)
    return hip_lib


model = cases.model
model3000 = cases.model3000


@pytest.fixture(scope="module")
def ltts(lib):
    return class_cases.build_logprob_tts(lib, max_batch=3)


# the shared bodies: collected here under the gpu mark, resolved against THIS module's `lib` / `ltts` fixtures
test_lse_epilogue_equals_the_specification = cases.test_lse_epilogue_equals_the_specification
test_lse_epilogue_with_large_logits = cases.test_lse_epilogue_with_large_logits
test_logprob_probe_refuses_bad_arguments = cases.test_logprob_probe_refuses_bad_arguments
test_record_on_the_tapped_rows = cases.test_record_on_the_tapped_rows
test_record_on_the_tapped_rows_vocabulary_3000 = cases.test_record_on_the_tapped_rows_vocabulary_3000
test_eos_token_has_an_entry = cases.test_eos_token_has_an_entry
test_record_follows_the_request = cases.test_record_follows_the_request
test_restricted_head_values_follow_the_compacted_row = cases.test_restricted_head_values_follow_the_compacted_row
test_read_finished_equals_read_and_state_errors = cases.test_read_finished_equals_read_and_state_errors
test_off_means_unchanged = cases.test_off_means_unchanged
test_signatures_and_defaults = class_cases.test_signatures_and_defaults
test_generate_codes_returns_the_engines_logprobs = class_cases.test_generate_codes_returns_the_engines_logprobs
test_scores_are_the_mean_logprob = class_cases.test_scores_are_the_mean_logprob
test_best_of_three_picks_the_highest_mean = class_cases.test_best_of_three_picks_the_highest_mean
test_best_of_per_utterance = class_cases.test_best_of_per_utterance
test_a_candidate_without_speech_tokens_cannot_win = class_cases.test_a_candidate_without_speech_tokens_cannot_win
test_bad_values_raise_before_the_engine_is_touched = class_cases.test_bad_values_raise_before_the_engine_is_touched
test_stream_entry_points_reject_the_keywords = class_cases.test_stream_entry_points_reject_the_keywords
test_a_suspended_stream_blocks_the_temporary_switch = class_cases.test_a_suspended_stream_blocks_the_temporary_switch


def test_constructor_switch_stays_on(lib):
    class_cases.check_constructor_switch(lib)


@pytest.mark.parametrize("variant,fp8", [("256x288", False), ("256x256", False), ("256x256", True)])
def test_probe_at_air_width(lib, variant, fp8):
    """V = 217 488 (no multiple of 288 nor of 256: the last tile is part padding; 2 266 - 3 400 partials per row), K = 896, 70 rows."""
    cases.check_logprob_probe(lib, variant, 70, 217_488, 896, fp8, seed=7)


def test_wide_shape_first_and_last_m_block(lib):
    """The wide lock-step step (640 slots: the 256 x 256 lm_head tile on three m-blocks) with a sampled, penalised request in row 0 and a greedy
    one in a row >= 512, other requests around them: ids and log-probabilities are bit for bit those of the same request run next to nothing
    else in another slot, and every entry is the specification's value on that step's tapped row."""
    cfg = br.BackboneConfig(vocab_size=3000, hidden_size=896, intermediate_size=1216, num_layers=2)
    w = br.make_weights(cfg, 41)
    eng = make_engine(cfg, w, lib, max_batch=640, max_context=128, max_prefill_tokens=4096)
    N, eos = 5, cfg.vocab_size - 1
    pa, pb = br.synthetic_prompt(cfg, 70, 33), br.synthetic_prompt(cfg, 71, 47)

    def sp(p, **kw):
        return _hip.Sampling(**dict(dict(max_length=len(p) + N, min_new_tokens=N, eos_token_id=eos, do_sample=False), **kw))

    ka, kb = dict(WARPED, repetition_penalty=1.3), dict()
    eng.set_logprobs(True)
    eng.set_debug(True)
    try:
        alone = {}
        for name, p, kw, slot in (("a", pa, ka, 300), ("b", pb, kb, 77)):                  # each request by itself, in some other slot
            eng.prefill([p], [slot], [sp(p, **kw)])
            eng.decode(N - 1)
            alone[name] = (eng.read(slot)[0], eng.read_logprobs(slot))
            eng.release(slot)
            assert len(alone[name][1]) == N and (alone[name][1] <= 0).all()
        fillers = [s for s in range(640) if s not in (0, 600)][::5]
        fp = [br.synthetic_prompt(cfg, 500 + s, 12 + s % 30) for s in fillers]
        eng.prefill([pa, pb] + fp, [0, 600] + fillers, [sp(pa, **ka), sp(pb, **kb)] + [sp(q, **(WARPED if i % 2 else {})) for i, q in enumerate(fp)])
        worst = 0.0
        for step in range(N):
            if step:
                eng.decode(1)
            for s in (0, 600, fillers[3], fillers[-1]):
                row, ids, lp = eng.read_logits(s), eng.read(s)[0], eng.read_logprobs(s)
                assert len(ids) == len(lp) == step + 1
                worst = max(worst, abs(float(lp[step]) - spec.logprob(row, ids[step])))
        print(f"[logprobs] wide shape: max |logprob - spec| = {worst:.3e} (bound {LSE_TOL:.0e})")
        assert worst <= LSE_TOL
        for s, name in ((0, "a"), (600, "b")):
            ids, lp = eng.read(s)[0], eng.read_logprobs(s)
            assert ids == alone[name][0] and np.array_equal(lp.view(np.uint32), alone[name][1].view(np.uint32)), (s, lp, alone[name][1])
    finally:
        eng.set_debug(False)
        eng.close()


def test_air_geometry_six_slots(lib):
    """256 slots at NeuTTS-Air geometry (V = 217 488: the 256 x 288 tile, 2 268 partials per row), the same prompt everywhere, sampled requests
    in three slots: the first token and three decode steps of six slots spread over the m-blocks, against the specification on their tapped
    rows.  (Every prompt pass runs the lm_head over ALL rows: the tap of a slot filled by an earlier pass is rewritten by the later ones from the
    same hidden state -- the same row, since nothing here is penalised and EOS stays masked.)"""
    z, cfg, w = load_fixture("backbone_air")
    eng = make_engine(cfg, w, lib, max_batch=256, max_context=1024, max_prefill_tokens=8192)
    S, eos = int(z["s_len"]), int(z["eos"])
    p = br.synthetic_prompt(cfg, 0, S)
    check = (0, 17, 63, 128 + 33, 241, 255)
    st = {s: dict(WARPED, seed=1000 + s) for s in (17, 128 + 33, 255)}
    eng.set_logprobs(True)
    eng.set_debug(True)
    try:
        for c in range(0, 256, 16):
            sps = [_hip.Sampling(**dict(dict(max_length=S + 8, min_new_tokens=8, eos_token_id=eos, do_sample=False), **st.get(s, {})))
                   for s in range(c, c + 16)]
            eng.prefill([p] * 16, list(range(c, c + 16)), sps)
        worst = 0.0
        for step in range(4):
            if step:
                eng.decode(1)
            ids, _ = eng.read_all()
            for s in check:
                row, lp = eng.read_logits(s), eng.read_logprobs(s)
                assert len(ids[s]) == len(lp) == step + 1 and row[eos] == -np.inf and lp[step] <= 0
                worst = max(worst, abs(float(lp[step]) - spec.logprob(row, ids[s][step])))
        print(f"[logprobs] NeuTTS-Air geometry: max |logprob - spec| = {worst:.3e} (bound {LSE_TOL:.0e})")
        assert worst <= LSE_TOL
        assert np.array_equal(eng.read_logprobs(0), eng.read_logprobs(254))                # greedy rows of one prompt: one record
    finally:
        eng.set_debug(False)
        eng.close()
