"""Repetition penalty on a real MI355X through libneutts_hip.so: the bodies of tests/test_emu_repetition.py and
tests/test_emu_neutts_repetition.py re-bound to the product library (captured step graphs included: the emulator has none), the
lm_head probe at NeuTTS-Air's real width on the tiles the 256-slot engines run, one NeuTTS-Air-geometry engine with penalties 1.0 / 1.3
alternating across its slots, and the wide lock-step shape (640 slots) with penalised requests in its first and its last m-block."""
import numpy as np
import pytest
import torch

from oracle import backbone_ref as br
from neutts import _hip
from common import load_fixture, make_engine
import repetition_spec as rspec
import test_emu_neutts_repetition as class_cases
import test_emu_repetition as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(hip_lib):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _hip.load_library(hip_lib)
    return hip_lib


model = cases.model
model3000 = cases.model3000


@pytest.fixture(scope="module")
def rtts(lib):
    return class_cases.build_repetition_tts(lib, max_batch=3)


# the shared bodies: collected here under the gpu mark, resolved against THIS module's `lib` / `rtts` fixtures
test_epilogue_equals_the_specification = cases.test_epilogue_equals_the_specification
test_probe_refuses_bad_arguments = cases.test_probe_refuses_bad_arguments
test_bitmap_follows_prompt_and_generated_tokens = cases.test_bitmap_follows_prompt_and_generated_tokens
test_bitmap_moves_with_a_parked_request = cases.test_bitmap_moves_with_a_parked_request
test_shared_prefix_prompt_marks_the_full_prompt = cases.test_shared_prefix_prompt_marks_the_full_prompt
test_restricted_head_bitmap_is_column_indexed = cases.test_restricted_head_bitmap_is_column_indexed
test_first_token_and_every_step_on_the_tapped_row = cases.test_first_token_and_every_step_on_the_tapped_row
test_first_token_and_every_step_vocabulary_3000 = cases.test_first_token_and_every_step_vocabulary_3000
test_unpenalised_batches_do_not_change = cases.test_unpenalised_batches_do_not_change
test_invalid_values_are_refused_and_touch_no_slot = cases.test_invalid_values_are_refused_and_touch_no_slot
test_signatures_keep_the_reference_positionals = class_cases.test_signatures_keep_the_reference_positionals
test_constructor_arguments_reach_the_engine = class_cases.test_constructor_arguments_reach_the_engine
test_per_call_overrides_and_per_utterance_lists = class_cases.test_per_call_overrides_and_per_utterance_lists
test_stream_entry_points = class_cases.test_stream_entry_points
test_bad_values_raise_before_the_engine_is_touched = class_cases.test_bad_values_raise_before_the_engine_is_touched


@pytest.mark.parametrize("variant,fp8", [("256x288", False), ("256x256", False), ("256x256", True)])
def test_probe_at_air_width(lib, variant, fp8):
    """V = 217 488 (no multiple of 288 nor of 256: the last tile is part padding), K = 896, 70 rows."""
    cases.check_head_probe(lib, variant, 70, 217_488, 896, fp8, seed=7)


def test_air_geometry_alternating_penalties(lib):
    """256 slots, the same prompt everywhere, penalty 1.0 in the even slots and 1.3 in the odd ones (three of them sampling): the first
    token's row is penalise(an even slot's row, set(prompt), 1.3) bit for bit, and over three decode steps every checked id is the
    specification's choice on that step's tapped row while the bitmap follows the ids."""
    z, cfg, w = load_fixture("backbone_air")
    eng = make_engine(cfg, w, lib, max_batch=256, max_context=1024, max_prefill_tokens=8192)
    S, eos = int(z["s_len"]), int(z["eos"])
    p = br.synthetic_prompt(cfg, 0, S)
    sampled = {17: 1017, 128 + 33: 2033, 255: 3255}                       # slot -> seed; first, middle and last m-block of the 256-row tile
    st = {s: dict(do_sample=True, top_k=50, temperature=1.0, top_p=0.95, min_p=0.05, seed=seed) for s, seed in sampled.items()}
    eng.set_debug(True)
    try:
        for c in range(0, 256, 16):
            sp = [_hip.Sampling(max_length=S + 8, min_new_tokens=8, eos_token_id=eos, repetition_penalty=1.3 if s % 2 else 1.0,
                                **st.get(s, dict(do_sample=False))) for s in range(c, c + 16)]
            eng.prefill([p] * 16, list(range(c, c + 16)), sp)
        plain = eng.read_logits(0)
        want = rspec.penalise(plain, set(p), 1.3)
        assert (want != plain).sum() >= len(set(p)) - 2
        ids, _ = eng.read_all()
        for s in (1, 17, 63, 161, 241, 255):                              # odd slots: penalised
            # every prompt pass runs the lm_head over ALL rows: the tap of a slot filled by an EARLIER pass was rewritten by the later ones, from
            # the same hidden state and with the bitmap as it stood by then -- its first token included; the last pass's slots (240 ..) show
            # the row their first token was chosen from
            row, seen = eng.read_logits(s), set(p) | ({ids[s][0]} if s < 240 else set())
            assert cases.seen_of(eng, s) == set(p) | {ids[s][0]}
            want_s = rspec.penalise(plain, seen, 1.3)
            assert np.array_equal(row.view(np.uint32), want_s.view(np.uint32)), (s, np.flatnonzero(row != want_s)[:8])
            assert cases.check_choice(want, ids[s][0], st.get(s, {}), 0) >= 0
        assert np.array_equal(eng.read_logits(254), plain) and ids[0][0] == rspec.first_argmax(plain) == ids[254][0]
        assert ids[1][0] == rspec.first_argmax(want)
        compared = 0
        for step in range(1, 4):
            eng.decode(1)
            ids, _ = eng.read_all()
            for s in sorted(sampled) + [1]:
                assert len(ids[s]) == step + 1
                row = eng.read_logits(s)
                compared += cases.check_choice(row, ids[s][step], st.get(s, {}), step)
                assert cases.seen_of(eng, s) == rspec.seen_set(p, ids[s])
                assert row[eos] == -np.inf and np.array_equal(rspec.bf16_round(row), row)      # bf16-valued, EOS masked
        assert compared >= 10                                              # of 12; the rest sat within MARGIN of a boundary
        assert cases.seen_of(eng, 0) == set() and cases.seen_of(eng, 254) == set()
    finally:
        eng.set_debug(False)
        eng.close()


def test_wide_shape_first_and_last_m_block(lib):
    """The wide lock-step step (640 slots: the 256 x 256 lm_head tile on three m-blocks) with a penalised request in row 0 and one in a
    row >= 512, unpenalised requests around them: their bitmaps and ids are their own -- equal to the same request run next to nothing
    else in another slot -- and each first-token row is penalise(its unpenalised twin's row)."""
    cfg = br.BackboneConfig(vocab_size=3000, hidden_size=896, intermediate_size=1216, num_layers=2)
    w = br.make_weights(cfg, 41)
    eng = make_engine(cfg, w, lib, max_batch=640, max_context=128, max_prefill_tokens=4096)
    N, eos = 6, cfg.vocab_size - 1
    pa, pb = br.synthetic_prompt(cfg, 70, 33), br.synthetic_prompt(cfg, 71, 47)

    def sp(p, **kw):
        return _hip.Sampling(max_length=len(p) + N, min_new_tokens=N, eos_token_id=eos, do_sample=False, **kw)

    ka, kb = dict(repetition_penalty=1.3), dict(repetition_penalty=2.0, prompt_ignore_length=10)
    # each request by itself, in some other slot
    alone = {}
    for name, p, kw, slot in (("a", pa, ka, 300), ("b", pb, kb, 77)):
        eng.prefill([p], [slot], [sp(p, **kw)])
        eng.decode(N - 1)
        alone[name] = (eng.read(slot)[0], cases.seen_of(eng, slot))
        eng.release(slot)
    assert alone["a"][1] == rspec.seen_set(pa, alone["a"][0]) and alone["b"][1] == rspec.seen_set(pb, alone["b"][0], 10)
    eng.set_debug(True)
    try:
        fillers = [s for s in range(640) if s not in (0, 1, 600, 601)][::5]
        fp = [br.synthetic_prompt(cfg, 500 + s, 12 + s % 30) for s in fillers]
        eng.prefill([pa, pa, pb, pb] + fp, [0, 1, 600, 601] + fillers, [sp(pa, **ka), sp(pa), sp(pb, **kb), sp(pb)] + [sp(q) for q in fp])
        for s, p, kw in ((0, pa, ka), (600, pb, kb)):
            row, plain = eng.read_logits(s), eng.read_logits(s + 1)
            want = rspec.penalise(plain, rspec.seen_set(p, (), kw.get("prompt_ignore_length", 0)), kw["repetition_penalty"])
            assert np.array_equal(row.view(np.uint32), want.view(np.uint32)) and (row != plain).any()
            assert eng.read(s)[0][0] == rspec.first_argmax(row)
        eng.decode(N - 1)
        for s, name in ((0, "a"), (600, "b")):
            assert eng.read(s)[0] == alone[name][0] and cases.seen_of(eng, s) == alone[name][1], (s, eng.read(s)[0], alone[name][0])
        assert cases.seen_of(eng, 1) == set() and cases.seen_of(eng, 601) == set() and cases.seen_of(eng, fillers[3]) == set()
        assert alone["a"][1] != alone["b"][1]
    finally:
        eng.set_debug(False)
        eng.close()
