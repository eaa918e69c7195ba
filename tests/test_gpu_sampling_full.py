"""Sampling over the whole vocabulary (top_k = -1) on a real MI355X through libneutts_hip.so: the bodies of tests/test_emu_sampling_full.py
and tests/test_emu_neutts_sampling_full.py re-bound to the product library, plus NeuTTS-Air geometry (24 layers, V = 217 488, 256 slots):
256 seeded first-token draws at top_k -1 / top_p 0.95 / T 1.0 and three decode steps against tests/sampling_full_spec.py on the tapped
rows, and the kernel-level probe on rows of that width with the row's maximum taken both ways."""
import numpy as np
import pytest
import torch

from oracle import backbone_ref as br
from neutts import _hip
from common import load_fixture, make_engine
import sampling_full_spec as full
import test_emu_neutts_sampling_full as class_cases
import test_emu_sampling_full as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(hip_lib):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _hip.load_library(hip_lib)
    return hip_lib


model = cases.model


@pytest.fixture(scope="module")
def tts(lib):
    return class_cases.build_sampling_tts(lib, max_batch=3)


@pytest.fixture(scope="module")
def tts_off(lib):
    return class_cases.build_off_tts(lib, max_batch=3)


# the shared bodies: collected here under the gpu mark, resolved against THIS module's `lib` / `tts` / `tts_off` fixtures
test_probe_survivors_draw_and_total_meet_the_specification = cases.test_probe_survivors_draw_and_total_meet_the_specification
test_probe_refuses_invalid_parameters = cases.test_probe_refuses_invalid_parameters
test_every_draw_meets_the_specification = cases.test_every_draw_meets_the_specification
test_mixed_step_ids_do_not_depend_on_the_neighbours = cases.test_mixed_step_ids_do_not_depend_on_the_neighbours
test_logprob_of_a_whole_vocabulary_draw_under_a_repetition_penalty = cases.test_logprob_of_a_whole_vocabulary_draw_under_a_repetition_penalty
test_compacted_head_maps_the_drawn_column_to_its_id = cases.test_compacted_head_maps_the_drawn_column_to_its_id
test_invalid_top_k_is_refused_and_greedy_ignores_the_field = cases.test_invalid_top_k_is_refused_and_greedy_ignores_the_field
test_constructor_value_reaches_the_engine = class_cases.test_constructor_value_reaches_the_engine
test_per_call_and_per_utterance_values_reach_the_engine = class_cases.test_per_call_and_per_utterance_values_reach_the_engine
test_both_stream_paths = class_cases.test_both_stream_paths
test_best_of_and_logprobs = class_cases.test_best_of_and_logprobs
test_bad_values_raise_before_the_engine_is_touched = class_cases.test_bad_values_raise_before_the_engine_is_touched

T, TOP_P, MIN_P = 1.0, 0.95, 0.0


def test_air_geometry_first_token_draws_and_decode_steps(lib):
    z, cfg, w = load_fixture("backbone_air")
    eng = make_engine(cfg, w, lib, max_batch=256, max_context=1024, max_prefill_tokens=8192)
    S, eos = int(z["s_len"]), int(z["eos"])
    p = br.synthetic_prompt(cfg, 0, S)
    eng.set_debug(True)
    try:
        for c in range(0, 256, 16):
            sp = [_hip.Sampling(max_length=S + 4, min_new_tokens=4, eos_token_id=eos, do_sample=True, top_k=_hip.TOP_K_OFF, temperature=T, top_p=TOP_P,
                                min_p=MIN_P, seed=91_000 + c + i) for i in range(16)]
            eng.prefill([p] * 16, list(range(c, c + 16)), sp)
        ids, _ = eng.read_all()
        row = eng.read_logits(0)
        assert np.array_equal(eng.read_logits(255), row)                          # same prompt -> same logits in every slot
        e, q = full.masses(row, T)
        keep = full.survivors(row, T, TOP_P, MIN_P, eq=(e, q))
        print(f"Air first token: {int(keep.sum())} of {row.size} columns survive top_p {TOP_P}")
        assert 512 < int(keep.sum()) < row.size                                   # more than the top-k sampler can hold, and the nucleus did cut
        inexact = 0
        for s in range(256):
            tok, Ssum, target = full.draw(keep, q, 91_000 + s, 0)
            d = full.FullDraw(tok, keep, Ssum, target, q, e)
            inexact += not cases.check_token(d, row, T, TOP_P, MIN_P, ids[s][0])
        assert inexact * 10 <= 256, inexact
        assert len({ids[s][0] for s in range(256)}) > 100                         # 256 seeds, a flat distribution: mostly different tokens
        inexact = 0
        for step in range(3):
            eng.decode(1)
            ids2, _ = eng.read_all()
            for s in (0, 17, 255):
                r2 = eng.read_logits(s)
                d = full.sample(r2, T, 91_000 + s, len(ids2[s]) - 1, TOP_P, MIN_P)
                inexact += not cases.check_token(d, r2, T, TOP_P, MIN_P, ids2[s][-1])
        assert inexact <= 0, inexact                                              # (10 % of nine)
        for s in range(256):
            eng.release(s)
    finally:
        eng.set_debug(False)
        eng.close()


def test_probe_at_air_vocabulary(lib):
    V = 217_488
    rows = cases.synthetic_rows(V, 11, n_random=6)
    a = cases.check_full_probe(lib, V, V, 96, rows)        # the lm_head epilogue's group width at this vocabulary
    b = cases.check_full_probe(lib, V, V, 0, rows)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
