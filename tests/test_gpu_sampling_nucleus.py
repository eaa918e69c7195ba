"""Nucleus / min-p sampling on a real MI355X through libneutts_hip.so: the bodies of tests/test_emu_sampling_nucleus.py and
tests/test_emu_neutts_sampling.py re-bound to the product library, plus NeuTTS-Air geometry (24 layers, V = 217 488, 256 slots):
1024 seeded first-token draws at top_k 50 / top_p 0.95 / min_p 0.05 against tests/sampling_spec.py, three decode steps, and the
kernel-level probe on rows of that width on both of its paths."""
import numpy as np
import pytest
import torch

from oracle import backbone_ref as br
from neutts import _hip
from common import load_fixture, make_engine
import sampling_spec as spec
import test_emu_neutts_sampling as class_cases
import test_emu_sampling_nucleus as cases

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


# the shared bodies: collected here under the gpu mark, resolved against THIS module's `lib` / `tts` fixtures
test_probe_survivors_and_draw_equal_the_specification = cases.test_probe_survivors_and_draw_equal_the_specification
test_probe_refuses_invalid_parameters = cases.test_probe_refuses_invalid_parameters
test_every_draw_equals_the_specification = cases.test_every_draw_equals_the_specification
test_defaults_are_the_topk_sampler_and_ids_do_not_depend_on_placement = cases.test_defaults_are_the_topk_sampler_and_ids_do_not_depend_on_placement
test_first_token_distribution_over_the_surviving_set = cases.test_first_token_distribution_over_the_surviving_set
test_invalid_values_are_refused_and_touch_no_slot = cases.test_invalid_values_are_refused_and_touch_no_slot
test_signatures_keep_the_reference_positionals = class_cases.test_signatures_keep_the_reference_positionals
test_constructor_arguments_reach_the_engine = class_cases.test_constructor_arguments_reach_the_engine
test_per_call_overrides_reach_the_engine = class_cases.test_per_call_overrides_reach_the_engine
test_per_utterance_lists_in_the_batch_entry_points = class_cases.test_per_utterance_lists_in_the_batch_entry_points
test_stream_entry_points = class_cases.test_stream_entry_points
test_bad_values_raise_before_the_engine_is_touched = class_cases.test_bad_values_raise_before_the_engine_is_touched

K, T, TOP_P, MIN_P = 50, 1.0, 0.95, 0.05


def test_air_geometry_first_token_draws_and_decode_steps(lib):
    z, cfg, w = load_fixture("backbone_air")
    eng = make_engine(cfg, w, lib, max_batch=256, max_context=1024, max_prefill_tokens=8192)
    S, eos = int(z["s_len"]), int(z["eos"])
    p = br.synthetic_prompt(cfg, 0, S)
    eng.set_debug(True)
    try:
        exact, surv = 0, None
        for rep in range(4):
            for c in range(0, 256, 16):
                sp = [_hip.Sampling(max_length=S + 4, min_new_tokens=4, eos_token_id=eos, do_sample=True, top_k=K, temperature=T, top_p=TOP_P,
                                    min_p=MIN_P, seed=77_000 * rep + c + i) for i in range(16)]
                eng.prefill([p] * 16, list(range(c, c + 16)), sp)
            ids, _ = eng.read_all()
            if surv is None:
                row = eng.read_logits(0)
                surv = spec.survivors(row, K, T, TOP_P, MIN_P)
                n0 = len(spec.candidates(row, K, T)[0])
                print(f"Air first token: {n0} top-k candidates, {len(surv[0])} survive top_p {TOP_P} / min_p {MIN_P}, cut margin {surv[2]:.2e}")
                assert surv[2] > cases.MARGIN and len(surv[0]) < n0
            assert np.array_equal(eng.read_logits(255), row)                       # same prompt -> same logits, every slot / repeat
            for s in range(256):
                t = ids[s][0]
                assert t in surv[0], (rep, s, t)
                want, margin = spec.draw(surv[0], surv[1], 77_000 * rep + s, 0)
                if margin > cases.MARGIN:
                    assert t == want, (rep, s, t, want, margin)
                    exact += 1
            if rep == 0:
                for step in range(3):
                    eng.decode(1)
                    ids2, _ = eng.read_all()
                    for s in (0, 17, 255):
                        d = spec.sample(eng.read_logits(s), K, T, s, len(ids2[s]) - 1, TOP_P, MIN_P)
                        assert ids2[s][-1] in d.ids, (step, s)
                        assert min(d.margin, d.cut_margin) <= cases.MARGIN or ids2[s][-1] == d.token, (step, s, ids2[s][-1], d.token, d.margin)
            for s in range(256):
                eng.release(s)
        assert exact >= 1000, exact                                               # (of 1024 draws; the rest sat within 1e-5 of a boundary)
    finally:
        eng.set_debug(False)
        eng.close()


@pytest.mark.parametrize("group_width", [96, 0])       # the lm_head epilogue's group width at this vocabulary / the full-row fallback
def test_probe_at_air_vocabulary(lib, group_width):
    V = 217_488
    rows = cases.synthetic_rows(V, 11, n_random=6, k_max=200)
    cases.check_probe(lib, V, V, group_width, rows)
