"""Teacher-forced scoring on a real MI355X through libneutts_hip.so: the bodies of tests/test_emu_score.py and tests/test_emu_neutts_score.py
re-bound to the product library, the scoring probe at NeuTTS-Air's real width on the 256-row tiles, and one NeuTTS-Air-geometry engine checked
against the specification on the tapped rows and against the fixture's golden greedy ids."""
import pytest
import torch

from oracle import backbone_ref as br
from neutts import _hip
from common import bf16_ulp, load_fixture, make_engine
import test_emu_score as cases
import test_emu_neutts_score as class_cases
import test_emu_neutts_logprobs as logprob_class_cases

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
    return logprob_class_cases.build_logprob_tts(lib, max_batch=3)


# the shared bodies: collected here under the gpu mark, resolved against THIS module's `lib` / `ltts` fixtures
test_target_epilogue_and_merge_equal_the_specification = cases.test_target_epilogue_and_merge_equal_the_specification
test_target_epilogue_with_large_logits = cases.test_target_epilogue_with_large_logits
test_score_probe_refuses_bad_arguments = cases.test_score_probe_refuses_bad_arguments
test_engine_on_the_tapped_rows = cases.test_engine_on_the_tapped_rows
test_engine_on_the_tapped_rows_vocabulary_3000 = cases.test_engine_on_the_tapped_rows_vocabulary_3000
test_engine_on_the_tapped_rows_general_attention = cases.test_engine_on_the_tapped_rows_general_attention
test_chunking_and_packing_do_not_change_a_bit = cases.test_chunking_and_packing_do_not_change_a_bit
test_against_the_oracle = cases.test_against_the_oracle
test_against_generation = cases.test_against_generation
test_running_requests_do_not_notice = cases.test_running_requests_do_not_notice
test_refusals_leave_the_engine_as_it_was = cases.test_refusals_leave_the_engine_as_it_was
test_pages_that_do_not_fit_and_a_tap_that_would_not = cases.test_pages_that_do_not_fit_and_a_tap_that_would_not
test_fp8_engine_on_the_tapped_rows = cases.test_fp8_engine_on_the_tapped_rows
test_score_signatures = class_cases.test_score_signatures
test_score_equals_the_engine_on_the_assembled_ids = class_cases.test_score_equals_the_engine_on_the_assembled_ids
test_top1_agreement_of_the_models_own_greedy_run = class_cases.test_top1_agreement_of_the_models_own_greedy_run
test_score_batch_equals_single_calls = class_cases.test_score_batch_equals_single_calls
test_bad_arguments_raise_before_the_engine_is_touched = class_cases.test_bad_arguments_raise_before_the_engine_is_touched


@pytest.mark.parametrize("variant,fp8", [("256x288", False), ("256x256", False), ("256x256", True)])
def test_score_probe_at_air_width(lib, variant, fp8):
    """V = 217 488 (no multiple of 288 nor of 256: the last tile is part padding; 2 266 - 3 400 partials per row), K = 896, 70 rows."""
    cases.check_score_probe(lib, variant, 70, 217_488, 896, fp8, seed=7)


def test_air_geometry_eight_rows(lib):
    """NeuTTS-Air geometry (24 layers, V = 217 488): the fixture's 500-token prompt followed by the first 8 ids of its golden greedy run, scored
    from 500 with the tap on.  Every value against the specification on its tapped row, argmax exact, and the argmax ids are transformers' greedy
    ids on the steps the fixture does not mark as near-tied (golden top-2 gap above 4 bf16 ulps).  With the tap on, scoring all 507 positions would
    keep 441 MB of rows: refused."""
    z, cfg, w = load_fixture("backbone_air")
    eng = make_engine(cfg, w, lib, max_batch=2, max_context=1024, max_prefill_tokens=1024)
    S = int(z["s_len"])
    gold, tv = [int(t) for t in z["bf16_ids_0"][:8]], z["bf16_topv_0"]
    seq = br.synthetic_prompt(cfg, 0, S) + gold
    try:
        lp, am, alp = cases.tapped_check(eng, [seq], [S], [1], tag="NeuTTS-Air geometry")
        assert len(lp) == 8
        clear = [k for k in range(8) if tv[k][0] - tv[k][1] > 4.0 * bf16_ulp(float(tv[k][0]))]
        print(f"[score] NeuTTS-Air geometry: argmax {am.tolist()}, golden {gold}, clear steps {clear}")
        assert len(clear) >= 4 and all(am[k] == gold[k] for k in clear)
        eng.set_debug(True)
        with pytest.raises(_hip.NeuTTSHipError, match="64 MB") as ei:
            eng.score_call([seq], [0], [1])
        assert ei.value.code == -1
        st = eng.kv_stats()
        assert st["free_pages"] == st["total_pages"]
    finally:
        eng.set_debug(False)
        eng.close()
