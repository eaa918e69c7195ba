"""loudness=: the codec's BS.1770 loudness normalisation (include/neutts_hip.h ntts_codec_normalize / ntts_codec_measure_loudness /
ntts_codec_decode_loud) on a real MI355X through libneutts_hip.so: the bodies of tests/test_emu_loudness.py -- loudness, peak, gain and samples
against tests/loudness_spec.py, the untouched default, the decode entry points, refusals, the class -- rebound to the real library."""
import pytest
import torch

from oracle import backbone_ref as br
from neutts import _hip
import test_emu_loudness as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(hip_lib):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _hip.load_library(hip_lib)
    return cases.make_engine(hip_lib, True)


@pytest.fixture(scope="module")
def deng(hip_lib):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _hip.load_library(hip_lib)
    return cases.make_engine(hip_lib, True, max_frames=256, max_rows=1024, hop=cases.DECODE_HOP)


@pytest.fixture(scope="module")
def tts(hip_lib):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _hip.load_library(hip_lib)
    return cases.build_class(
        hip_lib, bcfg=lambda v: br.BackboneConfig(vocab_size=v, hidden_size=896, intermediate_size=1216, num_layers=3),
        max_batch=4, max_context=256, max_prefill_tokens=1024, seed=33)


# the shared bodies: collected here under the gpu mark, resolved against THIS module's `eng` / `deng` / `tts` fixtures
test_measure_loudness_equals_the_spec = cases.test_measure_loudness_equals_the_spec
test_normalize_equals_the_spec_row_by_row = cases.test_normalize_equals_the_spec_row_by_row
test_rows_with_the_option_off_and_unmeasurable_rows_are_the_input = cases.test_rows_with_the_option_off_and_unmeasurable_rows_are_the_input
test_parameters_per_call = cases.test_parameters_per_call
test_normalize_with_a_format_equals_convert_of_the_normalized_f32 = cases.test_normalize_with_a_format_equals_convert_of_the_normalized_f32
test_normalize_splits_batches_larger_than_the_workspace = cases.test_normalize_splits_batches_larger_than_the_workspace
test_decode_with_loudness_equals_the_stages_one_by_one = cases.test_decode_with_loudness_equals_the_stages_one_by_one
test_decode_device_with_loudness_equals_decode = cases.test_decode_device_with_loudness_equals_decode
test_option_off_in_every_spelling_is_ntts_codec_decode_speed = cases.test_option_off_in_every_spelling_is_ntts_codec_decode_speed
test_refusals_name_the_problem_and_leave_the_engine_usable = cases.test_refusals_name_the_problem_and_leave_the_engine_usable
test_class_infer_batch_with_a_loudness_per_utterance = cases.test_class_infer_batch_with_a_loudness_per_utterance
test_class_instance_loudness_and_decode_codes = cases.test_class_instance_loudness_and_decode_codes
test_class_streams_refuse_a_loudness = cases.test_class_streams_refuse_a_loudness
test_class_watermarker_sees_the_normalized_24khz_float = cases.test_class_watermarker_sees_the_normalized_24khz_float
