"""speed=: the codec's pitch-preserving time stretch (include/neutts_hip.h ntts_codec_stretch / ntts_codec_decode_speed) on a real MI355X through
libneutts_hip.so: the bodies of tests/test_emu_time_stretch.py -- positions and samples against tests/time_stretch_spec.py, the untouched default,
the decode entry points, refusals, the class -- rebound to the real library."""
import pytest
import torch

from oracle import backbone_ref as br
from neutts import _hip
from common import load_codec_fixture, make_codec_engine
import test_emu_neutts_class as class_cases
import test_emu_time_stretch as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(hip_lib):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _hip.load_library(hip_lib)
    z, cfg, w = load_codec_fixture("codec_tiny")
    e = make_codec_engine(cfg, w, hip_lib, max_frames=256)
    e._fixture, e._on_gpu = z, True
    return e


@pytest.fixture(scope="module")
def tts(hip_lib):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _hip.load_library(hip_lib)
    return class_cases.build_tts(
        hip_lib, bcfg=lambda v: br.BackboneConfig(vocab_size=v, hidden_size=896, intermediate_size=1216, num_layers=3),
        max_batch=4, max_context=256, max_prefill_tokens=1024, seed=33)


# the shared bodies: collected here under the gpu mark, resolved against THIS module's `eng` / `tts` fixtures
test_positions_and_lengths_equal_the_spec = cases.test_positions_and_lengths_equal_the_spec
test_f32_output_within_the_derived_bound_and_exact_on_continuations = cases.test_f32_output_within_the_derived_bound_and_exact_on_continuations
test_unit_speed_rows_are_the_input_bit_for_bit = cases.test_unit_speed_rows_are_the_input_bit_for_bit
test_stretch_with_a_format_equals_convert_of_the_stretched_f32 = cases.test_stretch_with_a_format_equals_convert_of_the_stretched_f32
test_stretch_splits_batches_larger_than_the_workspace = cases.test_stretch_splits_batches_larger_than_the_workspace
test_decode_with_speed_equals_stretch_of_the_plain_decode = cases.test_decode_with_speed_equals_stretch_of_the_plain_decode
test_default_speed_makes_the_same_calls_and_bits = cases.test_default_speed_makes_the_same_calls_and_bits
test_decode_device_with_speed_equals_decode = cases.test_decode_device_with_speed_equals_decode
test_refusals_name_the_problem_and_leave_the_engine_usable = cases.test_refusals_name_the_problem_and_leave_the_engine_usable
test_class_infer_batch_with_a_speed_per_utterance = cases.test_class_infer_batch_with_a_speed_per_utterance
test_class_instance_speed_and_decode_codes = cases.test_class_instance_speed_and_decode_codes
test_class_streams_refuse_a_speed = cases.test_class_streams_refuse_a_speed
test_class_watermarker_sees_the_stretched_24khz_float = cases.test_class_watermarker_sees_the_stretched_24khz_float
