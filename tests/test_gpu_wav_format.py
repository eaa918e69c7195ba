"""The codec's device output stage (include/neutts_hip.h ntts_wav_format) on a real MI355X through libneutts_hip.so: the bodies of
tests/test_emu_wav_format.py -- the kernel against tests/wav_format_spec.py through ntts_codec_convert, exact encodings, the untouched default,
ntts_codec_decode_fmt / _dev_fmt plumbing, refusals, the class -- rebound to the real library."""
import pytest
import torch

from oracle import backbone_ref as br
from neutts import _hip
from common import load_codec_fixture, make_codec_engine
import test_emu_neutts_class as class_cases
import test_emu_wav_format as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(hip_lib):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _hip.load_library(hip_lib)
    z, cfg, w = load_codec_fixture("codec_tiny")
    e = make_codec_engine(cfg, w, hip_lib)
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
test_convert_f32_against_spec = cases.test_convert_f32_against_spec
test_encodings_are_exact_functions_of_the_f32_output = cases.test_encodings_are_exact_functions_of_the_f32_output
test_zeroed_format_is_the_plain_decode_bit_for_bit = cases.test_zeroed_format_is_the_plain_decode_bit_for_bit
test_decode_fmt_equals_convert_of_the_plain_decode = cases.test_decode_fmt_equals_convert_of_the_plain_decode
test_decode_device_with_a_format_equals_decode = cases.test_decode_device_with_a_format_equals_decode
test_refusals_name_the_problem_and_leave_the_engine_usable = cases.test_refusals_name_the_problem_and_leave_the_engine_usable
test_convert_splits_batches_larger_than_the_workspace = cases.test_convert_splits_batches_larger_than_the_workspace
test_class_infer_batch_in_a_telephony_format = cases.test_class_infer_batch_in_a_telephony_format
test_class_defaults_and_per_call_overrides = cases.test_class_defaults_and_per_call_overrides
test_class_streams_take_the_native_format_only = cases.test_class_streams_take_the_native_format_only
test_class_watermarker_sees_24khz_float_and_its_output_is_converted = cases.test_class_watermarker_sees_24khz_float_and_its_output_is_converted
