"""The codec's output stage on signals that arrive in chunks (include/neutts_hip.h ntts_wav_stream_*, ntts_streams_set_format /
ntts_streams_pump_end_fmt) on a real MI355X through libneutts_hip.so: the bodies of tests/test_emu_wav_stream.py -- wav_stream_kernel through
WavStream against the one-shot stage bit for bit and against tests/wav_format_spec.py, refusals, the stream set, the class on all three streaming
paths -- rebound to the real library."""
import pytest
import torch

from oracle import backbone_ref as br
from neutts import _hip
from common import load_codec_fixture, make_codec_engine
import test_emu_neutts_class as class_cases
import test_emu_wav_stream as cases

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
test_chunks_equal_the_one_shot_stage_bit_for_bit = cases.test_chunks_equal_the_one_shot_stage_bit_for_bit
test_one_sample_per_push = cases.test_one_sample_per_push
test_three_streams_in_one_call_at_different_phases = cases.test_three_streams_in_one_call_at_different_phases
test_refusals_name_the_problem_and_move_no_stream = cases.test_refusals_name_the_problem_and_move_no_stream
test_the_native_format_is_a_copy_without_history = cases.test_the_native_format_is_a_copy_without_history
test_stream_batch_in_a_format_equals_the_one_shot_stage_of_the_native_stream = cases.test_stream_batch_in_a_format_equals_the_one_shot_stage_of_the_native_stream
test_device_path_equals_host_loop_and_single_streams = cases.test_device_path_equals_host_loop_and_single_streams
test_the_native_format_spelled_out_is_the_plain_call = cases.test_the_native_format_spelled_out_is_the_plain_call
test_stream_batch_over_a_gang_in_a_format = cases.test_stream_batch_over_a_gang_in_a_format
test_watermarker_sees_24khz_float_windows_and_its_output_is_converted = cases.test_watermarker_sees_24khz_float_windows_and_its_output_is_converted
test_constructor_defaults_and_per_call_keywords = cases.test_constructor_defaults_and_per_call_keywords
test_a_stream_that_ends_on_a_window_edge_is_flushed = cases.test_a_stream_that_ends_on_a_window_edge_is_flushed
test_stream_set_abi_set_format_and_plain_pump_end = cases.test_stream_set_abi_set_format_and_plain_pump_end
