"""stream_speed=: the codec's time stretch on signals that arrive in chunks (include/neutts_hip.h ntts_speed_stream_*, ntts_streams_set_speed) on a real
MI355X through libneutts_hip.so: the bodies of tests/test_emu_stream_speed.py -- wav_stretch_stream_kernel through SpeedStream against the one-shot
stage bit for bit and against tests/time_stretch_spec.py, refusals, the stream set, the class on all three streaming paths -- rebound to the real
library."""
import pytest
import torch

from oracle import backbone_ref as br
from neutts import _hip
from common import load_codec_fixture, make_codec_engine
import test_emu_neutts_class as class_cases
import test_emu_stream_speed as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(hip_lib):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _hip.load_library(hip_lib)
    z, cfg, w = load_codec_fixture("codec_tiny")
    e = make_codec_engine(cfg, w, hip_lib, max_frames=1088, max_rows=1152)
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
test_three_streams_in_one_call_at_different_speeds_and_phases = cases.test_three_streams_in_one_call_at_different_speeds_and_phases
test_with_a_format_behind_the_stretch = cases.test_with_a_format_behind_the_stretch
test_refusals_name_the_problem_and_move_no_stream = cases.test_refusals_name_the_problem_and_move_no_stream
test_after_its_last_chunk_a_stream_starts_a_new_signal_at_another_speed = cases.test_after_its_last_chunk_a_stream_starts_a_new_signal_at_another_speed
test_stream_batch_at_speeds_equals_the_one_shot_stretch_of_the_plain_stream = cases.test_stream_batch_at_speeds_equals_the_one_shot_stretch_of_the_plain_stream
test_device_path_equals_host_loop_and_single_streams = cases.test_device_path_equals_host_loop_and_single_streams
test_stream_batch_over_a_gang_at_speeds = cases.test_stream_batch_over_a_gang_at_speeds
test_stream_batch_at_speeds_in_a_format = cases.test_stream_batch_at_speeds_in_a_format
test_watermarker_sees_speed_1_float_windows_and_its_output_is_stretched = cases.test_watermarker_sees_speed_1_float_windows_and_its_output_is_stretched
test_constructor_default_and_per_call_override = cases.test_constructor_default_and_per_call_override
test_a_stream_that_ends_on_a_window_edge_is_flushed = cases.test_a_stream_that_ends_on_a_window_edge_is_flushed
test_a_set_all_at_unit_speed_makes_the_calls_it_made_before = cases.test_a_set_all_at_unit_speed_makes_the_calls_it_made_before
test_set_speed_all_1000_through_the_abi_is_the_plain_set = cases.test_set_speed_all_1000_through_the_abi_is_the_plain_set
test_stream_set_abi_set_speed = cases.test_stream_set_abi_set_speed
