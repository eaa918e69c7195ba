"""The whole output chain in one decode call (time stretch, loudness, output format: every subset, from host codes and from device-resident
codes) on a real MI355X through libneutts_hip.so: the bodies of tests/test_emu_output_chain.py rebound to the real library."""
import pytest
import torch

from neutts import _hip
import test_emu_output_chain as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def deng(hip_lib):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _hip.load_library(hip_lib)
    return cases.make_engine(hip_lib, True)


# the shared bodies: collected here under the gpu mark, resolved against THIS module's `deng` fixture
chain_ref = cases.chain_ref
test_decode_equals_the_stages_one_by_one = cases.test_decode_equals_the_stages_one_by_one
test_decode_device_equals_the_stages_one_by_one = cases.test_decode_device_equals_the_stages_one_by_one
