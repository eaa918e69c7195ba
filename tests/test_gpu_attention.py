"""Paged attention as an operation on a real MI355X: the cases of tests/test_emu_attention.py (its tables and helpers) through
libneutts_hip.so, against the CPU spec tests/attention_spec.py only -- same inputs, same poison, same tolerance and cap."""
import pytest
import torch

import test_emu_attention as ta

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(hip_lib):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return hip_lib


@pytest.mark.parametrize("form,group", ta.DECODE_CASES)
def test_decode(lib, form, group):
    ta.decode_parity(lib, form, group)


@pytest.mark.parametrize("form", ["w4_2048", "w8"])
def test_decode_fp8(lib, form):
    ta.decode_fp8(lib, form)


@pytest.mark.parametrize("batch,xps", ta.XCD_CASES)
def test_decode_xcd_rows(lib, batch, xps):
    ta.decode_xcd(lib, batch, xps)


@pytest.mark.parametrize("nsplit", ta.SPLIT_N)
def test_decode_split(lib, nsplit):
    ta.decode_split(lib, nsplit)


def test_decode_form_picker(lib):
    ta.picker_table(lib)


@pytest.mark.parametrize("caps", ta.PF_CAPS)
def test_prefill_tiers(lib, caps):
    ta.prefill_parity(lib, ta.PF_LENS, 7, 64, caps, "tiers")


@pytest.mark.parametrize("group", [2, 8])
def test_prefill_groups(lib, group):
    ta.prefill_parity(lib, ta.PF_LENS, group, 64, (64, 128), "tiers")


@pytest.mark.parametrize("group", [1, 2, 4])
def test_prefill_hd128(lib, group):
    ta.prefill_parity(lib, ta.PF_LENS, group, 128, (0, 0), "generic")


@pytest.mark.parametrize("L", ta.PF_LONG)
def test_prefill_default_caps(lib, L):
    ta.prefill_parity(lib, (L,), 7, 64, ta.DEFAULT_CAPS, f"long {L}", seed=L)


@pytest.mark.parametrize("caps", [(0, 0), ta.DEFAULT_CAPS])
def test_prefill_head_spreading(lib, caps):
    ta.prefill_spread(lib, caps)


@pytest.mark.parametrize("caps", [(64, 128), (0, 0)])
def test_prefill_shared_prefix(lib, caps):
    ta.prefill_shared_prefix(lib, caps)


@pytest.mark.parametrize("lens,caps", ta.ONLY_LAST + [ta.ONLY_LAST_LONG])
def test_prefill_only_last(lib, lens, caps):
    ta.prefill_only_last(lib, lens, caps)


@pytest.mark.parametrize("hd,generic,pos0", ta.WRITER_CASES)
def test_writers(lib, hd, generic, pos0):
    ta.writer_case(lib, hd, generic, pos0)


@pytest.mark.parametrize("hd", [64, 128])
def test_writer_qk_norm(lib, hd):
    ta.writer_case(lib, hd, True, 32, normed=True)
