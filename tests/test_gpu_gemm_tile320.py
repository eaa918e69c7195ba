"""The 320-row GEMM tiles (gemm.h: 320 x 192 on 12 waves, 320 x 128 on 8 waves; wave tile 80 x 64) through ntts_k_gemm_bf16, variants 8 and 9.

Two checks per shape, with and without bias, operands seeded as in tests/test_gpu_kernels.py::test_gemm:
  * against bf16(x @ w^T + b) computed in fp32 on the host, under that test's bounds (2^-7 relative, fewer than 2 % of the elements different);
  * EXACT equality with variant 4 (256 x 256) on the same operands: a whole-K tile accumulates the same k-tiles in the same order whatever its
    extent, which is what lets an engine change tiles without changing a bit of its logits.

Shapes: one tile and one k-tile; one row in the second m-block with 8 columns in the tail n-block and a ring that wraps once; one live row
(every other LDS row clamped to it); the decode QKV width with ragged rows in the last wave; the flagship's gate/up width at 640 rows.
"""
import pytest
import torch

from neutts import _hip
from test_emu_kernels import run_gemm, _bf16

pytestmark = pytest.mark.gpu

SHAPES = [(320, 192, 64), (321, 200, 128), (1, 192, 64), (639, 1152, 896), (640, 9728, 896)]


@pytest.fixture(scope="module")
def lib(hip_lib):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _hip.load_library(hip_lib)


@pytest.fixture(scope="module")
def operands(lib):
    """Per (shape, bias): device operands, the host reference and variant 4's output, computed once and shared by both variants."""
    cache = {}

    def get(M, N, K, has_bias):
        key = (M, N, K, has_bias)
        if key not in cache:
            g = torch.Generator().manual_seed(M * 1000 + N)
            x = _bf16(torch.randn(M, K, generator=g))
            w = _bf16(torch.randn(N, K, generator=g) / K ** 0.5)
            b = _bf16(torch.randn(N, generator=g)) if has_bias else None
            ref = x.float() @ w.float().t()
            if b is not None:
                ref = ref + b.float()
            ref = _bf16(ref).float()
            xd, wd, bd = x.cuda(), w.cuda(), (b.cuda() if b is not None else None)
            xl = run_gemm(lib, xd, wd, bd, 4).float().cpu()
            cache[key] = (xd, wd, bd, ref, xl)
        return cache[key]
    return get


@pytest.mark.parametrize("has_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("M,N,K", SHAPES)
@pytest.mark.parametrize("variant", [8, 9], ids=["320x192", "320x128"])
def test_tile320_gemm(lib, operands, variant, M, N, K, has_bias):
    xd, wd, bd, ref, xl = operands(M, N, K, has_bias)
    out = run_gemm(lib, xd, wd, bd, variant).float().cpu()
    err = (out - ref).abs()
    tol = 2.0 ** -7 * ref.abs().clamp(min=1e-2)
    worst = int(err.argmax())
    print(f"tile320 variant {variant} {M}x{N}x{K} bias={has_bias}: max err {float(err.max()):.3g}, differing {float((out != ref).float().mean()):.4f}, "
          f"differing from 256x256 {int((out != xl).sum())}")
    assert bool((err <= tol).all()), f"max err {err.max()} at {(worst // N, worst % N)}"
    assert (out != ref).float().mean() < 0.02
    assert torch.equal(out, xl), f"{int((out != xl).sum())} elements differ from the 256 x 256 tile"
