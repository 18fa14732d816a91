"""The narrow-channel direct wgrad kernel (conv3x3_wgrad_narrow.hip) against
the float64 autograd of `ops.reference.frame_conv3x3` on the same bf16 values.

Elementwise bound: |got - want| <= N 2^-23 A, N = IMG*H*W pixels summed per
element, A = the reference wgrad of (|x|, |dy|): worst-case fp32 accumulation,
the fp32 output is not rounded again. Through the public interface the
dispatch casts to bf16 once more: + 2^-8 |want|."""

import math

import pytest
import torch

from novel_view_synthesis_3d_amd import ops
from novel_view_synthesis_3d_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

# (B, F, H, W, Cin, Cout)
SHAPES = [
    (1, 1, 1, 1, 32, 32),      # every tap but the centre is padding
    (1, 2, 16, 16, 32, 32),    # one wave tile, eight waves split K
    (1, 2, 5, 19, 32, 64),     # both dims ragged, W crosses a K step
    (2, 1, 33, 8, 96, 64),     # W below the K step, 3 ci tiles, two images
    (1, 2, 8, 40, 128, 32),    # two ci tiles of 64
    (1, 1, 17, 17, 64, 96),    # six wave tiles, no K split
    (1, 2, 16, 16, 32, 128),   # widest Cout
    (1, 1, 9, 24, 160, 32),    # Cin past 128: five ci tiles in the grid
    (3, 1, 7, 16, 64, 64),     # split-K ranges that cross image boundaries
]
IFACE_SHAPES = [(1, 2, 16, 16, 96, 64), (2, 2, 8, 24, 64, 32),
                (1, 2, 16, 16, 32, 96)]


def _inputs(shape, seed=0, integers=False):
    """bf16 x, w, bias, residual and upstream gradient dy, on the CPU."""
    B, F, H, W, Cin, Cout = shape
    g = torch.Generator().manual_seed(seed)
    if integers:
        rn = lambda lim, *s: torch.randint(-lim, lim + 1, s, generator=g)
        x, dy = rn(3, B, F, H, W, Cin), rn(2, B, F, H, W, Cout)
    else:
        x = torch.randn(B, F, H, W, Cin, generator=g)
        dy = torch.randn(B, F, H, W, Cout, generator=g)
    w = torch.randn(Cout, 3, 3, Cin, generator=g) * 0.1
    b = torch.randn(Cout, generator=g)
    res = torch.randn(B, F, H, W, Cout, generator=g)
    return [t.to(torch.bfloat16) for t in (x, w, b, res, dy)]


def _check(outs, x, dy, scale=1.0, cast=0.0, exact=False):
    """(dw[, db]) against the float64 autograd of (conv(x, w) + b) * scale
    under upstream dy: the module's bound, or equality when `exact`."""
    def grads(x64, dy64):
        w = torch.zeros(dy.shape[-1], 3, 3, x.shape[-1], dtype=torch.float64,
                        requires_grad=True)
        b = torch.zeros(dy.shape[-1], dtype=torch.float64, requires_grad=True)
        y = ref.frame_conv3x3(x64, w, b) * scale
        return torch.autograd.grad(y, (w, b), dy64)

    want = grads(x.double(), dy.double())
    A = grads(x.double().abs(), dy.double().abs())
    n = x[..., 0].numel()
    for name, got, w64, a in zip(("dw", "db"), outs, want, A):
        got = got.double().cpu()
        if exact:
            assert torch.equal(got, w64), name
            continue
        bound = n * 2.0 ** -23 * a + cast * w64.abs()
        excess = ((got - w64).abs() - bound).max().item()
        assert excess <= 0, f"{name}: {excess:.3e} over the bound"


@pytest.mark.parametrize("shape", SHAPES)
def test_exact_integers(shape):
    """Integer operands: every partial sum is an integer below 2^24, so the
    fp32 result does not depend on the order of the atomics."""
    from novel_view_synthesis_3d_amd.ops import hip_ops  # noqa: F401 (loads)
    x, _, _, _, dy = _inputs(shape, seed=1, integers=True)
    dw, db = torch.ops.nvs3d.conv3x3_wgrad(x.cuda(), dy.cuda(), True)
    assert dw.dtype == db.dtype == torch.float32
    _check((dw, db), x, dy, exact=True)


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("shape", SHAPES)
def test_random_fp64(shape, with_bias):
    from novel_view_synthesis_3d_amd.ops import hip_ops  # noqa: F401 (loads)
    x, _, _, _, dy = _inputs(shape)
    outs = torch.ops.nvs3d.conv3x3_wgrad(x.cuda(), dy.cuda(), with_bias)
    assert len(outs) == (2 if with_bias else 1)
    _check(outs, x, dy)


@pytest.mark.parametrize("route", ["mfma", "im2col"])
@pytest.mark.parametrize("tail", [False, True], ids=["plain", "tail"])
@pytest.mark.parametrize("shape", IFACE_SHAPES)
def test_public_interface_backward(shape, tail, route, monkeypatch):
    if route == "im2col":
        monkeypatch.setenv("NVS3D_WGRAD", "im2col")
    x, w, b, res, dy = _inputs(shape, seed=2)
    scale = 1.0 / math.sqrt(2.0) if tail else 1.0
    wc, bc = (t.cuda().requires_grad_(True) for t in (w, b))
    if tail:
        y = ops.frame_conv3x3_residual(x.cuda(), wc, bc, res.cuda(), scale)
    else:
        y = ops.frame_conv3x3(x.cuda(), wc, bc)
    y.backward(dy.cuda())
    if route == "mfma":
        _check((wc.grad, bc.grad), x, dy, scale, cast=2.0 ** -8)
        return
    wc64, bc64 = (t.double().requires_grad_(True) for t in (w, b))
    (ref.frame_conv3x3(x.double(), wc64, bc64) * scale).backward(dy.double())
    for got, want in ((wc.grad, wc64.grad), (bc.grad, bc64.grad)):
        rel = (got.double().cpu() - want).abs().max() / want.abs().max()
        assert rel < 5e-2, f"rel {rel:.3e}"


def test_no_patch_matrix():
    """dw is 36 KB; the 9-plane patch matrix would be 9x the bytes of x."""
    x, w, b, _, dy = (t.cuda() for t in _inputs((4, 2, 64, 64, 32, 32)))
    w.requires_grad_(True)
    y = ops.frame_conv3x3(x, w, b)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    torch.autograd.grad(y, w, dy)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    assert rise < 2 * x.numel() * 2, f"wgrad peak rise {rise} B"
