"""The halo-tile MFMA 3x3 conv (conv3x3_halo.hip) against the fp64 reference
(`ops.reference.frame_conv3x3` on float64 copies of the same bf16 values).

Elementwise bound: |got - want| <= 2^-8 |want| + 9 Cin 2^-23 A, with
A = (conv(|x|,|w|) + |b| + |res|) * out_scale: one bf16 rounding of the
output plus worst-case fp32 accumulation over the 9*Cin products."""

import math

import pytest
import torch

from novel_view_synthesis_3d_amd import ops
from novel_view_synthesis_3d_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

RS2 = 1.0 / math.sqrt(2.0)

# (B, F, H, W, Cin, Cout)
SHAPES = [
    (1, 2, 16, 16, 32, 32),    # one tile
    (1, 2, 5, 19, 32, 64),     # both dims ragged, W crosses a tile
    (2, 1, 33, 8, 96, 64),     # W below the tile, 3 chunks, multi-image
    (1, 2, 8, 40, 128, 32),    # 4 chunks
    (1, 1, 17, 17, 64, 96),    # one row and column past the tile
    (1, 2, 16, 16, 32, 128),   # widest Cout
    (1, 1, 1, 1, 32, 32),      # every tap but the centre is padding
]
IFACE_SHAPES = [(1, 2, 16, 16, 96, 64), (2, 2, 8, 24, 64, 32),
                (1, 2, 16, 16, 32, 96)]


def _inputs(shape, seed=0):
    """bf16 x, w, bias, residual and upstream gradient, on the CPU."""
    B, F, H, W, Cin, Cout = shape
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16)
    return (rn(B, F, H, W, Cin), rn(Cout, 3, 3, Cin) * 0.1, rn(Cout),
            rn(B, F, H, W, Cout), rn(B, F, H, W, Cout))


def _check(name, got, want, x, w, b, res, scale):
    """The module's bound; x, w, b, res are the float64 operands of want."""
    A = ref.frame_conv3x3(x.abs(), w.abs(), None)
    if b is not None:
        A = A + b.abs()
    if res is not None:
        A = A + res.abs()
    bound = 2.0 ** -8 * want.abs() + 9 * x.shape[-1] * 2.0 ** -23 * A * scale
    excess = ((got.double().cpu() - want).abs() - bound).max().item()
    assert excess <= 0, f"{name}: {excess:.3e} over the bound"


def _halo_op(x, w, b, res, scale):
    from novel_view_synthesis_3d_amd.ops import hip_ops  # noqa: F401 (loads)
    cu = lambda t: None if t is None else t.cuda()
    return torch.ops.nvs3d.conv3x3_halo_fwd(cu(x), cu(w), cu(b), cu(res),
                                            scale)


@pytest.mark.parametrize("tail", [False, True], ids=["plain", "tail"])
@pytest.mark.parametrize("shape", SHAPES)
def test_forward_fp64(shape, tail):
    x, w, b, res, _ = _inputs(shape)
    if not tail:
        b = res = None
    scale = RS2 if tail else 1.0
    got = _halo_op(x, w, b, res, scale)
    d = lambda t: None if t is None else t.double()
    want = ref.frame_conv3x3(d(x), d(w), d(b))
    if tail:
        want = (want + d(res)) * scale
    _check(f"y {shape}", got, want, d(x), d(w), d(b), d(res), scale)


@pytest.mark.parametrize("shape", SHAPES)
def test_exact_taps(shape):
    """One +-1 weight per (cout, tap): every output is an integer, |y| <= 27."""
    B, F, H, W, Cin, Cout = shape
    g = torch.Generator().manual_seed(1)
    x = torch.randint(-3, 4, (B, F, H, W, Cin), generator=g).to(torch.bfloat16)
    co, ky, kx = torch.meshgrid(torch.arange(Cout), torch.arange(3),
                                torch.arange(3), indexing="ij")
    sign = torch.randint(0, 2, (Cout, 3, 3), generator=g) * 2 - 1
    w = torch.zeros(Cout, 3, 3, Cin)
    w[co, ky, kx, (7 * co + 3 * ky + kx) % Cin] = sign.float()
    w = w.to(torch.bfloat16)
    got = _halo_op(x, w, None, None, 1.0)
    want = ref.frame_conv3x3(x.double(), w.double(), None)
    assert torch.equal(got.double().cpu(), want)


@pytest.mark.parametrize("tail", [False, True], ids=["plain", "tail"])
@pytest.mark.parametrize("shape", IFACE_SHAPES)
def test_public_interface_and_backward(shape, tail):
    x, w, b, res, dy = _inputs(shape, seed=2)
    scale = RS2 if tail else 1.0

    def run(cast, conv, conv_res):
        t = [cast(v).requires_grad_(True) for v in (x, w, b, res)]
        y = (conv_res(*t, scale) if tail else conv(t[0], t[1], t[2]))
        y.backward(cast(dy))
        return [y.detach()] + [v.grad for v in t]

    y, dx, dw, db, dres = run(lambda v: v.cuda(), ops.frame_conv3x3,
                              ops.frame_conv3x3_residual)
    y64, dx64, dw64, db64, dres64 = run(
        lambda v: v.double(), ref.frame_conv3x3,
        lambda a, k, c, r, s: (ref.frame_conv3x3(a, k, c) + r) * s)

    d = lambda t: t.double()
    _check("y", y, y64, d(x), d(w), d(b), d(res) if tail else None, scale)
    wt = torch.flip(d(w), dims=(1, 2)).permute(3, 1, 2, 0)
    _check("dx", dx, dx64, d(dy), wt, None, None, scale)
    for name, got, want in (("dw", dw, dw64), ("db", db, db64)):
        rel = ((got.double().cpu() - want).abs().max() / want.abs().max())
        assert rel < 5e-2, f"{name}: rel {rel:.3e}"
    if tail:
        err = (dres.double().cpu() - dres64).abs()
        assert (err <= 2.0 ** -8 * dres64.abs()).all()


def _peak_rise(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before, out


def test_no_materialised_im2col():
    """Output (or dx) is 1x the input's bytes; a patch matrix would be 9x."""
    x, w, b, _, _ = (t.cuda() for t in _inputs((4, 2, 64, 64, 32, 32)))
    with torch.no_grad():
        rise, _ = _peak_rise(lambda: ops.frame_conv3x3(x, w, b))
    assert rise < 2 * x.numel() * 2, f"forward peak rise {rise} B"

    x, w, _, _, dy = (t.cuda() for t in _inputs((4, 2, 64, 64, 64, 32)))
    x.requires_grad_(True)
    y = ops.frame_conv3x3(x, w, None)
    rise, _ = _peak_rise(lambda: torch.autograd.grad(y, x, dy))
    assert rise < 2 * x.numel() * 2, f"dgrad peak rise {rise} B"
