"""image_metrics.hip against the fp64 reference, and the Evaluator on it."""

import pytest
import torch

from image_metrics_cases import disc_pairs, make_synth_dataset
from novel_view_synthesis_3d_amd import ops
from novel_view_synthesis_3d_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

PSNR_TOL = 1e-3      # dB: fp32 sums with add chains <= 2^10, see the issue
SSIM_FLOOR = 2e-6    # single-window fp32 error


def _tile():
    from novel_view_synthesis_3d_amd.ops import hip_ops
    return hip_ops.IMAGE_METRICS_TILE


SHAPES = [(1, 11, 11), (3, 11, 12), (2, 13, 16), (5, 19, 27), (2, 26, 43),
          (2, 42, 18), (2, 45, 70), (3, 64, 64), (1, 33, 150), (2, 128, 128),
          "one_tile", "one_tile_plus_strip"]


def _shape(case):
    if case == "one_tile":
        return (2, _tile() + 10, _tile() + 10)
    if case == "one_tile_plus_strip":
        return (2, _tile() + 11, _tile() + 11)
    return case


def _inputs(case, dtype):
    """Pairs in `dtype`; with N >= 2 the last image equals its target."""
    n, h, w = _shape(case)
    pred, target = disc_pairs(n, h, w, seed=h * 1000 + w)
    if n >= 2:
        pred[-1] = target[-1]
    return pred.to(dtype), target.to(dtype)


def _references(pred, target, quantize):
    """fp64 reference on the same values (bf16 upcast first) and the SSIM
    bound max(4 * e_ref, floor), e_ref = |fp32 eager (CPU) - fp64|."""
    p64, s64 = ref.image_metrics(pred.double(), target.double(), quantize)
    _, s32 = ref.image_metrics(pred.float(), target.float(), quantize)
    e_ref = float((s32.double() - s64).abs().max())
    return p64, s64, e_ref, max(4.0 * e_ref, SSIM_FLOOR)


def _check(psnr, ssim, p64, s64, tol, label):
    psnr, ssim = psnr.double().cpu(), ssim.double().cpu()
    assert torch.isfinite(ssim).all(), label
    inf = torch.isinf(p64)
    assert torch.equal(torch.isinf(psnr), inf), (label, psnr, p64)
    assert (psnr[inf] > 0).all()
    perr = float((psnr[~inf] - p64[~inf]).abs().max()) if (~inf).any() else 0.0
    serr = float((ssim - s64).abs().max())
    print(f"{label}: psnr_err={perr:.2e} ssim_err={serr:.2e} tol={tol:.2e}")
    assert perr <= PSNR_TOL, label
    assert serr <= tol, label
    return serr


@pytest.mark.parametrize("quantize", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", SHAPES, ids=str)
def test_parity_with_fp64_reference(case, dtype, quantize):
    pred, target = _inputs(case, dtype)
    p64, s64, e_ref, tol = _references(pred, target, quantize)
    psnr, ssim = ops.image_metrics(pred.cuda(), target.cuda(), quantize)
    assert psnr.dtype == torch.float32 and psnr.is_cuda
    assert psnr.shape == ssim.shape == (pred.shape[0],)
    label = f"{_shape(case)} {dtype} q={int(quantize)} e_ref={e_ref:.2e}"
    _check(psnr, ssim, p64, s64, tol, label)
    if pred.shape[0] == 1:  # the identical pair of a one-image case
        p64, s64, e_ref, tol = _references(target, target, quantize)
        assert quantize or torch.isinf(p64).all()  # quantize: pred only
        psnr, ssim = ops.image_metrics(target.cuda(), target.cuda(), quantize)
        _check(psnr, ssim, p64, s64, tol, label + " identical")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", [(3, 11, 12), (2, 45, 70), (2, 128, 128)],
                         ids=str)
def test_reads_stay_inside_the_tensor(case, dtype):
    """The pair sits contiguously in NaN-filled buffers at a storage offset
    of one element: not 16-byte aligned, so the scalar load path runs, and
    any read outside the images would poison the result."""
    pred, target = _inputs(case, dtype)
    p64, s64, e_ref, tol = _references(pred, target, False)

    def embed(t):
        buf = torch.full((t.numel() + 64,), float("nan"), dtype=dtype,
                         device="cuda")
        view = buf[1:1 + t.numel()].view(t.shape)
        view.copy_(t)
        assert view.is_contiguous() and view.storage_offset() == 1
        assert view.data_ptr() % 16 != 0
        return view

    psnr, ssim = ops.image_metrics(embed(pred), embed(target))
    assert torch.isfinite(ssim).all()
    _check(psnr, ssim, p64, s64, tol, f"offset {case} {dtype}")
    # the aligned (vector load) path stages the same values: equal SSIM bits
    # (the squared error is summed in another order there)
    _, ssim_a = ops.image_metrics(pred.cuda(), target.cuda())
    assert torch.equal(ssim_a, ssim)


@pytest.mark.parametrize("case", [(5, 19, 27), (2, 128, 128)], ids=str)
def test_two_calls_are_bitwise_equal(case):
    pred, target = _inputs(case, torch.float32)
    pred, target = pred.cuda(), target.cuda()
    a = ops.image_metrics(pred, target)
    b = ops.image_metrics(pred, target)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_dispatch():
    from novel_view_synthesis_3d_amd.engine import metrics
    from novel_view_synthesis_3d_amd.ops import hip_ops
    assert "image_metrics" in hip_ops.HAS
    pred, target = _inputs((3, 64, 64), torch.float32)
    pred, target = pred[:2].cuda(), target[:2].cuda()
    _, ssim = ops.image_metrics(pred, target)
    assert metrics.ssim(pred, target) == pytest.approx(
        float(ssim.double().mean()), abs=1e-7)
    assert metrics.ssim(pred[0], target[0]) == pytest.approx(
        float(ssim[0]), abs=1e-7)
    with pytest.raises(ValueError):
        ops.image_metrics(pred[:, :10], target[:, :10])


def test_evaluator_on_gpu(tmp_path):
    """Tiny model (the configuration the GPU sampler tests use, 32x32) on
    the synthetic dataset: reported metrics equal the fp64 reference on the
    returned images."""
    from novel_view_synthesis_3d_amd.config import XUNetConfig
    from novel_view_synthesis_3d_amd.engine.evaluate import Evaluator
    from novel_view_synthesis_3d_amd.models.xunet import XUNet
    root = make_synth_dataset(tmp_path / "data")
    torch.manual_seed(0)
    cfg = XUNetConfig(ch=32, ch_mult=(1, 2), emb_ch=32, num_res_blocks=1,
                      attn_resolutions=(16,), dropout=0.0)
    model = XUNet(cfg, img_sidelength=32)
    with torch.no_grad():
        model.Conv_1.weight.normal_(0, 0.05)
    model = model.cuda()
    ev = Evaluator(model, num_steps=3, use_graph=False, batch_objects=2)
    res = ev.evaluate(root, 32, input_view=0, num_targets=3,
                      return_images=True)
    assert res["n_instances"] == 3 and res["n_views"] == 9
    imgs, tgts = res["images"], res["targets"]
    assert imgs.shape == (9, 32, 32, 3) and not imgs.is_cuda
    p64, s64, e_ref, tol = _references(imgs, tgts, False)
    print(f"evaluator: e_ref={e_ref:.2e} tol={tol:.2e} "
          f"psnr={res['psnr']:.4f} ssim={res['ssim']:.6f}")
    assert abs(res["psnr"] - float(p64.mean())) <= PSNR_TOL
    assert abs(res["ssim"] - float(s64.mean())) <= tol
    for i, e in enumerate(res["per_instance"]):
        assert abs(e["psnr"] - float(p64[3 * i:3 * i + 3].mean())) <= PSNR_TOL
        assert abs(e["ssim"] - float(s64[3 * i:3 * i + 3].mean())) <= tol
