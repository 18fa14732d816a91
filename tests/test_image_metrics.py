"""ops.image_metrics: the PSNR / SSIM definition (CPU, eager path)."""

import math

import numpy as np
import pytest
import torch

from image_metrics_cases import disc_pairs
from novel_view_synthesis_3d_amd import ops
from novel_view_synthesis_3d_amd.engine import metrics


def _u(x, quantize=False):
    u = np.clip(x, -1.0, 1.0) * 0.5 + 0.5
    return np.trunc(u * 255.0) / 255.0 if quantize else u


def scipy_oracle(pred, target):
    """skimage's structural_similarity(gaussian_weights=True, sigma=1.5,
    use_sample_covariance=False, data_range=1) spelled out: reflecting
    Gaussian filter, then a 5-pixel crop. Independent of torch's conv."""
    ndi = pytest.importorskip("scipy.ndimage")
    x, y = _u(pred.numpy()), _u(target.numpy())
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    psnr, ssim = [], []
    for n in range(x.shape[0]):
        mse = np.mean((x[n] - y[n]) ** 2)
        psnr.append(10.0 * math.log10(1.0 / mse) if mse > 0 else math.inf)
        vals = []
        for c in range(3):
            a, b = x[n, :, :, c], y[n, :, :, c]

            def f(img):
                return ndi.gaussian_filter(img, sigma=1.5, truncate=3.5,
                                           mode="reflect")
            ma, mb = f(a), f(b)
            va, vb = f(a * a) - ma * ma, f(b * b) - mb * mb
            cab = f(a * b) - ma * mb
            s = ((2 * ma * mb + C1) * (2 * cab + C2)
                 / ((ma * ma + mb * mb + C1) * (va + vb + C2)))
            vals.append(s[5:-5, 5:-5])
        ssim.append(np.mean(np.stack(vals)))
    return np.array(psnr), np.array(ssim)


@pytest.mark.parametrize("hw", [(11, 11), (13, 16), (45, 70)])
def test_matches_independent_oracle_fp64(hw):
    pred, target = disc_pairs(5, *hw, seed=1)
    psnr, ssim = ops.image_metrics(pred, target)
    assert psnr.dtype == torch.float64 and psnr.shape == (5,)
    want_p, want_s = scipy_oracle(pred, target)
    np.testing.assert_allclose(psnr.numpy(), want_p, rtol=0, atol=1e-9)
    np.testing.assert_allclose(ssim.numpy(), want_s, rtol=0, atol=1e-9)
    if hw == (45, 70):  # the images span the range the tests rely on
        assert ssim.max() > 0.8 and ssim.min() < 0.3


def test_fixed_points_and_errors():
    _, target = disc_pairs(2, 16, 19, seed=2)
    psnr, ssim = ops.image_metrics(target, target.clone())
    assert torch.isinf(psnr).all() and (psnr > 0).all()
    assert (ssim - 1.0).abs().max() <= 1e-12
    with pytest.raises(ValueError):
        ops.image_metrics(target[:, :10], target[:, :10])
    with pytest.raises(ValueError):
        ops.image_metrics(target[:, :, :10], target[:, :, :10])
    with pytest.raises(ValueError):
        ops.image_metrics(target, target[:1])
    with pytest.raises(ValueError):
        ops.image_metrics(target, target.float())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_psnr_equals_engine_psnr(dtype):
    pred, target = disc_pairs(4, 20, 23, seed=3)
    pred = pred.clamp(-1, 1).to(dtype)  # engine.metrics.psnr does not clamp
    target = target.to(dtype)
    psnr, _ = ops.image_metrics(pred, target)
    for n in range(4):
        want = metrics.psnr(pred[n], target[n], 2.0)
        assert abs(float(psnr[n]) - want) <= 1e-4


def test_engine_ssim_single_and_batch():
    pred, target = disc_pairs(3, 16, 16, seed=4)
    _, ssim = ops.image_metrics(pred, target)
    assert metrics.ssim(pred[1], target[1]) == pytest.approx(float(ssim[1]),
                                                             abs=1e-12)
    assert metrics.ssim(pred, target) == pytest.approx(float(ssim.mean()),
                                                       abs=1e-12)


def test_quantisation_round_trip(tmp_path):
    """Metrics of the float image with quantize=True equal the metrics of
    the PNG sample.py would write, read back by the dataset loader."""
    Image = pytest.importorskip("PIL.Image")
    from novel_view_synthesis_3d_amd.data.io import load_rgb
    pred, target = disc_pairs(3, 24, 24, seed=5)
    out = pred.float().clamp(-1, 1)
    # exact 8-bit ground truth, as a dataset image is
    k = torch.trunc((target.clamp(-1, 1) * 0.5 + 0.5) * 255.0)
    gt = (k / 255.0 * 2.0 - 1.0).float()
    img = ((out * 0.5 + 0.5) * 255).to(torch.uint8).numpy()  # as sample.py
    back = []
    for n in range(3):
        path = str(tmp_path / f"v{n}.png")
        Image.fromarray(img[n]).save(path)
        back.append(torch.from_numpy(load_rgb(path)).float())
    back = torch.stack(back)
    p_file, s_file = ops.image_metrics(back.double(), gt.double())
    p_q, s_q = ops.image_metrics(out.double(), gt.double(), quantize=True)
    assert (p_file - p_q).abs().max() <= 1e-6
    assert (s_file - s_q).abs().max() <= 1e-6
    # and quantisation is not a no-op on these images
    p_f, _ = ops.image_metrics(out.double(), gt.double())
    assert (p_f - p_q).abs().max() > 1e-6


def test_ssim_is_defined_on_unit_range():
    """SSIM is not shift-invariant: the same formula on the raw [-1,1]
    values with L=2 gives another number. Guards the [0,1] mapping."""
    import torch.nn.functional as F
    from novel_view_synthesis_3d_amd.ops.reference import ssim_window
    pred, target = disc_pairs(5, 45, 70, seed=1)
    pred = pred.clamp(-1, 1)
    _, ssim = ops.image_metrics(pred, target)

    g = ssim_window(torch.float64)
    C1, C2 = (0.01 * 2) ** 2, (0.03 * 2) ** 2

    def f(t):
        return F.conv2d(F.conv2d(t, g.view(1, 1, 1, -1)), g.view(1, 1, -1, 1))

    x = pred.permute(0, 3, 1, 2).reshape(15, 1, 45, 70)
    y = target.permute(0, 3, 1, 2).reshape(15, 1, 45, 70)
    mx, my = f(x), f(y)
    s = ((2 * mx * my + C1) * (2 * (f(x * y) - mx * my) + C2)
         / ((mx * mx + my * my + C1)
            * (f(x * x) - mx * mx + f(y * y) - my * my + C2)))
    raw = s.reshape(5, -1).mean(dim=1)
    assert (raw - ssim).abs().min() > 1e-3
