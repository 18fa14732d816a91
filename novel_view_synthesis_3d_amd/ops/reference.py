"""Eager PyTorch reference implementations of every fused op.

These are the numerics oracle (tests compare the HIP kernels against these in
fp32) and the CPU execution path. Shapes follow the framework's activation
layout: (B, F=2, H, W, C) contiguous — NHWC with a frame axis, the layout the
reference's FLAX model uses (/root/reference/model/xunet.py:228) and the
layout the CDNA4 kernels want for coalesced 64-lane access.

Kernel inventory: SURVEY.md §2.4 (K1-K20).
"""

from __future__ import annotations

import math
from typing import Optional, Tuple

import torch
import torch.nn.functional as F


SQRT_HALF = 1.0 / math.sqrt(2.0)


def _same_pad(size: int, k: int, s: int) -> Tuple[int, int]:
    """FLAX 'SAME' padding (asymmetric: low = total//2): matches nn.Conv."""
    out = -(-size // s)  # ceil
    total = max((out - 1) * s + k - size, 0)
    return total // 2, total - total // 2


def frame_conv3x3(x: torch.Tensor, weight: torch.Tensor,
                  bias: Optional[torch.Tensor], stride: int = 1) -> torch.Tensor:
    """K1/K2: per-frame 3x3 'SAME' conv over (B,F,H,W,Cin) -> (B,F,H',W',Cout).

    The reference's only conv type: kernel (1,3,3), stride (1,s,s)
    (/root/reference/model/xunet.py:81,85,199-202,229,276). `weight` is
    (Cout, 3, 3, Cin) contiguous (OHWI) — presented to conv2d as a
    channels-last (Cout,Cin,3,3) view so MIOpen takes the NHWC path with no
    transposes.
    """
    B, Fr, H, W, C = x.shape
    ph = _same_pad(H, 3, stride)
    pw = _same_pad(W, 3, stride)
    xf = x.reshape(B * Fr, H, W, C).permute(0, 3, 1, 2)  # NCHW view of NHWC data
    w = weight.permute(0, 3, 1, 2)  # channels-last view of OHWI storage
    if ph != (1, 1) or pw != (1, 1) or stride != 1:
        xf = F.pad(xf, (pw[0], pw[1], ph[0], ph[1]))
        y = F.conv2d(xf, w, bias, stride=stride)
    else:
        y = F.conv2d(xf, w, bias, stride=1, padding=1)
    Ho, Wo = y.shape[-2], y.shape[-1]
    return y.permute(0, 2, 3, 1).reshape(B, Fr, Ho, Wo, -1)


def joint_groupnorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
                    groups: int, eps: float = 1e-6,
                    film: Optional[torch.Tensor] = None,
                    silu: bool = False, p_drop: float = 0.0) -> torch.Tensor:
    """K3(+K5+K4): GroupNorm with statistics jointly over BOTH frames and all
    spatial positions per (batch, group) — the reference's frame-axis GroupNorm
    (/root/reference/model/xunet.py:46-52; flax GroupNorm reduces over all
    non-batch axes). Optionally fused FiLM modulate (xunet.py:54-61) and SiLU.

    x: (B, F, H, W, C); gamma/beta: (C,); film: (B, F, H, W, 2C) packed
    scale|shift (one Dense output, consumed strided — no split copies).
    Stats in fp32; output in x.dtype.
    """
    B, Fr, H, W, C = x.shape
    assert C % groups == 0, f"C={C} not divisible by groups={groups}"
    xf = x.to(torch.float32).reshape(B, Fr, H, W, groups, C // groups)
    mean = xf.mean(dim=(1, 2, 3, 5), keepdim=True)
    var = xf.var(dim=(1, 2, 3, 5), unbiased=False, keepdim=True)
    h = (xf - mean) * torch.rsqrt(var + eps)
    h = h.reshape(B, Fr, H, W, C)
    h = h * gamma.to(torch.float32) + beta.to(torch.float32)
    if film is not None:
        scale = film[..., :C].to(torch.float32)
        shift = film[..., C:].to(torch.float32)
        h = h * (1.0 + scale) + shift
    if silu:
        h = F.silu(h)
    if p_drop > 0.0:
        h = F.dropout(h, p_drop, training=True)
    return h.to(x.dtype)


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """K7: multi-head scaled dot-product attention over flattened H*W tokens.

    q/k/v: (B, L, h, d) -> (B, L, h, d). Matches flax nn.dot_product_attention
    (/root/reference/model/xunet.py:103): softmax(q k^T / sqrt(d)) v, softmax in
    fp32. NOTE the reference has NO output projection (xunet.py:126 commented
    out) — heads are just reshaped back by the caller.
    """
    B, L, h, d = q.shape
    qt = q.permute(0, 2, 1, 3)  # (B, h, L, d)
    kt = k.permute(0, 2, 1, 3)
    vt = v.permute(0, 2, 1, 3)
    scores = torch.matmul(qt, kt.transpose(-1, -2)) * (1.0 / math.sqrt(d))
    p = torch.softmax(scores.to(torch.float32), dim=-1).to(q.dtype)
    out = torch.matmul(p, vt)
    return out.permute(0, 2, 1, 3)


def swap_frame_pairs(t: torch.Tensor) -> torch.Tensor:
    """(2B', ...) -> batch entries (2i, 2i+1) exchanged: the k/v order of the
    model's cross-frame attention with both frames batched."""
    B2 = t.shape[0]
    return t.reshape(B2 // 2, 2, *t.shape[1:]).flip(1).reshape(t.shape)


def nearest_upsample2x(x: torch.Tensor) -> torch.Tensor:
    """K8: nearest-neighbor 2x upsample (/root/reference/model/xunet.py:14-18)."""
    B, Fr, H, W, C = x.shape
    x = x.reshape(B, Fr, H, 1, W, 1, C).expand(B, Fr, H, 2, W, 2, C)
    return x.reshape(B, Fr, 2 * H, 2 * W, C)


def avgpool_downsample2x(x: torch.Tensor) -> torch.Tensor:
    """K9: 2x2 average-pool downsample (/root/reference/model/xunet.py:20-21)."""
    B, Fr, H, W, C = x.shape
    x = x.reshape(B, Fr, H // 2, 2, W // 2, 2, C)
    return x.mean(dim=(3, 5))


def residual_scale_add(h: torch.Tensor, h_in: torch.Tensor) -> torch.Tensor:
    """K10: (h + h_in) / sqrt(2) (/root/reference/model/xunet.py:92,127)."""
    return (h + h_in) * SQRT_HALF


def posenc_ddpm(timesteps: torch.Tensor, emb_ch: int,
                max_time: float = 1000.0) -> torch.Tensor:
    """K12 part: DDPM sinusoidal positional encoding
    (/root/reference/model/xunet.py:23-35). timesteps: (B,) -> (B, emb_ch)."""
    timesteps = timesteps.to(torch.float32) * (1000.0 / max_time)
    half = emb_ch // 2
    freq = torch.exp(
        torch.arange(half, dtype=torch.float32, device=timesteps.device)
        * (-math.log(10000.0) / (half - 1)))
    ang = timesteps[:, None] * freq[None, :]
    return torch.cat([torch.sin(ang), torch.cos(ang)], dim=-1)


def squash_logsnr(logsnr: torch.Tensor) -> torch.Tensor:
    """K12 part: clip(+-20) then 2*atan(e^{-l/2})/pi in [0,1]
    (/root/reference/model/xunet.py:152-153)."""
    l = torch.clamp(logsnr.to(torch.float32), -20.0, 20.0)
    return 2.0 * torch.atan(torch.exp(-l / 2.0)) / math.pi


def posenc_nerf(x: torch.Tensor, min_deg: int = 0, max_deg: int = 15) -> torch.Tensor:
    """K14: NeRF positional encoding (/root/reference/model/xunet.py:37-44).

    Concat [x, sin(x*2^i), sin(x*2^i + pi/2)] for i in [min_deg, max_deg).
    x: (..., D) -> (..., D*(1 + 2*(max_deg-min_deg))).
    """
    if min_deg == max_deg:
        return x
    scales = torch.tensor([2.0 ** i for i in range(min_deg, max_deg)],
                          dtype=x.dtype, device=x.device)
    xb = (x[..., None, :] * scales[:, None]).reshape(*x.shape[:-1], -1)
    return torch.cat([x, torch.sin(xb), torch.sin(xb + math.pi / 2.0)], dim=-1)


def pose_embedding(R: torch.Tensor, t: torch.Tensor, K: torch.Tensor,
                   cond_mask: Optional[torch.Tensor], H: int, W: int,
                   out_dtype: torch.dtype) -> torch.Tensor:
    """K13+K14+K15 fused: per-pixel rays for BOTH cameras -> NeRF posenc ->
    CFG mask. R: (B,2,3,3), t: (B,2,3), K: (B,3,3). Returns (B,2,H,W,144).

    Eager oracle for the rays_posenc HIP kernel
    (reference model/xunet.py:159-179)."""
    from novel_view_synthesis_3d_amd.models.rays import camera_rays
    embs = []
    for f in range(2):
        pos, direc = camera_rays(R[:, f], t[:, f], K, H, W)
        embs.append(torch.cat([posenc_nerf(pos, 0, 15),
                               posenc_nerf(direc, 0, 8)], dim=-1))
    pe = torch.stack(embs, dim=1)
    if cond_mask is not None:
        pe = pe * cond_mask.to(pe.dtype).reshape(-1, 1, 1, 1, 1)
    return pe.to(out_dtype)


# ---------------------------------------------------------------------------
# Stochastic-conditioning sampler step (oracles for ops/hip/sampler_step.hip)
# ---------------------------------------------------------------------------

def stochastic_index(u: torch.Tensor, k) -> torch.Tensor:
    """The index rule: idx = min(floor(u * k), k - 1), evaluated in fp32.

    u: uniforms in [0,1) of any shape; k: number of valid bank entries (int
    or one-element tensor). Returns int64 indices of u's shape."""
    kf = torch.as_tensor(k, device=u.device).reshape(()).to(torch.float32)
    idx = torch.floor(u.to(torch.float32) * kf)
    idx = torch.minimum(idx, kf - 1.0).clamp_(min=0.0)
    return idx.to(torch.long)


def cond_emb_select(logsnr_emb: torch.Tensor, bank: torch.Tensor,
                    null_feat: torch.Tensor, tgt_feat: torch.Tensor,
                    u: torch.Tensor, step: torch.Tensor,
                    k: torch.Tensor) -> torch.Tensor:
    """Per-level FiLM input with the conditioning view picked from a bank.

    logsnr_emb (2B,E); bank (Kcap,B,H',W',E); null_feat (B|1,H',W',E);
    tgt_feat (2B,H',W',E); u (S,B) uniforms; step, k one-element int64.
    Returns (2B,2,H',W',E) = silu(logsnr_emb[r] + feat) in bank.dtype, where
    feat is bank[idx[b], b] (frame 0, rows < B), null_feat (frame 0, rows
    >= B) or tgt_feat (frame 1). fp32 arithmetic, one rounding."""
    B = bank.shape[1]
    idx = stochastic_index(u.index_select(0, step.reshape(1))[0], k)  # (B,)
    rows = torch.arange(B, device=bank.device)
    src = bank[idx, rows].to(torch.float32)                 # (B,H',W',E)
    null = null_feat.to(torch.float32).expand(B, *bank.shape[2:])
    frame0 = torch.cat([src, null], dim=0)
    feat = torch.stack([frame0, tgt_feat.to(torch.float32)], dim=1)
    e = logsnr_emb.to(torch.float32)[:, None, None, None, :] + feat
    return F.silu(e).to(bank.dtype)


def ddpm_cfg_step(z: torch.Tensor, out: torch.Tensor, noise: torch.Tensor,
                  c_a: torch.Tensor, c_b: torch.Tensor, c1: torch.Tensor,
                  c2: torch.Tensor, sigma: torch.Tensor, step: torch.Tensor,
                  u: torch.Tensor, k: torch.Tensor, bank_img: torch.Tensor,
                  x: torch.Tensor, w: float, clip: bool,
                  noise_scale: float = 1.0) -> None:
    """One post-network ancestral step, in place on z, step and x.

    eps = (1+w) out[:B] - w out[B:];  x0 = c_a z - c_b eps (clamped to
    [-1,1] if clip);  z <- c1 x0 + c2 z + noise_scale sigma noise, with the
    coefficients taken from the (S,) tables at `step`. Then step += 1 and,
    while steps remain, x (2B,...) <- bank_img[idx_next[b], b] for both CFG
    halves under the index rule at the advanced step."""
    B = z.shape[0]
    S = u.shape[0]
    s = step.reshape(1)
    o = out.to(torch.float32)
    eps = (1.0 + w) * o[:B] - w * o[B:]
    x0 = c_a.index_select(0, s) * z - c_b.index_select(0, s) * eps
    if clip:
        x0 = x0.clamp(-1.0, 1.0)
    mean = c1.index_select(0, s) * x0 + c2.index_select(0, s) * z
    z.copy_(mean + (noise_scale * sigma.index_select(0, s)) * noise)
    step.add_(1)
    # no data-dependent host branch: past the last step the clamped row is
    # gathered and then discarded by the where()
    s1 = step.reshape(1).clamp(max=S - 1)
    idx = stochastic_index(u.index_select(0, s1)[0], k)
    nxt = bank_img[idx, torch.arange(B, device=z.device)]
    live = (step.reshape(()) < S)
    x.copy_(torch.where(live, torch.cat([nxt, nxt], dim=0), x))


def solver_cfg_step(z: torch.Tensor, hist: Optional[torch.Tensor],
                    out: torch.Tensor, noise: Optional[torch.Tensor],
                    c_a: torch.Tensor, c_b: torch.Tensor,
                    coef_z: torch.Tensor, coef_x0: torch.Tensor,
                    coef_hist: torch.Tensor, sigma: torch.Tensor,
                    step: torch.Tensor, w: float, clip: bool,
                    noise_scale: float = 1.0, *, u=None, k=None,
                    bank_img=None, x=None) -> None:
    """One post-network step of a solver of diffusion/solvers.py, in place on
    z, hist, step and (with the bank arguments) x.

    eps = (1+w) out[:B] - w out[B:];  x0 = c_a z - c_b eps (clamped to
    [-1,1] if clip);  z <- coef_z z + coef_x0 x0 + coef_hist hist
    + noise_scale sigma noise;  hist <- x0;  step += 1, coefficients taken
    from the (S,) tables at `step`. hist enters only where coef_hist is
    nonzero, so whatever it holds at the first step of a view (stale values,
    NaN) never reaches z; hist=None is a first-order solver, noise=None a
    deterministic one. With u, k, bank_img and x the next step's x is
    gathered as in ddpm_cfg_step."""
    B = z.shape[0]
    S = coef_z.shape[0]
    s = step.reshape(1)
    o = out.to(torch.float32)
    eps = (1.0 + w) * o[:B] - w * o[B:]
    x0 = c_a.index_select(0, s) * z - c_b.index_select(0, s) * eps
    if clip:
        x0 = x0.clamp(-1.0, 1.0)
    new = coef_z.index_select(0, s) * z + coef_x0.index_select(0, s) * x0
    if hist is not None:
        ch = coef_hist.index_select(0, s)
        # where(), not a product: 0 * NaN is NaN (and no host branch)
        new = new + torch.where(ch != 0, ch * hist, torch.zeros_like(hist))
        hist.copy_(x0)
    if noise is not None:
        new = new + (noise_scale * sigma.index_select(0, s)) * noise
    z.copy_(new)
    step.add_(1)
    if bank_img is None:
        return
    s1 = step.reshape(1).clamp(max=S - 1)
    idx = stochastic_index(u.index_select(0, s1)[0], k)
    nxt = bank_img[idx, torch.arange(B, device=z.device)]
    live = (step.reshape(()) < S)
    x.copy_(torch.where(live, torch.cat([nxt, nxt], dim=0), x))


# ---------------------------------------------------------------------------
# Image quality metrics (oracle for ops/hip/image_metrics.hip)
# ---------------------------------------------------------------------------

SSIM_WINDOW = 11
SSIM_SIGMA = 1.5
SSIM_C1 = 0.01 ** 2
SSIM_C2 = 0.03 ** 2


def ssim_window(dtype=torch.float64, device=None) -> torch.Tensor:
    """The 11-tap Gaussian (sigma 1.5), normalised to sum 1 in fp64."""
    x = torch.arange(SSIM_WINDOW, dtype=torch.float64) - (SSIM_WINDOW - 1) / 2
    g = torch.exp(-(x * x) / (2.0 * SSIM_SIGMA ** 2))
    return (g / g.sum()).to(dtype=dtype, device=device)


def check_image_pair(pred: torch.Tensor, target: torch.Tensor) -> None:
    if pred.dim() != 4 or pred.shape[-1] != 3 or pred.shape != target.shape:
        raise ValueError("image_metrics: pred and target must both be "
                         f"(N,H,W,3), got {tuple(pred.shape)} and "
                         f"{tuple(target.shape)}")
    if pred.dtype != target.dtype:
        raise ValueError("image_metrics: pred and target dtypes differ "
                         f"({pred.dtype} vs {target.dtype})")
    if pred.shape[1] < SSIM_WINDOW or pred.shape[2] < SSIM_WINDOW:
        raise ValueError(f"image_metrics: H and W must be >= {SSIM_WINDOW} "
                         f"(the SSIM window), got {tuple(pred.shape[1:3])}")


def image_metrics(pred: torch.Tensor, target: torch.Tensor,
                  quantize: bool = False
                  ) -> Tuple[torch.Tensor, torch.Tensor]:
    """PSNR (dB) and SSIM per image of (N,H,W,3) pairs in [-1,1].

    Per element u = clamp(x,-1,1)*0.5+0.5 (data_range 1); `quantize`
    replaces pred's u with trunc(u*255)/255, the 8-bit value sample.py writes
    to PNG, so the metrics equal those of the saved file. The target is left
    alone: a dataset image holds 8-bit levels already, and truncating k/255
    again would drop a quarter of the levels by one (k/255*255 < k in floating
    point). PSNR = 10 log10(1/mse), +inf at mse 0. SSIM (Wang et al. 2004) per
    channel with the separable 11-tap Gaussian window, population moments,
    C1 = 0.01^2, C2 = 0.03^2, averaged over the valid (H-10)*(W-10) window
    positions of the 3 channels (no padding). Works in the dtype it is
    given (bf16/fp16 are upcast to fp32); returns two (N,) tensors."""
    check_image_pair(pred, target)
    dt = pred.dtype if pred.dtype in (torch.float32, torch.float64) \
        else torch.float32

    def prep(x, q):
        u = x.to(dt).clamp(-1.0, 1.0) * 0.5 + 0.5
        if q:
            u = torch.trunc(u * 255.0) / 255.0
        return u

    x, y = prep(pred, quantize), prep(target, False)
    N, H, W, _ = x.shape
    mse = ((x - y) ** 2).mean(dim=(1, 2, 3))
    psnr = 10.0 * torch.log10(1.0 / mse)

    g = ssim_window(dt, x.device)
    gh, gv = g.view(1, 1, 1, -1), g.view(1, 1, -1, 1)

    def filt(t):
        return F.conv2d(F.conv2d(t, gh), gv)

    xc = x.permute(0, 3, 1, 2).reshape(N * 3, 1, H, W)
    yc = y.permute(0, 3, 1, 2).reshape(N * 3, 1, H, W)
    mu_x, mu_y = filt(xc), filt(yc)
    var_x = filt(xc * xc) - mu_x * mu_x
    var_y = filt(yc * yc) - mu_y * mu_y
    cov = filt(xc * yc) - mu_x * mu_y
    s = ((2.0 * mu_x * mu_y + SSIM_C1) * (2.0 * cov + SSIM_C2)
         / ((mu_x * mu_x + mu_y * mu_y + SSIM_C1)
            * (var_x + var_y + SSIM_C2)))
    ssim = s.reshape(N, -1).mean(dim=1)
    return psnr, ssim
