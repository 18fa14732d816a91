"""Op dispatch: hand-written CDNA4 HIP kernels on MI355X, eager torch elsewhere.

Policy (see repo instructions / SURVEY.md §7):
  * On a CUDA(ROCm) device, ops that have a HIP implementation MUST run it —
    if the in-tree extension is missing on a GPU box this raises loudly
    instead of silently falling back to eager (set NVS3D_ALLOW_EAGER_GPU=1
    only for debugging).
  * On CPU, and for ops whose HIP kernel has not landed yet, the eager
    reference implementation (ops/reference.py) runs — it is also the
    numerics oracle for the GPU parity tests.
  * NVS3D_FORCE_EAGER=1 forces eager everywhere (parity testing on GPU).
"""

from __future__ import annotations

import os
from typing import Optional

import torch

from novel_view_synthesis_3d_amd.ops import reference as ref
from novel_view_synthesis_3d_amd.ops.reference import (  # noqa: F401  (pure host math)
    posenc_ddpm, squash_logsnr, posenc_nerf, SQRT_HALF,
)


def _force_eager() -> bool:
    return os.environ.get("NVS3D_FORCE_EAGER", "0") == "1"


def _hip():
    """Import the HIP op wrappers lazily; returns module or None (CPU-only)."""
    global _HIP_MOD, _HIP_TRIED
    if not _HIP_TRIED:
        _HIP_TRIED = True
        try:
            from novel_view_synthesis_3d_amd.ops import hip_ops
            _HIP_MOD = hip_ops
        except Exception as e:  # extension genuinely unavailable
            _HIP_MOD = None
            _HIP_IMPORT_ERROR.append(e)
    return _HIP_MOD


_HIP_MOD = None
_HIP_TRIED = False
_HIP_IMPORT_ERROR: list = []


def _use_hip(x: torch.Tensor, opname: str) -> bool:
    if not x.is_cuda or _force_eager():
        return False
    mod = _hip()
    if mod is None:
        if os.environ.get("NVS3D_ALLOW_EAGER_GPU", "0") == "1":
            return False
        raise RuntimeError(
            f"op '{opname}' invoked on a GPU tensor but the nvs3d_hip extension "
            f"is not available ({_HIP_IMPORT_ERROR}). Build it with "
            f"`python setup.py build_ext --inplace` (or __graft_entry__.build()); "
            f"set NVS3D_ALLOW_EAGER_GPU=1 only for debugging.")
    return opname in mod.HAS


def hip_available() -> bool:
    mod = _hip()
    return mod is not None


def _bf16_path(x: torch.Tensor) -> bool:
    """The bf16 HIP kernels take x as it is or as autocast will cast it."""
    return x.dtype == torch.bfloat16 or torch.is_autocast_enabled()


# ---------------------------------------------------------------------------
# Dispatched ops. Signatures match ops/reference.py.
# ---------------------------------------------------------------------------

def frame_conv3x3(x, weight, bias, stride: int = 1):
    if _use_hip(x, "frame_conv3x3"):
        if _bf16_path(x):  # MFMA igemm kernel or im2col+hipBLASLt — no MIOpen
            return _HIP_MOD.frame_conv3x3(x, weight, bias, stride)
    return ref.frame_conv3x3(x, weight, bias, stride)


def joint_groupnorm(x, gamma, beta, groups: int, eps: float = 1e-6,
                    film=None, silu: bool = False, p_drop: float = 0.0):
    if _use_hip(x, "joint_groupnorm"):
        return _HIP_MOD.joint_groupnorm(x, gamma, beta, groups, eps,
                                        film, silu, p_drop)
    return ref.joint_groupnorm(x, gamma, beta, groups, eps, film, silu,
                               p_drop)


def attention(q, k, v, kv_swap: bool = False):
    """kv_swap=True: batch b's queries attend batch b^1's keys/values —
    the model's cross-FRAME attention with both frames batched as (B*2)."""
    if _use_hip(q, "attention"):
        B, L, h, d = q.shape
        if _bf16_path(q) and L % 64 == 0 and d in (16, 32, 64, 128, 256):
            return _HIP_MOD.attention(q, k, v, kv_swap)
    if kv_swap:
        k = ref.swap_frame_pairs(k)
        v = ref.swap_frame_pairs(v)
    return ref.attention(q, k, v)


def linear(x, w, b=None):
    """nn.Linear forward; on MI355X the backward uses the split-K MFMA
    wgrad kernel for the tall-skinny shapes hipBLASLt collapses on."""
    if _use_hip(x, "linear"):
        if _bf16_path(x):
            return _HIP_MOD.linear(x, w, b)
    import torch.nn.functional as F
    return F.linear(x, w, b)


def nearest_upsample2x(x):
    if _use_hip(x, "nearest_upsample2x"):
        return _HIP_MOD.nearest_upsample2x(x)
    return ref.nearest_upsample2x(x)


def avgpool_downsample2x(x):
    if _use_hip(x, "avgpool_downsample2x"):
        return _HIP_MOD.avgpool_downsample2x(x)
    return ref.avgpool_downsample2x(x)


def residual_scale_add(h, h_in):
    if _use_hip(h, "residual_scale_add"):
        return _HIP_MOD.residual_scale_add(h, h_in)
    return ref.residual_scale_add(h, h_in)


def frame_conv3x3_residual(x, weight, bias, residual, res_scale: float):
    """Fused ResnetBlock tail: (conv(x,w)+bias+residual)*res_scale."""
    if _use_hip(x, "frame_conv3x3"):
        if _bf16_path(x):
            return _HIP_MOD.frame_conv3x3_residual(x, weight, bias,
                                                   residual, res_scale)
    y = ref.frame_conv3x3(x, weight, bias, 1)
    return (y + residual) * res_scale


def pose_embedding(R, t, K, cond_mask, H: int, W: int, out_dtype):
    if _use_hip(R, "pose_embedding"):
        return _HIP_MOD.pose_embedding(R, t, K, cond_mask, H, W, out_dtype)
    return ref.pose_embedding(R, t, K, cond_mask, H, W, out_dtype)


# ---------------------------------------------------------------------------
# Stochastic-conditioning sampler step (ops/hip/sampler_step.hip)
# ---------------------------------------------------------------------------

stochastic_index = ref.stochastic_index  # the index rule (pure torch)


def cond_emb_select(logsnr_emb, bank, null_feat, tgt_feat, u, step, k):
    """silu(logsnr_emb + pose feature) for one level, the frame-0 feature of
    the conditional half gathered from `bank` by the device-side index."""
    if _use_hip(bank, "cond_emb_select"):
        return _HIP_MOD.cond_emb_select(logsnr_emb, bank, null_feat,
                                        tgt_feat, u, step, k)
    return ref.cond_emb_select(logsnr_emb, bank, null_feat, tgt_feat, u,
                               step, k)


def ddpm_cfg_step(z, out, noise, c_a, c_b, c1, c2, sigma, step, u, k,
                  bank_img, x, w: float, clip: bool,
                  noise_scale: float = 1.0, step_scratch=None) -> None:
    """CFG combine + ancestral step in place on z; advances `step` and
    writes the next step's model input x from the image bank.
    `step_scratch` is a one-element int64 work slot of the HIP kernels."""
    if _use_hip(z, "ddpm_cfg_step"):
        return _HIP_MOD.ddpm_cfg_step(z, out, noise, c_a, c_b, c1, c2, sigma,
                                      step, u, k, bank_img, x, w, clip,
                                      noise_scale, step_scratch)
    return ref.ddpm_cfg_step(z, out, noise, c_a, c_b, c1, c2, sigma, step, u,
                             k, bank_img, x, w, clip, noise_scale)


def solver_cfg_step(z, hist, out, noise, c_a, c_b, coef_z, coef_x0, coef_hist,
                    sigma, step, w: float, clip: bool,
                    noise_scale: float = 1.0, *, u=None, k=None,
                    bank_img=None, x=None, step_scratch=None) -> None:
    """CFG combine + one step of a solver of diffusion/solvers.py in place on
    z; hist (or None) carries the previous step's x0, noise may be None.
    Advances `step`; with u, k, bank_img and x also writes the next step's
    model input x from the image bank, as ddpm_cfg_step does."""
    if _use_hip(z, "solver_cfg_step"):
        return _HIP_MOD.solver_cfg_step(
            z, hist, out, noise, c_a, c_b, coef_z, coef_x0, coef_hist, sigma,
            step, w, clip, noise_scale, u=u, k=k, bank_img=bank_img, x=x,
            step_scratch=step_scratch)
    return ref.solver_cfg_step(z, hist, out, noise, c_a, c_b, coef_z, coef_x0,
                               coef_hist, sigma, step, w, clip, noise_scale,
                               u=u, k=k, bank_img=bank_img, x=x)


# ---------------------------------------------------------------------------
# Image quality metrics (ops/hip/image_metrics.hip)
# ---------------------------------------------------------------------------

def image_metrics(pred, target, quantize: bool = False):
    """PSNR (dB) and SSIM of (N,H,W,3) image pairs in [-1,1]; two (N,)
    tensors on the inputs' device (definition: ref.image_metrics). fp32 and
    bf16 inputs on the GPU take the fused kernel: fp32 results, no host
    sync. H or W below the 11-pixel SSIM window raises ValueError."""
    ref.check_image_pair(pred, target)
    pred, target = pred.contiguous(), target.contiguous()
    if (_use_hip(pred, "image_metrics")
            and pred.dtype in (torch.float32, torch.bfloat16)):
        return _HIP_MOD.image_metrics(pred, target, quantize)
    return ref.image_metrics(pred, target, quantize)
