"""FusedAdam — single-launch multi-tensor Adam on MI355X (K18).

State layout matches torch.optim.Adam ('step', 'exp_avg', 'exp_avg_sq'),
so checkpoints interchange with the eager optimizer. Falls back to
torch.optim.Adam math on CPU / when the extension is unavailable.

Optional training recipe, all off by default:

  * ``max_grad_norm``: clip by the global L2 norm over every param group,
    ``g *= min(1, max_grad_norm / (norm + 1e-6))``. A step whose norm is not
    finite is skipped: p, m, v and the EMA stay bitwise unchanged and
    ``skipped_steps`` goes up by one. The per-param ``step`` counter still
    advances on a skipped step, because the bias-correction exponents are
    host scalars chosen before the device decides to skip; one skipped step
    therefore makes later bias corrections one step "older", which is
    harmless (they tend to 1) and keeps the host free of syncs.
  * ``ema_decay``: an exponential moving average of the parameters in
    ``state[p]["ema"]``, created as a copy of p together with the rest of
    the state, so it round-trips through ``state_dict()``. At step t
    (1-based) the decay is ``min(ema_decay, (1+t)/(10+t))`` with
    ``ema_warmup``, else ``ema_decay``.

On the GPU the norm, the clip factor and the skip flag stay on the device
(ops/hip/adam.hip): ``step()`` never syncs.
"""

from __future__ import annotations

import math
import warnings
from typing import Iterator, Optional, Tuple

import torch


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-4, betas=(0.9, 0.999), eps=1e-8,
                 max_grad_norm: Optional[float] = None,
                 ema_decay: Optional[float] = None,
                 ema_warmup: bool = True):
        if max_grad_norm is not None and not max_grad_norm > 0:
            raise ValueError(f"max_grad_norm must be > 0, got {max_grad_norm}")
        if ema_decay is not None and not 0.0 <= ema_decay < 1.0:
            raise ValueError(f"ema_decay must be in [0, 1), got {ema_decay}")
        defaults = dict(lr=lr, betas=betas, eps=eps)
        super().__init__(params, defaults)
        self.max_grad_norm = max_grad_norm
        self.ema_decay = ema_decay
        self.ema_warmup = ema_warmup
        self._plans = {}  # param-group index -> AdamPlan
        self._ctrl = None      # device [norm, scale, skip, skipped_steps]
        self._partials = None  # one fp32 partial per 64K-element chunk
        self._eager_norm = None
        self._eager_skipped = 0

    def _hip(self):
        try:
            from novel_view_synthesis_3d_amd.ops import hip_ops
            return hip_ops
        except Exception as e:
            import os
            if os.environ.get("NVS3D_ALLOW_EAGER_GPU", "0") == "1":
                return None
            # same fail-loudly policy as ops dispatch: a GPU box must not
            # silently fall back to the slow eager Adam
            raise RuntimeError(
                f"FusedAdam on GPU but nvs3d_hip extension unavailable: {e}"
            ) from e

    # -- recipe read-outs ------------------------------------------------
    @property
    def last_grad_norm(self) -> Optional[torch.Tensor]:
        """Global gradient norm of the last step as a 0-dim tensor on the
        params' device (None without max_grad_norm or before the first
        step). On the GPU it aliases the control buffer: reading it is the
        caller's sync, and the next step overwrites it."""
        if self._ctrl is not None:
            return self._ctrl[0]
        return self._eager_norm

    @property
    def skipped_steps(self) -> int:
        """Steps skipped for a non-finite gradient norm (syncs on GPU)."""
        if self._ctrl is not None:
            return int(self._ctrl[3].item())
        return self._eager_skipped

    def ema_parameters(self) -> Iterator[Tuple[torch.Tensor, torch.Tensor]]:
        """(param, ema) pairs for every param that has EMA state."""
        for group in self.param_groups:
            for p in group["params"]:
                st = self.state.get(p)
                if st is not None and "ema" in st:
                    yield p, st["ema"]

    def _ema_decay_at(self, step: int) -> float:
        d = self.ema_decay
        if self.ema_warmup:
            d = min(d, (1.0 + step) / (10.0 + step))
        return d

    # -- state -----------------------------------------------------------
    def _prepare_group(self, gi, group):
        """Lazy state init + step bookkeeping; returns (params, step)."""
        params = [p for p in group["params"] if p.grad is not None]
        if not params:
            return params, 0
        missing_ema = 0
        # lazy state init (torch.optim.Adam-compatible layout)
        for p in params:
            st = self.state[p]
            if len(st) == 0:
                st["step"] = torch.tensor(0.0)
                st["exp_avg"] = torch.zeros_like(p)
                st["exp_avg_sq"] = torch.zeros_like(p)
                if self.ema_decay is not None:
                    st["ema"] = p.detach().clone()
            elif self.ema_decay is not None and "ema" not in st:
                # state loaded from a checkpoint written without EMA
                st["ema"] = p.detach().clone()
                missing_ema += 1
        if missing_ema:
            warnings.warn(
                f"FusedAdam: optimizer state had no EMA for {missing_ema} "
                f"params of group {gi}; EMA initialised from the current "
                f"parameters")
        for p in params:
            self.state[p]["step"] += 1
        steps = {int(self.state[p]["step"].item()) for p in params}
        # the fused plan applies ONE bias correction to the whole group;
        # a param that skipped steps (no grad some iterations) would need
        # per-param correction — fail loudly instead of silently drifting
        if len(steps) != 1:
            raise RuntimeError(
                f"FusedAdam group {gi} has divergent per-param step counts "
                f"{sorted(steps)}; per-group fused bias correction is invalid")
        return params, steps.pop()

    def _plan(self, hip, gi, params):
        tuples = [(p, p.grad, self.state[p]["exp_avg"],
                   self.state[p]["exp_avg_sq"]) for p in params]
        emas = ([self.state[p]["ema"] for p in params]
                if self.ema_decay is not None else None)
        plan = self._plans.get(gi)
        if plan is None or not plan.matches(tuples, emas):
            plan = hip.AdamPlan(tuples, params[0].device, emas)
            self._plans[gi] = plan
        return plan

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        work = []  # (group index, group, params with grads, step)
        for gi, group in enumerate(self.param_groups):
            params, step = self._prepare_group(gi, group)
            if params:
                work.append((gi, group, params, step))
        if not work:
            return loss
        recipe = self.max_grad_norm is not None or self.ema_decay is not None
        first = work[0][2][0]
        hip = self._hip() if first.is_cuda else None

        if hip is not None:
            plans = [self._plan(hip, gi, params)
                     for gi, _, params, _ in work]
            ctrl = None
            if self.max_grad_norm is not None:
                # the global norm over ALL groups, before any group updates
                if self._ctrl is None:
                    self._ctrl = hip.grad_norm_ctrl(first.device)
                nparts = sum(pl.nchunks for pl in plans)
                if self._partials is None or self._partials.numel() != nparts:
                    self._partials = torch.empty(
                        nparts, dtype=torch.float32, device=first.device)
                hip.fused_grad_norm(plans, self._partials, self._ctrl,
                                    self.max_grad_norm)
                ctrl = self._ctrl
            for plan, (gi, group, params, step) in zip(plans, work):
                b1, b2 = group["betas"]
                if not recipe:
                    hip.fused_adam_step(plan, group["lr"], b1, b2,
                                        group["eps"], step)
                else:
                    d = (self._ema_decay_at(step)
                         if self.ema_decay is not None else None)
                    hip.fused_adam_recipe_step(plan, group["lr"], b1, b2,
                                               group["eps"], step,
                                               ctrl=ctrl, ema_decay=d)
            return loss

        # eager branch (CPU path / parity tests): the same math in fp32
        scale = None
        if self.max_grad_norm is not None:
            sq = [torch.sum(p.grad.float() ** 2)
                  for _, _, params, _ in work for p in params]
            norm = torch.sqrt(torch.stack(sq).sum())
            self._eager_norm = norm
            if not bool(torch.isfinite(norm)):
                self._eager_skipped += 1
                return loss
            scale = torch.clamp(self.max_grad_norm / (norm + 1e-6), max=1.0)
        for gi, group, params, step in work:
            b1, b2 = group["betas"]
            bc1 = 1 - b1 ** step
            bc2 = 1 - b2 ** step
            d = None
            if self.ema_decay is not None:
                # the kernel holds d in fp32 and forms 1-d from that
                d = float(torch.tensor(self._ema_decay_at(step),
                                       dtype=torch.float32))
            for p in params:
                st = self.state[p]
                g = p.grad if scale is None else p.grad * scale
                st["exp_avg"].mul_(b1).add_(g, alpha=1 - b1)
                st["exp_avg_sq"].mul_(b2).addcmul_(g, g, value=1 - b2)
                denom = (st["exp_avg_sq"] / bc2).sqrt_().add_(group["eps"])
                p.addcdiv_(st["exp_avg"] / bc1, denom, value=-group["lr"])
                if d is not None:
                    st["ema"].mul_(d).add_(p, alpha=1 - d)
        return loss
