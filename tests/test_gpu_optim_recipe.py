"""Fused grad-norm clip + Adam + EMA step on the MI355X (ops/hip/adam.hip)
against the float64 oracle of test_optim_recipe.py.

The problem includes one gradient that is an element-offset-1 view into a
flat buffer (4-byte, not 16-byte aligned): the data-parallel bucket layout,
which takes the kernels' scalar loops.
"""

import pytest
import torch

from test_optim_recipe import (  # tests/ is on sys.path via conftest
    EMA_DECAY, HYPER, MAX_NORM, TOL, max_err, oracle, problem, run_optimizer,
)

pytestmark = pytest.mark.gpu


def test_grad_norm_matches_float64_and_is_deterministic():
    """Relative tolerance 2e-5. Longest fp32 add chain in grad_sqnorm: 64
    FMAs per accumulator (4 accumulators per thread over a 64K chunk), at
    most 3 tail adds, 2 adds to join the accumulators, 6 shuffle levels and
    3 LDS adds = 78 roundings, fewer than the ~265 the bound was derived for
    (265 * 2^-24 = 1.6e-5 on the sum, halved by the square root); the
    partials are then summed in double."""
    opt, params, norms = run_optimizer("cuda", True, True, False)
    _, _, n64 = oracle(True, True, False)
    for k, (got, want) in enumerate(zip(norms, n64)):
        rel = abs(float(got) - want) / want
        print(f"step {k}: norm {float(got):.6g} want {want:.6g} rel {rel:.2e}")
        assert rel <= 2e-5, (k, rel)
    assert opt.skipped_steps == 0
    # same gradients again: bit-identical norm (fixed reduction order)
    first = opt.last_grad_norm.clone()
    opt.step()
    assert torch.equal(first, opt.last_grad_norm)


@pytest.mark.parametrize("clip,ema", [(True, False), (False, True),
                                      (True, True), (False, False)])
def test_fused_step_matches_float64_oracle(clip, ema):
    opt, params, _ = run_optimizer("cuda", True, clip, ema)
    p64, e64, _ = oracle(True, clip, ema)
    err = max_err(params, p64)
    print(f"clip={clip} ema={ema}: param err {err:.3e}")
    assert err < TOL, err
    pairs = list(opt.ema_parameters())
    if ema:
        assert len(pairs) == len(params)
        err = max_err([e for _, e in pairs], e64)
        print(f"clip={clip} ema={ema}: ema err {err:.3e}")
        assert err < TOL, err
    else:
        assert pairs == []


def test_no_options_is_bitwise_the_fused_adam_op():
    """Options unset: FusedAdam, and the recipe entry point with neither
    part enabled, give the bits of the existing fused_adam op."""
    from novel_view_synthesis_3d_amd.ops import hip_ops
    p0, grads = problem(True)
    _, params, _ = run_optimizer("cuda", True, False, False)

    def raw(step_fn):
        ps = [x.cuda().clone() for x in p0]
        ms = [torch.zeros_like(x) for x in ps]
        vs = [torch.zeros_like(x) for x in ps]
        gs = [torch.zeros_like(x) for x in ps]
        n = ps[-1].numel()
        flat = torch.zeros(n + 8, device="cuda")
        gs[-1] = flat[1:1 + n]
        plan = hip_ops.AdamPlan(list(zip(ps, gs, ms, vs)), ps[0].device)
        b1, b2 = HYPER["betas"]
        for t, step_grads in enumerate(grads, start=1):
            for g, src in zip(gs, step_grads):
                g.copy_(src)
            step_fn(plan, HYPER["lr"], b1, b2, HYPER["eps"], t)
        return ps

    old = raw(hip_ops.fused_adam_step)
    new = raw(hip_ops.fused_adam_recipe_step)
    for a, b, c in zip(old, new, params):
        assert torch.equal(a, b)
        assert torch.equal(a, c.detach())


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_non_finite_step_is_skipped_on_device(bad):
    from novel_view_synthesis_3d_amd.engine.optim import FusedAdam
    p0, grads = problem(False)
    params = [x.cuda().clone().requires_grad_(True) for x in p0]
    opt = FusedAdam(params, max_grad_norm=MAX_NORM, ema_decay=EMA_DECAY,
                    **HYPER)
    for p, g in zip(params, grads[1]):
        p.grad = g.cuda().clone()
    opt.step()
    keys = ("exp_avg", "exp_avg_sq", "ema")
    before = [[p.detach().clone()] + [opt.state[p][k].clone() for k in keys]
              for p in params]
    params[6].grad[70000] = bad  # second chunk of the 131077 tensor
    opt.step()
    assert opt.skipped_steps == 1
    assert not torch.isfinite(opt.last_grad_norm)
    for p, saved in zip(params, before):
        now = [p.detach()] + [opt.state[p][k] for k in keys]
        for a, b in zip(now, saved):
            assert torch.equal(a, b)
    # the next finite step updates normally
    for p, g in zip(params, grads[2]):
        p.grad.copy_(g.cuda())
    opt.step()
    assert opt.skipped_steps == 1
    assert torch.isfinite(opt.last_grad_norm)
    for p, saved in zip(params, before):
        assert torch.isfinite(p).all()
        assert not torch.equal(p.detach(), saved[0])
        assert not torch.equal(opt.state[p]["ema"], saved[3])


def test_trainer_recipe_checkpoint_and_ema_sampling(tmp_path):
    from novel_view_synthesis_3d_amd.config import TrainConfig, XUNetConfig
    from novel_view_synthesis_3d_amd.data.synthetic import synthetic_batch
    from novel_view_synthesis_3d_amd.diffusion.sampler import DDPMSampler
    from novel_view_synthesis_3d_amd.engine import checkpoint as ckpt
    from novel_view_synthesis_3d_amd.engine.trainer import Trainer
    from novel_view_synthesis_3d_amd.models.xunet import XUNet
    cfg = TrainConfig()
    cfg.data = "synthetic"
    cfg.log_every = 10 ** 9
    cfg.ckpt_folder = str(tmp_path / "ckpt")
    cfg.max_grad_norm = 1.0
    cfg.ema_decay = 0.999
    cfg.lr_warmup_steps = 2
    mc = XUNetConfig.named("small")
    trainer = Trainer(None, train_batch_size=2, train_lr=1e-3,
                      train_num_steps=10 ** 9, img_sidelength=64,
                      results_folder=str(tmp_path / "res"),
                      model_cfg=mc, train_cfg=cfg)
    lrs = []
    for k in range(3):
        trainer.step = k
        loss = trainer.train_step()
        lrs.append(trainer.opt.param_groups[0]["lr"])
    assert lrs == pytest.approx([5e-4, 1e-3, 1e-3])
    assert torch.isfinite(loss)
    assert trainer.opt.skipped_steps == 0
    assert float(trainer.opt.last_grad_norm) > 0
    pairs = list(trainer.opt.ema_parameters())
    assert len(pairs) == len(list(trainer.model.parameters()))
    assert any(not torch.equal(p.detach(), e) for p, e in pairs)

    path = ckpt.save_checkpoint(cfg.ckpt_folder, trainer.model, trainer.opt, 3)
    model = XUNet(mc, 64).cuda()
    ckpt.load_checkpoint(path, model, map_location="cuda", use_ema=True)
    for p, (_, e) in zip(model.parameters(), pairs):
        assert torch.equal(p.detach(), e)
    model.eval()
    g = torch.Generator(device="cuda").manual_seed(0)
    cond = synthetic_batch(1, 64, "cuda", g)
    cond.pop("x_target")
    out = DDPMSampler(model, num_steps=2, use_graph=False).sample(cond)
    assert torch.isfinite(out).all()
