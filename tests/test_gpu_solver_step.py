"""solver_cfg_step (sampler_step.hip) on the MI355X: parity with a float64
oracle on the same fp32 inputs, hipGraph replay vs eager, the multi-view
sampler vs the CPU oracle path, and the dispatch.

Tolerance of the kernel test, the rule of `_ddpm_bound` in
test_gpu_sampler_kernels.py: 8 fp32 ulps of the magnitudes entering each sum
(formula in `_solver_bounds`)."""

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from novel_view_synthesis_3d_amd import ops
    from novel_view_synthesis_3d_amd.ops import hip_ops

DEV = "cuda"
COEFS = ("sqrt_recip_abar", "sqrt_recipm1_abar", "coef_z", "coef_x0",
         "coef_hist", "sigma")
S = 6
SOLVERS = {                       # id -> (solver, spacing, eta)
    "ddpm": ("ddpm", "uniform", 0.0),
    "ddim": ("ddim", "uniform", 0.0),
    "ddim_eta": ("ddim", "logsnr", 0.5),
    "dpmpp2m": ("dpmpp2m", "logsnr", 0.0),
}


def _long(v):
    return torch.tensor([v], dtype=torch.long, device=DEV)


def _host_index(u_row, k):
    """The index rule on the host, in fp32 (numpy)."""
    import numpy as np
    u32 = u_row.cpu().numpy().astype(np.float32)
    return [min(int(np.floor(x * np.float32(k))), k - 1) for x in u32]


def _tables(name):
    from novel_view_synthesis_3d_amd.diffusion.schedules import (
        DiffusionSchedule,
    )
    from novel_view_synthesis_3d_amd.diffusion.solvers import (
        device_tables, solver_tables,
    )
    solver, spacing, eta = SOLVERS[name]
    return device_tables(solver_tables(DiffusionSchedule(1000), S, solver,
                                       spacing=spacing, eta=eta),
                         torch.device(DEV))


def _oracle64(c, z, hist, out, noise, w, clip):
    """(z', x0, bound on z', bound on x0) in float64; c: the step's fp32
    coefficients as Python floats."""
    B = z.shape[0]
    o, z = out.double(), z.double()
    eps = (1.0 + w) * o[:B] - w * o[B:]
    x0 = c["sqrt_recip_abar"] * z - c["sqrt_recipm1_abar"] * eps
    mag_x0 = ((c["sqrt_recip_abar"] * z).abs()
              + (c["sqrt_recipm1_abar"] * eps).abs())
    if clip:
        x0 = x0.clamp(-1.0, 1.0)
    new = c["coef_z"] * z + c["coef_x0"] * x0
    mag = (mag_x0 * abs(c["coef_x0"]) + (c["coef_z"] * z).abs()
           + (c["coef_x0"] * x0).abs())
    if hist is not None and c["coef_hist"] != 0.0:
        new = new + c["coef_hist"] * hist.double()
        mag = mag + (c["coef_hist"] * hist.double()).abs()
    if noise is not None:
        new = new + c["sigma"] * noise.double()
        mag = mag + (c["sigma"] * noise.double()).abs()
    ulp8 = 8.0 * 2.0 ** -23
    return new, x0, ulp8 * mag, ulp8 * mag_x0


@pytest.mark.parametrize("name", list(SOLVERS))
@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("shape", [(1, 2, 2, 3), (1, 3, 3, 3), (2, 8, 8, 3)],
                         ids=["n12", "n27", "n384"])
def test_solver_cfg_step_matches_f64_oracle(shape, out_dtype, name):
    Kcap, k = 3, 2
    B = shape[0]
    tab = _tables(name)
    g = torch.Generator(device=DEV).manual_seed(7)
    u = torch.rand(S, B, device=DEV, generator=g)
    bank_img = torch.randn(Kcap, *shape, device=DEV, generator=g)
    bank_img[k:] = float("nan")
    rows = torch.arange(B, device=DEV)
    worst_z = worst_h = -1.0
    max_z = max_h = 0.0

    def call(z, hist, out, noise, s, w, clip, x, bank):
        step = _long(s)
        kw = (dict(u=u, k=_long(k), bank_img=bank_img, x=x) if bank else {})
        hip_ops.solver_cfg_step(z, hist, out, noise,
                                *(tab[n] for n in COEFS), step, w, clip, 1.0,
                                **kw)
        return int(step)

    for s in (0, 1, S - 2, S - 1):
        c = {n: float(tab[n][s].double()) for n in COEFS}
        for clip in (True, False):
            for w in (0.0, 3.0):
                for with_noise in (True, False):
                    for bank in (True, False):
                        # hist=None where the solver has no history and the
                        # bank is off: both call forms on every solver
                        with_hist = name == "dpmpp2m" or bank
                        z0 = torch.randn(*shape, device=DEV, generator=g)
                        h0 = torch.randn(*shape, device=DEV, generator=g)
                        out = torch.randn(2 * B, *shape[1:], device=DEV,
                                          generator=g).to(out_dtype)
                        noise = (torch.randn(*shape, device=DEV, generator=g)
                                 if with_noise else None)
                        x = torch.full((2 * B, *shape[1:]), -7.0, device=DEV)
                        z = z0.clone()
                        hist = h0.clone() if with_hist else None
                        assert call(z, hist, out, noise, s, w, clip, x,
                                    bank) == s + 1
                        want, x0, bz, bh = _oracle64(
                            c, z0, h0 if with_hist else None, out, noise, w,
                            clip)
                        ez = (z.double() - want).abs()
                        worst_z = max(worst_z, (ez - bz).max().item())
                        max_z = max(max_z, ez.max().item())
                        print(f"{name} {shape} {out_dtype} s={s} clip={clip} "
                              f"w={w} noise={with_noise} bank={bank}: max "
                              f"err {ez.max().item():.3e}, max (err-bound) "
                              f"{(ez - bz).max().item():.3e}")
                        assert (ez <= bz).all(), (s, clip, w, with_noise,
                                                  bank, ez.max().item())
                        if with_hist:
                            eh = (hist.double() - x0).abs()
                            worst_h = max(worst_h, (eh - bh).max().item())
                            max_h = max(max_h, eh.max().item())
                            assert (eh <= bh).all(), (s, clip, w, eh.max())
                            if clip:
                                assert float(hist.abs().max()) <= 1.0
                        # next step's x: gathered under the index rule, left
                        # alone after the last step and without a bank
                        if bank and s + 1 < S:
                            idx = torch.tensor(_host_index(u[s + 1], k),
                                               device=DEV)
                            nxt = bank_img[idx, rows]
                            assert torch.equal(x, torch.cat([nxt, nxt]))
                        else:
                            assert (x == -7.0).all()
                        # a step that does not use the history: NaN in it
                        # changes nothing
                        if with_hist and c["coef_hist"] == 0.0:
                            z2 = z0.clone()
                            h2 = torch.full_like(h0, float("nan"))
                            call(z2, h2, out, noise, s, w, clip, x, bank)
                            assert torch.isfinite(z2).all()
                            assert torch.equal(z2, z)
                            assert torch.equal(h2, hist)
                        # sigma 0: noise given or not is the same step
                        if with_noise and c["sigma"] == 0.0:
                            z2 = z0.clone()
                            h2 = h0.clone() if with_hist else None
                            call(z2, h2, out, None, s, w, clip, x, bank)
                            assert torch.equal(z2, z)
    print(f"solver_cfg_step {name} {shape} {out_dtype}: z max err "
          f"{max_z:.3e}, max (err-bound) {worst_z:.3e}; hist max err "
          f"{max_h:.3e}, max (err-bound) {worst_h:.3e}")
    # the tables cover what the cases above rely on
    assert float(tab["coef_hist"][0]) == 0.0
    if name == "dpmpp2m":
        assert float(tab["coef_hist"][1]) != 0.0
        assert float(tab["coef_hist"][S - 2]) != 0.0
    if name in ("ddpm", "ddim_eta"):
        assert float(tab["sigma"][0]) != 0.0


def test_dispatch_reaches_the_hip_op(monkeypatch):
    shape, B = (2, 5, 5, 3), 2
    tab = _tables("dpmpp2m")
    g = torch.Generator(device=DEV).manual_seed(3)
    z0 = torch.randn(*shape, device=DEV, generator=g)
    h0 = torch.randn(*shape, device=DEV, generator=g)
    out = torch.randn(2 * B, *shape[1:], device=DEV, generator=g)
    calls = []
    real = hip_ops.solver_cfg_step

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    za, ha, sa = z0.clone(), h0.clone(), _long(1)
    real(za, ha, out, None, *(tab[n] for n in COEFS), sa, 3.0, True)
    monkeypatch.setattr(hip_ops, "solver_cfg_step", counted)
    zb, hb, sb = z0.clone(), h0.clone(), _long(1)
    ops.solver_cfg_step(zb, hb, out, None, *(tab[n] for n in COEFS), sb, 3.0,
                        True)
    assert calls == [1]
    assert torch.equal(za, zb) and torch.equal(ha, hb)
    assert int(sa) == int(sb) == 2
    assert not torch.equal(za, z0)


# ---------------------------------------------------------------------------
# whole sampler (helpers of test_gpu_sampler_kernels.py)
# ---------------------------------------------------------------------------

def _model32():
    from novel_view_synthesis_3d_amd.config import XUNetConfig
    from novel_view_synthesis_3d_amd.models.xunet import XUNet
    torch.manual_seed(0)
    cfg = XUNetConfig(ch=32, ch_mult=(1, 2), emb_ch=32, num_res_blocks=1,
                      attn_resolutions=(16,), dropout=0.0)
    model = XUNet(cfg, img_sidelength=32)
    with torch.no_grad():
        model.Conv_1.weight.normal_(0, 0.05)
    return model


def _scene(B, N):
    from novel_view_synthesis_3d_amd.data.synthetic import (
        random_cameras, synthetic_batch,
    )
    g = torch.Generator().manual_seed(0)
    cond = synthetic_batch(B, 32, generator=g)
    cams = [random_cameras(B, 32, generator=g) for _ in range(N)]
    tR = torch.stack([c[0] for c in cams])
    tt = torch.stack([c[1] for c in cams])
    z0 = torch.randn(N, B, 32, 32, 3, generator=g)
    return cond, tR, tt, z0


def _sample(sampler, cond, tR, tt, z0, dev, **kw):
    c = {k: v.to(dev) for k, v in cond.items()}
    return sampler.sample_views(c["x"], c["R1"], c["t1"], c["K"], tR.to(dev),
                                tt.to(dev), z_init=z0.to(dev),
                                guidance_weight=3.0, clip_denoised=True,
                                seed=3, solver="dpmpp2m", spacing="logsnr",
                                **kw)


class _ElementwiseNet(torch.nn.Module):
    """Bitwise-reproducible stand-in for XUNet with the same conditioning
    interface: the real ConditioningProcessor fills the bank, the forward
    consumes the fused per-level embeddings, x and z through elementwise ops
    and fixed-shape reductions only (no atomics anywhere)."""

    def __init__(self, real):
        super().__init__()
        self.cfg = real.cfg
        self.ConditioningProcessor_0 = real.ConditioningProcessor_0

    def forward(self, batch, cond_mask, pose_cache=None):
        lemb = ops.posenc_ddpm(ops.squash_logsnr(batch["logsnr"]),
                               emb_ch=self.cfg.emb_ch, max_time=1.0)
        x, z = batch["x"], batch["z"]
        out = 0.05 * z
        for lvl in range(self.cfg.num_resolutions):
            e = pose_cache.emb(lvl, lemb).float().mean(-1, keepdim=True)
            r = 2 ** lvl
            e = e.repeat_interleave(r, dim=2).repeat_interleave(r, dim=3)
            out = out + (0.3 * e[:, 0] * x + 0.2 * e[:, 1] * z) / (lvl + 1)
        return out


def test_graph_replay_equals_eager_exactly():
    """dpmpp2m on log-SNR spacing, 3 views x 6 steps: the history buffer is
    part of the one captured step and carries over from view to view."""
    from novel_view_synthesis_3d_amd.diffusion.sampler import (
        StochasticConditioningSampler,
    )
    net = _ElementwiseNet(_model32().cuda())
    cond, tR, tt, z0 = _scene(2, 3)
    sampler = StochasticConditioningSampler(net)
    rng = torch.cuda.get_rng_state()
    eager = _sample(sampler, cond, tR, tt, z0, DEV, num_steps=S,
                    use_graph=False)
    assert sampler.num_captures == 0
    assert sampler.state["hist"] is not None
    log_eager = [i.cpu() for i in sampler.index_log]
    graph = _sample(sampler, cond, tR, tt, z0, DEV, num_steps=S,
                    use_graph=True)
    assert sampler.num_captures == 1        # one capture for all N*S steps
    assert torch.equal(torch.cuda.get_rng_state(), rng)   # no randn issued
    assert all(torch.equal(a, b.cpu())
               for a, b in zip(log_eager, sampler.index_log))
    assert torch.isfinite(graph).all()
    assert not torch.equal(graph[0], graph[1])
    assert not torch.equal(graph[1], graph[2])
    assert torch.equal(graph, eager)


def test_single_view_sampler_graph_equals_eager():
    """DDPMSampler has no bank: the counter is published by the one-thread
    kernel, in the captured step as in the eager one."""
    from novel_view_synthesis_3d_amd.diffusion.sampler import DDPMSampler
    cond, _, _, z0 = _scene(2, 1)
    c = {k: v.to(DEV) for k, v in cond.items() if k != "x_target"}

    class _ListCacheNet(torch.nn.Module):
        """DDPMSampler hands the model a list of pose features, not a bank:
        the same elementwise forward on that list."""

        def __init__(self, inner):
            super().__init__()
            self.cfg = inner.cfg
            self.ConditioningProcessor_0 = inner.ConditioningProcessor_0

        def forward(self, batch, cond_mask, pose_cache=None):
            x, z = batch["x"], batch["z"]
            out = 0.05 * z + 0.01 * batch["logsnr"].reshape(-1, 1, 1, 1)
            for lvl, f in enumerate(pose_cache):
                e = f.float().mean(-1, keepdim=True)
                r = 2 ** lvl
                e = e.repeat_interleave(r, dim=2).repeat_interleave(r, dim=3)
                out = out + (0.3 * e[:, 0] * x + 0.2 * e[:, 1] * z) / (lvl + 1)
            return out

    net = _ListCacheNet(_model32().cuda())
    kw = dict(num_steps=S, solver="dpmpp2m", spacing="logsnr")
    eager = DDPMSampler(net, **kw).sample(c, z_init=z0[0].to(DEV))
    graph = DDPMSampler(net, use_graph=True, **kw).sample(
        c, z_init=z0[0].to(DEV))
    assert torch.isfinite(graph).all()
    assert torch.equal(graph, eager)
    other = DDPMSampler(net, num_steps=S, solver="ddim",
                        spacing="logsnr").sample(c, z_init=z0[0].to(DEV))
    assert not torch.equal(other, eager)    # the history is used


def test_gpu_sampler_matches_cpu_oracle_fp32():
    from novel_view_synthesis_3d_amd.diffusion.sampler import (
        StochasticConditioningSampler,
    )
    model = _model32()
    cond, tR, tt, z0 = _scene(2, 2)
    cpu = StochasticConditioningSampler(model)
    want = _sample(cpu, cond, tR, tt, z0, "cpu", num_steps=4)
    log_cpu = [i.clone() for i in cpu.index_log]

    gpu = StochasticConditioningSampler(model.cuda(), autocast=False)
    got = _sample(gpu, cond, tR, tt, z0, DEV, num_steps=4)
    assert all(torch.equal(a, b.cpu())
               for a, b in zip(log_cpu, gpu.index_log))
    err = (got.cpu() - want).abs().max().item()
    scale = want.abs().max().item()
    print(f"dpmpp2m sampler gpu vs cpu: max err {err:.3e}, scale {scale:.3e}")
    assert err < 5e-3 * max(scale, 1.0), (err, scale)
