"""Training recipe on CPU: grad-norm clip + Adam + EMA (FusedAdam's eager
branch), LR warmup, EMA checkpoints and EMA sampling.

The float64 oracle below (clip -> Adam -> EMA) is also the reference of the
GPU tests in test_gpu_optim_recipe.py.
"""

import copy
import functools
import os
import subprocess
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from novel_view_synthesis_3d_amd.engine import checkpoint as ckpt
from novel_view_synthesis_3d_amd.engine.optim import FusedAdam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(1,), (3,), (4,), (33,), (65536,), (65537,), (131077,),
          (256, 129), (7, 3, 3, 5)]
# an extra tensor whose gradient is an element-offset-1 view into a flat
# buffer (the data-parallel bucket layout): 4-byte but not 16-byte aligned
MISALIGNED_SHAPE = (70001,)
GRAD_SCALES = [1e-3, 1, 30, 1e-3, 5, 1e-4]
HYPER = dict(lr=1e-2, betas=(0.9, 0.99), eps=1e-8)
MAX_NORM = 1.0
EMA_DECAY = 0.9
TOL = 1e-5  # the project's Adam tolerance (test_gpu_kernels.py)


@functools.lru_cache(maxsize=None)
def problem(misaligned: bool = False):
    """(params, grads[step][i]) on CPU in fp32; never modified by tests."""
    shapes = SHAPES + ([MISALIGNED_SHAPE] if misaligned else [])
    g = torch.Generator().manual_seed(0)
    params = [torch.randn(s, generator=g) for s in shapes]
    grads = [[torch.randn(s, generator=g) * scale for s in shapes]
             for scale in GRAD_SCALES]
    return params, grads


@functools.lru_cache(maxsize=None)
def oracle(misaligned: bool, clip: bool, ema: bool, ema_warmup: bool = True):
    """float64 clip -> Adam -> EMA over all steps.
    Returns (params, emas, norms) with one norm per step."""
    params, grads = problem(misaligned)
    lr, (b1, b2), eps = HYPER["lr"], HYPER["betas"], HYPER["eps"]
    p = [x.double().clone() for x in params]
    m = [torch.zeros_like(x) for x in p]
    v = [torch.zeros_like(x) for x in p]
    e = [x.clone() for x in p]
    norms = []
    for t, gs in enumerate(grads, start=1):
        gs = [x.double() for x in gs]
        norm = torch.sqrt(sum((x * x).sum() for x in gs))
        norms.append(float(norm))
        scale = min(1.0, MAX_NORM / (float(norm) + 1e-6)) if clip else 1.0
        d = min(EMA_DECAY, (1 + t) / (10 + t)) if ema_warmup else EMA_DECAY
        for i, gi in enumerate(gs):
            gi = gi * scale
            m[i] = b1 * m[i] + (1 - b1) * gi
            v[i] = b2 * v[i] + (1 - b2) * gi * gi
            mhat = m[i] / (1 - b1 ** t)
            vhat = v[i] / (1 - b2 ** t)
            p[i] = p[i] - lr * mhat / (vhat.sqrt() + eps)
            if ema:
                e[i] = d * e[i] + (1 - d) * p[i]
    return p, e, norms


def run_optimizer(device, misaligned, clip, ema, ema_warmup=True):
    """FusedAdam over the shared problem; returns (opt, params, norms)."""
    p0, grads = problem(misaligned)
    params = [x.to(device).clone().requires_grad_(True) for x in p0]
    flat = None
    if misaligned:
        n = params[-1].numel()
        flat = torch.zeros(n + 8, device=device)
        params[-1].grad = flat[1:1 + n].view(params[-1].shape)
        assert params[-1].grad.data_ptr() % 16 == 4
    opt = FusedAdam(params, max_grad_norm=MAX_NORM if clip else None,
                    ema_decay=EMA_DECAY if ema else None,
                    ema_warmup=ema_warmup, **HYPER)
    norms = []
    for gs in grads:
        for i, (p, g) in enumerate(zip(params, gs)):
            if misaligned and i == len(params) - 1:
                p.grad.copy_(g)
            else:
                p.grad = g.to(device).clone()
        opt.step()
        if clip:
            norms.append(opt.last_grad_norm.clone())
    return opt, params, norms


def max_err(got, want):
    return max((a.detach().double().cpu() - b).abs().max().item()
               for a, b in zip(got, want))


def test_oracle_inputs_discriminate():
    """The figures that make the 1e-5 check meaningful: which steps clip,
    and how far a wrong clip / decay / warmup moves the result."""
    p, e, norms = oracle(False, True, True)
    clipped = [n > MAX_NORM for n in norms]
    assert clipped == [False, True, True, False, True, False], norms
    p_noclip, _, _ = oracle(False, False, True)
    _, e_nowarm, _ = oracle(False, True, True, False)
    assert max_err(p, p_noclip) > 1e-2
    assert max_err(e, p) > 1e-3
    assert max_err(e, e_nowarm) > 1e-2


@pytest.mark.parametrize("clip,ema", [(True, True), (True, False),
                                      (False, True)])
def test_eager_matches_float64_oracle(clip, ema):
    opt, params, norms = run_optimizer("cpu", False, clip, ema)
    p64, e64, n64 = oracle(False, clip, ema)
    err = max_err(params, p64)
    print(f"clip={clip} ema={ema}: param err {err:.3e}")
    assert err < TOL, err
    if ema:
        emas = [em for _, em in opt.ema_parameters()]
        assert len(emas) == len(params)
        err = max_err(emas, e64)
        print(f"clip={clip} ema={ema}: ema err {err:.3e}")
        assert err < TOL, err
    if clip:
        for got, want in zip(norms, n64):
            assert abs(float(got) - want) <= 2e-5 * want
        assert opt.skipped_steps == 0


def test_eager_no_ema_warmup_matches_oracle():
    opt, params, _ = run_optimizer("cpu", False, True, True, ema_warmup=False)
    _, e64, _ = oracle(False, True, True, False)
    err = max_err([em for _, em in opt.ema_parameters()], e64)
    assert err < TOL, err


def test_default_options_unchanged_vs_torch_adam():
    """All options unset: the eager branch is plain Adam, as before."""
    p0, grads = problem(False)
    opt, params, _ = run_optimizer("cpu", False, False, False)
    assert opt.last_grad_norm is None and opt.skipped_steps == 0
    assert list(opt.ema_parameters()) == []
    assert all("ema" not in st for st in opt.state.values())
    ref = [x.clone().requires_grad_(True) for x in p0]
    opt2 = torch.optim.Adam(ref, **HYPER)
    for gs in grads:
        for p, g in zip(ref, gs):
            p.grad = g.clone()
        opt2.step()
    for a, b in zip(params, ref):
        err = (a - b).abs().max().item()
        assert err < TOL, err


def _small_opt(**kw):
    torch.manual_seed(3)
    params = [torch.randn(5, 7).requires_grad_(True),
              torch.randn(11).requires_grad_(True)]
    opt = FusedAdam(params, lr=1e-2, max_grad_norm=1.0, ema_decay=0.9, **kw)
    return opt, params


def _set_grads(params, seed):
    g = torch.Generator().manual_seed(seed)
    for p in params:
        p.grad = torch.randn(p.shape, generator=g)


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_non_finite_step_is_skipped(bad):
    opt, params = _small_opt()
    _set_grads(params, 0)
    opt.step()
    before = [{k: v.clone() for k, v in opt.state[p].items()}
              for p in params]
    p_before = [p.detach().clone() for p in params]
    _set_grads(params, 1)
    params[1].grad[4] = bad
    opt.step()
    assert opt.skipped_steps == 1
    assert not torch.isfinite(opt.last_grad_norm)
    for p, pb, sb in zip(params, p_before, before):
        assert torch.equal(p, pb)
        for k in ("exp_avg", "exp_avg_sq", "ema"):
            assert torch.equal(opt.state[p][k], sb[k]), k
        # documented: the host step counter still advances
        assert float(opt.state[p]["step"]) == float(sb["step"]) + 1
    _set_grads(params, 2)
    opt.step()
    assert opt.skipped_steps == 1
    for p, pb, sb in zip(params, p_before, before):
        assert torch.isfinite(p).all() and not torch.equal(p, pb)
        assert not torch.equal(opt.state[p]["exp_avg"], sb["exp_avg"])
        assert not torch.equal(opt.state[p]["ema"], sb["ema"])


def test_divergent_step_counts_raise():
    opt, params = _small_opt()
    _set_grads(params, 0)
    params[1].grad = None
    opt.step()
    _set_grads(params, 1)
    with pytest.raises(RuntimeError, match="divergent"):
        opt.step()


def test_state_dict_roundtrip_keeps_ema():
    opt, params = _small_opt()
    for s in range(2):
        _set_grads(params, s)
        opt.step()
    sd = copy.deepcopy(opt.state_dict())
    assert all("ema" in st for st in sd["state"].values())

    opt2, params2 = _small_opt()
    opt2.load_state_dict(copy.deepcopy(sd))
    for (_, e1), (_, e2) in zip(opt.ema_parameters(), opt2.ema_parameters()):
        assert torch.equal(e1, e2)

    # a checkpoint written without EMA: initialised from the params, loudly
    for st in sd["state"].values():
        del st["ema"]
    opt3, params3 = _small_opt()
    opt3.load_state_dict(sd)
    assert list(opt3.ema_parameters()) == []
    old = [p.detach().clone() for p in params3]
    _set_grads(params3, 5)
    with pytest.warns(UserWarning, match="EMA initialised"):
        opt3.step()
    d = min(0.9, (1 + 3) / (10 + 3))  # third step of the loaded state
    for (p, e), po in zip(opt3.ema_parameters(), old):
        assert torch.allclose(e, d * po + (1 - d) * p.detach(), atol=1e-6)


# ---------------------------------------------------------------------------
# Trainer / checkpoint / CLI
# ---------------------------------------------------------------------------

def test_trainer_lr_warmup_and_resume(tmp_path):
    from test_trainer import make_trainer
    lr = 1e-3
    trainer = make_trainer(tmp_path, lr=lr, lr_warmup_steps=4)
    seen = []
    for k in range(6):
        trainer.step = k
        trainer.train_step()
        seen.append(trainer.opt.param_groups[0]["lr"])
    assert seen == pytest.approx([lr * f for f in (.25, .5, .75, 1, 1, 1)])
    # derived from the step, so a resumed trainer continues the ramp
    trainer2 = make_trainer(tmp_path, lr=lr, lr_warmup_steps=4)
    trainer2.step = 2
    trainer2.train_step()
    assert trainer2.opt.param_groups[0]["lr"] == pytest.approx(lr * .75)


def test_trainer_default_builds_what_it_built_before(tmp_path):
    from test_trainer import make_trainer
    trainer = make_trainer(tmp_path)
    assert type(trainer.opt) is torch.optim.Adam
    trainer.train_step()
    assert trainer.opt.param_groups[0]["lr"] == 1e-3


@pytest.fixture(scope="module")
def ema_run(tmp_path_factory):
    """Tiny CPU trainer with clip + EMA, 3 steps, one checkpoint."""
    from test_trainer import make_trainer
    tmp = tmp_path_factory.mktemp("ema_run")
    trainer = make_trainer(tmp, lr=3e-3, max_grad_norm=1.0, ema_decay=0.9)
    assert isinstance(trainer.opt, FusedAdam)
    for k in range(3):
        trainer.step = k
        loss = trainer.train_step()
    assert torch.isfinite(loss)
    trainer.step = 3
    path = ckpt.save_checkpoint(
        trainer.cfg.ckpt_folder, trainer.model, trainer.opt, trainer.step,
        extra={"model_cfg": vars(trainer.model_cfg), "img_sidelength": 16})
    return tmp, trainer, path


def test_ema_checkpoint_resume_and_load(ema_run, tmp_path):
    from test_trainer import make_trainer
    _, trainer, path = ema_run
    assert trainer.opt.skipped_steps == 0
    assert float(trainer.opt.last_grad_norm) > 0

    # resume: the EMA comes back through the optimizer state dict
    trainer2 = make_trainer(tmp_path, max_grad_norm=1.0, ema_decay=0.9)
    assert ckpt.load_checkpoint(path, trainer2.model, trainer2.opt) == 3
    pairs1 = list(trainer.opt.ema_parameters())
    pairs2 = list(trainer2.opt.ema_parameters())
    assert len(pairs1) == len(pairs2) == len(list(trainer.model.parameters()))
    for (p1, e1), (p2, e2) in zip(pairs1, pairs2):
        assert torch.equal(p1, p2) and torch.equal(e1, e2)
    trainer2.train_step()

    # use_ema: the model's params are the EMA, not the raw weights
    trainer3 = make_trainer(tmp_path)
    ckpt.load_checkpoint(path, trainer3.model, use_ema=True)
    differs = False
    for p3, (p1, e1) in zip(trainer3.model.parameters(), pairs1):
        assert torch.equal(p3, e1)
        differs |= not torch.equal(p3, p1)
    assert differs


def test_use_ema_on_ema_less_checkpoint_raises(tmp_path):
    from test_trainer import make_trainer
    trainer = make_trainer(tmp_path)
    trainer.train_step()
    path = ckpt.save_checkpoint(trainer.cfg.ckpt_folder, trainer.model,
                                trainer.opt, 1)
    with pytest.raises(KeyError, match="no EMA"):
        ckpt.load_checkpoint(path, trainer.model, use_ema=True)


def test_ema_state_dict_rejects_other_model(ema_run):
    from novel_view_synthesis_3d_amd.config import XUNetConfig
    from novel_view_synthesis_3d_amd.models.xunet import XUNet
    _, _, path = ema_run
    payload = torch.load(path, weights_only=False)
    other = XUNet(XUNetConfig(ch=16, ch_mult=(1, 2), emb_ch=8,
                              num_res_blocks=1, attn_resolutions=(8,),
                              dropout=0.0), 16)
    with pytest.raises(ValueError):
        ckpt.ema_state_dict(payload, other)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("flag,expect", [("--ema", "loaded EMA weights"),
                                         ("--no-ema", "loaded raw weights"),
                                         (None, "loaded EMA weights")])
def test_sample_cli_weight_choice(ema_run, tmp_path, flag, expect):
    _, _, path = ema_run
    cmd = [sys.executable, os.path.join(ROOT, "sample.py"),
           "--checkpoint", str(path), "--steps", "2", "--batch-size", "1",
           "--out", str(tmp_path / "samples"), "--no-graph"]
    if flag:
        cmd.append(flag)
    out = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert expect in out.stdout, out.stdout
    assert (list((tmp_path / "samples").glob("*.png"))
            + list((tmp_path / "samples").glob("*.npy")))


# ---------------------------------------------------------------------------
# Data parallel (gloo, world 2): identical clip factor and EMA on every rank
# ---------------------------------------------------------------------------

WORLD = 2
DP_STEPS = 3
# eps is chosen on purpose. With Adam's default 1e-8 the update
# lr*m/(sqrt(v)+eps) is invariant to a common gradient scale, so (a) a wrong
# clip factor would be invisible in the parameters, and (b) biases in front
# of a GroupNorm, whose true gradient is zero, carry only summation-order
# noise (~1e-9, sign differs between a sharded and a full batch) that Adam
# normalises to +-lr per step, for any optimizer. eps=1e-4 is the size of a
# clipped gradient element (0.05/sqrt(#params)), so the clip factor shows
# and 1e-9 of noise moves a parameter by at most lr*3*1e-9/eps = 3e-8.
DP_OPT = dict(lr=1e-3, eps=1e-4, max_grad_norm=0.05, ema_decay=0.9)


def _dp_step(model, engine, opt, batch, noise, mask):
    if engine is not None:
        engine.zero_flags()
    else:
        opt.zero_grad()
    out = model(batch, cond_mask=mask)
    torch.nn.functional.mse_loss(out, noise).backward()
    if engine is not None:
        engine.finish()
    opt.step()


def _dp_worker(rank, world, port, results_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["RANK"] = str(rank)
    os.environ["WORLD_SIZE"] = str(world)
    os.environ["LOCAL_RANK"] = str(rank)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from novel_view_synthesis_3d_amd.parallel.ddp import DataParallelEngine
        from test_ddp import _build_model, _full_batch
        model = _build_model(seed=100 + rank)
        engine = DataParallelEngine(model, bucket_mb=1.0)
        opt = FusedAdam(model.parameters(), **DP_OPT)
        batch, noise = _full_batch(B=4, H=16)
        sl = slice(rank * 2, rank * 2 + 2)
        shard = {k: v[sl] for k, v in batch.items()}
        for _ in range(DP_STEPS):
            _dp_step(model, engine, opt, shard, noise[sl], torch.ones(2))
        torch.save({"params": [p.detach() for p in model.parameters()],
                    "ema": [e for _, e in opt.ema_parameters()],
                    "norm": opt.last_grad_norm,
                    "skipped": opt.skipped_steps},
                   os.path.join(results_dir, f"recipe_rank{rank}.pt"))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_dp_clip_and_ema_identical_across_ranks(tmp_path):
    port = 29537
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_dp_worker,
                         args=(r, WORLD, port, str(tmp_path)))
             for r in range(WORLD)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(240)
        assert p.exitcode == 0, f"worker failed: {p.exitcode}"
    r0 = torch.load(tmp_path / "recipe_rank0.pt", weights_only=False)
    r1 = torch.load(tmp_path / "recipe_rank1.pt", weights_only=False)
    assert r0["skipped"] == r1["skipped"] == 0
    assert torch.equal(r0["norm"], r1["norm"])
    for key in ("params", "ema"):
        assert len(r0[key]) == len(r1[key]) > 0
        for a, b in zip(r0[key], r1[key]):
            assert torch.equal(a, b), key

    # single process on the concatenated batch
    from test_ddp import _build_model, _full_batch
    model = _build_model(seed=100)  # rank 0's init
    opt = FusedAdam(model.parameters(), **DP_OPT)
    batch, noise = _full_batch(B=4, H=16)
    for _ in range(DP_STEPS):
        _dp_step(model, None, opt, batch, noise, torch.ones(4))
    # the clip must be active for the test to mean anything
    assert float(opt.last_grad_norm) > DP_OPT["max_grad_norm"]
    ref = {"params": [p.detach() for p in model.parameters()],
           "ema": [e for _, e in opt.ema_parameters()]}
    # ... and the parameters must have moved far more than the tolerance
    moved = max((a - b).abs().max().item() for a, b in zip(
        ref["params"], _build_model(seed=100).parameters()))
    assert moved > 1e-3, moved
    for key in ("params", "ema"):
        err = max((a - b).abs().max().item()
                  for a, b in zip(r0[key], ref[key]))
        print(f"dp vs single {key}: {err:.3e}")
        assert err < 1e-5, (key, err)  # test_ddp.py's tolerance
