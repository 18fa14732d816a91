"""Stochastic-conditioning multi-view sampler (CPU, tiny model)."""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from novel_view_synthesis_3d_amd import ops
from novel_view_synthesis_3d_amd.config import XUNetConfig
from novel_view_synthesis_3d_amd.data.synthetic import (
    random_cameras, synthetic_batch,
)
from novel_view_synthesis_3d_amd.diffusion.sampler import (
    DDPMSampler, StochasticConditioningSampler,
)
from novel_view_synthesis_3d_amd.models.xunet import XUNet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tiny_model():
    torch.manual_seed(0)
    cfg = XUNetConfig(ch=8, ch_mult=(1, 2), emb_ch=8, num_res_blocks=1,
                      attn_resolutions=(8,), dropout=0.0)
    model = XUNet(cfg, img_sidelength=16)
    with torch.no_grad():  # nonzero head: the output depends on conditioning
        model.Conv_1.weight.normal_(0, 0.05)
    return model


def scene(B, N, seed=0):
    g = torch.Generator().manual_seed(seed)
    cond = synthetic_batch(B, 16, generator=g)
    cams = [random_cameras(B, 16, generator=g) for _ in range(N)]
    tR = torch.stack([c[0] for c in cams])
    tt = torch.stack([c[1] for c in cams])
    return cond, tR, tt


def run(sampler, cond, tR, tt, **kw):
    kw.setdefault("num_steps", 5)
    return sampler.sample_views(cond["x"], cond["R1"], cond["t1"], cond["K"],
                                tR, tt, **kw)


@pytest.mark.parametrize("k", [1, 2, 3, 7])  # 7 = Kcap of a 6-view run
def test_index_rule_exact(k):
    one_m = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
    u = torch.tensor([0.0, 0.4999, 0.5, one_m], dtype=torch.float32)
    want = [min(int(np.floor(np.float32(x) * np.float32(k))), k - 1)
            for x in u.numpy()]
    # closed form for these u: 0 -> 0; nextafter(1,0) -> k-1
    assert want[0] == 0 and want[3] == k - 1
    if k == 2:
        assert want == [0, 0, 1, 1]
    for kk in (k, torch.tensor([k])):
        got = ops.stochastic_index(u, kk)
        assert got.dtype == torch.long
        assert got.tolist() == want


def test_reduces_to_ddpm_sampler_with_one_view():
    model = tiny_model()
    cond, _, _ = scene(2, 1)
    cond.pop("x_target")
    z0 = torch.randn(2, 16, 16, 3, generator=torch.Generator().manual_seed(4))
    torch.manual_seed(5)
    want = DDPMSampler(model, num_steps=5).sample(cond, z_init=z0)
    torch.manual_seed(5)
    sampler = StochasticConditioningSampler(model)
    got = run(sampler, cond, cond["R2"][None], cond["t2"][None], z_init=z0,
              seed=1)
    assert got.shape == (1, 2, 16, 16, 3)
    assert torch.equal(got[0], want)


def test_bank_is_used():
    model = tiny_model()
    cond, tR, tt = scene(2, 3)
    sampler = StochasticConditioningSampler(model)
    z0 = torch.randn(3, 2, 16, 16, 3,
                     generator=torch.Generator().manual_seed(4))
    kw = dict(z_init=z0, seed=1, noise_scale=0.0, num_steps=6)

    base = run(sampler, cond, tR, tt, **kw)
    log = [i.clone() for i in sampler.index_log]
    assert len(log) == 3 and all(i.shape == (6, 2) for i in log)
    assert set(log[0].flatten().tolist()) == {0}
    assert set(log[1].flatten().tolist()) == {0, 1}   # both values occur
    assert set(log[2].flatten().tolist()) <= {0, 1, 2}
    assert 1 in log[2].flatten().tolist()  # view 3 does read entry 1

    def replace_entry_1(n, st):
        if n == 2:
            st["bank_img"][1].neg_()
            for f in st["cache"].src:
                f[1].mul_(-0.5)
    changed = run(sampler, cond, tR, tt, on_view_start=replace_entry_1, **kw)
    assert torch.equal(changed[:2], base[:2])
    assert not torch.equal(changed[2], base[2])

    def poison_beyond_k(n, st):
        k = int(st["k"])
        assert k == n + 1
        st["bank_img"][k:].fill_(float("nan"))
        for f in st["cache"].src:
            f[k:].fill_(float("nan"))
    same = run(sampler, cond, tR, tt, on_view_start=poison_beyond_k, **kw)
    assert torch.equal(same, base)


def test_shape_finite_reproducible_and_mode_restored():
    model = tiny_model()
    model.train()
    cond, tR, tt = scene(2, 2, seed=3)
    sampler = StochasticConditioningSampler(model)
    torch.manual_seed(11)
    a = run(sampler, cond, tR, tt, num_steps=4, seed=7)
    assert model.training
    torch.manual_seed(11)
    b = run(sampler, cond, tR, tt, num_steps=4, seed=7)
    assert a.shape == (2, 2, 16, 16, 3)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b)
    model.eval()
    run(sampler, cond, tR, tt, num_steps=4, seed=7)
    assert not model.training


def test_ring_bank_keeps_most_recent():
    model = tiny_model()
    cond, tR, tt = scene(1, 3)
    sampler = StochasticConditioningSampler(model, max_bank=2)
    out = run(sampler, cond, tR, tt, num_steps=4, seed=0)
    assert torch.isfinite(out).all()
    assert sampler.state["bank_img"].shape[0] == 2
    assert all(int(i.max()) <= 1 for i in sampler.index_log)
    # slot 0 was overwritten by the second generated view (ring)
    assert torch.equal(sampler.state["bank_img"][0], out[1].clamp(-1, 1))


def test_pose_cache_list_path_unchanged():
    """The bank features equal the per-frame slices of pose_features."""
    model = tiny_model().eval()
    cond, _, _ = scene(2, 1)
    cp = model.ConditioningProcessor_0
    full = cp.pose_features(cond, torch.tensor([1.0, 0.0]))
    for frame, (R, t) in enumerate(((cond["R1"], cond["t1"]),
                                    (cond["R2"], cond["t2"]))):
        feats, null = cp.frame_pose_features(R, t, cond["K"], frame, 16, 16)
        for lvl in range(len(full)):
            torch.testing.assert_close(feats[lvl][0], full[lvl][0, frame])
            torch.testing.assert_close(null[lvl][0], full[lvl][1, frame])


def test_cli_views(tmp_path):
    from novel_view_synthesis_3d_amd.engine import checkpoint as ckpt
    model = XUNet(XUNetConfig.named("tiny"), 16)
    path = ckpt.save_checkpoint(str(tmp_path / "ckpt"), model, None, 1)
    base = [sys.executable, os.path.join(ROOT, "sample.py"),
            "--checkpoint", path, "--model", "tiny", "--sidelength", "16",
            "--steps", "3", "--no-graph"]

    out = subprocess.run(base + ["--views", "2", "--out",
                                 str(tmp_path / "mv")],
                         cwd=str(tmp_path), capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    names = sorted(p.stem for p in (tmp_path / "mv").iterdir())
    assert names == ["view_000", "view_001"]

    out = subprocess.run(base + ["--out", str(tmp_path / "sv")],
                         cwd=str(tmp_path), capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    names = sorted(p.stem for p in (tmp_path / "sv").iterdir())
    assert names == ["sample_000"]
