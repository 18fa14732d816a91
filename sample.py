#!/usr/bin/env python3
"""Sampling entry point — replaces the reference's import-time script
(/root/reference/sampling.py: hardcoded dirs, blocking cv2.imshow — D10).

    python sample.py --checkpoint checkpoints/model_00001000.pt \
        --folder cars_train_val --steps 256 --guidance 3 --out results/

Multi-view (stochastic conditioning, 3DiM §2.2): N views of one object from
its first observation, each step conditioned on a random earlier view.

    python sample.py --checkpoint ... --folder cars_train_val --views 8

Few-step solvers (diffusion/solvers.py): --solver ddim [--eta E] or
--solver dpmpp2m, best with --spacing logsnr; both are deterministic in the
initial latent at eta 0.

    python sample.py --checkpoint ... --solver dpmpp2m --spacing logsnr \
        --steps 32

Checkpoints trained with --ema-decay carry an EMA copy of the weights; it is
used by default (--no-ema samples from the raw weights).
"""

import argparse
import os

import numpy as np
import torch

from novel_view_synthesis_3d_amd.config import XUNetConfig
from novel_view_synthesis_3d_amd.data.srn import (
    SceneClassDataset, SceneInstanceDataset,
)
from novel_view_synthesis_3d_amd.data.synthetic import (
    random_cameras, synthetic_batch,
)
from novel_view_synthesis_3d_amd.diffusion.sampler import (
    DDPMSampler, StochasticConditioningSampler,
)
from novel_view_synthesis_3d_amd.diffusion.solvers import (
    add_solver_args, check_solver_cli,
)
from novel_view_synthesis_3d_amd.engine import checkpoint as ckpt
from novel_view_synthesis_3d_amd.models.xunet import XUNet


def _save(img_u8: np.ndarray, path: str) -> None:
    try:
        from PIL import Image
        Image.fromarray(img_u8).save(path)
    except ImportError:
        np.save(path.replace(".png", ".npy"), img_u8)
    print(f"wrote {path}")


def sample_views(args, model, device) -> None:
    """--views N: one object, N target views, stochastic conditioning."""
    from glob import glob
    from novel_view_synthesis_3d_amd.engine.metrics import psnr
    N, H = args.views, args.sidelength
    gt = None
    if args.folder and os.path.isdir(args.folder):
        inst_dirs = sorted(glob(os.path.join(args.folder, "*/")))
        if not inst_dirs:
            raise FileNotFoundError(f"no instances under {args.folder!r}")
        inst = SceneInstanceDataset(0, inst_dirs[0], img_sidelength=H)
        if len(inst) < N + 1:
            raise ValueError(f"--views {N} needs {N + 1} observations, "
                             f"{inst_dirs[0]} has {len(inst)}")
        obs = [inst[i] for i in range(N + 1)]
        x0, R0, t0, K = (obs[0][k][None].to(device)
                         for k in ("x", "R1", "t1", "K"))
        tR = torch.stack([o["R1"] for o in obs[1:]])[:, None].to(device)
        tt = torch.stack([o["t1"] for o in obs[1:]])[:, None].to(device)
        gt = torch.stack([o["x"] for o in obs[1:]])[:, None]
    else:
        g = torch.Generator(device=device).manual_seed(args.seed)
        x0 = torch.rand(1, H, H, 3, device=device, generator=g) * 2 - 1
        R0, t0, K = random_cameras(1, H, device, g)
        cams = [random_cameras(1, H, device, g) for _ in range(N)]
        tR = torch.stack([c[0] for c in cams])
        tt = torch.stack([c[1] for c in cams])

    sampler = StochasticConditioningSampler(model, max_bank=args.max_bank)
    torch.manual_seed(args.seed)
    out = sampler.sample_views(
        x0, R0, t0, K, tR, tt, num_steps=args.steps,
        guidance_weight=args.guidance, clip_denoised=True, seed=args.seed,
        use_graph=(device == "cuda" and not args.no_graph),
        stochastic=args.stochastic_cond, solver=args.solver,
        spacing=args.spacing, eta=args.eta)

    os.makedirs(args.out, exist_ok=True)
    out = out.clamp(-1, 1).cpu()
    img = ((out * 0.5 + 0.5) * 255).to(torch.uint8).numpy()
    for n in range(N):
        _save(img[n, 0], os.path.join(args.out, f"view_{n:03d}.png"))
        if gt is not None:
            print(f"view {n:03d} PSNR {psnr(out[n], gt[n]):.2f} dB")


def main() -> None:
    ap = argparse.ArgumentParser(description="3DiM DDPM+CFG sampler (MI355X)")
    ap.add_argument("--checkpoint", required=True)
    ap.add_argument("--folder", default=None,
                    help="SRN dataset root for conditioning views; synthetic "
                         "conditioning if omitted")
    ap.add_argument("--model", default=None,
                    help="model config name; default: read from checkpoint")
    ap.add_argument("--sidelength", type=int, default=None,
                    help="image sidelength; default: read from checkpoint")
    ap.add_argument("--batch-size", type=int, default=1)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--guidance", type=float, default=3.0)
    add_solver_args(ap)
    ap.add_argument("--out", default="./results")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--views", type=int, default=None,
                    help="generate N views of one object with stochastic "
                         "conditioning (writes view_###.png)")
    ap.add_argument("--stochastic-cond", default=True,
                    action=argparse.BooleanOptionalAction,
                    help="with --views: condition each step on a random "
                         "earlier view (off: always the input view)")
    ap.add_argument("--max-bank", type=int, default=None,
                    help="with --views: keep only the M most recent views "
                         "in the conditioning bank")
    ap.add_argument("--ema", default=None,
                    action=argparse.BooleanOptionalAction,
                    help="sample from the EMA weights (default: use them "
                         "when the checkpoint carries them)")
    args = ap.parse_args()
    check_solver_cli(ap, args)

    device = "cuda" if torch.cuda.is_available() else "cpu"
    # the checkpoint's extra payload records the model config and sidelength;
    # CLI flags override, and are required only for configless checkpoints
    payload = torch.load(args.checkpoint, map_location=device,
                         weights_only=False)
    extra = payload.get("extra", {}) if isinstance(payload, dict) else {}
    if args.model is not None:
        model_cfg = XUNetConfig.named(args.model)
    elif extra.get("model_cfg"):
        model_cfg = XUNetConfig(**extra["model_cfg"])
    else:
        model_cfg = XUNetConfig.named("small")
    sidelength = (args.sidelength if args.sidelength is not None
                  else int(extra.get("img_sidelength", 64)))
    args.sidelength = sidelength
    model = XUNet(model_cfg, sidelength).to(device)
    use_ema = ckpt.has_ema(payload) if args.ema is None else args.ema
    ckpt.load_checkpoint(args.checkpoint, model, use_ema=use_ema,
                         payload=payload)
    print(f"loaded {'EMA' if use_ema else 'raw'} weights from "
          f"{args.checkpoint}")
    model.eval()

    if args.views is not None:
        sample_views(args, model, device)
        return

    if args.folder and os.path.isdir(args.folder):
        ds = SceneClassDataset(root_dir=args.folder, max_num_instances=-1,
                               max_observations_per_instance=50,
                               img_sidelength=args.sidelength,
                               samples_per_instance=1)
        dl = torch.utils.data.DataLoader(ds, batch_size=args.batch_size,
                                         shuffle=True, drop_last=True,
                                         collate_fn=ds.collate_fn)
        raw, _ = next(iter(dl))
        cond = {k: v.to(device) for k, v in raw.items()
                if k in ("x", "R1", "t1", "R2", "t2", "K")}
    else:
        g = torch.Generator(device=device).manual_seed(args.seed)
        cond = synthetic_batch(args.batch_size, args.sidelength, device, g)
        cond.pop("x_target")

    sampler = DDPMSampler(model, num_steps=args.steps,
                          guidance_weight=args.guidance,
                          use_graph=(device == "cuda" and not args.no_graph),
                          solver=args.solver, spacing=args.spacing,
                          eta=args.eta)
    out = sampler.sample(cond)

    os.makedirs(args.out, exist_ok=True)
    img = ((out.clamp(-1, 1) * 0.5 + 0.5) * 255).to(torch.uint8).cpu().numpy()
    for i in range(img.shape[0]):
        path = os.path.join(args.out, f"sample_{i:03d}.png")
        try:
            from PIL import Image
            Image.fromarray(img[i]).save(path)
        except ImportError:
            np.save(path.replace(".png", ".npy"), img[i])
        print(f"wrote {path}")


if __name__ == "__main__":
    main()
