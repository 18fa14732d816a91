#!/usr/bin/env python3
"""Evaluate a checkpoint on a test set: PSNR / SSIM of generated views.

SRN single-view protocol (PixelNeRF, 3DiM): per object one input view, every
other view (or --num-targets evenly spaced ones) is generated and compared
with the ground truth.

    python evaluate.py --checkpoint checkpoints/model_00100000.pt \
        --folder cars_test --steps 256 --input-view 64 --num-targets 16 \
        --batch-objects 4 --out results/eval

Few-step solvers: --solver {ddpm,ddim,dpmpp2m} --spacing {uniform,logsnr}
[--eta E], e.g. --solver dpmpp2m --spacing logsnr --steps 32.

Writes OUT/metrics.json (aggregate, per-instance values, settings) and prints
one summary line. Model config, sidelength and EMA weights come from the
checkpoint as in sample.py.
"""

import argparse
import json
import os

import torch

from novel_view_synthesis_3d_amd.config import XUNetConfig
from novel_view_synthesis_3d_amd.diffusion.solvers import (
    add_solver_args, check_solver_cli,
)
from novel_view_synthesis_3d_amd.engine import checkpoint as ckpt
from novel_view_synthesis_3d_amd.engine.evaluate import (
    MODES, Evaluator, to_serialisable,
)
from novel_view_synthesis_3d_amd.models.xunet import XUNet


def main() -> None:
    ap = argparse.ArgumentParser(
        description="3DiM test-set evaluation: PSNR / SSIM (MI355X)")
    ap.add_argument("--checkpoint", required=True)
    ap.add_argument("--folder", required=True,
                    help="SRN dataset root (one sub-directory per object)")
    ap.add_argument("--model", default=None,
                    help="model config name; default: read from checkpoint")
    ap.add_argument("--sidelength", type=int, default=None,
                    help="image sidelength; default: read from checkpoint")
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--guidance", type=float, default=3.0)
    add_solver_args(ap)
    ap.add_argument("--input-view", type=int, default=64,
                    help="index of the conditioning observation")
    ap.add_argument("--num-targets", type=int, default=None,
                    help="evaluate this many evenly spaced other views "
                         "(default: all of them)")
    ap.add_argument("--max-instances", type=int, default=-1)
    ap.add_argument("--batch-objects", type=int, default=1,
                    help="objects sampled together in one batch")
    ap.add_argument("--mode", choices=MODES, default="autoregressive",
                    help="autoregressive: stochastic conditioning on the "
                         "views generated so far; independent: always the "
                         "input view")
    ap.add_argument("--max-bank", type=int, default=None,
                    help="keep only the M most recent views in the "
                         "conditioning bank")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--quantize", action="store_true",
                    help="evaluate the 8-bit values written to PNG")
    ap.add_argument("--save-images", action="store_true",
                    help="write the generated views under OUT/images/")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--ema", default=None,
                    action=argparse.BooleanOptionalAction,
                    help="evaluate the EMA weights (default: use them when "
                         "the checkpoint carries them)")
    ap.add_argument("--out", default="./results/eval")
    args = ap.parse_args()
    check_solver_cli(ap, args)

    device = "cuda" if torch.cuda.is_available() else "cpu"
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
    model = XUNet(model_cfg, sidelength).to(device)
    use_ema = ckpt.has_ema(payload) if args.ema is None else args.ema
    ckpt.load_checkpoint(args.checkpoint, model, use_ema=use_ema,
                         payload=payload)
    print(f"loaded {'EMA' if use_ema else 'raw'} weights from "
          f"{args.checkpoint}")
    model.eval()

    ev = Evaluator(model, num_steps=args.steps,
                   guidance_weight=args.guidance, mode=args.mode,
                   max_bank=args.max_bank,
                   use_graph=(device == "cuda" and not args.no_graph),
                   batch_objects=args.batch_objects, seed=args.seed,
                   quantize=args.quantize, solver=args.solver,
                   spacing=args.spacing, eta=args.eta)
    os.makedirs(args.out, exist_ok=True)
    result = ev.evaluate(
        args.folder, sidelength, input_view=args.input_view,
        num_targets=args.num_targets, max_instances=args.max_instances,
        save_images_dir=(os.path.join(args.out, "images")
                         if args.save_images else None))
    data = to_serialisable(result)
    data["settings"].update(checkpoint=args.checkpoint, ema=bool(use_ema))
    path = os.path.join(args.out, "metrics.json")
    with open(path, "w") as f:
        json.dump(data, f, indent=2)
    psnr = "inf" if data["psnr"] is None else f"{data['psnr']:.3f}"
    print(f"eval: PSNR {psnr} dB  SSIM {data['ssim']:.4f}  "
          f"({data['n_instances']} instances, {data['n_views']} views) "
          f"-> {path}")


if __name__ == "__main__":
    main()
