#!/usr/bin/env python3
"""Flagship training benchmark — BASELINE.json north-star metric:
train images/sec (whole node), X-UNet 128x128 SRN-shaped synthetic data.

Contract (driver): `python bench.py --gpus N --steps K --warmup W`; for N>1
launched via torch.distributed.run with one rank per GPU. W untimed warmup
steps, then exactly K timed steps bracketed by barrier+synchronize on both
sides; elapsed is the MAX over ranks; rank 0 prints ONE JSON line.

The timed step is the COMPLETE training step: on-device synthetic batch
generation + forward noising, bf16 forward, loss, backward, bucketed RCCL
gradient all-reduce, fp32 Adam update.

A plain run does only what the headline figure needs: set up, warm up, time
the K steps, print the result line. `--dump-outputs DIR` additionally writes
what the last timed step computed as DIR/<name>.npy (float32), so two builds
can be compared output for output: seeds are fixed, so the same arguments
give the same inputs on every run. `--full` is the switch for any extra
measurement (baselines, other precisions or sizes, per-kernel figures); this
benchmark has none today, so it adds nothing to the run yet.
"""

import argparse
import json
import os
import shutil
import tempfile
import time

import numpy as np
import torch

from novel_view_synthesis_3d_amd.config import TrainConfig, XUNetConfig
from novel_view_synthesis_3d_amd.engine.trainer import Trainer

# --dump-outputs budget, in float32 elements: the denoiser output (4.7M at
# the default batch 96 x 128 x 128 x 3) is written whole up to 6M; parameters
# and gradients (336M each at the full config) as a fixed seeded sample of 4M
# each. (6 + 4 + 4)M x 4 bytes = 56 MiB at the most.
_DUMP_OUT_ELEMS = 6 * 1024 * 1024
_DUMP_SAMPLE_ELEMS = 4 * 1024 * 1024
_DUMP_SEED = 20240607


def _dump_array(t: torch.Tensor, max_elems: int) -> np.ndarray:
    """float32 host copy of `t`: whole if it fits the budget, otherwise the
    elements at a fixed, seeded, sorted set of flat indices."""
    t = t.detach().to(torch.float32)
    n = t.numel()
    if n <= max_elems:
        return t.cpu().numpy()
    idx = np.sort(np.random.default_rng(_DUMP_SEED).integers(
        0, n, size=max_elems))
    idx = torch.from_numpy(idx).to(t.device)
    return t.reshape(-1).index_select(0, idx).cpu().numpy()


def dump_outputs(out_dir: str, trainer: Trainer, loss: torch.Tensor,
                 model_out: torch.Tensor) -> None:
    """What the last timed train_step() left its caller: the returned loss,
    the denoiser output that loss was computed from, and the gradients and
    updated parameters the step left on the model."""
    os.makedirs(out_dir, exist_ok=True)
    with_grad = [p for p in trainer.model.parameters() if p.grad is not None]
    arrays = {
        "loss": _dump_array(loss, 1),
        "model_out": _dump_array(model_out, _DUMP_OUT_ELEMS),
        "params": _dump_array(torch.cat(
            [p.detach().reshape(-1).to(torch.float32)
             for p in trainer.model.parameters()]), _DUMP_SAMPLE_ELEMS),
        "grads": _dump_array(torch.cat(
            [p.grad.reshape(-1).to(torch.float32) for p in with_grad]),
            _DUMP_SAMPLE_ELEMS),
    }
    for name, arr in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), arr)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=96,
                    help="per-GPU batch size (weak scaling)")
    ap.add_argument("--model", default="full")
    ap.add_argument("--sidelength", type=int, default=128)
    ap.add_argument("--amp", default="bf16", choices=["bf16", "off"])
    ap.add_argument("--graph", default="off", choices=["on", "off"],
                    help="hipGraph-capture the train step (single-node)")
    ap.add_argument("--bucket-mb", type=float, default=40.0,
                    help="DDP gradient bucket size (xGMI sweep hook: "
                         "try 25/40/80)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one "
                         "computed as DIR/<name>.npy")
    ap.add_argument("--full", action="store_true",
                    help="also run the extended measurements (none today)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    n_gpus = world if world > 1 else args.gpus

    use_cuda = torch.cuda.is_available()
    model_cfg = XUNetConfig.named(args.model)
    train_cfg = TrainConfig()
    train_cfg.data = "synthetic"
    train_cfg.amp = args.amp
    train_cfg.seed = 1234
    train_cfg.use_graph = (args.graph == "on" and use_cuda)
    train_cfg.bucket_mb = args.bucket_mb

    # a private scratch folder: a fixed name under the temp dir fails with
    # PermissionError once another user has run the benchmark on the machine
    results_folder = tempfile.mkdtemp(prefix="nvs3d_bench_")
    trainer = Trainer(None,
                      train_batch_size=args.batch,
                      img_sidelength=args.sidelength,
                      train_num_steps=10 ** 9,
                      model_cfg=model_cfg,
                      train_cfg=train_cfg,
                      results_folder=results_folder)

    last_out = {}
    if args.dump_outputs and rank == 0:
        # keep a handle on the denoiser output of the most recent step (under
        # --graph on this is the captured static buffer, refreshed by replay)
        trainer.model.register_forward_hook(
            lambda mod, inp, out: last_out.__setitem__("out", out.detach()))

    def barrier_sync():
        if trainer.ddp.enabled:
            torch.distributed.barrier()
        if use_cuda:
            torch.cuda.synchronize()

    for _ in range(args.warmup):
        trainer.train_step()
    barrier_sync()

    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = trainer.train_step()
    barrier_sync()
    elapsed = time.perf_counter() - t0
    elapsed = trainer.ddp.max_scalar(elapsed)  # MAX over ranks

    if rank == 0:
        global_batch = args.batch * n_gpus
        images_per_sec = global_batch * args.steps / elapsed
        result = {
            "metric": "train images/sec (whole node), X-UNet 128x128 SRN",
            "value": round(images_per_sec, 2),
            "unit": "images/sec",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1000, 2),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,  # reference publishes no numbers
            "dtype": "bf16" if (args.amp == "bf16" and use_cuda) else "fp32",
            "data": "synthetic",
            "config": {
                "model": f"X-UNet {args.model} ch={model_cfg.ch} "
                         f"ch_mult={list(model_cfg.ch_mult)}",
                "img_sidelength": args.sidelength,
                "global_batch": global_batch,
                "per_gpu_batch": args.batch,
                "parallelism": f"dp{n_gpus}",
                "bucket_mb": args.bucket_mb,
                "final_loss": float(loss.item()),
                "params": trainer.model.num_params(),
                "graph": getattr(trainer, "graph_active", False),
                "peak_mem_gb": round(
                    torch.cuda.max_memory_allocated() / 1e9, 2)
                if use_cuda else None,
            },
        }
        if args.dump_outputs:  # after the figures above: it allocates
            dump_outputs(args.dump_outputs, trainer, loss, last_out["out"])
        print(json.dumps(result), flush=True)

    if trainer.ddp.enabled:
        torch.distributed.destroy_process_group()
    shutil.rmtree(results_folder, ignore_errors=True)


if __name__ == "__main__":
    main()
