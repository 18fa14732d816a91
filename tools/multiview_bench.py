#!/usr/bin/env python3
"""Multi-view sampling benchmark: the stochastic-conditioning sampler on the
model/batch/steps of tools/sample_bench.py (full 128x128, CFG w=3, hipGraph
step), N views per object. Prints one JSON line.

    python tools/multiview_bench.py --steps 256 --batch 64 --views 2
    python tools/multiview_bench.py --steps 32 --batch 64 --views 2 \
        --solver dpmpp2m --spacing logsnr --repeats 3

Reports ms/step and s/view (the median of --repeats timed passes, every pass
listed in ms_per_step_all).
"""

import argparse
import json
import sys
import time

import torch

sys.path.insert(0, ".")

from novel_view_synthesis_3d_amd.config import XUNetConfig
from novel_view_synthesis_3d_amd.data.synthetic import (
    random_cameras, synthetic_batch,
)
from novel_view_synthesis_3d_amd.diffusion.sampler import (
    StochasticConditioningSampler,
)
from novel_view_synthesis_3d_amd.diffusion.solvers import (
    add_solver_args, check_solver_cli,
)
from novel_view_synthesis_3d_amd.models.xunet import XUNet


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="full")
    ap.add_argument("--sidelength", type=int, default=128)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--views", type=int, default=2)
    ap.add_argument("--max-bank", type=int, default=None)
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--repeats", type=int, default=1,
                    help="timed passes after the warm-up pass")
    add_solver_args(ap)
    args = ap.parse_args()
    check_solver_cli(ap, args)
    assert torch.cuda.is_available()

    torch.manual_seed(0)
    model = XUNet(XUNetConfig.named(args.model), args.sidelength).cuda()
    model.eval()
    g = torch.Generator(device="cuda").manual_seed(0)
    cond = synthetic_batch(args.batch, args.sidelength, "cuda", g)
    cams = [random_cameras(args.batch, args.sidelength, "cuda", g)
            for _ in range(args.views)]
    tR = torch.stack([c[0] for c in cams])
    tt = torch.stack([c[1] for c in cams])

    sampler = StochasticConditioningSampler(model, max_bank=args.max_bank)

    def run():
        return sampler.sample_views(
            cond["x"], cond["R1"], cond["t1"], cond["K"], tR, tt,
            num_steps=args.steps, guidance_weight=3.0, clip_denoised=True,
            seed=0, use_graph=not args.no_graph, solver=args.solver,
            spacing=args.spacing, eta=args.eta)

    # warmup pass (library autotuning, allocator); each call captures its
    # own graph, so the timed pass includes one capture like sample_bench's
    out = run()
    torch.cuda.synchronize()
    times = []
    for _ in range(max(1, args.repeats)):
        t0 = time.perf_counter()
        out = run()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    dt = sorted(times)[len(times) // 2]
    assert torch.isfinite(out).all()
    total_steps = args.steps * args.views
    print(json.dumps({
        "metric": "stochastic-conditioning multi-view sampling (1 GPU)",
        "ms_per_step": round(dt / total_steps * 1000, 2),
        "ms_per_step_all": [round(t / total_steps * 1000, 2) for t in times],
        "sec_per_view": round(dt / args.views, 3),
        "views_per_sec": round(args.batch * args.views / dt, 3),
        "sec_total": round(dt, 2),
        "solver": args.solver, "spacing": args.spacing, "eta": args.eta,
        "batch": args.batch, "steps": args.steps, "views": args.views,
        "graph": not args.no_graph, "graph_captures": sampler.num_captures,
        "model": args.model, "sidelength": args.sidelength,
        "peak_mem_gb": round(torch.cuda.max_memory_allocated() / 1e9, 2),
    }), flush=True)


if __name__ == "__main__":
    main()
