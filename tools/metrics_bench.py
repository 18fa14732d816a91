#!/usr/bin/env python3
"""ops.image_metrics (image_metrics.hip: one metric launch + one finalize
launch) against the eager torch reference on the same GPU, fp32, at the two
evaluation batch shapes. The two are alternated in one process and timed
with device events after warmup. No pass/fail gate: sampling dominates an
evaluation run; the kernel exists to keep the metrics on the device in one
deterministic launch pair.

    python tools/metrics_bench.py --out profiles/image_metrics_bench.jsonl
"""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, ".")

from novel_view_synthesis_3d_amd import ops
from novel_view_synthesis_3d_amd.ops import reference as ref

SHAPES = [(64, 128, 128, 3), (64, 64, 64, 3)]


def timed(fn, iters):
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters  # ms per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="profiles/image_metrics_bench.jsonl")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "metrics_bench needs a GPU"

    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    for shape in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(0)
        target = torch.rand(shape, device="cuda", generator=g) * 2 - 1
        pred = (target + 0.1 * torch.randn(shape, device="cuda",
                                           generator=g)).clamp(-1, 1)
        fns = {"hip": lambda: ops.image_metrics(pred, target),
               "eager": lambda: ref.image_metrics(pred, target)}
        for fn in fns.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in fns}
        for _ in range(args.rounds):  # alternate inside every round
            for k, fn in fns.items():
                times[k].append(timed(fn, args.iters))
        ps, ss = fns["hip"]()
        pe, se = fns["eager"]()
        rec = {"bench": "image_metrics", "label": args.label,
               "shape": list(shape), "dtype": "fp32",
               "rounds": args.rounds, "iters": args.iters,
               "max_abs_ssim_diff": float((ss - se).abs().max()),
               "max_abs_psnr_diff_db": float((ps - pe).abs().max())}
        for k, ts in times.items():
            rec[f"{k}_ms_median"] = round(statistics.median(ts), 4)
            rec[f"{k}_ms_min"] = round(min(ts), 4)
            rec[f"{k}_ms_max"] = round(max(ts), 4)
            rec[f"{k}_window_s"] = round(sum(ts) * args.iters / 1e3, 3)
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
