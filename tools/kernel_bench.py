#!/usr/bin/env python3
"""Per-kernel microbenchmarks on MI355X: HIP kernels vs library/eager paths.

Run on a GPU box:  python tools/kernel_bench.py > gpurun_out/kernel_bench.json
"""

import json
import sys
import time

import torch

sys.path.insert(0, ".")


def timeit(fn, warmup=5, iters=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1000  # ms


def bench_conv():
    from novel_view_synthesis_3d_amd.ops import hip_ops
    from novel_view_synthesis_3d_amd.ops import reference as ref
    # (B,F,H,W,Cin,Cout) — the full-config hot shapes
    shapes = [
        (8, 2, 128, 128, 256, 256),
        (8, 2, 64, 64, 512, 512),
        (8, 2, 32, 32, 512, 512),
        (8, 2, 16, 16, 1024, 1024),
        (8, 2, 16, 16, 2048, 1024),  # up-path concat
    ]
    out = []
    for B, F, H, W, Ci, Co in shapes:
        x = torch.randn(B, F, H, W, Ci, device="cuda", dtype=torch.bfloat16)
        w = torch.randn(Co, 3, 3, Ci, device="cuda",
                        dtype=torch.bfloat16) * 0.02
        b = torch.randn(Co, device="cuda")
        flops = 2.0 * B * F * H * W * 9 * Ci * Co
        t_hip = timeit(
            lambda: torch.ops.nvs3d.conv3x3_fwd(x, w, b, None, 1.0))
        t_mio = timeit(lambda: ref.frame_conv3x3(x, w, b.to(torch.bfloat16)))
        rec = {"op": "conv3x3_fwd", "shape": [B, F, H, W, Ci, Co],
               "hip_ms": round(t_hip, 3), "miopen_ms": round(t_mio, 3),
               "hip_tflops": round(flops / t_hip / 1e9, 1),
               "miopen_tflops": round(flops / t_mio / 1e9, 1)}
        out.append(rec)
        print(json.dumps(rec), flush=True)
    return out


def bench_attn():
    from novel_view_synthesis_3d_amd.ops import reference as ref
    shapes = [
        (8, 1024, 4, 128),
        (8, 256, 4, 256),
        (16, 1024, 4, 128),
        (8, 1024, 4, 16),
    ]
    for B, L, h, d in shapes:
        q, k, v = (torch.randn(B, L, h, d, device="cuda",
                               dtype=torch.bfloat16) for _ in range(3))
        flops = 2.0 * B * h * L * L * d * 2
        t_hip = timeit(lambda: torch.ops.nvs3d.attn_fwd(q, k, v))
        t_ref = timeit(lambda: ref.attention(q, k, v))
        rec = {"op": "attn_fwd", "shape": [B, L, h, d],
               "hip_ms": round(t_hip, 3), "eager_ms": round(t_ref, 3),
               "hip_tflops": round(flops / t_hip / 1e9, 1),
               "eager_tflops": round(flops / t_ref / 1e9, 1)}
        print(json.dumps(rec), flush=True)


def bench_gn():
    from novel_view_synthesis_3d_amd.ops import hip_ops
    shapes = [(8, 2, 128, 128, 256), (8, 2, 64, 64, 512),
              (8, 2, 16, 16, 1024)]
    for B, F, H, W, C in shapes:
        x = torch.randn(B, F, H, W, C, device="cuda", dtype=torch.bfloat16)
        gm = torch.ones(C, device="cuda")
        bt = torch.zeros(C, device="cuda")
        fs = torch.randn_like(x) * 0.1
        ft = torch.randn_like(x) * 0.1
        nbytes = x.numel() * 2
        film = torch.cat([fs, ft], dim=-1).contiguous()
        t = timeit(lambda: torch.ops.nvs3d.gn_fwd(x, gm, bt, film, 32,
                                                  1e-6, True))
        # fwd traffic: read x twice + fs + ft + write y = 5 passes
        rec = {"op": "gn_fwd_film_silu", "shape": [B, F, H, W, C],
               "ms": round(t, 3),
               "eff_tb_s": round(5 * nbytes / t / 1e9, 2)}
        print(json.dumps(rec), flush=True)


def bench_pose():
    from novel_view_synthesis_3d_amd.ops import hip_ops
    from novel_view_synthesis_3d_amd.data.synthetic import random_cameras
    B, H = 8, 128
    g = torch.Generator(device="cuda").manual_seed(0)
    R1, t1, K = random_cameras(B, H, "cuda", g)
    R2, t2, _ = random_cameras(B, H, "cuda", g)
    R, t = torch.stack([R1, R2], 1), torch.stack([t1, t2], 1)
    m = torch.ones(B, device="cuda")
    tms = timeit(lambda: hip_ops.pose_embedding(R, t, K, m, H, H,
                                                torch.bfloat16))
    print(json.dumps({"op": "pose_embedding", "shape": [B, 2, H, H, 144],
                      "ms": round(tms, 3)}), flush=True)


def bench_conv_halo(out_path="profiles/conv_halo_bench.jsonl"):
    """Halo-tile conv against the route it replaces (im2col + hipBLASLt GEMM
    + eager tail) on the small config's shapes at batch 128: the two
    alternate in one process, three windows of >= 0.3 s each after warm-up.
    FLOPs and the HBM bytes the algorithm needs (x, w, y, residual once) are
    computed from the shapes; `bound` says which of the two peaks (2.5 PF/s
    bf16 dense, 8 TB/s) gives the larger least time."""
    import math
    from novel_view_synthesis_3d_amd.ops import hip_ops
    shapes = [(128, 2, 64, 64, 32, 32), (128, 2, 64, 64, 96, 32),
              (128, 2, 64, 64, 64, 32), (128, 2, 32, 32, 32, 64),
              (128, 2, 32, 32, 64, 64), (128, 2, 32, 32, 96, 64),
              (128, 2, 32, 32, 128, 64)]
    rs2 = 1.0 / math.sqrt(2.0)

    def window(fn, min_s=0.3):
        n, t0 = 0, time.perf_counter()
        while True:
            for _ in range(10):
                fn()
            n += 10
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if dt >= min_s:
                return dt / n * 1000  # ms

    with open(out_path, "w") as f, torch.no_grad():
        for B, F, H, W, Ci, Co in shapes:
            x = torch.randn(B, F, H, W, Ci, device="cuda",
                            dtype=torch.bfloat16)
            w = torch.randn(Co, 3, 3, Ci, device="cuda",
                            dtype=torch.bfloat16) * 0.05
            b = torch.randn(Co, device="cuda", dtype=torch.bfloat16)
            res = torch.randn(B, F, H, W, Co, device="cuda",
                              dtype=torch.bfloat16)
            px = B * F * H * W
            flops = 2.0 * px * 9 * Ci * Co
            for tail in (False, True):
                if tail:
                    new = lambda: torch.ops.nvs3d.conv3x3_halo_fwd(
                        x, w, b, res, rs2)
                    old = lambda: (hip_ops._gemm_conv_fwd(x, w, b, 1)
                                   + res) * rs2
                else:
                    new = lambda: torch.ops.nvs3d.conv3x3_halo_fwd(
                        x, w, b, None, 1.0)
                    old = lambda: hip_ops._gemm_conv_fwd(x, w, b, 1)
                nbytes = 2.0 * (px * (Ci + Co * (2 if tail else 1))
                                + 9 * Ci * Co)
                for fn in (new, old):
                    for _ in range(5):
                        fn()
                torch.cuda.synchronize()
                wins = {"halo": [], "route": []}
                for _ in range(3):
                    wins["halo"].append(round(window(new), 4))
                    wins["route"].append(round(window(old), 4))
                t = min(wins["halo"])
                rec = {"op": "conv3x3_halo_fwd",
                       "shape": [B, F, H, W, Ci, Co], "tail": tail,
                       "halo_ms": wins["halo"], "route_ms": wins["route"],
                       "speedup_min": round(min(wins["route"]) / t, 2),
                       "halo_tflops": round(flops / t / 1e9, 1),
                       "halo_tb_s": round(nbytes / t / 1e9, 2),
                       "bound": ("flops" if flops / 2.5e15 > nbytes / 8e12
                                 else "bytes")}
                f.write(json.dumps(rec) + "\n")
                print(json.dumps(rec), flush=True)


def bench_conv_wgrad_narrow(out_path="profiles/conv_wgrad_narrow_bench.jsonl"):
    """Narrow direct wgrad (the conv3x3_wgrad op) against the route it
    replaces (`_wgrad_im2col9`: 9-plane im2col + one hipBLASLt GEMM + the bias
    sum) on the small config's shapes at batch 128, with bias: the two
    alternate in one process, three windows of >= 0.3 s each after warm-up.
    TB/s counts x and dy once, TF/s 2*9*Cin*Cout per pixel, both over the
    kernel route's time."""
    from novel_view_synthesis_3d_amd.ops import hip_ops
    shapes = [(128, 2, 64, 64, 32, 32), (128, 2, 64, 64, 96, 32),
              (128, 2, 64, 64, 64, 32), (128, 2, 32, 32, 32, 64),
              (128, 2, 32, 32, 64, 64), (128, 2, 32, 32, 96, 64),
              (128, 2, 32, 32, 128, 64)]

    def window(fn, min_s=0.3):
        n, t0 = 0, time.perf_counter()
        while True:
            for _ in range(10):
                fn()
            n += 10
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if dt >= min_s:
                return dt / n * 1000  # ms

    with open(out_path, "w") as f, torch.no_grad():
        for B, F, H, W, Ci, Co in shapes:
            x = torch.randn(B, F, H, W, Ci, device="cuda",
                            dtype=torch.bfloat16)
            dy = torch.randn(B, F, H, W, Co, device="cuda",
                             dtype=torch.bfloat16)
            w = torch.empty(Co, 3, 3, Ci, device="cuda",
                            dtype=torch.bfloat16)
            px = B * F * H * W
            flops = 2.0 * px * 9 * Ci * Co
            nbytes = 2.0 * px * (Ci + Co)
            new = lambda: torch.ops.nvs3d.conv3x3_wgrad(x, dy, True)
            old = lambda: hip_ops._wgrad_im2col9(x, w, dy, True, 1)
            for fn in (new, old):
                for _ in range(5):
                    fn()
            torch.cuda.synchronize()
            dw_n, dw_o = new()[0], old()[0].float()
            rel = ((dw_n - dw_o).norm() / dw_n.norm()).item()
            wins = {"narrow": [], "route": []}
            for _ in range(3):
                wins["narrow"].append(round(window(new), 4))
                wins["route"].append(round(window(old), 4))
            t = min(wins["narrow"])
            rec = {"op": "conv3x3_wgrad_narrow",
                   "shape": [B, F, H, W, Ci, Co],
                   "narrow_ms": wins["narrow"], "route_ms": wins["route"],
                   "speedup_min": round(min(wins["route"]) / t, 2),
                   "narrow_tb_s": round(nbytes / t / 1e9, 2),
                   "narrow_tflops": round(flops / t / 1e9, 1),
                   "rel_l2_vs_route": float(f"{rel:.3e}")}
            f.write(json.dumps(rec) + "\n")
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available()
    if "--conv-halo" in sys.argv:
        bench_conv_halo()
        sys.exit(0)
    if "--conv-wgrad-narrow" in sys.argv:
        bench_conv_wgrad_narrow()
        sys.exit(0)
    bench_conv()
    bench_attn()
    bench_gn()
    bench_pose()
