#!/usr/bin/env python3
"""Real-data (SRN PNG pipeline) GPU evidence, closing two round-1 gaps:

1. full-config 128x128 training throughput on PNG data through the real
   DataLoader (does the input pipeline keep up with the synthetic rate?)
2. a small model overfit on a tiny SRN set, then (a) full DDPM+CFG samples
   and (b) the reference's own acceptance bar (README.md:49): denoise a
   noised training view — images written to gpurun_out/.

Run on a GPU box:  python tools/srn_gpu_evidence.py
"""

import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")

OUT = "gpurun_out"


def gen_dataset(path, instances, views, size, seed=0):
    if os.path.isdir(path):
        return
    import subprocess
    subprocess.run([sys.executable, "tools/make_synth_srn.py", path,
                    "--instances", str(instances), "--views", str(views),
                    "--size", str(size), "--seed", str(seed)], check=True)


def throughput_srn():
    from novel_view_synthesis_3d_amd.config import TrainConfig, XUNetConfig
    from novel_view_synthesis_3d_amd.engine.trainer import Trainer

    ds = "/tmp/srn128"
    t0 = time.time()
    gen_dataset(ds, instances=24, views=24, size=128)
    print(f"[srn-throughput] dataset gen {time.time()-t0:.1f}s", flush=True)
    tcfg = TrainConfig()
    tcfg.data = "srn"
    tcfg.num_workers = 8
    tcfg.log_every = 1000
    tr = Trainer(folder=ds, train_batch_size=16, img_sidelength=128,
                 train_num_steps=10 ** 6, model_cfg=XUNetConfig.full(),
                 train_cfg=tcfg)
    # warmup 3, time 10
    for _ in range(3):
        tr.train_step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 10
    for _ in range(n):
        loss = tr.train_step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    rec = {"evidence": "srn_png_training_throughput",
           "config": "full 128x128 b16, PNG data via DataLoader(8 workers)",
           "images_per_sec": round(16 * n / dt, 2),
           "ms_per_step": round(dt / n * 1e3, 2),
           "final_loss": float(loss.item())}
    print(json.dumps(rec), flush=True)
    with open(os.path.join(OUT, "srn_throughput.json"), "w") as f:
        json.dump(rec, f)
    del tr
    torch.cuda.empty_cache()


def overfit_and_sample():
    from novel_view_synthesis_3d_amd.config import TrainConfig, XUNetConfig
    from novel_view_synthesis_3d_amd.data.srn import SceneClassDataset
    from novel_view_synthesis_3d_amd.diffusion.sampler import (
        DDPMSampler, solver_state,
    )
    from novel_view_synthesis_3d_amd.engine.trainer import Trainer
    from PIL import Image

    ds = "/tmp/srn64tiny"
    gen_dataset(ds, instances=4, views=32, size=64, seed=5)
    tcfg = TrainConfig()
    tcfg.data = "srn"
    tcfg.num_workers = 4
    tcfg.log_every = 200
    tcfg.save_every = 10 ** 6
    tcfg.ckpt_folder = "/tmp/ckpt_small"
    mcfg = XUNetConfig.small()
    steps = int(os.environ.get("NVS3D_EVIDENCE_STEPS", "1500"))
    tr = Trainer(folder=ds, train_batch_size=32, img_sidelength=64,
                 train_num_steps=steps, model_cfg=mcfg, train_cfg=tcfg)
    t0 = time.time()
    tr._train_loop()
    print(f"[overfit] {steps} steps in {time.time()-t0:.1f}s", flush=True)
    model = tr.model
    model.eval()

    scene = SceneClassDataset(ds, img_sidelength=64, samples_per_instance=1)
    dl = torch.utils.data.DataLoader(scene, batch_size=4, shuffle=False,
                                     collate_fn=scene.collate_fn)
    raw, _ = next(iter(dl))
    cond = {k: v.cuda() for k, v in raw.items()
            if k in ("x", "R1", "t1", "R2", "t2", "K")}

    def save_grid(t, name):
        img = ((t.clamp(-1, 1) * 0.5 + 0.5) * 255).to(torch.uint8)
        img = img.cpu().numpy()
        row = np.concatenate(list(img), axis=1)
        Image.fromarray(row).save(os.path.join(OUT, name))
        print(f"[sample] wrote {name}", flush=True)

    save_grid(cond["x"], "evidence_cond_views.png")

    # (a) full generation from noise, 256-step subsequence, CFG w=3
    sampler = DDPMSampler(model, num_steps=256, guidance_weight=3.0,
                          use_graph=True)
    out = sampler.sample(cond)
    save_grid(out, "evidence_samples_256step.png")

    # (b) the reference's acceptance bar: denoise a noised target view.
    # Noise gt views to t=350 and run the tail of the reverse process by
    # initializing z at that level (subsequence matching t range).
    from novel_view_synthesis_3d_amd.diffusion.forward import q_sample
    from novel_view_synthesis_3d_amd.diffusion.schedules import DiffusionSchedule
    gt = raw["x_target"].cuda()
    save_grid(gt, "evidence_gt_views.png")
    sched = DiffusionSchedule(1000)
    t_noise = 350
    tvec = torch.full((gt.shape[0],), t_noise, dtype=torch.long,
                      device="cuda")
    z, _, _ = q_sample(gt, tvec, sched)
    save_grid(z, "evidence_noised_t350.png")
    # reverse from t=350: the LAST 350 entries of the full 1000-step table
    # (indices 650..999 = t 349..0); no guidance (w=0)
    sam2 = DDPMSampler(model, num_steps=1000, guidance_weight=0.0,
                       use_graph=False)
    sst = solver_state(z, sched, 1000)
    sst["tab"] = {k: v[1000 - t_noise:] for k, v in sst["tab"].items()}
    cond2, mask = sam2._make_cond2(cond)
    idx = torch.zeros(1, dtype=torch.long, device="cuda")
    cp = model.ConditioningProcessor_0
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        pose_cache = cp.pose_features(cond2, mask)
        for _ in range(t_noise):
            sam2._step(z, idx, cond2, mask, sst, pose_cache)
    save_grid(z, "evidence_denoised_from_t350.png")
    err = (z - gt).abs().mean().item()
    rec = {"evidence": "denoise_check", "t_noise": t_noise,
           "mean_abs_err_vs_gt": round(err, 4), "train_steps": steps}
    print(json.dumps(rec), flush=True)
    with open(os.path.join(OUT, "denoise_check.json"), "w") as f:
        json.dump(rec, f)


def main():
    os.makedirs(OUT, exist_ok=True)
    if "--sample-only" not in sys.argv:
        throughput_srn()
    overfit_and_sample()


if __name__ == "__main__":
    main()
