"""Trainer — the reference train.py Trainer re-designed for MI355X.

Keeps the reference's public surface (Trainer(folder, train_batch_size=...,
...).train(), reference train.py:78-127) and fixes its defects:
  * true DP instead of the pmap ensemble (D3) — parallel/ddp.py
  * per-step CFG mask + dropout randomness (D2: the reference bakes one mask
    at trace time)
  * on-device forward noising (K19 moved out of dataset workers)
  * resumable checkpoints with optimizer state (§5.4)
  * per-element MSE loss by default; `loss='frob'` reproduces the
    reference's whole-batch Frobenius-norm quirk (D8, train.py:67)
  * bf16 autocast on GPU; fp32 master weights + Adam
"""

from __future__ import annotations

import contextlib
import os
import time
from pathlib import Path
from typing import Dict, Optional

import torch
import torch.nn.functional as F

from novel_view_synthesis_3d_amd.config import TrainConfig, XUNetConfig
from novel_view_synthesis_3d_amd.data.srn import SceneClassDataset
from novel_view_synthesis_3d_amd.data.synthetic import synthetic_batch
from novel_view_synthesis_3d_amd.diffusion.forward import q_sample
from novel_view_synthesis_3d_amd.diffusion.schedules import DiffusionSchedule
from novel_view_synthesis_3d_amd.engine import checkpoint as ckpt
from novel_view_synthesis_3d_amd.engine.metrics import JsonlLogger, RateMeter
from novel_view_synthesis_3d_amd.models.xunet import XUNet
from novel_view_synthesis_3d_amd.parallel.ddp import (
    DataParallelEngine, init_distributed,
)


def _cycle(dl):
    while True:
        for d in dl:
            yield d


class Trainer:
    def __init__(self, folder: Optional[str] = None, *,
                 train_batch_size: int = 2,
                 train_lr: float = 1e-4,
                 train_num_steps: int = 100_000,
                 save_every: int = 1000,
                 img_sidelength: int = 64,
                 results_folder: str = "./results",
                 model_cfg: Optional[XUNetConfig] = None,
                 train_cfg: Optional[TrainConfig] = None,
                 device: Optional[str] = None):
        cfg = train_cfg or TrainConfig()
        cfg.train_batch_size = train_batch_size
        cfg.train_lr = train_lr
        cfg.train_num_steps = train_num_steps
        cfg.save_every = save_every
        cfg.img_sidelength = img_sidelength
        cfg.results_folder = results_folder
        self.cfg = cfg
        self.model_cfg = model_cfg or XUNetConfig()

        # --- distributed / device -------------------------------------
        self.rank, self.world, self.local_rank = init_distributed()
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        if device == "cuda":
            torch.cuda.set_device(self.local_rank)
            device = f"cuda:{self.local_rank}"
        self.device = torch.device(device)
        self.is_main = self.rank == 0

        torch.manual_seed(cfg.seed * 9176 + self.rank)

        # --- model / optimizer / DP -----------------------------------
        self.model = XUNet(self.model_cfg, img_sidelength).to(self.device)
        self.model.train()
        recipe = cfg.max_grad_norm is not None or cfg.ema_decay is not None
        if self.device.type == "cuda" or recipe:
            # on CPU the recipe runs on FusedAdam's eager branch
            from novel_view_synthesis_3d_amd.engine.optim import FusedAdam
            kw = dict(max_grad_norm=cfg.max_grad_norm,
                      ema_decay=cfg.ema_decay,
                      ema_warmup=cfg.ema_warmup) if recipe else {}
            self.opt = FusedAdam(self.model.parameters(), lr=cfg.train_lr,
                                 betas=cfg.adam_betas, eps=cfg.adam_eps, **kw)
        else:
            self.opt = torch.optim.Adam(self.model.parameters(),
                                        lr=cfg.train_lr,
                                        betas=cfg.adam_betas,
                                        eps=cfg.adam_eps)
        self.ddp = DataParallelEngine(self.model, bucket_mb=cfg.bucket_mb)
        self.schedule = DiffusionSchedule(1000)
        self.step = 0

        # --- data ------------------------------------------------------
        self.folder = folder
        mode = cfg.data
        if mode == "auto":
            mode = "srn" if (folder and os.path.isdir(folder)) else "synthetic"
        self.data_mode = mode
        self.dl = None
        if mode == "srn":
            ds = SceneClassDataset(root_dir=folder,
                                   max_num_instances=-1,
                                   max_observations_per_instance=50,
                                   img_sidelength=img_sidelength,
                                   specific_observation_idcs=None,
                                   samples_per_instance=1)
            assert len(ds) > 0
            sampler = None
            if self.world > 1:
                sampler = torch.utils.data.distributed.DistributedSampler(ds)
            self.dl = _cycle(torch.utils.data.DataLoader(
                ds, batch_size=train_batch_size, shuffle=(sampler is None),
                sampler=sampler, drop_last=True, collate_fn=ds.collate_fn,
                pin_memory=(self.device.type == "cuda"),
                num_workers=cfg.num_workers,
                # without persistent workers a small dataset (epoch = a few
                # batches) respawns worker processes every epoch — measured
                # 27 img/s instead of ~700 on the tiny overfit set
                persistent_workers=(cfg.num_workers > 0)))
        self._gen = torch.Generator(device=self.device)
        self._gen.manual_seed(cfg.seed * 131071 + self.rank + 1)

        # --- bookkeeping ----------------------------------------------
        self.results_folder = Path(results_folder)
        if self.is_main:
            self.results_folder.mkdir(exist_ok=True, parents=True)
        self.logger = JsonlLogger(
            str(self.results_folder / "train_log.jsonl"), enabled=self.is_main)
        self.meter = RateMeter()

        if cfg.resume:
            path = (ckpt.find_latest(cfg.ckpt_folder)
                    if cfg.resume == "auto" else cfg.resume)
            if path:
                self.step = ckpt.load_checkpoint(path, self.model, self.opt,
                                                 map_location=self.device)
                if self.is_main:
                    print(f"resumed from {path} at step {self.step}")

    # -----------------------------------------------------------------
    def next_batch(self) -> Dict[str, torch.Tensor]:
        """A raw batch (x, x_target, poses) on device."""
        if self.data_mode == "synthetic":
            return synthetic_batch(self.cfg.train_batch_size,
                                   self.cfg.img_sidelength,
                                   device=self.device, generator=self._gen)
        obs, _ = next(self.dl)
        return {k: v.to(self.device, non_blocking=True) for k, v in obs.items()}

    def prepare_model_inputs(self, raw: Dict[str, torch.Tensor]):
        """On-device forward noising (K19) + CFG mask (per-step randomness,
        fixing reference D2)."""
        B = raw["x"].shape[0]
        if "z" in raw:  # cpu_noising dataset path
            batch = dict(raw)
            noise = raw["noise"]
        else:
            t = torch.randint(0, self.schedule.timesteps, (B,),
                              device=self.device, generator=self._gen)
            z, noise, logsnr = q_sample(raw["x_target"], t, self.schedule,
                                        generator=self._gen)
            batch = {"x": raw["x"], "z": z, "logsnr": logsnr.to(self.device),
                     "R1": raw["R1"], "t1": raw["t1"],
                     "R2": raw["R2"], "t2": raw["t2"], "K": raw["K"]}
        cond_mask = (torch.rand(B, device=self.device, generator=self._gen)
                     > self.cfg.cond_drop_prob).to(torch.float32)
        return batch, cond_mask, noise

    def compute_loss(self, out: torch.Tensor, noise: torch.Tensor):
        out = out.to(torch.float32)
        noise = noise.to(torch.float32)
        if self.cfg.loss == "frob":  # reference train.py:67 (quirk D8)
            return torch.linalg.vector_norm(out - noise)
        return F.mse_loss(out, noise)

    def _autocast(self):
        if self.device.type == "cuda" and self.cfg.amp == "bf16":
            return torch.autocast("cuda", dtype=torch.bfloat16)
        return contextlib.nullcontext()

    def _set_lr(self) -> None:
        """Linear LR warmup, derived from self.step so it survives resume."""
        n = self.cfg.lr_warmup_steps
        if n > 0:
            lr = self.cfg.train_lr * min(1.0, (self.step + 1) / n)
            for group in self.opt.param_groups:
                group["lr"] = lr

    def train_step(self, raw: Optional[Dict[str, torch.Tensor]] = None
                   ) -> torch.Tensor:
        """One optimization step; returns the (local) loss tensor.
        Gradient clipping and the EMA update (when configured) happen
        inside opt.step(), i.e. after the data-parallel reduction."""
        self._set_lr()
        if self.cfg.use_graph and self.device.type == "cuda":
            return self._train_step_graphed(raw)
        if raw is None:
            raw = self.next_batch()
        batch, cond_mask, noise = self.prepare_model_inputs(raw)
        self.ddp.zero_flags()  # zeroes the flat grad buffers when DP is on
        if not self.ddp.enabled:
            # keep grad storage stable on GPU so FusedAdam's plan caches
            self.opt.zero_grad(set_to_none=(self.device.type != "cuda"))
        with self._autocast():
            out = self.model(batch, cond_mask)
        loss = self.compute_loss(out, noise)
        loss.backward()
        self.ddp.finish()
        self.opt.step()
        return loss.detach()

    # -- hipGraph-captured training step --------------------------------
    # Forward noising + CFG mask + bf16 forward + loss + backward are
    # captured as ONE hipGraph (kills per-kernel launch overhead and host
    # gaps). Gradients land in stable p.grad storage; the bucketed RCCL
    # all-reduce and the fused Adam update run after each replay (RCCL
    # collectives are kept outside the capture).
    # Off by default because it measured ~4% slower (the step is GPU-bound).
    # Randomness advances under replay: the fused-GN dropout seed is a
    # snapshot of a device-resident counter (ops/hip_ops.py _next_gn_seed),
    # so the clone + increment are captured and every replay draws a fresh
    # mask, and the Philox RNG ops (noise, cond_mask) advance as well.

    def _graph_body(self):
        if self.data_mode == "synthetic":
            raw = synthetic_batch(self.cfg.train_batch_size,
                                  self.cfg.img_sidelength, device=self.device)
        else:
            raw = self._static_raw
        B = raw["x"].shape[0]
        t = torch.randint(0, self.schedule.timesteps, (B,),
                          device=self.device)
        z, noise, logsnr = q_sample(raw["x_target"], t, self.schedule)
        batch = {"x": raw["x"], "z": z, "logsnr": logsnr,
                 "R1": raw["R1"], "t1": raw["t1"],
                 "R2": raw["R2"], "t2": raw["t2"], "K": raw["K"]}
        cond_mask = (torch.rand(B, device=self.device)
                     > self.cfg.cond_drop_prob).to(torch.float32)
        grads = [p.grad for p in self.model.parameters()
                 if p.grad is not None]
        if grads:  # zero the stable grad storage in one fused launch
            torch._foreach_zero_(grads)
        with self._autocast():
            out = self.model(batch, cond_mask)
        loss = self.compute_loss(out, noise)
        with self.ddp.no_sync():  # collectives stay outside the graph
            loss.backward()
        return loss

    def _init_graph(self):
        if self.data_mode != "synthetic":
            raw = self.next_batch()
            self._static_raw = {k: v.clone() for k, v in raw.items()}
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):  # warmup allocates grads + caches plans
                loss = self._graph_body()
                self.opt.step()
        torch.cuda.current_stream().wait_stream(s)
        self._graph = torch.cuda.CUDAGraph()
        # capture on the SAME stream the warmup ran on: the parameters' grad
        # accumulators were created on `s` during warmup, and accumulation
        # escapes the capture (-> NaN on replay) if the capture stream
        # differs from theirs. Replays then also run on `s`
        # (_train_step_graphed): replaying a graph on a stream other than
        # its capture stream raced with the out-of-graph optimizer work and
        # corrupted the loss buffer when replays were queued back-to-back.
        import os as _os
        if _os.environ.get("NVS3D_GRAPH_CAPTURE", "warmup") == "default":
            self._graph_stream = torch.cuda.current_stream()
            with torch.cuda.graph(self._graph):
                self._static_loss = self._graph_body()
        else:
            self._graph_stream = s
            with torch.cuda.graph(self._graph, stream=s):
                self._static_loss = self._graph_body()
        self.graph_active = True
        if self.is_main:
            print("[trainer] hipGraph captured for the training step",
                  flush=True)

    def _train_step_graphed(self, raw):
        if not hasattr(self, "_graph"):
            try:
                self._init_graph()
            except Exception as e:
                print(f"[trainer] hipGraph capture FAILED ({e}); falling "
                      f"back to eager stepping", flush=True)
                self.graph_active = False
                self.cfg.use_graph = False
                torch.cuda.synchronize()
                return self.train_step(raw)
        if self.data_mode != "synthetic":
            if raw is None:
                raw = self.next_batch()
            for k, v in raw.items():
                self._static_raw[k].copy_(v, non_blocking=True)
        import os as _os
        if _os.environ.get("NVS3D_GRAPH_REPLAY", "capture") == "current":
            self._graph.replay()
            self.ddp.reduce_all()
            self.opt.step()
        else:
            # replay AND the out-of-graph tail on the capture stream, so
            # queued replays never interleave with another stream's work
            cur = torch.cuda.current_stream()
            self._graph_stream.wait_stream(cur)
            with torch.cuda.stream(self._graph_stream):
                self._graph.replay()
                self.ddp.reduce_all()  # in-place on the flat grad buffers
                self.opt.step()
            cur.wait_stream(self._graph_stream)
        return self._static_loss.detach()

    def train(self) -> None:
        """Run to train_num_steps. Interrupts (SIGINT/SIGTERM) and crashes
        checkpoint before exiting, so `--resume auto` continues where the
        run stopped (the reference loses up to save_every steps on any
        failure — SURVEY.md §5.3/§5.4)."""
        try:
            self._train_loop()
        except (KeyboardInterrupt, Exception) as e:
            if self.is_main and self.step > 0:
                path = ckpt.save_checkpoint(
                    self.cfg.ckpt_folder, self.model, self.opt, self.step,
                    extra={"model_cfg": vars(self.model_cfg),
                           "img_sidelength": self.cfg.img_sidelength,
                           "interrupted": repr(e)})
                print(f"[trainer] interrupted at step {self.step}; "
                      f"checkpoint saved to {path}", flush=True)
            raise

    def _train_loop(self) -> None:
        cfg = self.cfg
        while self.step < cfg.train_num_steps:
            t0 = time.perf_counter()
            loss = self.train_step()
            self.meter.update(cfg.train_batch_size * self.world)
            if self.step % cfg.log_every == 0:
                lval = float(self.ddp.all_reduce_scalar(loss).item()) \
                    if self.ddp.enabled else float(loss.item())
                # recipe read-outs share this sync point (never per step)
                recipe_log = {}
                gnorm = getattr(self.opt, "last_grad_norm", None)
                if gnorm is not None:
                    recipe_log = {"grad_norm": float(gnorm.item()),
                                  "skipped_steps": self.opt.skipped_steps}
                if self.is_main:
                    rate = self.meter.rate()
                    tail = "".join(f" {k}={v:.4g}"
                                   for k, v in recipe_log.items())
                    print(f"{self.step}: loss={lval:.5f} "
                          f"images/sec={rate:.1f}{tail}", flush=True)
                    self.logger.log(step=self.step, loss=lval,
                                    images_per_sec=rate,
                                    step_time=time.perf_counter() - t0,
                                    **recipe_log)
            if self.step % cfg.save_every == 0 and self.step > 0 and self.is_main:
                ckpt.save_checkpoint(
                    cfg.ckpt_folder, self.model, self.opt, self.step,
                    extra={"model_cfg": vars(self.model_cfg),
                           "img_sidelength": cfg.img_sidelength})
            self.step += 1
        if self.is_main:
            ckpt.save_checkpoint(
                cfg.ckpt_folder, self.model, self.opt, self.step,
                extra={"model_cfg": vars(self.model_cfg),
                       "img_sidelength": cfg.img_sidelength})
            print("training completed")
