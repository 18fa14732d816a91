"""Shared inputs for the image-metric and evaluator tests (not a test file)."""

import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMAS = (0.0, 0.01, 0.03, 0.1, 0.3)  # noise added to pred, per image index


def disc_pairs(n, h, w, seed=0, sigmas=SIGMAS):
    """(pred, target), each (n,h,w,3) float64 in the [-1,1] convention.

    target: white background (+1) with a shaded coloured disc. pred: the same
    disc shifted by 2 px plus Gaussian noise whose sigma grows with the image
    index (SSIM from about 0.9 down to about 0.2); pred is left unclamped, so
    some values lie outside [-1,1]."""
    g = torch.Generator().manual_seed(seed)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float64),
                            torch.arange(w, dtype=torch.float64),
                            indexing="ij")
    r = 0.35 * min(h, w)

    def disc(cy, cx, colour):
        dist = torch.sqrt((ys - cy) ** 2 + (xs - cx) ** 2)
        alpha = ((r - dist) / 3.0 + 0.5).clamp(0.0, 1.0)[..., None]  # soft rim
        shade = 0.35 + 0.65 * (0.5 + ((xs - cx) + (ys - cy)) / (4.0 * r))
        body = (colour[None, None] * shade[..., None]) * 2.0 - 1.0
        return alpha * body + (1.0 - alpha)  # exactly +1 off the disc

    pred, target = [], []
    for i in range(n):
        colour = 0.2 + 0.8 * torch.rand(3, generator=g, dtype=torch.float64)
        t = disc(h / 2.0, w / 2.0, colour)
        p = disc(h / 2.0 + 2.0, w / 2.0 + 2.0, colour)
        p = p + sigmas[i % len(sigmas)] * torch.randn(
            h, w, 3, generator=g, dtype=torch.float64)
        pred.append(p)
        target.append(t)
    return torch.stack(pred), torch.stack(target)


def make_synth_dataset(path, instances=3, views=6, size=16):
    subprocess.run(
        [sys.executable, os.path.join(ROOT, "tools", "make_synth_srn.py"),
         str(path), "--instances", str(instances), "--views", str(views),
         "--size", str(size)],
        check=True, capture_output=True, timeout=120)
    return str(path)
