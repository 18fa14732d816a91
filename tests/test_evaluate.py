"""Evaluator + evaluate.py CLI (CPU, tiny model, sidelength 16)."""

import json
import math
import os
import subprocess
import sys

import pytest
import torch

from image_metrics_cases import ROOT, make_synth_dataset
from novel_view_synthesis_3d_amd import ops
from novel_view_synthesis_3d_amd.config import XUNetConfig
from novel_view_synthesis_3d_amd.engine.evaluate import (
    Evaluator, to_serialisable,
)
from novel_view_synthesis_3d_amd.models.xunet import XUNet


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    return make_synth_dataset(tmp_path_factory.mktemp("srn") / "data")


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    m = XUNet(XUNetConfig.named("tiny"), 16)
    with torch.no_grad():  # nonzero head: the output depends on the input
        m.Conv_1.weight.normal_(0, 0.05)
    return m


@pytest.fixture(scope="module")
def result(model, dataset):
    model.train()  # evaluate() must put this back
    ev = Evaluator(model, num_steps=3, batch_objects=2)
    res = ev.evaluate(dataset, 16, input_view=0, num_targets=3,
                      return_images=True)
    assert model.training
    return res


def test_counts_and_entries(result):
    assert result["n_instances"] == 3 and result["n_views"] == 9
    assert [e["name"] for e in result["per_instance"]] == [
        "inst_0000", "inst_0001", "inst_0002"]
    for e in result["per_instance"]:
        assert e["n_views"] == 3
        assert math.isfinite(e["psnr"]) and 0.0 < e["psnr"] < 60.0
        assert -1.0 <= e["ssim"] <= 1.0
    s = result["settings"]
    assert s["num_steps"] == 3 and s["batch_objects"] == 2
    assert s["mode"] == "autoregressive" and s["quantize"] is False
    assert result["images"].shape == (9, 16, 16, 3)
    assert result["targets"].shape == (9, 16, 16, 3)
    assert float(result["images"].abs().max()) <= 1.0


def test_reported_metrics_match_fp64_reference(result):
    psnr, ssim = ops.image_metrics(result["images"].double(),
                                   result["targets"].double())
    assert abs(result["psnr"] - float(psnr.mean())) <= 1e-4
    assert abs(result["ssim"] - float(ssim.mean())) <= 1e-5
    for i, e in enumerate(result["per_instance"]):  # instance-major order
        assert abs(e["psnr"] - float(psnr[3 * i:3 * i + 3].mean())) <= 1e-4
        assert abs(e["ssim"] - float(ssim[3 * i:3 * i + 3].mean())) <= 1e-5


def test_second_run_is_identical(model, dataset, result):
    ev = Evaluator(model, num_steps=3, batch_objects=2)
    again = ev.evaluate(dataset, 16, input_view=0, num_targets=3,
                        return_images=True)
    assert torch.equal(again["images"], result["images"])
    assert again["psnr"] == result["psnr"]
    assert again["ssim"] == result["ssim"]
    assert again["per_instance"] == result["per_instance"]


def test_other_settings_run(model, dataset, tmp_path):
    one = Evaluator(model, num_steps=3, batch_objects=1).evaluate(
        dataset, 16, input_view=0, num_targets=3)
    assert one["n_instances"] == 3 and one["n_views"] == 9
    assert "images" not in one
    ind = Evaluator(model, num_steps=3, batch_objects=2, mode="independent",
                    quantize=True).evaluate(
        dataset, 16, input_view=5, max_instances=2,
        save_images_dir=str(tmp_path / "img"))
    assert ind["n_instances"] == 2 and ind["n_views"] == 10  # all 5 others
    assert ind["settings"]["mode"] == "independent"
    saved = sorted(p.stem for p in (tmp_path / "img" / "inst_0001").iterdir())
    assert saved == [f"{v:06d}" for v in range(5)]
    json.dumps(to_serialisable(ind))
    with pytest.raises(ValueError):
        Evaluator(model, num_steps=3, mode="both")


def test_too_few_views_raises_and_restores_mode(model, dataset):
    model.train()
    ev = Evaluator(model, num_steps=3)
    with pytest.raises(ValueError, match=r"inst_0000.*--input-view 64"):
        ev.evaluate(dataset, 16, input_view=64)
    assert model.training
    model.eval()
    ev.evaluate(dataset, 16, input_view=0, num_targets=1, max_instances=1)
    assert not model.training


def test_non_finite_psnr_serialises_as_none():
    res = {"psnr": math.inf, "ssim": 1.0, "n_instances": 1, "n_views": 1,
           "per_instance": [{"name": "a", "psnr": math.inf, "ssim": 1.0,
                             "n_views": 1}],
           "settings": {}, "images": torch.zeros(1), "targets": torch.zeros(1)}
    data = json.loads(json.dumps(to_serialisable(res)))
    assert data["psnr"] is None and data["per_instance"][0]["psnr"] is None
    assert "images" not in data and "targets" not in data


@pytest.mark.timeout(600)
def test_evaluate_cli(tmp_path, dataset):
    from novel_view_synthesis_3d_amd.engine import checkpoint as ckpt
    m = XUNet(XUNetConfig.named("tiny"), 16)
    path = ckpt.save_checkpoint(str(tmp_path / "ckpt"), m, None, 1)
    out_dir = tmp_path / "eval"
    out = subprocess.run(
        [sys.executable, os.path.join(ROOT, "evaluate.py"),
         "--checkpoint", path, "--model", "tiny", "--sidelength", "16",
         "--folder", dataset, "--steps", "3", "--input-view", "0",
         "--num-targets", "2", "--no-graph", "--out", str(out_dir)],
        cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "eval: PSNR" in out.stdout
    data = json.loads((out_dir / "metrics.json").read_text())
    for key in ("psnr", "ssim", "n_instances", "n_views", "per_instance",
                "settings"):
        assert key in data
    assert data["n_instances"] == 3 and data["n_views"] == 6
    assert {"name", "psnr", "ssim", "n_views"} <= set(data["per_instance"][0])
