"""-m gpu: the surface distances (HD95 / ASD) on a real MI355X -- tests/surface_checks.py against libbcp_hip.so, and the two train scripts
with --val_surface."""
import logging
import math
import re

import pytest
import torch

import surface_checks as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu_ops():
    from bcp_amd.hip_ops import Ops
    assert torch.cuda.is_available(), "the gpu tests need a GPU"
    return Ops.product()  # raises loudly if libbcp_hip.so is missing


@pytest.fixture()
def dev():
    yield torch.device("cuda:0")
    torch.cuda.synchronize()


@pytest.mark.parametrize("shape", SC.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernels(gpu_ops, dev, shape):
    SC.check_kernels(gpu_ops, dev, shape)


def test_nosite(gpu_ops, dev):
    SC.check_nosite(gpu_ops, dev)


@pytest.mark.parametrize("shape", SC.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_metrics(gpu_ops, dev, shape):
    SC.check_metrics(gpu_ops, dev, shape)


def test_empty_raises(gpu_ops, dev):
    SC.check_empty_raises(gpu_ops, dev)


def test_refusals(gpu_ops):
    SC.check_refusals(gpu_ops.b)


def test_wiring_percase(gpu_ops, dev):
    SC.check_wiring_percase(gpu_ops, dev)


def test_wiring_val_2d(gpu_ops, dev):
    SC.check_wiring_val_2d(gpu_ops, dev)


def test_wiring_pancreas(gpu_ops, dev, golden_dir):
    SC.check_wiring_pancreas(gpu_ops, dev, golden_dir)


def test_wiring_la(gpu_ops, dev, golden_dir):
    SC.check_wiring_la(gpu_ops, dev, golden_dir)


def _logged(caplog, pattern):
    """the float groups of every log line that matches"""
    return [tuple(float(v) for v in m.groups()) for r in caplog.records for m in [re.search(pattern, r.getMessage())] if m]


def test_acdc_script_val_surface(tmp_path, monkeypatch, caplog):
    monkeypatch.chdir(tmp_path)
    caplog.set_level(logging.INFO)
    from bcp_amd import ACDC_BCP_train as T
    T.main(["--labelnum", "7", "--batch_size", "24", "--labeled_bs", "12", "--pre_iterations", "2", "--max_iterations", "3", "--log_every", "1",
            "--val_every", "2", "--val_cases", "1", "--exp", "BCP_surface", "--val_surface"])
    got = _logged(caplog, r"mean_dice : (\S+) mean_hd95 : (\S+)")
    assert got and all(math.isfinite(d) and math.isfinite(h) and h >= 0.0 for d, h in got), got
    sd = torch.load(tmp_path / "model/BCP/ACDC_BCP_surface_7_labeled/self_train/unet_best_model.pth")
    assert len(sd) == 226 and all(torch.isfinite(v.float()).all() for v in sd.values())


def test_pancreas_script_val_surface(tmp_path, monkeypatch, caplog):
    monkeypatch.chdir(tmp_path)
    caplog.set_level(logging.INFO)
    from bcp_amd.pancreas import train_pancreas as T
    T.main(["--pretraining_epochs", "1", "--self_training_epochs", "1", "--steps_per_epoch", "2", "--batch_size", "1", "--val_every", "1",
            "--val_stride", "48", "48", "--result_dir", str(tmp_path / "out"), "--val_surface"])
    got = _logged(caplog, r"val_hd95: (\S+), val_asd: (\S+)")
    assert len(got) == 2 and all(math.isfinite(h) and math.isfinite(a) and h >= 0.0 and a >= 0.0 for h, a in got), got
    st = torch.load(tmp_path / "out" / "self_train/best_ema_20_self.pth")
    assert len(st["net"]) == 60 and all(torch.isfinite(v.float()).all() for v in st["net"].values())
