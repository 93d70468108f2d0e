"""-m gpu: the offline evaluation entry points on a real MI355X -- tests/eval_cli_checks.py against libbcp_hip.so through the product's
net_factory, the pancreas driver with --test, and train-then-evaluate for LA and ACDC from one working directory."""
import logging
import math
import os
import re

import numpy as np
import pytest
import torch

import eval_cli_checks as EC
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


@pytest.mark.parametrize("nms", (0, 1))
def test_la_cli_equals_library(gpu_ops, dev, golden_dir, tmp_path, monkeypatch, capsys, nms):
    EC.check_la_cli_equals_library(gpu_ops, dev, golden_dir, tmp_path, monkeypatch, capsys, nms)


def test_la_no_surface(gpu_ops, dev, golden_dir, tmp_path, monkeypatch):
    EC.check_la_no_surface(gpu_ops, dev, golden_dir, tmp_path, monkeypatch)


def test_la_golden_case_numpy_and_reference(gpu_ops, dev, golden_dir, tmp_path, monkeypatch):
    EC.check_la_golden_case(gpu_ops, dev, golden_dir, tmp_path, monkeypatch)


def test_checkpoint_formats(gpu_ops, dev, golden_dir, tmp_path, monkeypatch, caplog):
    EC.check_checkpoint_formats(gpu_ops, dev, golden_dir, tmp_path, monkeypatch, caplog)


@pytest.mark.parametrize("shape", ((7, 13, 70), (5, 66, 3)), ids=lambda s: "x".join(map(str, s)))
def test_acdc_case_metrics(gpu_ops, dev, shape):
    EC.check_acdc_pure(gpu_ops, dev, shape)


def test_acdc_cli(gpu_ops, dev, tmp_path, monkeypatch, capsys):
    EC.check_acdc_cli(gpu_ops, dev, tmp_path, monkeypatch, capsys)


def test_pancreas_test_model(gpu_ops, dev, golden_dir, tmp_path):
    EC.check_pancreas_test_model(gpu_ops, dev, golden_dir, tmp_path)


_PANCREAS = ["--pretraining_epochs", "1", "--self_training_epochs", "1", "--steps_per_epoch", "2", "--batch_size", "1", "--val_every", "0"]


def test_pancreas_script_test_pass(gpu_ops, dev, tmp_path, monkeypatch, caplog):
    """7: main --test logs four finite averages and returns them; without --test main runs none of the surface kernels"""
    monkeypatch.chdir(tmp_path)
    caplog.set_level(logging.INFO)
    from bcp_amd.pancreas import train_pancreas as T
    pattern = r"Test: dice: (\S+), jc: (\S+), hd95: (\S+), asd: (\S+)"
    with SC.count_surface_ops(gpu_ops) as seen:
        assert T.main(_PANCREAS) is None
    assert not seen and not [r for r in caplog.records if re.search(pattern, r.getMessage())]
    with SC.count_surface_ops(gpu_ops) as seen:
        avg = T.main(_PANCREAS + ["--test"])
    logged = [tuple(float(v) for v in m.groups()) for r in caplog.records for m in [re.search(pattern, r.getMessage())] if m]
    assert len(logged) == 1 and all(math.isfinite(v) for v in logged[0]), logged
    assert 0.0 <= logged[0][1] <= logged[0][0] <= 1.0 and logged[0][2] >= 0.0 and logged[0][3] >= 0.0, logged
    assert np.abs(np.asarray(avg) - np.asarray(logged[0])).max() <= 0.5e-4 + 1e-12          # logged with four decimals
    assert seen in ({}, {"surface_border": 2, "edt_sq": 2, "surface_hist": 2}), seen          # one case: none if its prediction is empty


def _forget(run_dir):
    """so that the next run's performance.txt is its own"""
    path = os.path.join(run_dir, "performance.txt")
    if os.path.exists(path):
        os.remove(path)


def _evaluated(metric, run_dir):
    assert math.isfinite(float(metric[0])) and 0.0 <= float(metric[0]) <= 1.0, metric
    assert os.path.getsize(os.path.join(run_dir, "performance.txt")) > 0


def test_la_train_then_evaluate(gpu_ops, dev, tmp_path, monkeypatch):
    """8: LA_BCP_train.main for 3 + 3 iterations, then test_LA.main for both stages from the same working directory"""
    monkeypatch.chdir(tmp_path)
    from bcp_amd import LA_BCP_train as T
    from bcp_amd import test_LA as TL
    T.main(["--labelnum", "8", "--batch_size", "4", "--labeled_bs", "2", "--pre_max_iteration", "3", "--self_max_iteration", "3", "--log_every", "1",
            "--val_every", "2", "--val_cases", "1"])
    for stage in ("self_train", "pre_train"):
        _forget("model/BCP/LA_BCP_8_labeled")
        avg = TL.main(["--labelnum", "8", "--stage_name", stage, "--root_path", str(tmp_path / "no_data"), "--cases", "1"])
        assert len(avg) == 4
        _evaluated(avg, "model/BCP/LA_BCP_8_labeled")


def test_acdc_train_then_evaluate(gpu_ops, dev, tmp_path, monkeypatch):
    """8: ACDC_BCP_train.main for 3 + 3 iterations, then test_ACDC.main for both stages from the same working directory"""
    monkeypatch.chdir(tmp_path)
    from bcp_amd import ACDC_BCP_train as T
    from bcp_amd import test_ACDC as TA
    T.main(["--labelnum", "7", "--batch_size", "24", "--labeled_bs", "12", "--pre_iterations", "3", "--max_iterations", "3", "--log_every", "1",
            "--val_every", "2", "--val_cases", "1"])
    for stage in ("self_train", "pre_train"):
        _forget("model/BCP/ACDC_BCP_7_labeled")
        metric, save = TA.main(["--labelnum", "7", "--stage_name", stage, "--root_path", str(tmp_path / "no_data"), "--cases", "1"])
        assert len(metric) == 3 and all(len(m) == 4 for m in metric) and save == "./model/BCP/ACDC_BCP_7_labeled/unet_predictions/"
        for m in metric:
            _evaluated(m, "model/BCP/ACDC_BCP_7_labeled")
