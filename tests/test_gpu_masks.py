"""-m gpu: the multi-box copy-paste regions on a real MI355X -- tests/mask_checks.py against libbcp_hip.so, the product sizes, one
full-size step per configuration and the three train scripts with --mask_strategy."""
import pytest
import torch

import mask_checks as M

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


def test_mask_boxes(gpu_ops, dev):
    M.check_mask_boxes(gpu_ops, dev)


def test_mask_boxes_refusals(gpu_ops):
    M.check_mask_boxes_refusals(gpu_ops.b)


def test_mix_mask(gpu_ops, dev):
    M.check_mix_mask(gpu_ops, dev)


def test_region_loss(gpu_ops, dev):
    M.check_region_loss(gpu_ops, dev)


@pytest.mark.parametrize("variant", ["la", "pancreas"])
def test_la_step_regions(gpu_ops, dev, monkeypatch, variant):
    M.check_la_step_regions(gpu_ops, dev, monkeypatch, variant=variant)


def test_la_step_dispatch(gpu_ops, dev):
    M.check_la_step_dispatch(gpu_ops, dev)


def test_acdc_step_regions(gpu_ops, dev, monkeypatch):
    M.check_acdc_step_regions(gpu_ops, dev, monkeypatch)


def test_pre_train_regions(gpu_ops, dev):
    M.check_pre_train_regions(gpu_ops, dev)


def test_full_size_region_properties(gpu_ops, dev):
    M.check_full_size_properties(gpu_ops, dev)


@pytest.mark.parametrize("config", ["la", "pancreas", "acdc"])
def test_full_size_step_random(gpu_ops, dev, config):
    M.check_full_size_step(gpu_ops, dev, config)


def test_la_script_mask_strategies(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    from bcp_amd import LA_BCP_train as T
    for strategy in ("random", "concat"):
        T.main(["--labelnum", "8", "--batch_size", "4", "--labeled_bs", "2", "--pre_max_iteration", "2", "--self_max_iteration", "3", "--log_every", "1",
                "--val_every", "2", "--val_cases", "1", "--exp", "BCP_" + strategy, "--mask_strategy", strategy])
        sd = torch.load(tmp_path / f"model/BCP/LA_BCP_{strategy}_8_labeled/self_train/VNet_best_model.pth")
        assert len(sd) == 259 and all(torch.isfinite(v.float()).all() for v in sd.values())
    with pytest.raises(SystemExit):
        T.main(["--mask_strategy", "contact"])


def test_acdc_script_mask_strategies(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    from bcp_amd import ACDC_BCP_train as T
    for strategy in ("random", "contact"):
        T.main(["--labelnum", "7", "--batch_size", "24", "--labeled_bs", "12", "--pre_iterations", "2", "--max_iterations", "3", "--log_every", "1",
                "--val_every", "2", "--val_cases", "1", "--exp", "BCP_" + strategy, "--mask_strategy", strategy])
        sd = torch.load(tmp_path / f"model/BCP/ACDC_BCP_{strategy}_7_labeled/self_train/unet_best_model.pth")
        assert len(sd) == 226 and all(torch.isfinite(v.float()).all() for v in sd.values())
    with pytest.raises(SystemExit):
        T.main(["--mask_strategy", "concat"])


def test_pancreas_script_mask_strategies(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    from bcp_amd.pancreas import train_pancreas as T
    for strategy in ("random", "concat"):
        out = tmp_path / strategy
        T.main(["--pretraining_epochs", "1", "--self_training_epochs", "1", "--steps_per_epoch", "2", "--batch_size", "1", "--val_every", "1",
                "--val_stride", "48", "48", "--result_dir", str(out), "--mask_strategy", strategy])
        st = torch.load(out / "self_train/best_ema_20_self.pth")
        assert len(st["net"]) == 60 and all(torch.isfinite(v.float()).all() for v in st["net"].values())
    with pytest.raises(SystemExit):
        T.main(["--mask_strategy", "contact"])
