"""-m gpu: GroupNorm (normalization='groupnorm') on a real MI355X -- tests/gnorm_checks.py against libbcp_hip.so, and the drivers with
--normalization groupnorm."""
import pytest
import torch

import gnorm_checks as G

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


def test_gnorm_widths(gpu_ops, dev):
    G.check_gnorm_widths(gpu_ops, dev)


def test_gnorm_epilogues(gpu_ops, dev):
    G.check_gnorm_epilogues(gpu_ops, dev)


def test_gnorm_partial_in(gpu_ops, dev):
    G.check_gnorm_partial_in(gpu_ops, dev)


def test_gnorm_refusals(gpu_ops):
    G.check_gnorm_refusals(gpu_ops.b)


def test_gn_keys(dev):
    G.check_gn_keys(dev)


@pytest.mark.parametrize("variant", ["la", "pancreas"])
def test_gn_pattern_grads(gpu_ops, dev, monkeypatch, variant):
    G.check_gn_pattern_grads(gpu_ops, dev, monkeypatch, variant)


def test_gn_eval(gpu_ops, dev, monkeypatch):
    G.check_gn_eval(gpu_ops, dev, monkeypatch)


def test_gn_batch_split(gpu_ops, dev):
    G.check_gn_batch_split(gpu_ops, dev)


@pytest.mark.parametrize("variant", ["la", "pancreas"])
def test_gn_step(gpu_ops, dev, monkeypatch, variant):
    G.check_gn_step(gpu_ops, dev, monkeypatch, variant)


def test_gn_launch_plans(gpu_ops, dev, monkeypatch):
    G.check_gn_launch_plans(gpu_ops, dev, monkeypatch, steps=2)                                     # per-launch replays
    G.check_gn_launch_plans(gpu_ops, dev, monkeypatch, steps=4, graphs=1, overlap=False)            # forward passes as graphs


def test_la_scripts_groupnorm(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    from bcp_amd import LA_BCP_train as T
    from bcp_amd import eval_LA as E
    T.main(["--labelnum", "8", "--batch_size", "4", "--labeled_bs", "2", "--pre_max_iteration", "2", "--self_max_iteration", "3", "--log_every", "1",
            "--val_every", "2", "--val_cases", "1", "--exp", "BCP_gn", "--normalization", "groupnorm"])
    sd = torch.load(tmp_path / "model/BCP/LA_BCP_gn_8_labeled/self_train/VNet_best_model.pth")
    assert len(sd) == 172 and all(torch.isfinite(v.float()).all() for v in sd.values())
    ev = ["--labelnum", "8", "--exp", "BCP_gn", "--root_path", str(tmp_path / "no_data"), "--cases", "1", "--stride", "64", "64"]
    avg = E.main(ev + ["--normalization", "groupnorm"])
    assert len(avg) == 4 and 0.0 <= float(avg[0]) <= 1.0
    with pytest.raises(RuntimeError):      # a checkpoint of the other normalisation fails loudly
        E.main(ev)
    for M in (T, E):
        with pytest.raises(SystemExit):
            M.main(["--normalization", "instancenorm"])


def test_pancreas_script_groupnorm(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    from bcp_amd.pancreas import train_pancreas as T
    out = tmp_path / "gn"
    avg = T.main(["--pretraining_epochs", "1", "--self_training_epochs", "1", "--steps_per_epoch", "2", "--batch_size", "1", "--val_every", "1",
                  "--val_stride", "48", "48", "--result_dir", str(out), "--normalization", "groupnorm", "--test"])
    assert len(avg) == 4
    st = torch.load(out / "self_train/best_ema_20_self.pth")
    assert len(st["net"]) == 118 and all(torch.isfinite(v.float()).all() for v in st["net"].values())
    with pytest.raises(SystemExit):
        T.main(["--normalization", "batchnorm"])
