"""-m gpu: the residual V-Net (has_residual=True) on a real MI355X -- tests/residual_checks.py against libbcp_hip.so, and the LA drivers with
--has_residual."""
import pytest
import torch

import residual_checks as R

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


# ---- kernels
def test_res_widths(gpu_ops, dev):
    R.check_res_widths(gpu_ops, dev)


def test_res_grouped(gpu_ops, dev):
    R.check_res_grouped(gpu_ops, dev)


def test_res_epilogues(gpu_ops, dev):
    R.check_res_epilogues(gpu_ops, dev)


def test_res_partial_in(gpu_ops, dev):
    R.check_res_partial_in(gpu_ops, dev)


def test_res_eval_kernel(gpu_ops, dev):
    R.check_res_eval_kernel(gpu_ops, dev)


def test_res_refusals(gpu_ops):
    R.check_res_refusals(gpu_ops.b)


# ---- loop and branch edges of csrc/norm_res.hip, element by element against fp64 (tests/product_ops.py's references and bounds)
def test_edge_apply_wrap_option(gpu_ops, dev):
    R.check_edge_apply_wrap_option(gpu_ops, dev)


def test_edge_apply_wrap_default(gpu_ops, dev):
    R.check_edge_apply_wrap_default(gpu_ops, dev)


def test_edge_eval_wrap(gpu_ops, dev):
    R.check_edge_eval_wrap(gpu_ops, dev)


def test_edge_wide(gpu_ops, dev):
    R.check_edge_wide(gpu_ops, dev)


def test_edge_spg2_nbps2(gpu_ops, dev):
    R.check_edge_spg2_nbps2(gpu_ops, dev)


def test_edge_block_one_route(gpu_ops, dev):
    R.check_edge_block_one_route(gpu_ops, dev)


# ---- network
def test_res_keys(dev):
    R.check_res_keys(dev)


def test_res_golden_tiny(gpu_ops, dev):
    R.check_res_golden_tiny(gpu_ops, dev)


def test_res_pattern_grads(gpu_ops, dev):
    R.check_res_pattern_grads(gpu_ops, dev)


def test_res_eval(gpu_ops, dev):
    R.check_res_eval(gpu_ops, dev)


def test_res_groups(gpu_ops, dev):
    R.check_res_groups(gpu_ops, dev)


def test_res_routes(gpu_ops, dev):
    R.check_res_routes(gpu_ops, dev)


@pytest.mark.parametrize("case", sorted(R.PLAN_CASES))
def test_planned_equals_ran(gpu_ops, dev, case):
    R.check_planned_equals_ran(gpu_ops, dev, case)


# ---- step and plans
def test_res_step(gpu_ops, dev, monkeypatch):
    R.check_res_step(gpu_ops, dev, monkeypatch)


def test_res_launch_plans(gpu_ops, dev, monkeypatch):
    R.check_res_launch_plans(gpu_ops, dev, monkeypatch, steps=2)                                     # per-launch replays
    R.check_res_launch_plans(gpu_ops, dev, monkeypatch, steps=4, graphs=1, overlap=False)            # forward passes as graphs


# ---- scripts
def test_la_scripts_residual(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    from bcp_amd import LA_BCP_train as T
    from bcp_amd import eval_LA as E
    T.main(["--labelnum", "8", "--batch_size", "4", "--labeled_bs", "2", "--pre_max_iteration", "2", "--self_max_iteration", "3", "--log_every", "1",
            "--val_every", "2", "--val_cases", "1", "--exp", "BCP_res", "--has_residual"])
    sd = torch.load(tmp_path / "model/BCP/LA_BCP_res_8_labeled/self_train/VNet_best_model.pth")
    assert len(sd) == 259 and all(torch.isfinite(v.float()).all() for v in sd.values())
    ev = ["--labelnum", "8", "--exp", "BCP_res", "--root_path", str(tmp_path / "no_data"), "--cases", "1", "--stride", "64", "64"]
    res = E.main(ev + ["--has_residual"])
    assert len(res) == 4 and all(float(v) == float(v) and abs(float(v)) != float("inf") for v in res) and 0.0 <= float(res[0]) <= 1.0
    plain = E.main(ev)      # the same keys load into the plain net: another function, another result
    assert [float(v) for v in plain] != [float(v) for v in res], "evaluating a residual checkpoint without --has_residual must not run the residual net"


def test_refused_configurations():
    from bcp_amd.networks.VNet import VNet
    from bcp_amd.networks.net_factory import net_factory
    with pytest.raises(NotImplementedError):
        VNet(n_channels=1, n_classes=2, normalization="groupnorm", has_residual=True)
    with pytest.raises(NotImplementedError):
        VNet(n_channels=1, n_classes=2, normalization="instancenorm", has_residual=True, variant="pancreas")
    with pytest.raises(NotImplementedError):
        net_factory("VNet", in_chns=1, class_num=2, mode="train", normalization="groupnorm", has_residual=True)
    assert net_factory("VNet", in_chns=1, class_num=2, mode="train", has_residual=True).has_residual
