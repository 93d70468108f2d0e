"""-m gpu: every producer -> GroupNorm seam on a real MI355X -- tests/gnorm_seam_checks.py against libbcp_hip.so; the simulator twin is
tests/test_emu_gnorm_seams.py."""
import pytest
import torch

import gnorm_seam_checks as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu_ops():
    from bcp_amd.hip_ops import Ops
    assert torch.cuda.is_available(), "the gpu tests need a GPU"
    yield Ops.product()  # raises loudly if libbcp_hip.so is missing
    S.report("device")


@pytest.fixture()
def dev():
    yield torch.device("cuda:0")
    torch.cuda.synchronize()


def test_finalize_rows(gpu_ops, dev):
    S.check_finalize_rows(gpu_ops, dev)


@pytest.mark.parametrize("case", S.FWD_SEAMS + S.FWD_SEAMS_GPU, ids=lambda c: f"{c[0]}-{c[2]}to{c[3]}-N{c[1]}-{'x'.join(map(str, c[4]))}")
def test_fwd_seam(gpu_ops, dev, case):
    S.check_fwd_seams(gpu_ops, dev, (case,))


@pytest.mark.parametrize("case", S.BWD_SEAMS, ids=lambda c: f"{c[0]}-{c[2]}-N{c[1]}-act{c[5]}")
def test_bwd_seam(gpu_ops, dev, case):
    S.check_bwd_seams(gpu_ops, dev, (case,))


def test_bwd_seams_k2(gpu_ops, dev):
    S.check_bwd_seams_k2(gpu_ops, dev)


def test_head(gpu_ops, dev):
    S.check_head(gpu_ops, dev)


def test_own_pass_edges(gpu_ops, dev):
    S.check_own_pass_edges(gpu_ops, dev)


@pytest.mark.parametrize("case", S.OWN_BLOCK_CASES, ids=lambda c: f"N{c[0]}-C{c[1]}-nb{c[3]}")
def test_own_blocks(gpu_ops, dev, case):
    S.check_own_blocks(gpu_ops, dev, case)


def test_apply_past_cap(gpu_ops, dev):
    S.check_apply_past_cap(gpu_ops, dev)


def test_route_census(gpu_ops):
    S.check_route_census(gpu_ops)
