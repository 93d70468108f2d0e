"""-m gpu: tests/wgrad_checks.py on the device -- the fp16 planes' magnitude domain on the full grid, the weight gradient's zero / NaN /
Inf semantics, and every weight-gradient kernel instance against fp64 (the queries must give the route fixture's answers there)."""
import pytest
import torch

import wgrad_checks as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu_ops():
    from bcp_amd.hip_ops import Ops
    assert torch.cuda.is_available(), "the gpu tests need a GPU"
    return Ops.product()  # raises loudly if libbcp_hip.so is missing


@pytest.mark.parametrize("case", W.F16_CASES)
def test_f16_range(gpu_ops, case):
    report = []
    try:
        W.check_f16_range(gpu_ops, torch.device("cuda:0"), case, ks=W.K_FULL, report=report)
    finally:
        print("\n".join(report))
    torch.cuda.synchronize()


def test_wgrad_nonfinite(gpu_ops):
    W.check_wgrad_nonfinite(gpu_ops, torch.device("cuda:0"))
    torch.cuda.synchronize()


@pytest.mark.parametrize("ident,d,opts,symbols,log", [pytest.param(*r, id=r[0]) for r in W.INSTANCE_ROWS])
def test_wgrad_instance(gpu_ops, ident, d, opts, symbols, log):
    report = []
    W.check_wgrad_instance(gpu_ops, torch.device("cuda:0"), d, opts, symbols, log, report=report)
    print("\n".join(report))
    torch.cuda.synchronize()
