"""tests/wgrad_checks.py on the HOST simulator (CPU tensors): the fp16 planes' magnitude domain at the default grid (the full grid is
`extended`: the device runs it every time), the weight gradient's zero / NaN / Inf semantics, and every weight-gradient kernel instance
against fp64 with the launch log compared with the route fixture's row."""
import pytest
import torch

import wgrad_checks as W
from bcp_amd import _lib
from bcp_amd.hip_ops import Ops

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def emu_ops():
    import make_golden_conv3_routes as R      # (tools/ is on the path: wgrad_checks reads the route fixture through it)
    return Ops(_lib.Binding(R.build_emu()), allow_cpu=True)


@pytest.mark.parametrize("case", W.F16_CASES)
def test_f16_range(emu_ops, case):
    W.check_f16_range(emu_ops, CPU, case, ks=W.K_DEFAULT)


@pytest.mark.extended
@pytest.mark.parametrize("case", W.F16_CASES)
def test_f16_range_full_grid(emu_ops, case):
    W.check_f16_range(emu_ops, CPU, case, ks=W.K_FULL)


def test_wgrad_nonfinite(emu_ops):
    W.check_wgrad_nonfinite(emu_ops, CPU)


@pytest.mark.parametrize("ident,d,opts,symbols,log", [
    pytest.param(*r, id=r[0], marks=[pytest.mark.extended] if W.row_voxels(r[1]) > W.SIM_EXTENDED_VOX else []) for r in W.INSTANCE_ROWS])
def test_wgrad_instance(emu_ops, ident, d, opts, symbols, log):
    W.check_wgrad_instance(emu_ops, CPU, d, opts, symbols, log)
