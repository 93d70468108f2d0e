"""The residual V-Net (has_residual=True) on the HOST simulator (tools/emu), CPU tensors: tests/residual_checks.py against the very kernel
sources of bcp_amd/csrc compiled for x86; the -m gpu twin is tests/test_gpu_residual.py."""
import os
import subprocess

import pytest
import torch

import residual_checks as R
from bcp_amd import _lib
from bcp_amd.hip_ops import Ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "_emu", "libbcp_emu.so")
CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def emu_ops():
    """the simulator handle, built the way tests/test_emu_kernels.py builds it"""
    csrc = os.path.join(ROOT, "bcp_amd", "csrc")
    srcs = [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hip", ".h"))]
    srcs += [os.path.join(ROOT, "tools", "emu", "emu_runtime.cpp"), os.path.join(ROOT, "tools", "emu", "hip", "hip_runtime.h")]
    if not os.path.exists(EMU) or any(os.path.getmtime(s) > os.path.getmtime(EMU) for s in srcs):
        subprocess.check_call([os.path.join(ROOT, "tools", "emu", "build_emu.sh")])
    return Ops(_lib.Binding(EMU), allow_cpu=True)


# ---- kernels
def test_res_widths(emu_ops):
    R.check_res_widths(emu_ops, CPU)


def test_res_grouped(emu_ops):
    R.check_res_grouped(emu_ops, CPU)


def test_res_epilogues(emu_ops):
    R.check_res_epilogues(emu_ops, CPU)


def test_res_partial_in(emu_ops):
    R.check_res_partial_in(emu_ops, CPU)


def test_res_eval_kernel(emu_ops):
    R.check_res_eval_kernel(emu_ops, CPU)


def test_res_refusals(emu_ops):
    R.check_res_refusals(emu_ops.b)


def test_res_refusals_product_library():
    """the gfx950 library refuses the same calls before it launches anything: no GPU needed"""
    assert os.path.exists(_lib.LIB_PATH), "libbcp_hip.so missing -- run __graft_entry__.build()"
    R.check_res_refusals(_lib.Binding(_lib.LIB_PATH))


# ---- loop and branch edges of csrc/norm_res.hip, element by element against fp64 (tests/product_ops.py's references and bounds)
def test_edge_apply_wrap_option(emu_ops):
    R.check_edge_apply_wrap_option(emu_ops, CPU)


def test_edge_apply_wrap_default(emu_ops):
    R.check_edge_apply_wrap_default(emu_ops, CPU)


def test_edge_eval_wrap(emu_ops):
    R.check_edge_eval_wrap(emu_ops, CPU)


def test_edge_wide(emu_ops):
    R.check_edge_wide(emu_ops, CPU)


def test_edge_spg2_nbps2(emu_ops):
    R.check_edge_spg2_nbps2(emu_ops, CPU)


def test_edge_block_one_route(emu_ops):
    R.check_edge_block_one_route(emu_ops, CPU)


# ---- the fixture and the restatement (torch fp64 on the CPU only)
def test_restatement_equals_reference_fixture():
    R.check_restatement_vs_fixture()


# ---- network.  Whole passes on the simulator cost about half a minute each: the default CPU run takes the structural checks and one
# forward / backward against the fixture; the rest are twins of what tests/test_gpu_residual.py runs on the device every time.
def test_res_keys():
    R.check_res_keys(CPU)


def test_res_golden_tiny(emu_ops):
    R.check_res_golden_tiny(emu_ops, CPU)


def test_res_routes(emu_ops):
    R.check_res_routes(emu_ops, CPU)


def test_res_eval(emu_ops):
    R.check_res_eval(emu_ops, CPU)


@pytest.mark.extended
@pytest.mark.parametrize("case", sorted(R.PLAN_CASES))
def test_planned_equals_ran(emu_ops, case):
    R.check_planned_equals_ran(emu_ops, CPU, case)


def test_routes_reached(emu_ops):
    R.check_routes_reached(emu_ops)


def test_routes_reached_product_library():
    """the gfx950 library's shape queries give the same set: no GPU needed"""
    assert os.path.exists(_lib.LIB_PATH), "libbcp_hip.so missing -- run __graft_entry__.build()"
    R.check_routes_reached(Ops(_lib.Binding(_lib.LIB_PATH), allow_cpu=True))


def test_refused_configurations():
    from bcp_amd.networks.VNet import VNet
    for kw in (dict(normalization="groupnorm"), dict(normalization="instancenorm", variant="pancreas")):
        with pytest.raises(NotImplementedError):
            VNet(n_channels=1, n_classes=2, has_residual=True, **kw)
