"""The surface distances (HD95 / ASD) on the HOST simulator (tools/emu), CPU tensors: tests/surface_checks.py against the very kernel sources
of bcp_amd/csrc compiled for x86; the -m gpu twin is tests/test_gpu_surface.py."""
import os
import subprocess

import pytest
import torch

import surface_checks as SC
from bcp_amd import _lib
from bcp_amd.hip_ops import Ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "_emu", "libbcp_emu.so")
EMU_OVERRIDE = os.environ.get("BCP_EMU_LIB")
CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def emu_ops():
    """the simulator handle, built the way tests/test_emu_kernels.py builds it"""
    if EMU_OVERRIDE:
        return Ops(_lib.Binding(EMU_OVERRIDE), allow_cpu=True)
    csrc = os.path.join(ROOT, "bcp_amd", "csrc")
    srcs = [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hip", ".h"))]
    srcs += [os.path.join(ROOT, "tools", "emu", "emu_runtime.cpp"), os.path.join(ROOT, "tools", "emu", "hip", "hip_runtime.h")]
    if not os.path.exists(EMU) or any(os.path.getmtime(s) > os.path.getmtime(EMU) for s in srcs):
        subprocess.check_call([os.path.join(ROOT, "tools", "emu", "build_emu.sh")])
    return Ops(_lib.Binding(EMU), allow_cpu=True)


@pytest.mark.parametrize("shape", SC.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernels(emu_ops, shape):
    SC.check_kernels(emu_ops, CPU, shape)


def test_nosite(emu_ops):
    SC.check_nosite(emu_ops, CPU)


@pytest.mark.parametrize("shape", SC.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_metrics(emu_ops, shape):
    SC.check_metrics(emu_ops, CPU, shape)


def test_empty_raises(emu_ops):
    SC.check_empty_raises(emu_ops, CPU)


def test_refusals(emu_ops):
    SC.check_refusals(emu_ops.b)


def test_refusals_product_library():
    """the gfx950 library refuses the same calls before it launches anything: no GPU needed"""
    assert os.path.exists(_lib.LIB_PATH), "libbcp_hip.so missing -- run __graft_entry__.build()"
    SC.check_refusals(_lib.Binding(_lib.LIB_PATH))


def test_surface_ops_are_not_profiled():
    """the product-op table replays the validation passes: the new ops stay out of bench.py's per-op rows"""
    from bcp_amd import hip_ops
    assert not {"surface_border", "edt_sq", "surface_hist"} & set(hip_ops._PROFILED)


def test_wiring_percase(emu_ops):
    SC.check_wiring_percase(emu_ops, CPU)


def test_wiring_val_2d(emu_ops):
    SC.check_wiring_val_2d(emu_ops, CPU)


def test_wiring_pancreas(emu_ops, golden_dir):
    SC.check_wiring_pancreas(emu_ops, CPU, golden_dir)


def test_wiring_la(emu_ops, golden_dir):
    SC.check_wiring_la(emu_ops, CPU, golden_dir)


def test_parser_defaults():
    SC.check_parser_defaults()
