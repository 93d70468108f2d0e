"""Every producer -> GroupNorm seam on the HOST simulator (tools/emu), CPU tensors: tests/gnorm_seam_checks.py against the very kernel
sources of bcp_amd/csrc compiled for x86; the -m gpu twin is tests/test_gpu_gnorm_seams.py."""
import os
import subprocess

import pytest
import torch

import gnorm_seam_checks as S
from bcp_amd import _lib
from bcp_amd.hip_ops import Ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "_emu", "libbcp_emu.so")
CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def emu_ops():
    """the simulator handle, built the way tests/test_emu_gnorm.py builds it"""
    csrc = os.path.join(ROOT, "bcp_amd", "csrc")
    srcs = [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hip", ".h"))]
    srcs += [os.path.join(ROOT, "tools", "emu", "emu_runtime.cpp"), os.path.join(ROOT, "tools", "emu", "hip", "hip_runtime.h")]
    if not os.path.exists(EMU) or any(os.path.getmtime(s) > os.path.getmtime(EMU) for s in srcs):
        subprocess.check_call([os.path.join(ROOT, "tools", "emu", "build_emu.sh")])
    yield Ops(_lib.Binding(EMU), allow_cpu=True)
    S.report("simulator")


def test_finalize_rows(emu_ops):
    S.check_finalize_rows(emu_ops, CPU)


@pytest.mark.parametrize("case", S.FWD_SEAMS, ids=lambda c: f"{c[0]}-{c[2]}to{c[3]}-N{c[1]}")
def test_fwd_seam(emu_ops, case):
    S.check_fwd_seams(emu_ops, CPU, (case,))


@pytest.mark.parametrize("case", S.BWD_SEAMS, ids=lambda c: f"{c[0]}-{c[2]}-N{c[1]}-act{c[5]}")
def test_bwd_seam(emu_ops, case):
    S.check_bwd_seams(emu_ops, CPU, (case,))


def test_bwd_seams_k2(emu_ops):
    S.check_bwd_seams_k2(emu_ops, CPU)


def test_head(emu_ops):
    S.check_head(emu_ops, CPU)


def test_own_pass_edges(emu_ops):
    S.check_own_pass_edges(emu_ops, CPU)


@pytest.mark.parametrize("case", S.OWN_BLOCK_CASES, ids=lambda c: f"N{c[0]}-C{c[1]}-nb{c[3]}")
def test_own_blocks(emu_ops, case):
    """part H (a) .. (f); the sample past the library's own apply-grid cap (check_apply_past_cap) is left to the device"""
    S.check_own_blocks(emu_ops, CPU, case)


def test_route_census(emu_ops):
    S.check_route_census(emu_ops)


def test_route_census_product_library():
    """the gfx950 library answers the row queries on the host: no GPU needed"""
    assert os.path.exists(_lib.LIB_PATH), "libbcp_hip.so missing -- run __graft_entry__.build()"
    S.check_route_census(Ops(_lib.Binding(_lib.LIB_PATH), allow_cpu=True))
