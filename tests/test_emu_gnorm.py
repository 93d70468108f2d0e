"""GroupNorm (normalization='groupnorm') on the HOST simulator (tools/emu), CPU tensors: tests/gnorm_checks.py against the very kernel sources
of bcp_amd/csrc compiled for x86; the -m gpu twin is tests/test_gpu_gnorm.py."""
import os
import subprocess

import pytest
import torch

import gnorm_checks as G
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
def test_gnorm_widths(emu_ops):
    G.check_gnorm_widths(emu_ops, CPU)


def test_gnorm_epilogues(emu_ops):
    G.check_gnorm_epilogues(emu_ops, CPU)


def test_gnorm_partial_in(emu_ops):
    G.check_gnorm_partial_in(emu_ops, CPU)


def test_gnorm_refusals(emu_ops):
    G.check_gnorm_refusals(emu_ops.b)


def test_gnorm_refusals_product_library():
    """the gfx950 library refuses the same calls before it launches anything: no GPU needed"""
    assert os.path.exists(_lib.LIB_PATH), "libbcp_hip.so missing -- run __graft_entry__.build()"
    G.check_gnorm_refusals(_lib.Binding(_lib.LIB_PATH))


# ---- networks.  Whole passes on the simulator cost from half a minute to a few minutes each: the default CPU run takes one representative
# of every check; the rest are twins of what tests/test_gpu_gnorm.py runs on the device every time (marker `extended`, BCP_EXTENDED=1).
def test_gn_keys():
    G.check_gn_keys(CPU)


def test_gn_pattern_grads(emu_ops, monkeypatch):
    G.check_gn_pattern_grads(emu_ops, CPU, monkeypatch, "la")


def test_gn_eval(emu_ops, monkeypatch):
    G.check_gn_eval(emu_ops, CPU, monkeypatch, variants=("la",), sliding_window=False)


def test_gn_batch_split(emu_ops):
    G.check_gn_batch_split(emu_ops, CPU)


def test_gn_step(emu_ops, monkeypatch):
    G.check_gn_step(emu_ops, CPU, monkeypatch, "la")


def test_gn_launch_plans(emu_ops, monkeypatch):
    G.check_gn_launch_plans(emu_ops, CPU, monkeypatch, steps=2, cases=(("la", True),))


@pytest.mark.extended
def test_gn_pattern_grads_pancreas(emu_ops, monkeypatch):
    G.check_gn_pattern_grads(emu_ops, CPU, monkeypatch, "pancreas")


@pytest.mark.extended
def test_gn_eval_full(emu_ops, monkeypatch):
    G.check_gn_eval(emu_ops, CPU, monkeypatch)


@pytest.mark.extended
def test_gn_step_pancreas(emu_ops, monkeypatch):
    G.check_gn_step(emu_ops, CPU, monkeypatch, "pancreas")


@pytest.mark.extended
def test_gn_launch_plans_pancreas(emu_ops, monkeypatch):
    G.check_gn_launch_plans(emu_ops, CPU, monkeypatch, steps=2, cases=(("pancreas", True),))


def test_driver_flags_reject_unknown_normalizations():
    """--normalization is restricted with `choices` in the three command lines; the default is the present network"""
    from bcp_amd import LA_BCP_train as TL
    from bcp_amd import eval_LA as EL
    from bcp_amd.pancreas import train_pancreas as TP
    for parser, default, other in ((TL.parser, "batchnorm", "instancenorm"), (EL.parser, "batchnorm", "instancenorm"),
                                   (TP.build_parser(), "instancenorm", "batchnorm")):
        assert parser.parse_args([]).normalization == default
        assert parser.parse_args(["--normalization", "groupnorm"]).normalization == "groupnorm"
        for bad in (other, "layernorm"):
            with pytest.raises(SystemExit):
                parser.parse_args(["--normalization", bad])
