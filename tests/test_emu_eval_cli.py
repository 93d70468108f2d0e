"""The offline evaluation entry points (test_LA, test_ACDC, the pancreas test pass) on the HOST simulator (tools/emu), CPU tensors:
tests/eval_cli_checks.py against the kernel sources of bcp_amd/csrc compiled for x86; the -m gpu twin is tests/test_gpu_eval_cli.py.
The training drivers need a GPU, so the checks that run them (main --test of the pancreas driver, train-then-evaluate) live in the twin."""
import os
import subprocess

import pytest
import torch

import eval_cli_checks as EC
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


@pytest.mark.parametrize("nms", (0, 1))
def test_la_cli_equals_library(emu_ops, golden_dir, tmp_path, monkeypatch, capsys, nms):
    EC.check_la_cli_equals_library(emu_ops, CPU, golden_dir, tmp_path, monkeypatch, capsys, nms)


def test_la_no_surface(emu_ops, golden_dir, tmp_path, monkeypatch):
    EC.check_la_no_surface(emu_ops, CPU, golden_dir, tmp_path, monkeypatch)


def test_la_golden_case_numpy_and_reference(emu_ops, golden_dir, tmp_path, monkeypatch):
    EC.check_la_golden_case(emu_ops, CPU, golden_dir, tmp_path, monkeypatch)


def test_checkpoint_formats(emu_ops, golden_dir, tmp_path, monkeypatch, caplog):
    EC.check_checkpoint_formats(emu_ops, CPU, golden_dir, tmp_path, monkeypatch, caplog)


@pytest.mark.parametrize("shape", ((7, 13, 70), (5, 66, 3)), ids=lambda s: "x".join(map(str, s)))
def test_acdc_case_metrics(emu_ops, shape):
    EC.check_acdc_pure(emu_ops, CPU, shape)


def test_acdc_cli(emu_ops, tmp_path, monkeypatch, capsys):
    EC.check_acdc_cli(emu_ops, CPU, tmp_path, monkeypatch, capsys)


def test_pancreas_test_model(emu_ops, golden_dir, tmp_path):
    EC.check_pancreas_test_model(emu_ops, CPU, golden_dir, tmp_path)


def test_no_heavy_imports():
    EC.check_no_heavy_imports()
