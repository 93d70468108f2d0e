"""The multi-box copy-paste regions on the HOST simulator (tools/emu), CPU tensors: tests/mask_checks.py against the very kernel sources of
bcp_amd/csrc compiled for x86; the -m gpu twin is tests/test_gpu_masks.py."""
import os
import subprocess

import pytest
import torch

import mask_checks as M
from bcp_amd import _lib
from bcp_amd.hip_ops import Ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "_emu", "libbcp_emu.so")
EMU_OVERRIDE = os.environ.get("BCP_EMU_LIB")      # tools/emu/run_asan.sh: the AddressSanitizer build of the simulator
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


def test_mask_boxes(emu_ops):
    M.check_mask_boxes(emu_ops, CPU)


def test_mask_boxes_refusals(emu_ops):
    M.check_mask_boxes_refusals(emu_ops.b)


def test_mask_boxes_refusals_product_library():
    """the gfx950 library refuses the same calls before it launches anything: no GPU needed (tests/test_abi.py does so for bcp_mix_box)"""
    assert os.path.exists(_lib.LIB_PATH), "libbcp_hip.so missing -- run __graft_entry__.build()"
    M.check_mask_boxes_refusals(_lib.Binding(_lib.LIB_PATH))


def test_mix_mask(emu_ops):
    M.check_mix_mask(emu_ops, CPU)


def test_draws_match_the_reference(golden_dir):
    M.check_draws_golden(golden_dir)


def test_region_loss(emu_ops):
    M.check_region_loss(emu_ops, CPU)


# Whole steps on the simulator cost about half a minute each.  The default CPU run takes one representative of every check; the full
# versions are twins of what tests/test_gpu_masks.py runs on the device every time (marker `extended`, BCP_EXTENDED=1 runs them here).
def test_la_step_regions(emu_ops, monkeypatch):
    M.check_la_step_regions(emu_ops, CPU, monkeypatch, variant="la", modes=(True,))


def test_la_step_dispatch(emu_ops):
    M.check_la_step_dispatch(emu_ops, CPU, one_box_modes=(True,), strategies=("random",))


def test_acdc_step_regions(emu_ops, monkeypatch):
    M.check_acdc_step_regions(emu_ops, CPU, monkeypatch, modes=(True,), dispatch=False)


def test_pre_train_regions(emu_ops):
    M.check_pre_train_regions(emu_ops, CPU, acdc=False)


@pytest.mark.extended
@pytest.mark.parametrize("variant", ["la", "pancreas"])
def test_la_step_regions_full(emu_ops, monkeypatch, variant):
    M.check_la_step_regions(emu_ops, CPU, monkeypatch, variant=variant)


@pytest.mark.extended
def test_step_dispatch_full(emu_ops, monkeypatch):
    M.check_la_step_dispatch(emu_ops, CPU)
    M.check_acdc_step_regions(emu_ops, CPU, monkeypatch)
    M.check_pre_train_regions(emu_ops, CPU)


def test_driver_flags_reject_unknown_strategies():
    """--mask_strategy is restricted with `choices` in all three drivers; the default leaves the step's keyword at None"""
    from bcp_amd import ACDC_BCP_train as TA
    from bcp_amd import LA_BCP_train as TL
    for parser, ok, bad in ((TL.parser, ("box", "random", "concat"), "contact"), (TA.parser, ("box", "random", "contact"), "concat")):
        assert parser.parse_args([]).mask_strategy == "box"
        for v in ok:
            assert parser.parse_args(["--mask_strategy", v]).mask_strategy == v
        with pytest.raises(SystemExit):
            parser.parse_args(["--mask_strategy", bad])
    from bcp_amd import train_step
    assert train_step.cli_mask_strategy(TL.parser.parse_args([]).mask_strategy) is None
    assert train_step.cli_mask_strategy(TA.parser.parse_args(["--mask_strategy", "contact"]).mask_strategy) == "contact"
    from bcp_amd.pancreas import train_pancreas as TP
    with pytest.raises(SystemExit):
        TP.main(["--mask_strategy", "contact"])
