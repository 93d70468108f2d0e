"""The persistent 16 -> 16 channel conv's two weight forms (option c3d16_form: weight fragments in the LDS, 1, or streamed from global
memory, 0) on the HOST simulator: bit-identical y and statistics partials, and the result is the convolution."""
import os
import subprocess

import pytest
import torch

from bcp_amd import _lib
from bcp_amd import hip_ops as H
from bcp_amd.hip_ops import Ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "_emu", "libbcp_emu.so")


@pytest.fixture(scope="module")
def emu_ops():
    srcs = [os.path.join(ROOT, "bcp_amd", "csrc", f) for f in os.listdir(os.path.join(ROOT, "bcp_amd", "csrc")) if f.endswith((".hip", ".h"))]
    srcs += [os.path.join(ROOT, "tools", "emu", "emu_runtime.cpp"), os.path.join(ROOT, "tools", "emu", "hip", "hip_runtime.h")]
    if not os.path.exists(EMU) or any(os.path.getmtime(s) > os.path.getmtime(EMU) for s in srcs):
        subprocess.check_call([os.path.join(ROOT, "tools", "emu", "build_emu.sh")])
    return Ops(_lib.Binding(EMU), allow_cpu=True)


@pytest.mark.parametrize("shape, p", [((2, 5, 9, 17), 0), ((2, 8, 16, 16), 3)], ids=["edge", "p3"])
def test_c3d16_forms_emu(emu_ops, shape, p):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(*shape, 16, generator=g)
    x._bcp_amax = H.amax_slots(float(x.abs().max()), x.device)
    w = torch.randn(16, 16, 3, 3, 3, generator=g) * 0.05
    b = torch.randn(16, generator=g) * 0.1
    wf, _ = emu_ops.conv3_pack(w, 3)
    outs = []
    for form in ("0", ""):
        emu_ops.set_option("c3d16_form", form)
        emu_ops.set_option("conv3_b6", "3")      # k_c3d below its 256 K-voxel threshold
        if p:
            emu_ops.set_option("conv3_p", str(p))
        try:
            y, part, rows = emu_ops.conv3_fwd_stats(x, wf, b, 16, 3, 2)
            assert rows == (p or rows) and rows > 0      # (the persistent kernel: one statistics row per workgroup)
            outs.append((y.clone(), part[: 2 * rows * 16 * 16].clone()))
        finally:
            emu_ops.set_option("conv3_p")
            emu_ops.set_option("conv3_b6")
            emu_ops.set_option("c3d16_form")
    assert torch.equal(outs[0][0].view(torch.uint8), outs[1][0].view(torch.uint8))
    assert torch.equal(outs[0][1], outs[1][1])
    ref = torch.nn.functional.conv3d(x.permute(0, 4, 1, 2, 3).double(), w.double(), b.double(), padding=1).permute(0, 2, 3, 4, 1)
    err = (outs[1][0].double() - ref).abs().max().item()
    assert err < 1e-4 * max(1.0, ref.abs().max().item()), err
