"""The 3-D 32 -> 32 channel conv's two forms (option c3d32_form: persistent workgroups with one statistics row per tile, 1, or one tile per
workgroup, 0) on the HOST simulator: bit-identical y and statistics rows, the same row count, and the result is the convolution."""
import os
import subprocess

import pytest
import torch

from bcp_amd import _lib
from bcp_amd import hip_ops as H
from bcp_amd.hip_ops import Ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "_emu", "libbcp_emu.so")
C = 32


@pytest.fixture(scope="module")
def emu_ops():
    srcs = [os.path.join(ROOT, "bcp_amd", "csrc", f) for f in os.listdir(os.path.join(ROOT, "bcp_amd", "csrc")) if f.endswith((".hip", ".h"))]
    srcs += [os.path.join(ROOT, "tools", "emu", "emu_runtime.cpp"), os.path.join(ROOT, "tools", "emu", "hip", "hip_runtime.h")]
    if not os.path.exists(EMU) or any(os.path.getmtime(s) > os.path.getmtime(EMU) for s in srcs):
        subprocess.check_call([os.path.join(ROOT, "tools", "emu", "build_emu.sh")])
    return Ops(_lib.Binding(EMU), allow_cpu=True)


def _tiles(shape, tile):
    n, d, h, w = shape
    return n * -(-d // tile[0]) * -(-h // tile[1]) * -(-w // tile[2])


# The 4x8x8 tile, the one with a persistent form, serves a shape below 64 K voxels only when W is a multiple of 8; other widths go to the
# 4x4x8 tile's staged kernel on three planes, which has one form ("edge": the two runs are the same launch).  "edge-dh" has partial tiles along
# D and H on the persistent kernel; partial tiles along W on it need 64 K voxels, which the simulator leaves to tests/test_gpu_c3d32.py.
@pytest.mark.parametrize("shape, p, tile", [((2, 5, 9, 17), 0, (4, 4, 8)), ((2, 5, 9, 16), 0, (4, 8, 8)), ((2, 8, 16, 16), 3, (4, 8, 8))],
                         ids=["edge", "edge-dh", "p3"])
def test_c3d32_forms_emu(emu_ops, shape, p, tile):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(*shape, C, generator=g)
    x._bcp_amax = H.amax_slots(float(x.abs().max()), x.device)
    w = torch.randn(C, C, 3, 3, 3, generator=g) * 0.05
    b = torch.randn(C, generator=g) * 0.1
    wf, _ = emu_ops.conv3_pack(w, 3)
    outs = []
    for form in ("0", ""):
        emu_ops.set_option("c3d32_form", form)
        emu_ops.set_option("conv3_b6", "3")      # k_c3d below its 256 K-voxel threshold
        if p:
            emu_ops.set_option("conv3_p", str(p))
        try:
            if tile == (4, 8, 8):
                assert emu_ops.b.call("bcp_conv3_planes", *shape, C, C, 3, 0) == 2      # an operand with its |max| takes the two-plane kernel here
            y, part, rows = emu_ops.conv3_fwd_stats(x, wf, b, C, 3, 2)
            assert rows == _tiles(shape, tile) // 2      # one statistics row per TILE in both forms
            outs.append((y.clone(), part[: 2 * rows * C * 16].clone()))
        finally:
            emu_ops.set_option("conv3_p")
            emu_ops.set_option("conv3_b6")
            emu_ops.set_option("c3d32_form")
    assert torch.equal(outs[0][0].view(torch.uint8), outs[1][0].view(torch.uint8))
    assert torch.equal(outs[0][1], outs[1][1])
    ref = torch.nn.functional.conv3d(x.permute(0, 4, 1, 2, 3).double(), w.double(), b.double(), padding=1).permute(0, 2, 3, 4, 1)
    err = (outs[1][0].double() - ref).abs().max().item()
    assert err < 1e-4 * max(1.0, ref.abs().max().item()), err
    # the rows sum to the column sums of y
    pt = outs[1][1].view(torch.float64).view(2, -1, C, 2).sum(1)
    yv = outs[1][0].double().view(2, -1, C)
    assert torch.allclose(pt[..., 0], yv.sum(1), rtol=1e-9, atol=1e-9) and torch.allclose(pt[..., 1], (yv * yv).sum(1), rtol=1e-9, atol=1e-9)
