"""-m gpu: the 3-D 32 -> 32 channel conv (k_c3d, 32-channel slabs on two fp16 planes) as persistent workgroups that fetch the next tile's halo
under the current tile's tap pairs (option c3d32_form = 1, the default) against one tile per workgroup (c3d32_form = 0).  Same fragment values,
same MFMA order per accumulator, one statistics row per TILE in both forms: y, the statistics rows, the row count, the += path and the
backward-statistics dgrad must be bit-identical."""
import pytest
import torch

from bcp_amd import hip_ops as H

pytestmark = pytest.mark.gpu

C = 32
# The 4x8x8 tile, the one with a persistent form, serves a shape below 64 K voxels only when W is a multiple of 8; other widths go to the 4x4x8
# tile's staged kernel on three planes, which has one form (there the two runs are the same launch).  T48 cases do not reach the persistent
# kernel; "edge64k" is the shape with partial tiles on every axis that does.
T88, T48 = (4, 8, 8), (4, 4, 8)


@pytest.fixture(scope="module")
def gpu_ops():
    from bcp_amd.hip_ops import Ops
    assert torch.cuda.is_available(), "the gpu tests need a GPU"
    return Ops.product()


def _operands(shape, seed):
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(*shape, C, generator=g).to(dev)
    x._bcp_amax = H.amax_slots(float(x.abs().max()), dev)      # as in the step: the operand carries its |max| -> two fp16 planes
    w = (torch.randn(C, C, 3, 3, 3, generator=g) * 0.05).to(dev)
    b = (torch.randn(C, generator=g) * 0.1).to(dev)
    return x, w, b


def _tiles_per_group(shape, groups, tile):
    n, d, h, w = shape
    t = n * -(-d // tile[0]) * -(-h // tile[1]) * -(-w // tile[2])
    assert t % groups == 0
    return t // groups


def _both_forms(ops, fn, **opts):
    """fn() -> tuple of tensors, once under c3d32_form = 0 and once under the default, each with the extra options set"""
    out = []
    for form in ("0", ""):
        ops.set_option("c3d32_form", form)
        for k, v in opts.items():
            ops.set_option(k, str(v))
        try:
            out.append(tuple(t.clone() for t in fn()))
            torch.cuda.synchronize()
        finally:
            for k in opts:
                ops.set_option(k)
            ops.set_option("c3d32_form")
    return out


def _same(a, b):
    for u, v in zip(a, b):
        assert u.shape == v.shape
        assert torch.equal(u.view(torch.uint8), v.view(torch.uint8)), (u.view(-1)[:4], v.view(-1)[:4])


@pytest.mark.parametrize("shape, opts, tile", [
    ((2, 8, 16, 16), {"conv3_b6": 3}, T88),                  # 16 whole tiles, the group changes between two tiles (conv3_b6 = 3: the bf16 pipe below its voxel threshold too)
    ((2, 13, 21, 30), {"conv3_b6": 3}, T48),                 # partial tiles on every axis (of the 4x4x8 tile)
    ((2, 21, 42, 38), {"conv3_b6": 3}, T88),                 # partial tiles on every axis of the 4x8x8 tile: 360 tiles, one per workgroup
    ((2, 21, 42, 38), {"conv3_b6": 3, "conv3_p": 24}, T88),  # ... and 15 tiles per workgroup, each XCD walking its eighth of the list
    ((2, 24, 40, 48), {"conv3_b6": 3, "conv3_p": 7}, T88),   # few workgroups: many tiles each, uneven counts, workgroups that cross the group boundary
    ((2, 56, 56, 40), {}, T88),                              # the LA product shape: 980 tiles, two per workgroup
], ids=["whole", "edge", "edge64k", "edge64k-p24", "p7", "la"])
def test_fwd_stats_bit_identical(gpu_ops, shape, opts, tile):
    groups = 2
    x, w, b = _operands(shape, 7)
    wf, _ = gpu_ops.conv3_pack(w, 3)
    rows_seen, planes = [], []

    def run():
        y, part, rows = gpu_ops.conv3_fwd_stats(x, wf, b, C, 3, groups)
        rows_seen.append(rows)
        planes.append(gpu_ops.b.call("bcp_conv3_planes", *shape, C, C, 3, 0))      # (shape query under the options of this run)
        return y, part[: groups * rows * C * 16]
    old, new = _both_forms(gpu_ops, run, **opts)
    assert rows_seen[0] == rows_seen[1] == _tiles_per_group(shape, groups, tile), rows_seen      # one statistics row per tile in BOTH forms
    if tile == T88:
        assert planes == [2, 2], planes                                                           # an operand with its |max| takes the two-plane kernel here
    _same(old, new)
    # and the result is the convolution (loose: fp32-equivalent arithmetic, the tight bounds live in the product-op checks)
    if x.numel() <= 2 * 21 * 42 * 38 * C and "conv3_p" not in opts:
        ref = torch.nn.functional.conv3d(x.permute(0, 4, 1, 2, 3).double().cpu(), w.double().cpu(), b.double().cpu(), padding=1)
        err = (new[0].permute(0, 4, 1, 2, 3).double().cpu() - ref).abs().max().item()
        assert err < 1e-4 * max(1.0, ref.abs().max().item()), err
        # the rows sum to the column sums of y
        pt = new[1].view(torch.float64).view(groups, rows_seen[1], C, 2).sum(1).cpu()
        yv = new[0].double().cpu().view(groups, -1, C)
        assert torch.allclose(pt[..., 0], yv.sum(1), rtol=1e-9, atol=1e-9) and torch.allclose(pt[..., 1], (yv * yv).sum(1), rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("shape, opts", [((1, 13, 21, 30), {"conv3_b6": 3}), ((1, 9, 13, 16), {"conv3_b6": 3}), ((2, 24, 40, 48), {"conv3_b6": 3, "conv3_p": 7})],
                         ids=["edge", "edge-dh", "p7"])
def test_dgrad_pack_bit_identical(gpu_ops, shape, opts):
    """the 32 -> 32 dgrad: conv3_fwd on the dgrad pack"""
    dy, w, _ = _operands(shape, 11)
    _, wd = gpu_ops.conv3_pack(w, 3)
    old, new = _both_forms(gpu_ops, lambda: (gpu_ops.conv3_fwd(dy, wd, None, C, 3),), **opts)
    _same(old, new)
    if dy.numel() <= 2 * 13 * 21 * 30 * C:
        ref = torch.nn.functional.conv_transpose3d(dy.permute(0, 4, 1, 2, 3).double().cpu(), w.double().cpu(), padding=1)
        err = (new[0].permute(0, 4, 1, 2, 3).double().cpu() - ref).abs().max().item()
        assert err < 1e-4 * max(1.0, ref.abs().max().item()), err


def test_accumulate_bit_identical(gpu_ops):
    shape = (2, 13, 21, 32)      # (W a multiple of 8: the 4x8x8 tile, partial along D and H)
    x, w, b = _operands(shape, 13)
    wf, _ = gpu_ops.conv3_pack(w, 3)
    base = torch.randn(*shape, C, generator=torch.Generator(device="cpu").manual_seed(5)).to(x.device)

    def run():
        y = base.clone()
        gpu_ops.conv3_fwd(x, wf, b, C, 3, out=y, accumulate=True)
        return (y,)
    old, new = _both_forms(gpu_ops, run, conv3_b6=3, conv3_p=5)
    _same(old, new)
    assert not torch.equal(new[0], base)


@pytest.mark.parametrize("shape, opts, tile", [
    ((2, 8, 16, 16), {"conv3_b6": 3}, T88),
    ((2, 13, 21, 30), {"conv3_b6": 3}, T48),
    ((2, 24, 40, 48), {"conv3_b6": 3, "conv3_p": 7}, T88),
], ids=["whole", "edge", "p7"])
def test_dgrad_bwdstats_bit_identical(gpu_ops, shape, opts, tile):
    """the dgrad whose epilogue accumulates the consumer norm layer's backward statistics: dx, the rows and the row count, whichever form
    serves the backward-statistics instance"""
    groups = 2
    dy, w, _ = _operands(shape, 17)
    _, wd = gpu_ops.conv3_pack(w, 3)
    g = torch.Generator(device="cpu").manual_seed(19)
    dev = dy.device
    yprev = (torch.randn(*shape, C, generator=g) * 1.3 + 0.2).to(dev)
    gam, bet = (torch.rand(C, generator=g) + 0.5).to(dev), (torch.rand(C, generator=g) * 0.6 - 0.3).to(dev)
    _, st = gpu_ops.norm_fwd(yprev, groups, gam, bet, torch.zeros(C).to(dev), torch.ones(C).to(dev), H.ACT_RELU)
    rows_seen = []

    def run():
        dx, part, rows = gpu_ops.conv3_dgrad_bwdstats(dy, wd, C, 3, yprev, st, H.ACT_RELU, groups)
        rows_seen.append(rows)
        return dx, part[: groups * rows * C * 16]
    old, new = _both_forms(gpu_ops, run, **opts)
    assert rows_seen[0] == rows_seen[1] == _tiles_per_group(shape, groups, tile), rows_seen
    _same(old, new)
    # dx is the plain dgrad (which, without the statistics epilogue, runs in the persistent form under the default)
    _, plain = _both_forms(gpu_ops, lambda: (gpu_ops.conv3_fwd(dy, wd, None, C, 3),), **opts)
    assert torch.equal(new[0], plain[0])
