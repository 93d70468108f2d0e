"""-m gpu: the persistent 16 -> 16 channel conv (k_c3d, two fp16 planes) with its weight fragments held in the LDS (option
c3d16_form = 1, the default) against the form that streams them from global memory (c3d16_form = 0).  Same fragment values and the
same MFMA order: y, the statistics partials and the += path must be bit-identical."""
import pytest
import torch

from bcp_amd import hip_ops as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu_ops():
    from bcp_amd.hip_ops import Ops
    assert torch.cuda.is_available(), "the gpu tests need a GPU"
    return Ops.product()


def _operands(shape, seed):
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(*shape, 16, generator=g).to(dev)
    x._bcp_amax = H.amax_slots(float(x.abs().max()), dev)      # as in the step: the operand carries its |max| -> two fp16 planes
    w = (torch.randn(16, 16, 3, 3, 3, generator=g) * 0.05).to(dev)
    b = (torch.randn(16, generator=g) * 0.1).to(dev)
    return x, w, b


def _both_forms(ops, fn, **opts):
    """fn() -> tuple of tensors, once under c3d16_form = 0 and once under the default, each with the extra options set"""
    out = []
    for form in ("0", ""):
        ops.set_option("c3d16_form", form)
        for k, v in opts.items():
            ops.set_option(k, str(v))
        try:
            out.append(tuple(t.clone() for t in fn()))
            torch.cuda.synchronize()
        finally:
            for k in opts:
                ops.set_option(k)
            ops.set_option("c3d16_form")
    return out


def _same(a, b):
    for u, v in zip(a, b):
        assert u.shape == v.shape
        assert torch.equal(u.view(torch.uint8), v.view(torch.uint8)), (u.view(-1)[:4], v.view(-1)[:4])


@pytest.mark.parametrize("shape, groups, opts", [
    ((2, 112, 112, 80), 2, {}),                 # LA block_nine forward (teacher and student)
    ((2, 96, 96, 96), 2, {}),                   # pancreas
    ((2, 13, 21, 30), 2, {"conv3_b6": 3}),      # not a multiple of the 4x8x8 tile (conv3_b6 = 3: k_c3d below its 256 K-voxel threshold too)
    ((2, 24, 40, 48), 2, {"conv3_b6": 3, "conv3_p": 7}),   # few workgroups: many tiles each, statistics flushed at the group change
], ids=["la", "pancreas", "edge", "p7"])
def test_fwd_stats_bit_identical(gpu_ops, shape, groups, opts):
    x, w, b = _operands(shape, 7)
    wf, _ = gpu_ops.conv3_pack(w, 3)

    def run():
        y, part, rows = gpu_ops.conv3_fwd_stats(x, wf, b, 16, 3, groups)
        assert rows > 0 and (rows == opts["conv3_p"] if "conv3_p" in opts else True)       # (the persistent kernel: one row per workgroup)
        return y, part[: groups * rows * 16 * 16]
    old, new = _both_forms(gpu_ops, run, **opts)
    _same(old, new)
    # and the result is the convolution (loose: fp32-equivalent arithmetic, the tight bounds live in the product-op checks)
    if x.numel() <= 2 * 13 * 21 * 30 * 16:
        ref = torch.nn.functional.conv3d(x.permute(0, 4, 1, 2, 3).double().cpu(), w.double().cpu(), b.double().cpu(), padding=1)
        err = (new[0].permute(0, 4, 1, 2, 3).double().cpu() - ref).abs().max().item()
        assert err < 1e-4 * max(1.0, ref.abs().max().item()), err


@pytest.mark.parametrize("shape", [(2, 112, 112, 80), (1, 13, 21, 30)], ids=["la", "edge"])
def test_dgrad_pack_bit_identical(gpu_ops, shape):
    """block_nine's dgrad: conv3_fwd on the dgrad pack"""
    dy, w, _ = _operands(shape, 11)
    _, wd = gpu_ops.conv3_pack(w, 3)
    old, new = _both_forms(gpu_ops, lambda: (gpu_ops.conv3_fwd(dy, wd, None, 16, 3),), conv3_b6=3)
    _same(old, new)


def test_accumulate_bit_identical(gpu_ops):
    x, w, b = _operands((2, 24, 40, 48), 13)
    wf, _ = gpu_ops.conv3_pack(w, 3)
    base = torch.randn(2, 24, 40, 48, 16, generator=torch.Generator(device="cpu").manual_seed(5)).to(x.device)

    def run():
        y = base.clone()
        gpu_ops.conv3_fwd(x, wf, b, 16, 3, out=y, accumulate=True)
        return (y,)
    old, new = _both_forms(gpu_ops, run, conv3_b6=3)
    _same(old, new)
    assert not torch.equal(new[0], base)
