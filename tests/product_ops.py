"""The ops the three product steps launch, at their in-step shapes, with fp64 references and an elementwise comparator.

STEP_KEYS holds what `Ops.profile_end()` records for each call of a replayed step: (op, shapes of the first three tensor arguments, first
three int arguments, number of the first two tensors that carry `_bcp_amax`).  The key carries no keyword arguments, so STEP_VARIANTS adds,
per norm key, the epilogues the step's norm calls really use (fused partials, channel scale, dropout, residual, statistics only, slab
output), read off a step by `record_step_variants`.  tests/test_gpu_product_ops.py asserts that a real step records nothing outside the
two tables and runs DRIVERS over the rows whose op family has one (`driven_rows()`).

This covers part of the steps' ops only.  Families without a driver, still checked only by tests/kernel_checks.py at small shapes and by
the whole-step comparisons: the fused first-layer convs (conv3_c1_*), the k2s2 / transposed / pointwise convs (down_*, up_*, k2_*,
pw_*, pw16_*), norm_*_slabs, the losses (mixloss_pair_*, ACDC dice_prob), mix_box and the weight packs.

The comparator: every element is held to |out - ref64| <= tau * cond, where cond is the same linear op applied in fp64 to |x| and |w| (a
per-element bound on what rounding can do).  A rel-L2 test spreads an error confined to one tile over the whole tensor; this one does not.
"""
from __future__ import annotations

import numpy as np
import torch

# -------------------------------------------------------------------------------------------------- comparator


def where(idx, shape, tile=(4, 8, 8)):
    """'face' if the voxel touches the volume's border, 'seam' if it lies on a tile border of `tile`, else 'interior'.
    idx: (n, d, h, w, c) of a channels-last [N, D, H, W, C] tensor (2-D tensors: D == 1)."""
    sp = shape[1:4]
    v = idx[1:4]
    if any(s > 1 and (i == 0 or i == s - 1) for i, s in zip(v, sp)):
        return "face"
    if any(s > 1 and (i % t == 0 or i % t == t - 1) for i, t, s in zip(v, tile, sp)):
        return "seam"
    return "interior"


def elementwise_ratio(out, ref, cond, tiny=1e-300):
    """worst |out - ref| / cond and its flat index (float64 CPU tensors of one shape).  Where cond == 0 the output must equal ref: the
    ratio is then inf unless the difference is 0."""
    d = (out.double() - ref.double()).abs()
    c = cond.double()
    r = torch.where(c > 0, d / c.clamp_min(tiny), torch.where(d > 0, torch.full_like(d, float("inf")), torch.zeros_like(d)))
    r = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), r)
    k = int(torch.argmax(r.reshape(-1)))
    return float(r.reshape(-1)[k]), k


def check_elementwise(out, ref, cond, tau, tag, tile=(4, 8, 8)):
    """assert |out - ref| <= tau * cond everywhere; return (worst ratio / tau, location) for the report line"""
    out, ref, cond = (t.detach().double().cpu() for t in (out, ref, cond))
    assert out.shape == ref.shape == cond.shape, (tag, out.shape, ref.shape, cond.shape)
    r, k = elementwise_ratio(out, ref, cond)
    idx = np.unravel_index(k, tuple(out.shape))
    loc = where(idx, tuple(out.shape), tile) if out.dim() == 5 else "flat"
    assert r <= tau, (f"{tag}: |out - ref64| = {r:.3e} x cond at {tuple(int(i) for i in idx)} ({loc}), bound {tau:.3e} x cond "
                      f"(out {float(out.reshape(-1)[k]):.9g}, ref {float(ref.reshape(-1)[k]):.9g}, cond {float(cond.reshape(-1)[k]):.3e})")
    return r / tau, loc


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


# -------------------------------------------------------------------------------------------------- inputs as the step produces them


def activation(g, shape, decades=4.0):
    """ReLU-like activation: non-negative with a few small negatives (the residual sums), magnitudes spread over `decades` per element"""
    x = torch.randn(shape, generator=g, dtype=torch.float64).clamp_(min=-0.25)
    return (x * torch.pow(10.0, torch.rand(shape, generator=g, dtype=torch.float64) * decades - decades / 2)).float()


def gradient(g, shape, lo=-6.0, hi=-2.0):
    """backward-sized values: signed, magnitudes 10^lo .. 10^hi per element"""
    x = torch.randn(shape, generator=g, dtype=torch.float64)
    return (x * torch.pow(10.0, lo + torch.rand(shape, generator=g, dtype=torch.float64) * (hi - lo))).float()


# -------------------------------------------------------------------------------------------------- fp64 references (channels-last)


def conv3_cl64(x, w, pad=1, chunk=8):
    """stride-1 'same' 3-D convolution of a channels-last [N, D, H, W, Cin] tensor with w [Cout, Cin, k, k, k] (or [Cout, Cin, k, k] on
    a D == 1 tensor), in fp64 on the host: the sum of k^3 shifted-view matmuls over the channels, D in chunks (no im2col)"""
    x = x.double().cpu()
    w = w.double().cpu()
    two_d = w.dim() == 4
    if two_d:
        w = w.unsqueeze(2)
    N, D, H, W, Ci = x.shape
    Co, _, kd, kh, kw = w.shape
    pd = (kd - 1) // 2
    ph, pw = (kh - 1) // 2, (kw - 1) // 2
    xp = torch.nn.functional.pad(x, (0, 0, pw, pw, ph, ph, pd, pd))
    wt = w.permute(2, 3, 4, 1, 0).contiguous()        # [kd, kh, kw, Ci, Co]
    y = torch.zeros(N, D, H, W, Co, dtype=torch.float64)
    for d0 in range(0, D, chunk):
        d1 = min(D, d0 + chunk)
        acc = y[:, d0:d1]
        for a in range(kd):
            for b in range(kh):
                for c in range(kw):
                    acc += xp[:, d0 + a:d1 + a, b:b + H, c:c + W, :] @ wt[a, b, c]
    return y


def conv3_wgrad64(x, dy, k=3, two_d=False):
    """dW[co, ci, a, b, c] = sum over voxels of dy[v, co] * x[v + (a, b, c) - 1, ci], in fp64 (channels-last operands)"""
    x, dy = x.double().cpu(), dy.double().cpu()
    N, D, H, W, Ci = x.shape
    Co = dy.shape[-1]
    p = (k - 1) // 2
    pd = 0 if two_d else p
    xp = torch.nn.functional.pad(x, (0, 0, p, p, p, p, pd, pd))
    kd = 1 if two_d else k
    g = torch.zeros(Co, Ci, kd, k, k, dtype=torch.float64)
    dyf = dy.reshape(-1, Co)
    for a in range(kd):
        for b in range(k):
            for c in range(k):
                g[:, :, a, b, c] = dyf.t() @ xp[:, a:a + D, b:b + H, c:c + W, :].reshape(-1, Ci)
    return g[:, :, 0] if two_d else g


# -------------------------------------------------------------------------------------------------- the steps' keys


def make_step(workload, dev):
    """one workload's step as bench.py builds it (configs[1] LA batch 4 / 2 labeled, ACDC 24 / 12, pancreas 4 x 96^3)"""
    from bcp_amd import synth, train_step
    seed = 1337
    np.random.seed(seed)
    if workload == "la":
        from bcp_amd.networks.net_factory import net_factory
        torch.manual_seed(seed)
        model = net_factory(net_type="VNet", in_chns=1, class_num=2, mode="train")
        ema_model = net_factory(net_type="VNet", in_chns=1, class_num=2, mode="train")
        for p in ema_model.parameters():
            p.detach_()
        ema_model.load_state_dict(model.state_dict())
        model.train(); ema_model.train()
        opt = train_step.FlatSGD(model, lr=0.01, momentum=0.9, weight_decay=1e-4)
        vol, lab = synth.la_batch(4, seed=seed)
        vol, lab = vol.to(dev), lab.to(dev)

        def step():
            return train_step.la_self_train_step(model, ema_model, opt, vol, lab, 2)
    elif workload == "acdc":
        from bcp_amd.networks.net_factory import BCP_net
        torch.manual_seed(seed)
        model, ema_model = BCP_net(in_chns=1, class_num=4), BCP_net(in_chns=1, class_num=4, ema=True)
        ema_model.load_state_dict(model.state_dict())
        model.train(); ema_model.train()
        opt = train_step.FlatSGD(model, lr=0.01, momentum=0.9, weight_decay=1e-4)
        vol, lab = synth.acdc_batch(24, seed=seed)
        vol, lab = vol.to(dev), lab.to(dev)

        def step():
            return train_step.acdc_self_train_step(model, ema_model, opt, vol, lab, 12)
    elif workload == "pancreas":
        from bcp_amd.pancreas import train_pancreas as TP
        from bcp_amd.pancreas.Vnet import create_Vnet
        torch.manual_seed(seed)
        model, ema_model = create_Vnet(), create_Vnet(ema=True)
        ema_model.load_state_dict(model.state_dict())
        opt = train_step.FlatAdam(model, lr=1e-3)
        streams = TP._streams(dev, 4, 1, seed=seed)

        def step():
            return TP.ema_cutmix(model, ema_model, opt, streams, 1)
    else:
        raise ValueError(workload)
    model.volatile_io = ema_model.volatile_io = True
    return step


def record_step_keys(workload, steps=1):
    """the set of (op, shapes, ints, namax) keys one replayed step of `workload` records under the profile hooks (two set-up steps first:
    the first records the launch plans, the second captures them -- the timed steps of bench.py are replays)"""
    from bcp_amd import plan
    from bcp_amd.hip_ops import Ops
    dev = torch.device("cuda:0")
    step = make_step(workload, dev)
    for _ in range(2):
        step()
    torch.cuda.synchronize()
    ops = Ops.product()
    plan.PROFILE, plan.PROFILE_ONLY = ops, None
    try:
        ops.profile_begin()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        recs = ops.profile_end()
    finally:
        plan.PROFILE, plan.PROFILE_ONLY = None, None
    return {(r[0], tuple(tuple(s) for s in r[1]), tuple(r[2]), int(r[4])) for r in recs}


# -------------------------------------------------------------------------------------------------- the table
# Every key one replayed step of each product workload records (LA configs[1]: batch 4, two labeled, networks grouped 2; pancreas 4 x 96^3;
# ACDC 24 slices of 256 x 256 in groups of 12).  A new shape or dispatch route changes the set: test_step_keys_in_table then fails until
# the key is added here (and, where its family has a driver below, checked).
STEP_KEYS = {
    "la": (
        ('conv3_c1_norm_bwd_wgrad', ((2, 112, 112, 80, 1), (16, 1, 3, 3, 3), (16,)), (3, 2, 1), 0),
        ('conv3_c1_norm_fwd', ((2, 112, 112, 80, 1), (16, 1, 3, 3, 3), (16,)), (3, 2, 1), 0),
        ('conv3_dgrad_bwdstats', ((2, 28, 28, 20, 64), (397344,), (2, 28, 28, 20, 64)), (64, 3, 1), 1),
        ('conv3_dgrad_bwdstats', ((2, 56, 56, 40, 32), (99360,), (2, 56, 56, 40, 32)), (32, 3, 1), 1),
        ('conv3_fwd', ((2, 112, 112, 80, 16), (24864,)), (16, 3), 1),
        ('conv3_fwd_raw', ((2, 7, 7, 5, 256), (6357024,)), (256, 3, 8), 1),
        ('conv3_fwd_raw', ((2, 14, 14, 10, 128), (1589280,)), (128, 3, 4), 1),
        ('conv3_fwd_stats', ((2, 28, 28, 20, 64), (397344,), (64,)), (64, 3, 2), 1),
        ('conv3_fwd_stats', ((2, 56, 56, 40, 32), (99360,), (32,)), (32, 3, 2), 1),
        ('conv3_fwd_stats', ((2, 112, 112, 80, 16), (24864,), (16,)), (16, 3, 2), 1),
        ('conv3_pack_many', ((800,),), (20,), 0),
        ('conv3_pack_many', ((1600,),), (40,), 0),
        ('conv3_wgrad', ((2, 7, 7, 5, 256), (2, 7, 7, 5, 256), (256, 256, 3, 3, 3)), (3,), 2),
        ('conv3_wgrad', ((2, 14, 14, 10, 128), (2, 14, 14, 10, 128), (128, 128, 3, 3, 3)), (3,), 2),
        ('conv3_wgrad', ((2, 28, 28, 20, 64), (2, 28, 28, 20, 64), (64, 64, 3, 3, 3)), (3,), 2),
        ('conv3_wgrad', ((2, 56, 56, 40, 32), (2, 56, 56, 40, 32), (32, 32, 3, 3, 3)), (3,), 2),
        ('conv3_wgrad', ((2, 112, 112, 80, 16), (2, 112, 112, 80, 16), (16, 16, 3, 3, 3)), (3,), 2),
        ('down_dgrad', ((2, 7, 7, 5, 256), (262144,)), (128,), 1),
        ('down_dgrad', ((2, 14, 14, 10, 128), (65536,)), (64,), 1),
        ('down_dgrad', ((2, 28, 28, 20, 64), (16384,)), (32,), 1),
        ('down_dgrad', ((2, 56, 56, 40, 32), (4096,)), (16,), 1),
        ('down_fwd', ((2, 14, 14, 10, 128), (262144,), (256,)), (256,), 1),
        ('down_fwd', ((2, 28, 28, 20, 64), (65536,), (128,)), (128,), 1),
        ('down_fwd', ((2, 56, 56, 40, 32), (16384,), (64,)), (64,), 1),
        ('down_fwd', ((2, 112, 112, 80, 16), (4096,), (32,)), (32,), 1),
        ('ema', ((9457332,), (9457332,)), (), 0),
        ('k2_fwd_stats', ((2, 56, 56, 40, 32), (4096,), (16,)), (1, 16, 2), 1),
        ('k2_pack_many', ((512,),), (8,), 0),
        ('k2_pack_many', ((1024,),), (16,), 0),
        ('k2_wgrad', ((2, 7, 7, 5, 256), (2, 14, 14, 10, 128), (256, 128, 2, 2, 2)), (1,), 2),
        ('k2_wgrad', ((2, 14, 14, 10, 128), (2, 7, 7, 5, 256), (256, 128, 2, 2, 2)), (0,), 2),
        ('k2_wgrad', ((2, 14, 14, 10, 128), (2, 28, 28, 20, 64), (128, 64, 2, 2, 2)), (1,), 2),
        ('k2_wgrad', ((2, 28, 28, 20, 64), (2, 14, 14, 10, 128), (128, 64, 2, 2, 2)), (0,), 2),
        ('k2_wgrad', ((2, 28, 28, 20, 64), (2, 56, 56, 40, 32), (64, 32, 2, 2, 2)), (1,), 2),
        ('k2_wgrad', ((2, 56, 56, 40, 32), (2, 28, 28, 20, 64), (64, 32, 2, 2, 2)), (0,), 2),
        ('k2_wgrad', ((2, 56, 56, 40, 32), (2, 112, 112, 80, 16), (32, 16, 2, 2, 2)), (1,), 2),
        ('k2_wgrad', ((2, 112, 112, 80, 16), (2, 56, 56, 40, 32), (32, 16, 2, 2, 2)), (0,), 2),
        ('mix_box', ((1, 112, 112, 80, 1), (1, 112, 112, 80, 1)), (), 0),
        ('mixloss_pair_bwd', ((2, 112, 112, 80, 2), (1, 112, 112, 80), (1, 112, 112, 80)), (0,), 0),
        ('mixloss_pair_fwd', ((2, 112, 112, 80, 2), (1, 112, 112, 80), (1, 112, 112, 80)), (0,), 0),
        ('norm_bwd', ((2, 7, 7, 5, 256), (2, 7, 7, 5, 256), (5, 2, 256)), (2, 1, True), 0),
        ('norm_bwd', ((2, 14, 14, 10, 128), (2, 14, 14, 10, 128), (5, 2, 128)), (2, 1, True), 0),
        ('norm_bwd', ((2, 28, 28, 20, 64), (2, 28, 28, 20, 64), (5, 2, 64)), (2, 1, True), 0),
        ('norm_bwd', ((2, 56, 56, 40, 32), (2, 56, 56, 40, 32), (5, 2, 32)), (2, 1, True), 0),
        ('norm_bwd', ((2, 112, 112, 80, 16), (2, 112, 112, 80, 16), (5, 2, 16)), (2, 1, True), 0),
        ('norm_bwd_slabs', ((2, 7, 7, 5, 256), (8, 2, 7, 7, 5, 256), (5, 2, 256)), (8, 2, 1), 0),
        ('norm_bwd_slabs', ((2, 14, 14, 10, 128), (4, 2, 14, 14, 10, 128), (5, 2, 128)), (4, 2, 1), 0),
        ('norm_fwd', ((2, 7, 7, 5, 256), (256,), (256,)), (2, 1), 0),
        ('norm_fwd', ((2, 14, 14, 10, 128), (128,), (128,)), (2, 1), 0),
        ('norm_fwd', ((2, 28, 28, 20, 64), (64,), (64,)), (2, 1), 0),
        ('norm_fwd', ((2, 56, 56, 40, 32), (32,), (32,)), (2, 1), 0),
        ('norm_fwd', ((2, 112, 112, 80, 16), (16,), (16,)), (2, 1), 0),
        ('norm_fwd_slabs', ((4, 2, 14, 14, 10, 128), (128,), (128,)), (4, 2, 1), 0),
        ('norm_fwd_slabs', ((8, 2, 7, 7, 5, 256), (256,), (256,)), (8, 2, 1), 0),
        ('plabel_cc_largest', ((2, 112, 112, 80, 2),), (3,), 0),
        ('pw16_bwd_norm_bwd', ((2, 112, 112, 80, 16), (5, 2, 16), (2, 16)), (2, 1), 0),
        ('pw16_fwd_norm', ((2, 112, 112, 80, 16), (5, 2, 16), (2, 16)), (2, 1, 2), 0),
        ('sgd', ((9448868,), (9448868,), (9448868,)), (), 0),
        ('up_dgrad', ((2, 14, 14, 10, 128), (262144,)), (256,), 1),
        ('up_dgrad', ((2, 28, 28, 20, 64), (65536,)), (128,), 1),
        ('up_dgrad', ((2, 56, 56, 40, 32), (16384,)), (64,), 1),
        ('up_dgrad', ((2, 112, 112, 80, 16), (4096,)), (32,), 1),
        ('up_fwd', ((2, 7, 7, 5, 256), (262144,), (128,)), (128,), 1),
        ('up_fwd', ((2, 14, 14, 10, 128), (65536,), (64,)), (64,), 1),
        ('up_fwd', ((2, 28, 28, 20, 64), (16384,), (32,)), (32,), 1),
    ),
    "pancreas": (
        ('adam', ((9443268,), (9443268,), (9443268,)), (3,), 0),
        ('conv3_c1_norm_bwd_wgrad', ((2, 96, 96, 96, 1), (16, 1, 3, 3, 3), (16,)), (3, 2, 1), 0),
        ('conv3_c1_norm_fwd', ((2, 96, 96, 96, 1), (16, 1, 3, 3, 3), (16,)), (3, 2, 1), 0),
        ('conv3_dgrad_bwdstats', ((2, 24, 24, 24, 64), (397344,), (2, 24, 24, 24, 64)), (64, 3, 1), 1),
        ('conv3_dgrad_bwdstats', ((2, 48, 48, 48, 32), (99360,), (2, 48, 48, 48, 32)), (32, 3, 1), 1),
        ('conv3_fwd', ((2, 96, 96, 96, 16), (24864,)), (16, 3), 1),
        ('conv3_fwd_raw', ((2, 6, 6, 6, 256), (6357024,)), (256, 3, 8), 1),
        ('conv3_fwd_raw', ((2, 12, 12, 12, 128), (1589280,)), (128, 3, 4), 1),
        ('conv3_fwd_stats', ((2, 24, 24, 24, 64), (397344,), (64,)), (64, 3, 2), 1),
        ('conv3_fwd_stats', ((2, 48, 48, 48, 32), (99360,), (32,)), (32, 3, 2), 1),
        ('conv3_fwd_stats', ((2, 96, 96, 96, 16), (24864,), (16,)), (16, 3, 2), 1),
        ('conv3_pack_many', ((800,),), (20,), 0),
        ('conv3_pack_many', ((1600,),), (40,), 0),
        ('conv3_wgrad', ((2, 6, 6, 6, 256), (2, 6, 6, 6, 256), (256, 256, 3, 3, 3)), (3,), 2),
        ('conv3_wgrad', ((2, 12, 12, 12, 128), (2, 12, 12, 12, 128), (128, 128, 3, 3, 3)), (3,), 2),
        ('conv3_wgrad', ((2, 24, 24, 24, 64), (2, 24, 24, 24, 64), (64, 64, 3, 3, 3)), (3,), 2),
        ('conv3_wgrad', ((2, 48, 48, 48, 32), (2, 48, 48, 48, 32), (32, 32, 3, 3, 3)), (3,), 2),
        ('conv3_wgrad', ((2, 96, 96, 96, 16), (2, 96, 96, 96, 16), (16, 16, 3, 3, 3)), (3,), 2),
        ('down_dgrad', ((2, 6, 6, 6, 256), (262144,)), (128,), 1),
        ('down_dgrad', ((2, 12, 12, 12, 128), (65536,)), (64,), 1),
        ('down_dgrad', ((2, 24, 24, 24, 64), (16384,)), (32,), 1),
        ('down_dgrad', ((2, 48, 48, 48, 32), (4096,)), (16,), 1),
        ('down_fwd', ((2, 12, 12, 12, 128), (262144,), (256,)), (256,), 1),
        ('down_fwd', ((2, 24, 24, 24, 64), (65536,), (128,)), (128,), 1),
        ('down_fwd', ((2, 48, 48, 48, 32), (16384,), (64,)), (64,), 1),
        ('down_fwd', ((2, 96, 96, 96, 16), (4096,), (32,)), (32,), 1),
        ('ema', ((9443268,), (9443268,)), (), 0),
        ('k2_fwd_stats', ((2, 48, 48, 48, 32), (4096,), (16,)), (1, 16, 2), 1),
        ('k2_pack_many', ((512,),), (8,), 0),
        ('k2_pack_many', ((1024,),), (16,), 0),
        ('k2_wgrad', ((2, 6, 6, 6, 256), (2, 12, 12, 12, 128), (256, 128, 2, 2, 2)), (1,), 2),
        ('k2_wgrad', ((2, 12, 12, 12, 128), (2, 6, 6, 6, 256), (256, 128, 2, 2, 2)), (0,), 2),
        ('k2_wgrad', ((2, 12, 12, 12, 128), (2, 24, 24, 24, 64), (128, 64, 2, 2, 2)), (1,), 2),
        ('k2_wgrad', ((2, 24, 24, 24, 64), (2, 12, 12, 12, 128), (128, 64, 2, 2, 2)), (0,), 2),
        ('k2_wgrad', ((2, 24, 24, 24, 64), (2, 48, 48, 48, 32), (64, 32, 2, 2, 2)), (1,), 2),
        ('k2_wgrad', ((2, 48, 48, 48, 32), (2, 24, 24, 24, 64), (64, 32, 2, 2, 2)), (0,), 2),
        ('k2_wgrad', ((2, 48, 48, 48, 32), (2, 96, 96, 96, 16), (32, 16, 2, 2, 2)), (1,), 2),
        ('k2_wgrad', ((2, 96, 96, 96, 16), (2, 48, 48, 48, 32), (32, 16, 2, 2, 2)), (0,), 2),
        ('mix_box', ((1, 96, 96, 96, 1), (1, 96, 96, 96, 1)), (), 0),
        ('mixloss_pair_bwd', ((2, 96, 96, 96, 2), (1, 96, 96, 96), (1, 96, 96, 96)), (0,), 0),
        ('mixloss_pair_fwd', ((2, 96, 96, 96, 2), (1, 96, 96, 96), (1, 96, 96, 96)), (0,), 0),
        ('norm_bwd', ((2, 6, 6, 6, 256), (2, 6, 6, 6, 256), (5, 2, 256)), (2, 1, False), 0),
        ('norm_bwd', ((2, 12, 12, 12, 128), (2, 12, 12, 12, 128), (5, 2, 128)), (2, 1, False), 0),
        ('norm_bwd', ((2, 24, 24, 24, 64), (2, 24, 24, 24, 64), (5, 2, 64)), (2, 1, False), 0),
        ('norm_bwd', ((2, 48, 48, 48, 32), (2, 48, 48, 48, 32), (5, 2, 32)), (2, 1, False), 0),
        ('norm_bwd', ((2, 96, 96, 96, 16), (2, 96, 96, 96, 16), (5, 2, 16)), (2, 1, False), 0),
        ('norm_bwd_slabs', ((2, 6, 6, 6, 256), (8, 2, 6, 6, 6, 256), (5, 2, 256)), (8, 2, 1), 0),
        ('norm_bwd_slabs', ((2, 12, 12, 12, 128), (4, 2, 12, 12, 12, 128), (5, 2, 128)), (4, 2, 1), 0),
        ('norm_fwd', ((2, 6, 6, 6, 256),), (2, 1), 0),
        ('norm_fwd', ((2, 12, 12, 12, 128),), (2, 1), 0),
        ('norm_fwd', ((2, 24, 24, 24, 64),), (2, 1), 0),
        ('norm_fwd', ((2, 48, 48, 48, 32),), (2, 1), 0),
        ('norm_fwd', ((2, 96, 96, 96, 16),), (2, 1), 0),
        ('norm_fwd_slabs', ((4, 2, 12, 12, 12, 128), (128,)), (4, 2, 1), 0),
        ('norm_fwd_slabs', ((8, 2, 6, 6, 6, 256), (256,)), (8, 2, 1), 0),
        ('plabel_cc_largest', ((2, 96, 96, 96, 2),), (2,), 0),
        ('pw16_bwd_norm_bwd', ((2, 96, 96, 96, 16), (5, 2, 16), (2, 96, 96, 96, 2)), (2, 1), 0),
        ('pw16_fwd_norm', ((2, 96, 96, 96, 16), (5, 2, 16), (2, 16, 1, 1, 1)), (2, 1, 2), 0),
        ('up_dgrad', ((2, 12, 12, 12, 128), (262144,)), (256,), 1),
        ('up_dgrad', ((2, 24, 24, 24, 64), (65536,)), (128,), 1),
        ('up_dgrad', ((2, 48, 48, 48, 32), (16384,)), (64,), 1),
        ('up_dgrad', ((2, 96, 96, 96, 16), (4096,)), (32,), 1),
        ('up_fwd', ((2, 6, 6, 6, 256), (262144,), (128,)), (128,), 1),
        ('up_fwd', ((2, 12, 12, 12, 128), (65536,), (64,)), (64,), 1),
        ('up_fwd', ((2, 24, 24, 24, 64), (16384,), (32,)), (32,), 1),
    ),
    "acdc": (
        ('bilinear2x_bwd', ((12, 1, 32, 32, 256),), (128, 128), 0),
        ('bilinear2x_bwd', ((12, 1, 64, 64, 128),), (64, 64), 0),
        ('bilinear2x_bwd', ((12, 1, 128, 128, 64),), (32, 32), 0),
        ('bilinear2x_bwd', ((12, 1, 256, 256, 32),), (16, 16), 0),
        ('bilinear2x_fwd', ((12, 1, 16, 16, 128), (12, 1, 32, 32, 256)), (128,), 1),
        ('bilinear2x_fwd', ((12, 1, 32, 32, 64), (12, 1, 64, 64, 128)), (64,), 1),
        ('bilinear2x_fwd', ((12, 1, 64, 64, 32), (12, 1, 128, 128, 64)), (32,), 1),
        ('bilinear2x_fwd', ((12, 1, 128, 128, 16), (12, 1, 256, 256, 32)), (16,), 1),
        ('conv3_c1_norm_bwd_wgrad', ((12, 1, 256, 256, 1), (16, 1, 3, 3), (16,)), (1, 2, 2), 0),
        ('conv3_c1_norm_fwd', ((12, 1, 256, 256, 1), (16, 1, 3, 3), (16,)), (1, 2, 2), 0),
        ('conv3_dgrad_bwdstats', ((12, 1, 128, 128, 32), (34848,), (12, 1, 128, 128, 32)), (32, 1, 2), 1),
        ('conv3_fwd', ((12, 1, 16, 16, 256), (1114144,)), (128, 1), 1),
        ('conv3_fwd', ((12, 1, 32, 32, 128), (278560,)), (64, 1), 1),
        ('conv3_fwd', ((12, 1, 32, 32, 128), (557088,)), (128, 1), 1),
        ('conv3_fwd', ((12, 1, 32, 32, 128), (1114144,)), (256, 1), 1),
        ('conv3_fwd', ((12, 1, 64, 64, 64), (69664,)), (32, 1), 1),
        ('conv3_fwd', ((12, 1, 64, 64, 64), (139296,)), (64, 1), 1),
        ('conv3_fwd', ((12, 1, 64, 64, 64), (278560,)), (128, 1), 1),
        ('conv3_fwd', ((12, 1, 128, 128, 32), (17440,)), (16, 1), 1),
        ('conv3_fwd', ((12, 1, 128, 128, 32), (34848,)), (32, 1), 1),
        ('conv3_fwd', ((12, 1, 128, 128, 32), (69664,)), (64, 1), 1),
        ('conv3_fwd', ((12, 1, 256, 256, 4), (8736,)), (16, 1), 0),
        ('conv3_fwd', ((12, 1, 256, 256, 16), (8736,)), (16, 1), 1),
        ('conv3_fwd', ((12, 1, 256, 256, 16), (8736,), (4,)), (4, 1), 1),
        ('conv3_fwd', ((12, 1, 256, 256, 16), (17440,)), (32, 1), 1),
        ('conv3_fwd_raw', ((12, 1, 16, 16, 128), (1114144,)), (256, 1, 4), 1),
        ('conv3_fwd_raw', ((12, 1, 16, 16, 256), (2228256,)), (256, 1, 4), 1),
        ('conv3_fwd_stats', ((12, 1, 32, 32, 64), (278560,), (128,)), (128, 1, 2), 1),
        ('conv3_fwd_stats', ((12, 1, 32, 32, 128), (557088,), (128,)), (128, 1, 2), 1),
        ('conv3_fwd_stats', ((12, 1, 32, 32, 256), (1114144,), (128,)), (128, 1, 2), 1),
        ('conv3_fwd_stats', ((12, 1, 64, 64, 32), (69664,), (64,)), (64, 1, 2), 1),
        ('conv3_fwd_stats', ((12, 1, 64, 64, 64), (139296,), (64,)), (64, 1, 2), 1),
        ('conv3_fwd_stats', ((12, 1, 64, 64, 128), (278560,), (64,)), (64, 1, 2), 1),
        ('conv3_fwd_stats', ((12, 1, 128, 128, 16), (17440,), (32,)), (32, 1, 2), 1),
        ('conv3_fwd_stats', ((12, 1, 128, 128, 32), (34848,), (32,)), (32, 1, 2), 1),
        ('conv3_fwd_stats', ((12, 1, 128, 128, 64), (69664,), (32,)), (32, 1, 2), 1),
        ('conv3_fwd_stats', ((12, 1, 256, 256, 16), (8736,), (16,)), (16, 1, 2), 1),
        ('conv3_fwd_stats', ((12, 1, 256, 256, 32), (17440,), (16,)), (16, 1, 2), 1),
        ('conv3_pack_many', ((720,),), (18,), 0),
        ('conv3_pack_many', ((1440,),), (36,), 0),
        ('conv3_wgrad', ((12, 1, 16, 16, 128), (12, 1, 16, 16, 256), (256, 128, 3, 3)), (1,), 2),
        ('conv3_wgrad', ((12, 1, 16, 16, 256), (12, 1, 16, 16, 256), (256, 256, 3, 3)), (1,), 2),
        ('conv3_wgrad', ((12, 1, 32, 32, 64), (12, 1, 32, 32, 128), (128, 64, 3, 3)), (1,), 2),
        ('conv3_wgrad', ((12, 1, 32, 32, 128), (12, 1, 32, 32, 128), (128, 128, 3, 3)), (1,), 2),
        ('conv3_wgrad', ((12, 1, 32, 32, 256), (12, 1, 32, 32, 128), (128, 256, 3, 3)), (1,), 2),
        ('conv3_wgrad', ((12, 1, 64, 64, 32), (12, 1, 64, 64, 64), (64, 32, 3, 3)), (1,), 2),
        ('conv3_wgrad', ((12, 1, 64, 64, 64), (12, 1, 64, 64, 64), (64, 64, 3, 3)), (1,), 2),
        ('conv3_wgrad', ((12, 1, 64, 64, 128), (12, 1, 64, 64, 64), (64, 128, 3, 3)), (1,), 2),
        ('conv3_wgrad', ((12, 1, 128, 128, 16), (12, 1, 128, 128, 32), (32, 16, 3, 3)), (1,), 2),
        ('conv3_wgrad', ((12, 1, 128, 128, 32), (12, 1, 128, 128, 32), (32, 32, 3, 3)), (1,), 2),
        ('conv3_wgrad', ((12, 1, 128, 128, 64), (12, 1, 128, 128, 32), (32, 64, 3, 3)), (1,), 2),
        ('conv3_wgrad', ((12, 1, 256, 256, 16), (12, 1, 256, 256, 4), (4, 16, 3, 3)), (1,), 1),
        ('conv3_wgrad', ((12, 1, 256, 256, 16), (12, 1, 256, 256, 16), (16, 16, 3, 3)), (1,), 2),
        ('conv3_wgrad', ((12, 1, 256, 256, 32), (12, 1, 256, 256, 16), (16, 32, 3, 3)), (1,), 2),
        ('ema', ((1830436,), (1830436,)), (), 0),
        ('k2_pack_many', ((256,),), (4,), 0),
        ('k2_pack_many', ((512,),), (8,), 0),
        ('k2_wgrad', ((12, 1, 16, 16, 256), (12, 1, 16, 16, 128), (128, 256, 1, 1)), (2,), 1),
        ('k2_wgrad', ((12, 1, 32, 32, 128), (12, 1, 32, 32, 64), (64, 128, 1, 1)), (2,), 1),
        ('k2_wgrad', ((12, 1, 64, 64, 64), (12, 1, 64, 64, 32), (32, 64, 1, 1)), (2,), 1),
        ('k2_wgrad', ((12, 1, 128, 128, 32), (12, 1, 128, 128, 16), (16, 32, 1, 1)), (2,), 1),
        ('maxpool2d_bwd', ((12, 1, 32, 32, 128), (12, 1, 16, 16, 128), (12, 1, 32, 32, 128)), (), 1),
        ('maxpool2d_bwd', ((12, 1, 64, 64, 64), (12, 1, 32, 32, 64), (12, 1, 64, 64, 64)), (), 1),
        ('maxpool2d_bwd', ((12, 1, 128, 128, 32), (12, 1, 64, 64, 32), (12, 1, 128, 128, 32)), (), 1),
        ('maxpool2d_bwd', ((12, 1, 256, 256, 16), (12, 1, 128, 128, 16), (12, 1, 256, 256, 16)), (), 1),
        ('maxpool2d_fwd', ((12, 1, 32, 32, 128),), (), 1),
        ('maxpool2d_fwd', ((12, 1, 64, 64, 64),), (), 1),
        ('maxpool2d_fwd', ((12, 1, 128, 128, 32),), (), 1),
        ('maxpool2d_fwd', ((12, 1, 256, 256, 16),), (), 1),
        ('mix_box', ((6, 1, 256, 256, 1), (6, 1, 256, 256, 1)), (), 0),
        ('mixloss_pair_bwd', ((12, 1, 256, 256, 4), (6, 1, 256, 256), (6, 1, 256, 256)), (1,), 0),
        ('mixloss_pair_fwd', ((12, 1, 256, 256, 4), (6, 1, 256, 256), (6, 1, 256, 256)), (1,), 0),
        ('norm_bwd', ((12, 1, 16, 16, 256), (12, 1, 16, 16, 256), (5, 2, 256)), (2, 2, True), 0),
        ('norm_bwd', ((12, 1, 32, 32, 128), (12, 1, 32, 32, 128), (5, 2, 128)), (2, 2, True), 0),
        ('norm_bwd', ((12, 1, 64, 64, 64), (12, 1, 64, 64, 64), (5, 2, 64)), (2, 2, True), 0),
        ('norm_bwd', ((12, 1, 128, 128, 32), (12, 1, 128, 128, 32), (5, 2, 32)), (2, 2, True), 0),
        ('norm_bwd', ((12, 1, 256, 256, 16), (12, 1, 256, 256, 16), (5, 2, 16)), (2, 2, True), 0),
        ('norm_bwd_slabs', ((12, 1, 16, 16, 256), (4, 12, 1, 16, 16, 256), (5, 2, 256)), (4, 2, 2), 0),
        ('norm_fwd', ((12, 1, 32, 32, 128), (128,), (128,)), (2, 2), 0),
        ('norm_fwd', ((12, 1, 64, 64, 64), (64,), (64,)), (2, 2), 0),
        ('norm_fwd', ((12, 1, 128, 128, 32), (32,), (32,)), (2, 2), 0),
        ('norm_fwd', ((12, 1, 256, 256, 16), (16,), (16,)), (2, 2), 0),
        ('norm_fwd_slabs', ((4, 12, 1, 16, 16, 256), (256,), (256,)), (4, 2, 2), 0),
        ('plabel_cc_largest', ((12, 1, 256, 256, 4),), (2,), 0),
        ('pw_fwd', ((12, 1, 16, 16, 128), (32768,)), (256,), 0),
        ('pw_fwd', ((12, 1, 16, 16, 256), (32768,), (128,)), (128,), 1),
        ('pw_fwd', ((12, 1, 32, 32, 64), (8192,)), (128,), 0),
        ('pw_fwd', ((12, 1, 32, 32, 128), (8192,), (64,)), (64,), 1),
        ('pw_fwd', ((12, 1, 64, 64, 32), (2048,)), (64,), 0),
        ('pw_fwd', ((12, 1, 64, 64, 64), (2048,), (32,)), (32,), 1),
        ('pw_fwd', ((12, 1, 128, 128, 16), (512,)), (32,), 0),
        ('pw_fwd', ((12, 1, 128, 128, 32), (512,), (16,)), (16,), 1),
        ('sgd', ((1813764,), (1813764,), (1813764,)), (), 0),
    ),
}

TAU = 2.0 ** -14            # elementwise bound for convolutions, GEMMs and norms: |out - ref64| <= TAU * cond
TAU_OPT = 2.0 ** -22        # optimiser / EMA updates: |out - ref64| <= TAU_OPT * (|p| + |update|)
TAU_ADAM = 2.0 ** -21       # Adam's update goes through six fp32 roundings (sqrt, / bc2, + eps, m / den, lr / bc1, the product): up to
                            # ~6 * 2^-24 of |update|; 1.3 * 2^-22 measured on the device and on the simulator (correctly rounded host math)
STEP_GROUPS = 2             # every product step runs its networks grouped 2 (norm statistics per group of samples)
EPS = 1e-5


def _acts(act, z):
    if act == 1:
        return torch.relu(z), (z > 0).double()
    if act == 2:
        return torch.nn.functional.leaky_relu(z, 0.01), torch.where(z > 0, 1.0, 0.01).double()
    return z, torch.ones_like(z)


def _amax(H, t, dev):
    t._bcp_amax = H.amax_slots(float(t.abs().max()), dev)
    return t


def _conv_weight(g, Cout, Cin, KD):
    k = (3, 3, 3) if KD == 3 else (3, 3)
    return (torch.randn((Cout, Cin) + k, generator=g, dtype=torch.float64) * (2.0 / (Cin * 9 * KD)) ** 0.5).float()


def _pre_norm(g, shape):
    """a conv output as a norm layer sees it: per-channel offset and scale spread over three decades, signed"""
    C = shape[-1]
    sc = torch.pow(10.0, torch.rand(C, generator=g, dtype=torch.float64) * 3 - 1.5)
    off = torch.randn(C, generator=g, dtype=torch.float64) * sc
    return (torch.randn(shape, generator=g, dtype=torch.float64) * sc + off).float()


def drive_conv(ops, dev, key, g):
    """conv3_fwd / conv3_fwd_stats / conv3_fwd_raw / conv3_dgrad_bwdstats: the output against sum over 27 (9) shifted matmuls in fp64"""
    from bcp_amd import hip_ops as H
    op, shapes, ints, namax = key
    xs = shapes[0]
    two_d = ints[1] == 1
    KD = ints[1]
    Cx = xs[-1]
    out = []
    if op == "conv3_dgrad_bwdstats":
        Cin = ints[0]
        w = _conv_weight(g, Cx, Cin, KD)              # the forward layer maps Cin -> Cx; the launch takes dy (Cx channels) to da (Cin)
        x = gradient(g, xs)
        wf, wd = ops.conv3_pack(w.to(dev), KD)
        xd = x.to(dev)
        if namax:
            _amax(H, xd, dev)
        yp = _pre_norm(g, shapes[2]).to(dev)
        act, Gn = ints[2], STEP_GROUPS       # (the key's ints are Cin, KD, act: the groups argument comes fourth)
        C = yp.shape[-1]
        gam = (torch.rand(C, generator=g) + 0.5).to(dev)
        bet = (torch.rand(C, generator=g) - 0.5).to(dev)
        _, st = ops.norm_fwd(yp, Gn, gam, bet, torch.zeros(C, device=dev), torch.ones(C, device=dev), act)
        res, part, rows = ops.conv3_dgrad_bwdstats(xd, wd, Cin, KD, yp, st, act, Gn)
        assert rows > 0 or dev.type == "cpu", f"{op} {xs}: no fused backward statistics at the step's shape"
        if rows:
            # the epilogue's (sum dz, sum dz * xhat) partials of the norm layer behind: fp64 sums of the kernel's own da
            _, z, xh, _, _, fcond = norm_ref64(yp.cpu(), Gn, gam.cpu(), bet.cpu(), act)
            dact = _acts(act, z)[1]
            da64 = res.cpu().double()
            dz, xg = (da64 * dact).reshape(Gn, -1, C), xh.reshape(Gn, -1, C)
            dk = (da64 * _kink(z, fcond)).abs().reshape(Gn, -1, C)
            ps = _partials(part, Gn, rows, C)
            for j, (s_, c, k) in enumerate(((dz.sum(1), dz.abs().sum(1), dk.sum(1)),
                                            ((dz * xg).sum(1), (dz * xg).abs().sum(1), (dk * xg.abs()).sum(1)))):
                err = ((ps[..., j] - s_).abs() - k).clamp_min(0)
                r, _ = elementwise_ratio(err, torch.zeros_like(err), c)
                assert r <= TAU, f"{op} {xs}: backward-statistics partial {j} off by {r:.3e} x sum|.|"
        wk = w.double().flip(*(range(2, w.dim()))).transpose(0, 1)
    else:
        Cout = ints[0]
        w = _conv_weight(g, Cout, Cx, KD)
        x = activation(g, xs)
        wf, wd = ops.conv3_pack(w.to(dev), KD)
        xd = x.to(dev)
        if namax:
            _amax(H, xd, dev)
        has_b = op in ("conv3_fwd", "conv3_fwd_stats") and len(shapes) > 2
        b = (torch.randn(Cout, generator=g) * 0.1).to(dev) if has_b else None
        if op == "conv3_fwd":
            res = ops.conv3_fwd(xd, wf, b, Cout, KD)
        elif op == "conv3_fwd_stats":
            res, part, rows = ops.conv3_fwd_stats(xd, wf, b, Cout, KD, ints[2])
            assert rows > 0 or dev.type == "cpu", f"{op} {xs}: no fused statistics at the step's shape"
        elif op == "conv3_fwd_raw":
            nsl = ops.conv3_nslabs(xs, Cout, KD)          # (ints[2] at the in-step shape; the reduced simulator shapes may not be served raw)
            assert nsl == ints[2] or dev.type == "cpu", f"{op} {xs}: {nsl} split-K slabs, the step launches {ints[2]}"
            res = ops.conv3_fwd_raw(xd, wf, Cout, KD, nsl).double().sum(0) if nsl else ops.conv3_fwd(xd, wf, None, Cout, KD)
        else:
            raise KeyError(op)
        wk = w.double()
    xc = x.double()
    if two_d:
        wk = wk.reshape(wk.shape[0], wk.shape[1], 3, 3)
    ref = conv3_cl64(xc, wk)
    cond = conv3_cl64(xc.abs(), wk.abs())
    if op in ("conv3_fwd", "conv3_fwd_stats") and b is not None:
        ref += b.double().cpu()
        cond += b.double().cpu().abs()
    tile = (1, 16, 16) if two_d else (4, 8, 8)
    rc = res.cpu()
    out.append((op, check_elementwise(rc, ref, cond, TAU, f"{op} {xs}", tile)))
    if op == "conv3_fwd_stats" and rows:
        # the fused statistics partials: fp64 column sums / sums of squares of the kernel's own output, per group
        Gn = ints[2]
        pt = torch.frombuffer(bytearray(part.cpu().numpy().tobytes()[:Gn * rows * Cout * 16]), dtype=torch.float64).view(Gn, rows, Cout, 2).sum(1)
        yg = rc.double().reshape(Gn, -1, Cout)
        for j, (s, c) in enumerate(((yg.sum(1), yg.abs().sum(1)), ((yg * yg).sum(1), (yg * yg).sum(1)))):
            r = float(((pt[..., j] - s).abs() / c.clamp_min(1e-300)).max())
            assert r <= 1e-12, f"{op} {xs}: fused statistics partial {j} off by {r:.3e} x sum|.|"
    return out


def norm_ref64(y, G, gamma, beta, act, eps=EPS):
    """fp64 grouped BatchNorm (G groups of consecutive samples) / InstanceNorm (gamma None, G == N) -> (a, z, xhat, mean, var, cond)"""
    y = y.double().cpu()
    C = y.shape[-1]
    yg = y.reshape(G, -1, C)
    mu = yg.mean(1, keepdim=True)
    var = ((yg - mu) ** 2).mean(1, keepdim=True)
    xh = (yg - mu) / torch.sqrt(var + eps)
    gm = torch.ones(C, dtype=torch.float64) if gamma is None else gamma.double().cpu()
    bt = torch.zeros(C, dtype=torch.float64) if beta is None else beta.double().cpu()
    z = gm * xh + bt
    a, _ = _acts(act, z)
    cond = gm.abs() * (xh.abs() + 1) + bt.abs()
    return a.reshape(y.shape), z.reshape(y.shape), xh.reshape(y.shape), mu, var, cond.reshape(y.shape)


def _epilogue(ops, dev, g, ys, flags):
    """the step's apply-pass epilogue inputs for `flags`: (chan_scale | None, SeedMask | None, its keep bits as float64 | None,
    elem_scale, residual | None) -- Dropout3d channel scales {0, 2}, an elementwise dropout mask evaluated from a seed (p 0.5)"""
    from bcp_amd import hip_ops as H
    N, C = ys[0], ys[-1]
    cs = ((torch.rand(N, C, generator=g) < 0.5).float() * 2.0) if "chan_scale" in flags else None
    sm = m64 = None
    es = 1.0
    if "elem_mask" in flags:
        seed = int(torch.randint(1, 1 << 62, (1,), generator=g))
        like = torch.empty(1, device=dev)
        sm = ops.seed_mask(tuple(ys), 0.5, seed, like)
        m64 = ops.bernoulli(torch.empty(tuple(ys), dtype=torch.uint8, device=dev), 0.5, 1.0, seed).cpu().double()
        es = 2.0
    res = activation(g, ys) if "residual" in flags else None
    mult = torch.ones(ys, dtype=torch.float64)
    if cs is not None:
        mult = mult * cs.double().view(N, *([1] * (len(ys) - 2)), C)
    if m64 is not None:
        mult = mult * m64 * es
    return cs, sm, es, res, mult, H


def _conv_partial_source(ops, dev, g, ys, G, fwd=True, yprev=None, stats=None, act=1):
    """a conv launch of the step's kind producing a tensor of shape ys WITH its fused statistics partials: conv3_fwd_stats (fwd) or
    conv3_dgrad_bwdstats (bwd, against the norm layer (yprev, stats)).  -> (tensor, partial, rows); rows == 0 where the route does not
    fuse the statistics at this shape (the simulator's reduced shapes only: on the device the caller asserts rows > 0)"""
    from bcp_amd import hip_ops as H
    C = ys[-1]
    KD = 1 if ys[1] == 1 else 3
    w = _conv_weight(g, C, C, KD)
    wf, wd = ops.conv3_pack(w.to(dev), KD)
    if fwd:
        x = _amax(H, activation(g, ys).to(dev), dev)
        return ops.conv3_fwd_stats(x, wf, (torch.randn(C, generator=g) * 0.1).to(dev), C, KD, G)
    dy = _amax(H, gradient(g, ys).to(dev), dev)
    return ops.conv3_dgrad_bwdstats(dy, wd, C, KD, yprev, stats, act, G)


def _partials(part, G, rows, C):
    """[G][rows][C][2] fp64 partial rows -> their sums per (group, channel): [G, C, 2]"""
    return torch.frombuffer(bytearray(part.cpu().numpy().tobytes()[:G * rows * C * 16]), dtype=torch.float64).view(G, rows, C, 2).sum(1)


def _stats_check(st, mu, var, tag):
    """stats[5][G][C] {mean, rstd, ...} against fp64: mean to TAU * sqrt(var) (the spread it is measured against), rstd relative"""
    m = st[0].double().cpu()
    r = st[1].double().cpu()
    mu, var = mu[:, 0], var[:, 0]
    em = float(((m - mu).abs() / var.sqrt().clamp_min(1e-300)).max())
    er = float(((r - 1 / (var + EPS).sqrt()).abs() * (var + EPS).sqrt()).max())
    assert em <= TAU and er <= TAU, f"{tag}: statistics off (mean {em:.3e}, rstd {er:.3e})"


def drive_norm_fwd(ops, dev, key, g, variants=((),)):
    """norm_fwd with each epilogue the step uses at this key (STEP_VARIANTS): statistics from a real conv3_fwd_stats launch's fused
    partials, channel scale, seeded elementwise dropout, residual, statistics only, a concat-buffer slab as output; ReLU (V-Net) /
    LeakyReLU (U-Net); BatchNorm with running statistics or InstanceNorm"""
    op, shapes, ints, namax = key
    ys = shapes[0]
    G, act = ints[0], ints[1]
    C = ys[-1]
    out = []
    for flags in variants:
        tag = f"{op} {ys} [{'+'.join(flags) or 'plain'}]"
        part, rows = None, 0
        if "partial" in flags:
            yd, part, rows = _conv_partial_source(ops, dev, g, ys, G)
            assert rows > 0 or dev.type == "cpu", f"{tag}: conv3_fwd_stats left no partials at the step's shape"
            y = yd.cpu()
        else:
            y = _pre_norm(g, ys)
            yd = y.to(dev)
        affine = len(shapes) > 1
        gam = (torch.rand(C, generator=g) + 0.5) if affine else None
        bet = (torch.rand(C, generator=g) - 0.5) if affine else None
        rm0, rv0 = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
        rm, rv = (rm0.clone().to(dev), rv0.clone().to(dev)) if affine else (None, None)
        cs, sm, es, res, mult, H = _epilogue(ops, dev, g, ys, flags)
        kw = dict(chan_scale=None if cs is None else cs.to(dev), elem_mask=sm, elem_scale=es, residual=None if res is None else res.to(dev))
        if rows:
            kw.update(partial=part, nb=rows)
        wide = None
        if "stats_only" in flags:
            kw = dict(chan_scale=kw["chan_scale"], stats_only=True, **({"partial": part, "nb": rows} if rows else {}))
        elif "out_slab" in flags:
            wide = torch.full(ys[:-1] + (2 * C,), 7.0, device=dev)
            kw["out"] = ops.channel_slab(wide, C)
        a, st = ops.norm_fwd(yd, G, *((gam.to(dev), bet.to(dev)) if affine else (None, None)), rm, rv, act, **kw)
        ar, z, xh, mu, var, cond = norm_ref64(y, G, gam, bet, act)
        _stats_check(st, mu, var, tag)
        if a is not None:
            ref = ar * mult + (0 if res is None else res.double())
            cnd = cond * mult.abs() + (0 if res is None else res.double().abs())
            out.append((op + ("" if not flags else " " + "+".join(flags)), check_elementwise(a.cpu(), ref, cnd, TAU, tag)))
            if wide is not None:
                assert bool((wide[..., C:] == 7.0).all()), f"{tag}: wrote outside its channel slab"
        else:
            out.append((op + " " + "+".join(flags), (0.0, "stats")))
        if rm is not None:
            n = y.numel() // C // G
            m64, v64 = rm0.double(), rv0.double()
            for gi in range(G):
                m64 = 0.9 * m64 + 0.1 * mu[gi, 0]
                v64 = 0.9 * v64 + 0.1 * var[gi, 0] * n / (n - 1)
            for t, r in ((rm, m64), (rv, v64)):
                e = float(((t.double().cpu() - r).abs() / (r.abs() + mu.abs().amax((0, 1)) + 1e-30)).max())
                assert e <= TAU, f"{tag}: running statistics off by {e:.3e}"
    return out


def _kink(z, fcond):
    """elements whose pre-activation lies within 2^-18 of its magnitude of the activation's kink: the fp32 kernel computes z from fp32
    statistics (a few ulps of fcond off the fp64 value), so there it may take the other branch -- a whole |da| of difference, not a
    rounding error (one such element, z = 3.9e-8 at fcond 1.35, moved dbeta by 9e-5 of sum |dz| at 2 x 14 x 14 x 10 x 128)"""
    return z.abs() <= 2.0 ** -18 * fcond


def drive_norm_bwd(ops, dev, key, g, variants=((),)):
    """norm_bwd (activation gradient recomputed from y and the forward statistics; dgamma / dbeta accumulated as the step does) with each
    epilogue the step uses at this key: channel scale, seeded elementwise dropout, or the backward statistics from a real
    conv3_dgrad_bwdstats launch's fused partials -- those partials are checked against fp64 sums first"""
    op, shapes, ints, namax = key
    ys = shapes[0]
    G, act, accumulate = ints[0], ints[1], bool(ints[2])
    C = ys[-1]
    N = ys[0]
    out = []
    for flags in variants:
        tag = f"{op} {ys} [{'+'.join(flags) or 'plain'}]"
        y = _pre_norm(g, ys)
        affine = accumulate or G != N
        gam = (torch.rand(C, generator=g) + 0.5) if affine else None
        bet = (torch.rand(C, generator=g) - 0.5) if affine else None
        yd = y.to(dev)
        _, st = ops.norm_fwd(yd, G, *((gam.to(dev), bet.to(dev), torch.zeros(C, device=dev), torch.ones(C, device=dev)) if affine else (None,) * 4), act)
        cs, sm, es, _, mult, H = _epilogue(ops, dev, g, ys, flags)
        _, z, xh, _, var, fcond = norm_ref64(y, G, gam, bet, act)
        kink = _kink(z, fcond)
        _, dact = _acts(act, z)
        part, rows = None, 0
        if "partial" in flags:
            dad, part, rows = _conv_partial_source(ops, dev, g, ys, G, fwd=False, yprev=yd, stats=st, act=act)
            assert rows > 0 or dev.type == "cpu", f"{tag}: conv3_dgrad_bwdstats left no partials at the step's shape"
            da = dad.cpu()
        else:
            da = gradient(g, ys)
            dad = da.to(dev)
        dz = (da.double() * mult * dact).reshape(G, -1, C)
        xg = xh.reshape(G, -1, C)
        dk = (da.double() * mult * kink).abs().reshape(G, -1, C)      # (a kink element may take either branch: its whole term is allowed)
        if rows:
            ps = _partials(part, G, rows, C)
            for j, (s, c, k) in enumerate(((dz.sum(1), dz.abs().sum(1), dk.sum(1)),
                                           ((dz * xg).sum(1), (dz * xg).abs().sum(1), (dk * xg.abs()).sum(1)))):
                err = ((ps[..., j] - s).abs() - k).clamp_min(0)
                r, _ = elementwise_ratio(err, torch.zeros_like(err), c)
                assert r <= TAU, f"{tag}: dgrad epilogue's backward-statistics partial {j} off by {r:.3e} x sum|.|"
        dg0, db0 = (torch.randn(C, generator=g) * 1e-2, torch.randn(C, generator=g) * 1e-2) if accumulate else (torch.zeros(C), torch.zeros(C))
        dg, db = (dg0.clone().to(dev), db0.clone().to(dev)) if affine else (None, None)
        kw = dict(chan_scale=None if cs is None else cs.to(dev), elem_mask=sm, elem_scale=es)
        if rows:
            kw.update(partial=part, nb=rows)
        dx = ops.norm_bwd(yd, dad, G, st, act, dg, db, accumulate, **kw)
        rstd = 1.0 / torch.sqrt(var + EPS)
        gm = torch.ones(C, dtype=torch.float64) if gam is None else gam.double()
        m1, m2 = dz.mean(1, keepdim=True), (dz * xg).mean(1, keepdim=True)
        ref = (gm * rstd * (dz - m1 - xg * m2)).reshape(ys)
        # the two means are fp32-staged reductions over n = voxels per group; their rounding grows with the reduction depth, ~log2(n).
        # Without the factor the pancreas InstanceNorm at 2 x 48^3 x 32 (n = 110 592) measured 2.1 x TAU, with it 0.32 x TAU at worst.
        kap = float(np.log2(dz.shape[1]))
        cond = (gm * rstd * (dz.abs() + kap * (dz.abs().mean(1, keepdim=True) + xg.abs() * (dz * xg).abs().mean(1, keepdim=True)))).reshape(ys)
        cond = torch.where(kink, torch.full_like(cond, float("inf")), cond)
        out.append((op + ("" if not flags else " " + "+".join(flags)), check_elementwise(dx.cpu(), ref, cond, TAU, tag)))
        if affine:
            sdb, sdg = dz.sum((0, 1)), (dz * xg).sum((0, 1))
            for name, t, base, s_, c, k in (("dbeta", db, db0, sdb, dz.abs().sum((0, 1)), dk.sum((0, 1))),
                                            ("dgamma", dg, dg0, sdg, (dz * xg).abs().sum((0, 1)), (dk * xg.abs()).sum((0, 1)))):
                err = ((t.double().cpu() - (base.double() + s_)).abs() - k).clamp_min(0)
                r, _ = elementwise_ratio(err, torch.zeros_like(err), base.double().abs() + c)
                assert r <= TAU, f"{tag}: {name} off by {r:.3e} x cond"
    return out


def drive_wgrad(ops, dev, key, g):
    """conv3_wgrad over all voxels of the step's operands (activation x, gradient dy)"""
    from bcp_amd import hip_ops as H
    op, shapes, ints, namax = key
    xs, dys, ws = shapes
    KD = ints[0]
    assert tuple(ws) == (dys[-1], xs[-1]) + (3,) * (KD == 3 and 3 or 2) and tuple(xs[:4]) == tuple(dys[:4]), key   # (the kernel writes all of ws)
    x, dy = activation(g, xs), gradient(g, dys)
    xd, dyd = x.to(dev), dy.to(dev)
    for t in (xd, dyd)[:namax]:
        _amax(H, t, dev)
    dw = ops.conv3_wgrad(xd, dyd, torch.empty(ws, device=dev), KD)
    ref = conv3_wgrad64(x, dy, 3, KD == 1)
    cond = conv3_wgrad64(x.abs(), dy.abs(), 3, KD == 1)
    return [(op, check_elementwise(dw.cpu(), ref, cond, TAU, f"{op} {xs} -> {ws}"))]


def drive_optim(ops, dev, key, g):
    """sgd (momentum 0.9, weight decay 1e-4, steady state), ema (0.99), adam (step 3) over the flat parameter vector"""
    op, shapes, ints, namax = key
    n = shapes[0][0]
    f32 = lambda v: float(np.float32(v))          # noqa: E731  (the hyper-parameters as the kernels receive them)
    p = torch.randn(n, generator=g, dtype=torch.float64) * 0.05
    gr = gradient(g, (n,)).double()
    if op == "ema":
        src = p + torch.randn(n, generator=g, dtype=torch.float64) * 1e-3
        dst, srcd = p.float().to(dev), src.float().to(dev)
        ops.ema(dst, srcd, 0.99)
        p32, s32 = p.float().double(), src.float().double()
        al, oma = f32(0.99), f32(1 - 0.99)
        ref = al * p32 + oma * s32
        cond = al * p32.abs() + oma * s32.abs()
        return [(op, check_elementwise(dst.cpu(), ref, cond, TAU_OPT, f"{op} {n}"))]
    if op == "sgd":
        buf = gradient(g, (n,))
        pd, gd, bd = p.float().to(dev), gr.float().to(dev), buf.clone().to(dev)
        ops.sgd(pd, gd, bd, 0.01, 0.9, 1e-4, first_step=False)
        p32, g32, b32 = p.float().double(), gr.float().double(), buf.double()
        lr, mo, wd = f32(0.01), f32(0.9), f32(1e-4)
        bref = mo * b32 + (g32 + wd * p32)
        bcond = mo * b32.abs() + g32.abs() + wd * p32.abs()
        r1 = check_elementwise(bd.cpu(), bref, bcond, TAU_OPT, f"{op} {n} momentum")
        r2 = check_elementwise(pd.cpu(), p32 - lr * bref, p32.abs() + lr * bcond, TAU_OPT, f"{op} {n}")
        return [(op + " buf", r1), (op, r2)]
    if op == "adam":
        step = ints[0]
        m = gradient(g, (n,)).double() * 0.1
        v = (gradient(g, (n,)).double() ** 2) * 0.01
        pd, gd, md, vd = p.float().to(dev), gr.float().to(dev), m.float().to(dev), v.float().to(dev)
        ops.adam(pd, gd, md, vd, 1e-3, step)
        p32, g32, m32, v32 = (t.float().double() for t in (p, gr, m, v))
        b1, b2, lr, eps = f32(0.9), f32(0.999), f32(1e-3), f32(1e-8)
        m1 = b1 * m32 + (1 - b1) * g32
        v1 = b2 * v32 + (1 - b2) * g32 * g32
        bc1, bc2s = f32(1 - b1 ** step), f32((1 - b2 ** step) ** 0.5)       # (the bias corrections reach the kernel as fp32 arguments)
        den = torch.sqrt(v1) / bc2s + eps
        upd = lr * (m1 / bc1) / den
        ucond = lr * ((b1 * m32.abs() + (1 - b1) * g32.abs()) / bc1) / den      # (m1 may be a cancellation)
        ref = p32 - upd
        r1 = check_elementwise(md.cpu(), m1, b1 * m32.abs() + (1 - b1) * g32.abs(), TAU_OPT, f"{op} {n} m")
        r2 = check_elementwise(vd.cpu(), v1, v1, TAU_OPT, f"{op} {n} v")
        r3 = check_elementwise(pd.cpu(), ref, p32.abs() + ucond, TAU_ADAM, f"{op} {n}")
        return [(op + " m", r1), (op + " v", r2), (op, r3)]
    raise KeyError(op)


def bilinear_matrix(n):
    """[2n, n] fp64 matrix of the x2 align_corners=True interpolation along one axis, its weights formed as torch's fp32 kernels form
    them (scale and source coordinate rounded to fp32, lambda = src - floor(src)): the fp32 weight rounding is part of the op the
    U-Net computes (up to an ulp of the source coordinate, which is 2.4e-4 relative where a neighbour is 1e3 times larger)"""
    f = np.float32
    out = 2 * n
    scale = f(n - 1) / f(out - 1) if out > 1 else f(0)
    A = torch.zeros(out, n, dtype=torch.float64)
    for o in range(out):
        src = f(scale * f(o))
        i0 = int(src)
        i1 = i0 + (1 if i0 < n - 1 else 0)
        l1 = f(src - f(i0))
        A[o, i0] += float(f(1) - l1)
        A[o, i1] += float(l1)
    return A


def drive_pool(ops, dev, key, g):
    """U-Net: maxpool2d fwd / bwd bit for bit against torch, bilinear x2 (align_corners) fwd / bwd against fp64"""
    from bcp_amd import hip_ops as H
    F = torch.nn.functional
    op, shapes, ints, namax = key
    xs = shapes[0]
    if op in ("maxpool2d_fwd", "maxpool2d_bwd"):
        x = activation(g, xs)
        xd = x.to(dev)
        if namax:
            _amax(H, xd, dev)
        xn = x.permute(0, 4, 1, 2, 3)[:, :, 0].contiguous().requires_grad_(op == "maxpool2d_bwd")
        yr = F.max_pool2d(xn, 2)
        if op == "maxpool2d_fwd":
            y = ops.maxpool2d_fwd(xd)
            assert torch.equal(y.cpu()[:, 0].permute(0, 3, 1, 2), yr.detach()), f"{op} {xs}"
            return [(op, (0.0, "exact"))]
        dy = gradient(g, shapes[1])
        yr.backward(dy[:, 0].permute(0, 3, 1, 2))
        dx = ops.maxpool2d_bwd(xd, dy.to(dev), torch.empty_like(xd))
        assert torch.equal(dx.cpu()[:, 0].permute(0, 3, 1, 2), xn.grad), f"{op} {xs}"
        return [(op, (0.0, "exact"))]
    if op == "bilinear2x_fwd":
        ys = shapes[1]
        off = ints[0]
        assert ys[:2] == xs[:2] and ys[2:4] == (2 * xs[2], 2 * xs[3]) and off + xs[-1] <= ys[-1], key
        x = activation(g, xs)
        y = torch.zeros(ys, device=dev)
        if namax:
            y._bcp_amax = H.amax_slots(0.0, dev)             # (the concat buffer's slots: the launch max-reduces its half into them)
        ops.bilinear2x_fwd(x.to(dev), y, off)
        C = xs[-1]
        Ah, Aw = bilinear_matrix(xs[2]), bilinear_matrix(xs[3])
        x64 = x.double()[:, 0]
        ref = torch.einsum("oh,pw,nhwc->nopc", Ah, Aw, x64).unsqueeze(1)
        cond = torch.einsum("oh,pw,nhwc->nopc", Ah, Aw, x64.abs()).unsqueeze(1)
        if namax:
            assert H.amax_value(y._bcp_amax) == float(y.abs().max()), f"{op} {xs}: |max| slots"
        return [(op, check_elementwise(y.cpu()[..., off:off + C], ref, cond, TAU, f"{op} {xs}", (1, 16, 16)))]
    if op == "bilinear2x_bwd":
        dys = xs
        off, C = ints[0], ints[1]
        assert off + C <= dys[-1] and dys[2] % 2 == 0 and dys[3] % 2 == 0, key
        dy = gradient(g, dys)
        dx = ops.bilinear2x_bwd(dy.to(dev), off, C)
        Ah, Aw = bilinear_matrix(dys[2] // 2), bilinear_matrix(dys[3] // 2)
        d = dy.double()[:, 0, ..., off:off + C]
        ref = torch.einsum("oh,pw,nopc->nhwc", Ah, Aw, d).unsqueeze(1)
        cond = torch.einsum("oh,pw,nopc->nhwc", Ah, Aw, d.abs()).unsqueeze(1)
        return [(op, check_elementwise(dx.cpu(), ref, cond, TAU, f"{op} {dys}", (1, 16, 16)))]
    raise KeyError(op)


def cc_maps(shape, g, two_d=False):
    """structured binary maps for largest-CC at `shape` [N, D, H, W]: (name, uint8 map)
    - smooth: thresholded smoothed noise, many components of similar size straddling tile borders;
    - comb: one thin comb spanning the volume (teeth one voxel apart) beside smaller blobs;
    - near-tie: two slabs whose sizes differ by one voxel, the larger one later in raster order."""
    F = torch.nn.functional
    N, D, H, W = shape
    noise = torch.randn((N, 1, D, H, W), generator=g, dtype=torch.float64)
    if two_d:
        sm = F.avg_pool2d(noise[:, :, 0], 5, 1, 2).unsqueeze(2)
    else:
        sm = F.avg_pool3d(noise, 5, 1, 2)
    smooth = (sm[:, 0] > 0.12).to(torch.uint8)
    comb = (torch.rand(shape, generator=g) < 0.01).to(torch.uint8)                      # specks
    comb[:, :, :, 0::2] = 0
    comb[:, :, max(1, H // 2), :] = 1                                                   # the spine: one row along W ...
    comb[:, :, 1:H - 1, 1::4] = 1                                                       # ... and a tooth along H every 4th column
    tie = torch.zeros(shape, dtype=torch.uint8)
    a = max(1, H // 4)
    d1 = max(1, D // 2) if D > 1 else 1
    tie[:, :d1, 1:1 + a, 1:1 + a] = 1                                                   # size s
    tie[:, :d1, H - 1 - a:H - 1, W - 1 - a:W - 1] = 1                                   # size s ...
    tie[:, 0, H - 2 - a, W - 1 - a] = 1                                                 # ... + 1, touching only its own slab
    return (("smooth", smooth.contiguous()), ("comb", comb.contiguous()), ("near-tie", tie.contiguous()))


def drive_cc(ops, dev, key, g):
    """plabel_cc_largest (and cc_largest on the same maps) at the step's shape and connectivity vs the scipy oracle, bit for bit"""
    import bcp_oracle as O
    op, shapes, ints, namax = key
    N, D, H, W, C = shapes[0]
    conn = ints[0]
    out = []
    for name, m in cc_maps((N, D, H, W), g, two_d=(D == 1)):
        if C == 2:
            lg = torch.zeros(N, D, H, W, 2)
            lg[..., 1] = m.float() * 2 - 1                                              # softmax channel 1 >= 0.5 exactly where m
            ref = O.largest_cc(m.long(), None if conn == 3 else conn)
        else:
            cls = (m.long() * (1 + (torch.arange(W) * 3 // max(W, 1)).view(1, 1, 1, W))).clamp(max=3)      # three classes in bands along W
            lg = torch.nn.functional.one_hot(cls, 4).float() * 3
            ref = O.largest_cc_acdc(cls[:, 0]).unsqueeze(1)
        o = ops.plabel_cc_largest(lg.to(dev).contiguous(), 0.5, conn)
        assert torch.equal(o.cpu().float(), ref.float()), f"{op} {shapes[0]} conn {conn} map {name}: {int((o.cpu().float() != ref.float()).sum())} voxels differ"
        seg = (m if C == 2 else cls).to(torch.uint8).contiguous()
        o2 = ops.cc_largest(seg.to(dev), 1 if C == 2 else 3, conn)
        assert torch.equal(o2.cpu().float(), ref.float()), f"cc_largest {tuple(seg.shape)} conn {conn} map {name}: {int((o2.cpu().float() != ref.float()).sum())} voxels differ"
        out.append((f"{op} {name}", (0.0, "exact")))
    return out


DRIVERS = {"conv3_fwd": drive_conv, "conv3_fwd_stats": drive_conv, "conv3_fwd_raw": drive_conv, "conv3_dgrad_bwdstats": drive_conv,
           "conv3_wgrad": drive_wgrad, "norm_fwd": drive_norm_fwd, "norm_bwd": drive_norm_bwd,
           "sgd": drive_optim, "ema": drive_optim, "adam": drive_optim,
           "maxpool2d_fwd": drive_pool, "maxpool2d_bwd": drive_pool, "bilinear2x_fwd": drive_pool, "bilinear2x_bwd": drive_pool,
           "plabel_cc_largest": drive_cc}


def table_rows():
    """[(workload, key)] in table order"""
    return [(wl, k) for wl, keys in STEP_KEYS.items() for k in keys]


def driven_rows():
    """table rows with a driver, plus norm keys only a statistics-only call uses (the profile does not record those)"""
    rows = [(wl, k) for wl, k in table_rows() if k[0] in DRIVERS]
    have = set(rows)
    for wl, v in STEP_VARIANTS.items():
        rows += [(wl, k) for k in v if (wl, k) not in have]
    return rows


def row_id(wl, key):
    op, shapes, ints, _ = key
    return f"{wl}-{op}-" + "x".join(str(v) for v in shapes[0]) + ("-" + "-".join(str(int(i)) for i in ints) if ints else "")


def reduce_key(key, f=8):
    """the key with every spatial extent divided by f (at least 2, even where a pool needs it) and flat sizes by f^3: the host
    simulator's twin of an in-step shape"""
    op, shapes, ints, namax = key

    def red(s):
        if len(s) == 5:
            N, D, H, W, C = s
            return (N, D if D == 1 else max(2, D // f), max(2, H // f) // 2 * 2, max(2, W // f) // 2 * 2, C)
        if len(s) == 6:
            return (s[0],) + red(s[1:])
        if len(s) == 1 and op in ("sgd", "ema", "adam"):
            return (max(64, s[0] // f ** 3),)
        return s
    shapes = tuple(s if (i == 2 and op.endswith("wgrad")) else red(s) for i, s in enumerate(shapes))      # (a weight gradient's shape stays)
    if op in ("maxpool2d_bwd",):
        x = shapes[0]
        shapes = (x, (x[0], 1, x[2] // 2, x[3] // 2, x[4]), x)
    if op == "bilinear2x_fwd":
        x = shapes[0]
        shapes = (x, (x[0], 1, x[2] * 2, x[3] * 2, shapes[1][4]))
    return op, shapes, ints, namax


# -------------------------------------------------------------------------------------------------- epilogue variants
# The profile key carries no keyword arguments, yet the norm kwargs pick different kernels (statistics from a conv's fused partials ->
# finalize -> apply; the apply pass's channel-scale / dropout / residual epilogue; statistics only).  `record_step_variants` reads them
# off the step itself: during the eager recording pass it notes, per key, which epilogue each norm call used.
_VARIANT_OPS = ("norm_fwd", "norm_bwd")


def _variant_flags(name, kw):
    f = []
    if kw.get("chan_scale") is not None:
        f.append("chan_scale")
    em = kw.get("elem_mask")
    if em is not None:
        f.append("elem_mask")
    if kw.get("partial") is not None:
        f.append("partial")
    if name == "norm_fwd":
        if kw.get("residual") is not None:
            f.append("residual")
        if kw.get("stats_only"):
            f.append("stats_only")
        out = kw.get("out")
        if out is not None and out.dim() >= 2 and out.stride(-2) != out.shape[-1]:
            f.append("out_slab")
    return tuple(f)


def variant_key(name, a):
    """the profile key of a call (hip_ops._profiled's arithmetic)"""
    ts = [t for t in a if isinstance(t, torch.Tensor)]
    return (name, tuple(tuple(t.shape) for t in ts[:3]), tuple(x for x in a if isinstance(x, int))[:3],
            sum(1 for t in ts[:2] if getattr(t, "_bcp_amax", None) is not None))


def record_step_variants(workload):
    """{key: set of epilogue flag tuples} of the norm calls of one step of `workload` (its eager recording pass)"""
    from bcp_amd.hip_ops import Ops
    seen = {}
    saved = {n: getattr(Ops, n) for n in _VARIANT_OPS}

    def wrap(name, fn):
        def w(self, *a, **kw):
            k = variant_key(name, a)
            k = (k[0], tuple(tuple(int(v) for v in s) for s in k[1]), tuple(int(v) for v in k[2]), k[3])
            seen.setdefault(k, set()).add(_variant_flags(name, kw))
            return fn(self, *a, **kw)
        return w
    for n in _VARIANT_OPS:
        setattr(Ops, n, wrap(n, saved[n]))
    try:
        step = make_step(workload, torch.device("cuda:0"))
        for _ in range(2):
            step()
        torch.cuda.synchronize()
    finally:
        for n in _VARIANT_OPS:
            setattr(Ops, n, saved[n])
    return seen


STEP_VARIANTS = {   # {workload: {norm key: epilogues the step uses}} (record_step_variants)
    "la": {
        ('norm_bwd', ((2, 7, 7, 5, 256), (2, 7, 7, 5, 256), (5, 2, 256)), (2, 1, 1), 0): (('chan_scale',),),
        ('norm_bwd', ((2, 14, 14, 10, 128), (2, 14, 14, 10, 128), (5, 2, 128)), (2, 1, 1), 0): ((),),
        ('norm_bwd', ((2, 28, 28, 20, 64), (2, 28, 28, 20, 64), (5, 2, 64)), (2, 1, 1), 0): ((), ('partial',)),
        ('norm_bwd', ((2, 56, 56, 40, 32), (2, 56, 56, 40, 32), (5, 2, 32)), (2, 1, 1), 0): ((), ('partial',)),
        ('norm_bwd', ((2, 112, 112, 80, 16), (2, 112, 112, 80, 16), (5, 2, 16)), (2, 1, 1), 0): ((),),
        ('norm_fwd', ((2, 7, 7, 5, 256), (256,), (256,)), (2, 1), 0): ((),),
        ('norm_fwd', ((2, 14, 14, 10, 128), (128,), (128,)), (2, 1), 0): ((), ('residual',)),
        ('norm_fwd', ((2, 28, 28, 20, 64), (64,), (64,)), (2, 1), 0): ((), ('partial',), ('residual',)),
        ('norm_fwd', ((2, 56, 56, 40, 32), (32,), (32,)), (2, 1), 0): ((), ('partial',), ('residual',)),
        ('norm_fwd', ((2, 112, 112, 80, 16), (16,), (16,)), (2, 1), 0): (('chan_scale', 'partial', 'stats_only'), ('partial', 'residual')),
    },
    "pancreas": {
        ('norm_bwd', ((2, 6, 6, 6, 256), (2, 6, 6, 6, 256), (5, 2, 256)), (2, 1, 0), 0): ((),),
        ('norm_bwd', ((2, 12, 12, 12, 128), (2, 12, 12, 12, 128), (5, 2, 128)), (2, 1, 0), 0): ((),),
        ('norm_bwd', ((2, 24, 24, 24, 64), (2, 24, 24, 24, 64), (5, 2, 64)), (2, 1, 0), 0): ((), ('partial',)),
        ('norm_bwd', ((2, 48, 48, 48, 32), (2, 48, 48, 48, 32), (5, 2, 32)), (2, 1, 0), 0): ((), ('partial',)),
        ('norm_bwd', ((2, 96, 96, 96, 16), (2, 96, 96, 96, 16), (5, 2, 16)), (2, 1, 0), 0): ((),),
        ('norm_fwd', ((2, 6, 6, 6, 256),), (2, 1), 0): ((),),
        ('norm_fwd', ((2, 12, 12, 12, 128),), (2, 1), 0): ((), ('residual',)),
        ('norm_fwd', ((2, 24, 24, 24, 64),), (2, 1), 0): ((), ('partial',), ('residual',)),
        ('norm_fwd', ((2, 48, 48, 48, 32),), (2, 1), 0): ((), ('partial',), ('residual',)),
        ('norm_fwd', ((2, 96, 96, 96, 16),), (2, 1), 0): (('partial', 'residual'), ('partial', 'stats_only')),
    },
    "acdc": {
        ('norm_bwd', ((12, 1, 16, 16, 256), (12, 1, 16, 16, 256), (5, 2, 256)), (2, 2, 1), 0): ((),),
        ('norm_bwd', ((12, 1, 32, 32, 128), (12, 1, 32, 32, 128), (5, 2, 128)), (2, 2, 1), 0): ((), ('elem_mask',)),
        ('norm_bwd', ((12, 1, 64, 64, 64), (12, 1, 64, 64, 64), (5, 2, 64)), (2, 2, 1), 0): ((), ('elem_mask',)),
        ('norm_bwd', ((12, 1, 128, 128, 32), (12, 1, 128, 128, 32), (5, 2, 32)), (2, 2, 1), 0): ((), ('elem_mask',), ('partial',)),
        ('norm_bwd', ((12, 1, 256, 256, 16), (12, 1, 256, 256, 16), (5, 2, 16)), (2, 2, 1), 0): ((),),
        ('norm_fwd', ((12, 1, 32, 32, 128), (128,), (128,)), (2, 2), 0): (('elem_mask', 'partial'), ('partial',), ('partial', 'out_slab')),
        ('norm_fwd', ((12, 1, 64, 64, 64), (64,), (64,)), (2, 2), 0): (('elem_mask', 'partial'), ('partial',), ('partial', 'out_slab')),
        ('norm_fwd', ((12, 1, 128, 128, 32), (32,), (32,)), (2, 2), 0): (('elem_mask', 'partial'), ('partial',), ('partial', 'out_slab')),
        ('norm_fwd', ((12, 1, 256, 256, 16), (16,), (16,)), (2, 2), 0): (('partial',), ('partial', 'out_slab')),
    },
}


def variants_of(wl, key):
    """the epilogues the step uses at a norm key (STEP_VARIANTS); other ops: one plain call"""
    return STEP_VARIANTS.get(wl, {}).get(key, ((),))


def run_row(ops, dev, wl, key, g):
    fn = DRIVERS[key[0]]
    if key[0] in _VARIANT_OPS:
        return fn(ops, dev, key, g, variants_of(wl, key))
    return fn(ops, dev, key, g)
