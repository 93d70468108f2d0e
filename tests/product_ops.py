"""The ops the three product steps launch, at their in-step shapes, with fp64 references and an elementwise comparator.

STEP_KEYS holds what `Ops.profile_end()` records for each call of a replayed step: (op, shapes of the first three tensor arguments, first
three int arguments, number of the first two tensors that carry `_bcp_amax`).  The key carries no keyword arguments, so STEP_VARIANTS adds,
per key, the flags the step's calls really pass (norm epilogues: fused partials, channel scale, dropout, residual, statistics only, slab
output; elsewhere: accumulate, an output buffer given, an upstream gradient on the device), read off a step by `record_step_variants`.
tests/test_gpu_product_ops.py asserts that a real step records nothing outside the two tables and runs DRIVERS over every row
(`driven_rows()`); tests/test_product_ops_cpu.py asserts that every op of the table has a driver.

Every op family of the three steps has one: the 3x3(x3) convs and their weight gradients, the norms (plain and on split-K slabs), the
fused first layer (conv3_c1_*), the k2s2 / transposed / pointwise convs on the GEMM route (down_*, up_*, k2_*, pw_fwd), the fused 16 -> C
head (pw16_*), the pools and the bilinear x2, the paired mix loss and its gradient against a closed form pinned to the oracle's
autograd, mix_box and the largest-component filter bit for bit, the networks' batched weight packs bit for bit against the single-layer
packs, the optimisers.  Rows stay at the in-step shapes because the route is a function of the shape (csrc/gemm.hip: pick_nt, stat_plan,
tn_groups; split-K slab counts; fused statistics): each driver asserts on the device that the in-step route was taken.

Beside the three self-training steps the table holds the other phases the drivers run: one pre-training step per driver (la_pre,
pancreas_pre, acdc_pre: the labeled half of the batch, one norm group, the single mix loss with the all-zero box), one validation pass
per driver (la_val, pancreas_val, acdc_val: eval-mode networks on a full chunk and a remainder chunk of one, operands without |max|,
norm_eval, the sliding-window accumulation, the overlap counts) and the LA step at the driver's default batch 8 (la8).  A key that
already stands under an earlier workload with the same flags is driven once.

lares, lares_pre and lares_val are la, la_pre and la_val with residual V-Nets (has_residual=True): the closing layers' norms
(norm_fwd_res / norm_bwd_res / norm_eval_res of csrc/norm_res.hip, whose activation pattern is that of z + r), the join of a block's two
gradients (axpy), and the unfused routes the closing layers take instead of the fused first layer, the fused head and the slab routes
(conv3_c1_fwd_stats, conv3_c1_wgrad, pw16_fwd / pw16_bwd in a training step, conv3_fwd at the deep levels).  Their references can be
made wrong on purpose (NEAR_MISS): tests/test_product_ops_cpu.py shows that the same bound on the same inputs then rejects the kernel.

lagn, lagn_pre, lagn_val and pancreasgn are la, la_pre, la_val and pancreas with GroupNorm V-Nets (normalization='groupnorm',
csrc/gnorm.hip): gnorm_fwd / gnorm_bwd at every level with the step's flags (the statistics rows of the producer the planner names, the
kernels' own pass at 245 .. 980 blocks per sample, channel scale, the skip add, the table alone, the conv-bias gradient buffer), the fused
head forward and backward on a GroupNorm table (pw16_fwd_norm, pw16_bwd_norm), and the producers and the dgrad whose rows feed or read such
a table.  pancreasgn_pre and pancreasgn_val are left out on purpose: they differ from pancreasgn only in N, and the N = 1 and N = 4
GroupNorm launches are covered by lagn_pre / lagn_val.  Their checks are those of tests/gnorm_seam_checks.py, sample by sample, and their
references too can be made wrong on purpose (GN_NEAR_MISSES).

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


_SUBS = [(a, b, c) for a in range(2) for b in range(2) for c in range(2)]       # the (a, b, c) sub-positions of a 2x2x2 stride-2 kernel


def down64(x, w):
    """k2s2 conv of a channels-last [N, D, H, W, Cin] tensor (even extents) with w [Cout, Cin, 2, 2, 2], in fp64:
    y[n, d, h, w, :] = sum over (a, b, c) of x[n, 2d+a, 2h+b, 2w+c, :] @ W[:, :, a, b, c].T -- eight strided-view matmuls.
    With w a ConvTranspose3d weight [Cin_t, Cout_t, 2, 2, 2] and x = dy this is that layer's dgrad."""
    x, w = x.double().cpu(), w.double().cpu()
    N, D, H, W, Ci = x.shape
    assert D % 2 == 0 and H % 2 == 0 and W % 2 == 0 and w.shape[1] == Ci, (x.shape, w.shape)
    y = torch.zeros(N, D // 2, H // 2, W // 2, w.shape[0], dtype=torch.float64)
    for a, b, c in _SUBS:
        y += x[:, a::2, b::2, c::2] @ w[:, :, a, b, c].t()
    return y


def up64(x, w):
    """transposed k2s2 conv of a channels-last [N, D, H, W, Cin] tensor with w [Cin, Cout, 2, 2, 2], in fp64:
    y[n, 2d+a, 2h+b, 2w+c, :] = x[n, d, h, w, :] @ W[:, :, a, b, c].  With w a Conv3d weight [Cout_c, Cin_c, 2, 2, 2] and x = dy this is
    that layer's dgrad."""
    x, w = x.double().cpu(), w.double().cpu()
    N, D, H, W, Ci = x.shape
    assert w.shape[0] == Ci, (x.shape, w.shape)
    y = torch.zeros(N, 2 * D, 2 * H, 2 * W, w.shape[1], dtype=torch.float64)
    for a, b, c in _SUBS:
        y[:, a::2, b::2, c::2] = x @ w[:, :, a, b, c]
    return y


def k2_wgrad64(x, dy, kind):
    """weight gradient of the down conv (kind 0: x fine, dy coarse -> [Cout, Cin, 2, 2, 2]), the transposed conv (1: x coarse, dy fine ->
    [Cin, Cout, 2, 2, 2]) and the 1x1 conv (2: one grid -> [Cout, Cin, 1, 1]): per sub-position dy^T @ x (resp. x^T @ dy), in fp64"""
    x, dy = x.double().cpu(), dy.double().cpu()
    Cx, Cy = x.shape[-1], dy.shape[-1]
    if kind == 2:
        return (dy.reshape(-1, Cy).t() @ x.reshape(-1, Cx)).reshape(Cy, Cx, 1, 1)
    g = torch.zeros(((Cy, Cx) if kind == 0 else (Cx, Cy)) + (2, 2, 2), dtype=torch.float64)
    for a, b, c in _SUBS:
        if kind == 0:
            g[:, :, a, b, c] = dy.reshape(-1, Cy).t() @ x[:, a::2, b::2, c::2].reshape(-1, Cx)
        else:
            g[:, :, a, b, c] = x.reshape(-1, Cx).t() @ dy[:, a::2, b::2, c::2].reshape(-1, Cy)
    return g


# -------------------------------------------------------------------------------------------------- the steps' keys


VAL_CASES = {"la_val": (112, 112, 96), "pancreas_val": (96, 96, 112), "acdc_val": (17, 256, 256), "lares_val": (112, 112, 96), "lagn_val": (112, 112, 96)}


def make_step(workload, dev):
    """one workload's step as bench.py builds it (configs[1] LA batch 4 / 2 labeled, ACDC 24 / 12, pancreas 4 x 96^3; la8: the LA
    driver's default batch 8 / 4 labeled), the pre-training step of the same driver on the labeled half of that batch (*_pre), or one
    validation pass through the function the driver calls (*_val) on a synthetic case of VAL_CASES' extents: one full chunk of patches
    (slices) and a remainder chunk of one.  lares, lares_pre, lares_val: la, la_pre, la_val with residual V-Nets (has_residual=True);
    lagn, lagn_pre, lagn_val, pancreasgn: la, la_pre, la_val, pancreas with GroupNorm V-Nets (normalization='groupnorm')"""
    from bcp_amd import synth, train_step
    seed = 1337
    np.random.seed(seed)
    base, _, phase = workload.partition("_")
    if workload == "la8":
        base, phase = "la", "8"
    ema_model = None
    if base in ("la", "lares", "lagn"):
        from bcp_amd.networks.net_factory import net_factory
        torch.manual_seed(seed)
        kw = dict(has_residual=base == "lares", normalization="groupnorm" if base == "lagn" else "batchnorm")
        model = net_factory(net_type="VNet", in_chns=1, class_num=2, mode="train", **kw)
        ema_model = net_factory(net_type="VNet", in_chns=1, class_num=2, mode="train", **kw)
        for p in ema_model.parameters():
            p.detach_()
        ema_model.load_state_dict(model.state_dict())
        model.train(); ema_model.train()
        opt = train_step.FlatSGD(model, lr=0.01, momentum=0.9, weight_decay=1e-4)
        if phase == "val":
            from bcp_amd.utils import test_3d_patch as T3
            vol, lab = synth.la_batch(1, shape=VAL_CASES[workload], seed=seed)
            case = [(vol[0, 0].to(dev), lab[0].to(dev))]

            def step():
                return T3.var_all_case_LA(model, 2, patch_size=(112, 112, 80), stride_xy=18, stride_z=4, cases=case)
        else:
            batch = 8 if phase == "8" else 4
            vol, lab = synth.la_batch(batch, seed=seed)
            vol, lab = vol.to(dev), lab.to(dev)
            if phase == "pre":
                def step():
                    return train_step.la_pre_train_step(model, opt, vol[:batch // 2], lab[:batch // 2])
            else:
                def step():
                    return train_step.la_self_train_step(model, ema_model, opt, vol, lab, batch // 2)
    elif base == "acdc":
        from bcp_amd.networks.net_factory import BCP_net
        torch.manual_seed(seed)
        model, ema_model = BCP_net(in_chns=1, class_num=4), BCP_net(in_chns=1, class_num=4, ema=True)
        ema_model.load_state_dict(model.state_dict())
        model.train(); ema_model.train()
        opt = train_step.FlatSGD(model, lr=0.01, momentum=0.9, weight_decay=1e-4)
        if phase == "val":
            from bcp_amd.utils import val_2d
            vol, lab = synth.acdc_batch(VAL_CASES[workload][0], seed=seed)
            image, label = vol[:, 0].unsqueeze(0).to(dev), lab.reshape(1, -1, 256, 256).to(dev)

            def step():
                return val_2d.test_single_volume(image, label, model, classes=4)
        else:
            vol, lab = synth.acdc_batch(24, seed=seed)
            vol, lab = vol.to(dev), lab.to(dev)
            if phase == "pre":
                def step():
                    return train_step.acdc_pre_train_step(model, opt, vol[:12], lab[:12])
            else:
                def step():
                    return train_step.acdc_self_train_step(model, ema_model, opt, vol, lab, 12)
    elif base in ("pancreas", "pancreasgn"):
        from bcp_amd.pancreas import train_pancreas as TP
        from bcp_amd.pancreas.Vnet import create_Vnet
        torch.manual_seed(seed)
        norm = "groupnorm" if base == "pancreasgn" else "instancenorm"
        model, ema_model = create_Vnet(normalization=norm), create_Vnet(ema=True, normalization=norm)
        ema_model.load_state_dict(model.state_dict())
        opt = train_step.FlatAdam(model, lr=1e-3)
        if phase == "val":
            from bcp_amd.pancreas.test_util import test_calculate_metric
            vol, lab = synth.la_batch(1, shape=VAL_CASES[workload], seed=seed)
            case = [(vol[0, 0].to(dev), lab[0].to(dev))]
            stride = (18, 4)                   # (train_pancreas.py's --val_stride default)

            def step():
                return test_calculate_metric(model, case, num_classes=2, dim=(96, 96, 96), s_xy=stride[0], s_z=stride[1])
        else:
            streams = TP._streams(dev, 4, 1, seed=seed)
            if phase == "pre":
                def step():
                    return TP.pretrain(model, opt, streams, 1)
            else:
                def step():
                    return TP.ema_cutmix(model, ema_model, opt, streams, 1)
    else:
        raise ValueError(workload)
    model.volatile_io = ema_model.volatile_io = True
    return step


def setup_steps(workload):
    """steps before the profiled one: a training pass is replayed from a plan (the first step records it, the second captures it); a
    validation pass runs eagerly -- eval() takes no plan"""
    return 0 if workload.endswith("_val") else 2


def record_step_keys(workload, steps=1):
    """the set of (op, shapes, ints, namax) keys one replayed step of `workload` records under the profile hooks (two set-up steps first:
    the first records the launch plans, the second captures them -- the timed steps of bench.py are replays; a validation pass is
    eager and needs none)"""
    from bcp_amd import plan
    from bcp_amd.hip_ops import Ops
    dev = torch.device("cuda:0")
    step = make_step(workload, dev)
    for _ in range(setup_steps(workload)):
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
# ACDC 24 slices of 256 x 256 in groups of 12), then the pre-training steps, the validation passes and the LA batch-8 step (make_step).  A new shape or dispatch route changes the set: test_step_keys_in_table then fails until
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
    "la_pre": (
        ('conv3_c1_norm_bwd_wgrad', ((1, 112, 112, 80, 1), (16, 1, 3, 3, 3), (16,)), (3, 1, 1), 0),
        ('conv3_c1_norm_fwd', ((1, 112, 112, 80, 1), (16, 1, 3, 3, 3), (16,)), (3, 1, 1), 0),
        ('conv3_dgrad_bwdstats', ((1, 56, 56, 40, 32), (99360,), (1, 56, 56, 40, 32)), (32, 3, 1), 1),
        ('conv3_fwd', ((1, 112, 112, 80, 16), (24864,)), (16, 3), 1),
        ('conv3_fwd', ((1, 28, 28, 20, 64), (397344,)), (64, 3), 1),
        ('conv3_fwd', ((1, 7, 7, 5, 256), (6357024,)), (256, 3), 1),
        ('conv3_fwd', ((1, 7, 7, 5, 256), (6357024,), (256,)), (256, 3), 1),
        ('conv3_fwd_raw', ((1, 14, 14, 10, 128), (1589280,)), (128, 3, 4), 1),
        ('conv3_fwd_stats', ((1, 112, 112, 80, 16), (24864,), (16,)), (16, 3, 1), 1),
        ('conv3_fwd_stats', ((1, 28, 28, 20, 64), (397344,), (64,)), (64, 3, 1), 1),
        ('conv3_fwd_stats', ((1, 56, 56, 40, 32), (99360,), (32,)), (32, 3, 1), 1),
        ('conv3_pack_many', ((1600,),), (40,), 0),
        ('conv3_wgrad', ((1, 112, 112, 80, 16), (1, 112, 112, 80, 16), (16, 16, 3, 3, 3)), (3,), 2),
        ('conv3_wgrad', ((1, 14, 14, 10, 128), (1, 14, 14, 10, 128), (128, 128, 3, 3, 3)), (3,), 2),
        ('conv3_wgrad', ((1, 28, 28, 20, 64), (1, 28, 28, 20, 64), (64, 64, 3, 3, 3)), (3,), 2),
        ('conv3_wgrad', ((1, 56, 56, 40, 32), (1, 56, 56, 40, 32), (32, 32, 3, 3, 3)), (3,), 2),
        ('conv3_wgrad', ((1, 7, 7, 5, 256), (1, 7, 7, 5, 256), (256, 256, 3, 3, 3)), (3,), 2),
        ('down_dgrad', ((1, 14, 14, 10, 128), (65536,)), (64,), 1),
        ('down_dgrad', ((1, 28, 28, 20, 64), (16384,)), (32,), 1),
        ('down_dgrad', ((1, 56, 56, 40, 32), (4096,)), (16,), 1),
        ('down_dgrad', ((1, 7, 7, 5, 256), (262144,)), (128,), 1),
        ('down_fwd', ((1, 112, 112, 80, 16), (4096,), (32,)), (32,), 1),
        ('down_fwd', ((1, 14, 14, 10, 128), (262144,), (256,)), (256,), 1),
        ('down_fwd', ((1, 28, 28, 20, 64), (65536,), (128,)), (128,), 1),
        ('down_fwd', ((1, 56, 56, 40, 32), (16384,), (64,)), (64,), 1),
        ('k2_pack_many', ((1024,),), (16,), 0),
        ('k2_wgrad', ((1, 112, 112, 80, 16), (1, 56, 56, 40, 32), (32, 16, 2, 2, 2)), (0,), 2),
        ('k2_wgrad', ((1, 14, 14, 10, 128), (1, 28, 28, 20, 64), (128, 64, 2, 2, 2)), (1,), 2),
        ('k2_wgrad', ((1, 14, 14, 10, 128), (1, 7, 7, 5, 256), (256, 128, 2, 2, 2)), (0,), 2),
        ('k2_wgrad', ((1, 28, 28, 20, 64), (1, 14, 14, 10, 128), (128, 64, 2, 2, 2)), (0,), 2),
        ('k2_wgrad', ((1, 28, 28, 20, 64), (1, 56, 56, 40, 32), (64, 32, 2, 2, 2)), (1,), 2),
        ('k2_wgrad', ((1, 56, 56, 40, 32), (1, 112, 112, 80, 16), (32, 16, 2, 2, 2)), (1,), 2),
        ('k2_wgrad', ((1, 56, 56, 40, 32), (1, 28, 28, 20, 64), (64, 32, 2, 2, 2)), (0,), 2),
        ('k2_wgrad', ((1, 7, 7, 5, 256), (1, 14, 14, 10, 128), (256, 128, 2, 2, 2)), (1,), 2),
        ('mix_box', ((1, 112, 112, 80, 1), (1, 112, 112, 80, 1)), (), 0),
        ('mixloss_bwd', ((1, 112, 112, 80, 2), (1, 112, 112, 80), (1, 112, 112, 80)), (0,), 0),
        ('mixloss_fwd', ((1, 112, 112, 80, 2), (1, 112, 112, 80), (1, 112, 112, 80)), (0,), 0),
        ('norm_bwd', ((1, 112, 112, 80, 16), (1, 112, 112, 80, 16), (5, 1, 16)), (1, 1, True), 0),
        ('norm_bwd', ((1, 14, 14, 10, 128), (1, 14, 14, 10, 128), (5, 1, 128)), (1, 1, True), 0),
        ('norm_bwd', ((1, 28, 28, 20, 64), (1, 28, 28, 20, 64), (5, 1, 64)), (1, 1, True), 0),
        ('norm_bwd', ((1, 56, 56, 40, 32), (1, 56, 56, 40, 32), (5, 1, 32)), (1, 1, True), 0),
        ('norm_bwd', ((1, 7, 7, 5, 256), (1, 7, 7, 5, 256), (5, 1, 256)), (1, 1, True), 0),
        ('norm_bwd_slabs', ((1, 14, 14, 10, 128), (4, 1, 14, 14, 10, 128), (5, 1, 128)), (4, 1, 1), 0),
        ('norm_fwd', ((1, 112, 112, 80, 16), (16,), (16,)), (1, 1), 0),
        ('norm_fwd', ((1, 14, 14, 10, 128), (128,), (128,)), (1, 1), 0),
        ('norm_fwd', ((1, 28, 28, 20, 64), (64,), (64,)), (1, 1), 0),
        ('norm_fwd', ((1, 56, 56, 40, 32), (32,), (32,)), (1, 1), 0),
        ('norm_fwd', ((1, 7, 7, 5, 256), (256,), (256,)), (1, 1), 0),
        ('norm_fwd_slabs', ((4, 1, 14, 14, 10, 128), (128,), (128,)), (4, 1, 1), 0),
        ('pw16_bwd_norm_bwd', ((1, 112, 112, 80, 16), (5, 1, 16), (1, 16)), (1, 1), 0),
        ('pw16_fwd_norm', ((1, 112, 112, 80, 16), (5, 1, 16), (1, 16)), (1, 1, 2), 0),
        ('sgd', ((9448868,), (9448868,), (9448868,)), (), 0),
        ('up_dgrad', ((1, 112, 112, 80, 16), (4096,)), (32,), 1),
        ('up_dgrad', ((1, 14, 14, 10, 128), (262144,)), (256,), 1),
        ('up_dgrad', ((1, 28, 28, 20, 64), (65536,)), (128,), 1),
        ('up_dgrad', ((1, 56, 56, 40, 32), (16384,)), (64,), 1),
        ('up_fwd', ((1, 14, 14, 10, 128), (65536,), (64,)), (64,), 1),
        ('up_fwd', ((1, 28, 28, 20, 64), (16384,), (32,)), (32,), 1),
        ('up_fwd', ((1, 56, 56, 40, 32), (4096,), (16,)), (16,), 1),
        ('up_fwd', ((1, 7, 7, 5, 256), (262144,), (128,)), (128,), 1),
    ),
    "pancreas_pre": (
        ('adam', ((9443268,), (9443268,), (9443268,)), (3,), 0),
        ('conv3_c1_norm_bwd_wgrad', ((1, 96, 96, 96, 1), (16, 1, 3, 3, 3), (16,)), (3, 1, 1), 0),
        ('conv3_c1_norm_fwd', ((1, 96, 96, 96, 1), (16, 1, 3, 3, 3), (16,)), (3, 1, 1), 0),
        ('conv3_dgrad_bwdstats', ((1, 48, 48, 48, 32), (99360,), (1, 48, 48, 48, 32)), (32, 3, 1), 1),
        ('conv3_fwd', ((1, 24, 24, 24, 64), (397344,)), (64, 3), 1),
        ('conv3_fwd', ((1, 24, 24, 24, 64), (397344,), (64,)), (64, 3), 1),
        ('conv3_fwd', ((1, 6, 6, 6, 256), (6357024,)), (256, 3), 1),
        ('conv3_fwd', ((1, 6, 6, 6, 256), (6357024,), (256,)), (256, 3), 1),
        ('conv3_fwd', ((1, 96, 96, 96, 16), (24864,)), (16, 3), 1),
        ('conv3_fwd_raw', ((1, 12, 12, 12, 128), (1589280,)), (128, 3, 4), 1),
        ('conv3_fwd_stats', ((1, 48, 48, 48, 32), (99360,), (32,)), (32, 3, 1), 1),
        ('conv3_fwd_stats', ((1, 96, 96, 96, 16), (24864,), (16,)), (16, 3, 1), 1),
        ('conv3_pack_many', ((1600,),), (40,), 0),
        ('conv3_wgrad', ((1, 12, 12, 12, 128), (1, 12, 12, 12, 128), (128, 128, 3, 3, 3)), (3,), 2),
        ('conv3_wgrad', ((1, 24, 24, 24, 64), (1, 24, 24, 24, 64), (64, 64, 3, 3, 3)), (3,), 2),
        ('conv3_wgrad', ((1, 48, 48, 48, 32), (1, 48, 48, 48, 32), (32, 32, 3, 3, 3)), (3,), 2),
        ('conv3_wgrad', ((1, 6, 6, 6, 256), (1, 6, 6, 6, 256), (256, 256, 3, 3, 3)), (3,), 2),
        ('conv3_wgrad', ((1, 96, 96, 96, 16), (1, 96, 96, 96, 16), (16, 16, 3, 3, 3)), (3,), 2),
        ('down_dgrad', ((1, 12, 12, 12, 128), (65536,)), (64,), 1),
        ('down_dgrad', ((1, 24, 24, 24, 64), (16384,)), (32,), 1),
        ('down_dgrad', ((1, 48, 48, 48, 32), (4096,)), (16,), 1),
        ('down_dgrad', ((1, 6, 6, 6, 256), (262144,)), (128,), 1),
        ('down_fwd', ((1, 12, 12, 12, 128), (262144,), (256,)), (256,), 1),
        ('down_fwd', ((1, 24, 24, 24, 64), (65536,), (128,)), (128,), 1),
        ('down_fwd', ((1, 48, 48, 48, 32), (16384,), (64,)), (64,), 1),
        ('down_fwd', ((1, 96, 96, 96, 16), (4096,), (32,)), (32,), 1),
        ('k2_pack_many', ((1024,),), (16,), 0),
        ('k2_wgrad', ((1, 12, 12, 12, 128), (1, 24, 24, 24, 64), (128, 64, 2, 2, 2)), (1,), 2),
        ('k2_wgrad', ((1, 12, 12, 12, 128), (1, 6, 6, 6, 256), (256, 128, 2, 2, 2)), (0,), 2),
        ('k2_wgrad', ((1, 24, 24, 24, 64), (1, 12, 12, 12, 128), (128, 64, 2, 2, 2)), (0,), 2),
        ('k2_wgrad', ((1, 24, 24, 24, 64), (1, 48, 48, 48, 32), (64, 32, 2, 2, 2)), (1,), 2),
        ('k2_wgrad', ((1, 48, 48, 48, 32), (1, 24, 24, 24, 64), (64, 32, 2, 2, 2)), (0,), 2),
        ('k2_wgrad', ((1, 48, 48, 48, 32), (1, 96, 96, 96, 16), (32, 16, 2, 2, 2)), (1,), 2),
        ('k2_wgrad', ((1, 6, 6, 6, 256), (1, 12, 12, 12, 128), (256, 128, 2, 2, 2)), (1,), 2),
        ('k2_wgrad', ((1, 96, 96, 96, 16), (1, 48, 48, 48, 32), (32, 16, 2, 2, 2)), (0,), 2),
        ('mix_box', ((1, 96, 96, 96, 1), (1, 96, 96, 96, 1)), (), 0),
        ('mixloss_bwd', ((1, 96, 96, 96, 2), (1, 96, 96, 96), (1, 96, 96, 96)), (0,), 0),
        ('mixloss_fwd', ((1, 96, 96, 96, 2), (1, 96, 96, 96), (1, 96, 96, 96)), (0,), 0),
        ('norm_bwd', ((1, 12, 12, 12, 128), (1, 12, 12, 12, 128), (5, 1, 128)), (1, 1, False), 0),
        ('norm_bwd', ((1, 24, 24, 24, 64), (1, 24, 24, 24, 64), (5, 1, 64)), (1, 1, False), 0),
        ('norm_bwd', ((1, 48, 48, 48, 32), (1, 48, 48, 48, 32), (5, 1, 32)), (1, 1, False), 0),
        ('norm_bwd', ((1, 6, 6, 6, 256), (1, 6, 6, 6, 256), (5, 1, 256)), (1, 1, False), 0),
        ('norm_bwd', ((1, 96, 96, 96, 16), (1, 96, 96, 96, 16), (5, 1, 16)), (1, 1, False), 0),
        ('norm_bwd_slabs', ((1, 12, 12, 12, 128), (4, 1, 12, 12, 12, 128), (5, 1, 128)), (4, 1, 1), 0),
        ('norm_fwd', ((1, 12, 12, 12, 128),), (1, 1), 0),
        ('norm_fwd', ((1, 24, 24, 24, 64),), (1, 1), 0),
        ('norm_fwd', ((1, 48, 48, 48, 32),), (1, 1), 0),
        ('norm_fwd', ((1, 6, 6, 6, 256),), (1, 1), 0),
        ('norm_fwd', ((1, 96, 96, 96, 16),), (1, 1), 0),
        ('norm_fwd_slabs', ((4, 1, 12, 12, 12, 128), (128,)), (4, 1, 1), 0),
        ('pw16_bwd_norm_bwd', ((1, 96, 96, 96, 16), (5, 1, 16), (1, 96, 96, 96, 2)), (1, 1), 0),
        ('pw16_fwd_norm', ((1, 96, 96, 96, 16), (5, 1, 16), (2, 16, 1, 1, 1)), (1, 1, 2), 0),
        ('up_dgrad', ((1, 12, 12, 12, 128), (262144,)), (256,), 1),
        ('up_dgrad', ((1, 24, 24, 24, 64), (65536,)), (128,), 1),
        ('up_dgrad', ((1, 48, 48, 48, 32), (16384,)), (64,), 1),
        ('up_dgrad', ((1, 96, 96, 96, 16), (4096,)), (32,), 1),
        ('up_fwd', ((1, 12, 12, 12, 128), (65536,), (64,)), (64,), 1),
        ('up_fwd', ((1, 24, 24, 24, 64), (16384,), (32,)), (32,), 1),
        ('up_fwd', ((1, 48, 48, 48, 32), (4096,), (16,)), (16,), 1),
        ('up_fwd', ((1, 6, 6, 6, 256), (262144,), (128,)), (128,), 1),
    ),
    "acdc_pre": (
        ('bilinear2x_bwd', ((6, 1, 128, 128, 64),), (32, 32), 0),
        ('bilinear2x_bwd', ((6, 1, 256, 256, 32),), (16, 16), 0),
        ('bilinear2x_bwd', ((6, 1, 32, 32, 256),), (128, 128), 0),
        ('bilinear2x_bwd', ((6, 1, 64, 64, 128),), (64, 64), 0),
        ('bilinear2x_fwd', ((6, 1, 128, 128, 16), (6, 1, 256, 256, 32)), (16,), 1),
        ('bilinear2x_fwd', ((6, 1, 16, 16, 128), (6, 1, 32, 32, 256)), (128,), 1),
        ('bilinear2x_fwd', ((6, 1, 32, 32, 64), (6, 1, 64, 64, 128)), (64,), 1),
        ('bilinear2x_fwd', ((6, 1, 64, 64, 32), (6, 1, 128, 128, 64)), (32,), 1),
        ('conv3_c1_norm_bwd_wgrad', ((6, 1, 256, 256, 1), (16, 1, 3, 3), (16,)), (1, 1, 2), 0),
        ('conv3_c1_norm_fwd', ((6, 1, 256, 256, 1), (16, 1, 3, 3), (16,)), (1, 1, 2), 0),
        ('conv3_dgrad_bwdstats', ((6, 1, 128, 128, 32), (34848,), (6, 1, 128, 128, 32)), (32, 1, 2), 1),
        ('conv3_fwd', ((6, 1, 128, 128, 32), (17440,)), (16, 1), 1),
        ('conv3_fwd', ((6, 1, 128, 128, 32), (34848,)), (32, 1), 1),
        ('conv3_fwd', ((6, 1, 128, 128, 32), (69664,)), (64, 1), 1),
        ('conv3_fwd', ((6, 1, 16, 16, 256), (1114144,)), (128, 1), 1),
        ('conv3_fwd', ((6, 1, 256, 256, 16), (17440,)), (32, 1), 1),
        ('conv3_fwd', ((6, 1, 256, 256, 16), (8736,)), (16, 1), 1),
        ('conv3_fwd', ((6, 1, 256, 256, 16), (8736,), (4,)), (4, 1), 1),
        ('conv3_fwd', ((6, 1, 256, 256, 4), (8736,)), (16, 1), 0),
        ('conv3_fwd', ((6, 1, 32, 32, 128), (1114144,)), (256, 1), 1),
        ('conv3_fwd', ((6, 1, 32, 32, 128), (278560,)), (64, 1), 1),
        ('conv3_fwd', ((6, 1, 32, 32, 128), (557088,)), (128, 1), 1),
        ('conv3_fwd', ((6, 1, 32, 32, 128), (557088,), (128,)), (128, 1), 1),
        ('conv3_fwd', ((6, 1, 32, 32, 256), (1114144,), (128,)), (128, 1), 1),
        ('conv3_fwd', ((6, 1, 32, 32, 64), (278560,), (128,)), (128, 1), 1),
        ('conv3_fwd', ((6, 1, 64, 64, 64), (139296,)), (64, 1), 1),
        ('conv3_fwd', ((6, 1, 64, 64, 64), (278560,)), (128, 1), 1),
        ('conv3_fwd', ((6, 1, 64, 64, 64), (69664,)), (32, 1), 1),
        ('conv3_fwd_raw', ((6, 1, 16, 16, 128), (1114144,)), (256, 1, 4), 1),
        ('conv3_fwd_raw', ((6, 1, 16, 16, 256), (2228256,)), (256, 1, 4), 1),
        ('conv3_fwd_stats', ((6, 1, 128, 128, 16), (17440,), (32,)), (32, 1, 1), 1),
        ('conv3_fwd_stats', ((6, 1, 128, 128, 32), (34848,), (32,)), (32, 1, 1), 1),
        ('conv3_fwd_stats', ((6, 1, 128, 128, 64), (69664,), (32,)), (32, 1, 1), 1),
        ('conv3_fwd_stats', ((6, 1, 256, 256, 16), (8736,), (16,)), (16, 1, 1), 1),
        ('conv3_fwd_stats', ((6, 1, 256, 256, 32), (17440,), (16,)), (16, 1, 1), 1),
        ('conv3_fwd_stats', ((6, 1, 64, 64, 128), (278560,), (64,)), (64, 1, 1), 1),
        ('conv3_fwd_stats', ((6, 1, 64, 64, 32), (69664,), (64,)), (64, 1, 1), 1),
        ('conv3_fwd_stats', ((6, 1, 64, 64, 64), (139296,), (64,)), (64, 1, 1), 1),
        ('conv3_pack_many', ((1440,),), (36,), 0),
        ('conv3_wgrad', ((6, 1, 128, 128, 16), (6, 1, 128, 128, 32), (32, 16, 3, 3)), (1,), 2),
        ('conv3_wgrad', ((6, 1, 128, 128, 32), (6, 1, 128, 128, 32), (32, 32, 3, 3)), (1,), 2),
        ('conv3_wgrad', ((6, 1, 128, 128, 64), (6, 1, 128, 128, 32), (32, 64, 3, 3)), (1,), 2),
        ('conv3_wgrad', ((6, 1, 16, 16, 128), (6, 1, 16, 16, 256), (256, 128, 3, 3)), (1,), 2),
        ('conv3_wgrad', ((6, 1, 16, 16, 256), (6, 1, 16, 16, 256), (256, 256, 3, 3)), (1,), 2),
        ('conv3_wgrad', ((6, 1, 256, 256, 16), (6, 1, 256, 256, 16), (16, 16, 3, 3)), (1,), 2),
        ('conv3_wgrad', ((6, 1, 256, 256, 16), (6, 1, 256, 256, 4), (4, 16, 3, 3)), (1,), 1),
        ('conv3_wgrad', ((6, 1, 256, 256, 32), (6, 1, 256, 256, 16), (16, 32, 3, 3)), (1,), 2),
        ('conv3_wgrad', ((6, 1, 32, 32, 128), (6, 1, 32, 32, 128), (128, 128, 3, 3)), (1,), 2),
        ('conv3_wgrad', ((6, 1, 32, 32, 256), (6, 1, 32, 32, 128), (128, 256, 3, 3)), (1,), 2),
        ('conv3_wgrad', ((6, 1, 32, 32, 64), (6, 1, 32, 32, 128), (128, 64, 3, 3)), (1,), 2),
        ('conv3_wgrad', ((6, 1, 64, 64, 128), (6, 1, 64, 64, 64), (64, 128, 3, 3)), (1,), 2),
        ('conv3_wgrad', ((6, 1, 64, 64, 32), (6, 1, 64, 64, 64), (64, 32, 3, 3)), (1,), 2),
        ('conv3_wgrad', ((6, 1, 64, 64, 64), (6, 1, 64, 64, 64), (64, 64, 3, 3)), (1,), 2),
        ('k2_pack_many', ((512,),), (8,), 0),
        ('k2_wgrad', ((6, 1, 128, 128, 32), (6, 1, 128, 128, 16), (16, 32, 1, 1)), (2,), 1),
        ('k2_wgrad', ((6, 1, 16, 16, 256), (6, 1, 16, 16, 128), (128, 256, 1, 1)), (2,), 1),
        ('k2_wgrad', ((6, 1, 32, 32, 128), (6, 1, 32, 32, 64), (64, 128, 1, 1)), (2,), 1),
        ('k2_wgrad', ((6, 1, 64, 64, 64), (6, 1, 64, 64, 32), (32, 64, 1, 1)), (2,), 1),
        ('maxpool2d_bwd', ((6, 1, 128, 128, 32), (6, 1, 64, 64, 32), (6, 1, 128, 128, 32)), (), 1),
        ('maxpool2d_bwd', ((6, 1, 256, 256, 16), (6, 1, 128, 128, 16), (6, 1, 256, 256, 16)), (), 1),
        ('maxpool2d_bwd', ((6, 1, 32, 32, 128), (6, 1, 16, 16, 128), (6, 1, 32, 32, 128)), (), 1),
        ('maxpool2d_bwd', ((6, 1, 64, 64, 64), (6, 1, 32, 32, 64), (6, 1, 64, 64, 64)), (), 1),
        ('maxpool2d_fwd', ((6, 1, 128, 128, 32),), (), 1),
        ('maxpool2d_fwd', ((6, 1, 256, 256, 16),), (), 1),
        ('maxpool2d_fwd', ((6, 1, 32, 32, 128),), (), 1),
        ('maxpool2d_fwd', ((6, 1, 64, 64, 64),), (), 1),
        ('mix_box', ((6, 1, 256, 256, 1), (6, 1, 256, 256, 1)), (), 0),
        ('mixloss_bwd', ((6, 1, 256, 256, 4), (6, 1, 256, 256), (6, 1, 256, 256)), (1,), 0),
        ('mixloss_fwd', ((6, 1, 256, 256, 4), (6, 1, 256, 256), (6, 1, 256, 256)), (1,), 0),
        ('norm_bwd', ((6, 1, 128, 128, 32), (6, 1, 128, 128, 32), (5, 1, 32)), (1, 2, True), 0),
        ('norm_bwd', ((6, 1, 16, 16, 256), (6, 1, 16, 16, 256), (5, 1, 256)), (1, 2, True), 0),
        ('norm_bwd', ((6, 1, 256, 256, 16), (6, 1, 256, 256, 16), (5, 1, 16)), (1, 2, True), 0),
        ('norm_bwd', ((6, 1, 32, 32, 128), (6, 1, 32, 32, 128), (5, 1, 128)), (1, 2, True), 0),
        ('norm_bwd', ((6, 1, 64, 64, 64), (6, 1, 64, 64, 64), (5, 1, 64)), (1, 2, True), 0),
        ('norm_bwd_slabs', ((6, 1, 16, 16, 256), (4, 6, 1, 16, 16, 256), (5, 1, 256)), (4, 1, 2), 0),
        ('norm_fwd', ((6, 1, 128, 128, 32), (32,), (32,)), (1, 2), 0),
        ('norm_fwd', ((6, 1, 256, 256, 16), (16,), (16,)), (1, 2), 0),
        ('norm_fwd', ((6, 1, 32, 32, 128), (128,), (128,)), (1, 2), 0),
        ('norm_fwd', ((6, 1, 64, 64, 64), (64,), (64,)), (1, 2), 0),
        ('norm_fwd_slabs', ((4, 6, 1, 16, 16, 256), (256,), (256,)), (4, 1, 2), 0),
        ('pw_fwd', ((6, 1, 128, 128, 16), (512,)), (32,), 0),
        ('pw_fwd', ((6, 1, 128, 128, 32), (512,), (16,)), (16,), 1),
        ('pw_fwd', ((6, 1, 16, 16, 128), (32768,)), (256,), 0),
        ('pw_fwd', ((6, 1, 16, 16, 256), (32768,), (128,)), (128,), 1),
        ('pw_fwd', ((6, 1, 32, 32, 128), (8192,), (64,)), (64,), 1),
        ('pw_fwd', ((6, 1, 32, 32, 64), (8192,)), (128,), 0),
        ('pw_fwd', ((6, 1, 64, 64, 32), (2048,)), (64,), 0),
        ('pw_fwd', ((6, 1, 64, 64, 64), (2048,), (32,)), (32,), 1),
        ('sgd', ((1813764,), (1813764,), (1813764,)), (), 0),
    ),
    "la_val": (
        ('conv3_c1_fwd', ((1, 112, 112, 80, 1), (16, 1, 3, 3, 3), (16,)), (3,), 0),
        ('conv3_c1_fwd', ((4, 112, 112, 80, 1), (16, 1, 3, 3, 3), (16,)), (3,), 0),
        ('conv3_fwd', ((1, 112, 112, 80, 16), (24864,), (16,)), (16, 3), 0),
        ('conv3_fwd', ((1, 14, 14, 10, 128), (1589280,), (128,)), (128, 3), 0),
        ('conv3_fwd', ((1, 28, 28, 20, 64), (397344,), (64,)), (64, 3), 0),
        ('conv3_fwd', ((1, 56, 56, 40, 32), (99360,), (32,)), (32, 3), 0),
        ('conv3_fwd', ((1, 7, 7, 5, 256), (6357024,), (256,)), (256, 3), 0),
        ('conv3_fwd', ((4, 112, 112, 80, 16), (24864,), (16,)), (16, 3), 0),
        ('conv3_fwd', ((4, 14, 14, 10, 128), (1589280,), (128,)), (128, 3), 0),
        ('conv3_fwd', ((4, 28, 28, 20, 64), (397344,), (64,)), (64, 3), 0),
        ('conv3_fwd', ((4, 56, 56, 40, 32), (99360,), (32,)), (32, 3), 0),
        ('conv3_fwd', ((4, 7, 7, 5, 256), (6357024,), (256,)), (256, 3), 0),
        ('conv3_pack_many', ((800,),), (20,), 0),
        ('down_fwd', ((1, 112, 112, 80, 16), (4096,), (32,)), (32,), 0),
        ('down_fwd', ((1, 14, 14, 10, 128), (262144,), (256,)), (256,), 0),
        ('down_fwd', ((1, 28, 28, 20, 64), (65536,), (128,)), (128,), 0),
        ('down_fwd', ((1, 56, 56, 40, 32), (16384,), (64,)), (64,), 0),
        ('down_fwd', ((4, 112, 112, 80, 16), (4096,), (32,)), (32,), 0),
        ('down_fwd', ((4, 14, 14, 10, 128), (262144,), (256,)), (256,), 0),
        ('down_fwd', ((4, 28, 28, 20, 64), (65536,), (128,)), (128,), 0),
        ('down_fwd', ((4, 56, 56, 40, 32), (16384,), (64,)), (64,), 0),
        ('k2_pack_many', ((512,),), (8,), 0),
        ('norm_eval', ((1, 112, 112, 80, 16), (16,), (16,)), (1,), 0),
        ('norm_eval', ((1, 14, 14, 10, 128), (128,), (128,)), (1,), 0),
        ('norm_eval', ((1, 28, 28, 20, 64), (64,), (64,)), (1,), 0),
        ('norm_eval', ((1, 56, 56, 40, 32), (32,), (32,)), (1,), 0),
        ('norm_eval', ((1, 7, 7, 5, 256), (256,), (256,)), (1,), 0),
        ('norm_eval', ((4, 112, 112, 80, 16), (16,), (16,)), (1,), 0),
        ('norm_eval', ((4, 14, 14, 10, 128), (128,), (128,)), (1,), 0),
        ('norm_eval', ((4, 28, 28, 20, 64), (64,), (64,)), (1,), 0),
        ('norm_eval', ((4, 56, 56, 40, 32), (32,), (32,)), (1,), 0),
        ('norm_eval', ((4, 7, 7, 5, 256), (256,), (256,)), (1,), 0),
        ('overlap_counts', ((112, 112, 96), (112, 112, 96)), (0,), 0),
        ('pw16_fwd', ((1, 112, 112, 80, 16), (2, 16, 1, 1, 1), (2,)), (2,), 0),
        ('pw16_fwd', ((4, 112, 112, 80, 16), (2, 16, 1, 1, 1), (2,)), (2,), 0),
        ('sw_accumulate', ((112, 112, 80, 2), (112, 112, 96), (112, 112, 96)), (), 0),
        ('sw_finish', ((112, 112, 96), (112, 112, 96)), (), 0),
        ('up_fwd', ((1, 14, 14, 10, 128), (65536,), (64,)), (64,), 0),
        ('up_fwd', ((1, 28, 28, 20, 64), (16384,), (32,)), (32,), 0),
        ('up_fwd', ((1, 56, 56, 40, 32), (4096,), (16,)), (16,), 0),
        ('up_fwd', ((1, 7, 7, 5, 256), (262144,), (128,)), (128,), 0),
        ('up_fwd', ((4, 14, 14, 10, 128), (65536,), (64,)), (64,), 0),
        ('up_fwd', ((4, 28, 28, 20, 64), (16384,), (32,)), (32,), 0),
        ('up_fwd', ((4, 56, 56, 40, 32), (4096,), (16,)), (16,), 0),
        ('up_fwd', ((4, 7, 7, 5, 256), (262144,), (128,)), (128,), 0),
    ),
    "pancreas_val": (
        ('conv3_c1_fwd', ((1, 96, 96, 96, 1), (16, 1, 3, 3, 3), (16,)), (3,), 0),
        ('conv3_c1_fwd', ((4, 96, 96, 96, 1), (16, 1, 3, 3, 3), (16,)), (3,), 0),
        ('conv3_fwd', ((1, 12, 12, 12, 128), (1589280,), (128,)), (128, 3), 1),
        ('conv3_fwd', ((1, 24, 24, 24, 64), (397344,), (64,)), (64, 3), 1),
        ('conv3_fwd', ((1, 6, 6, 6, 256), (6357024,), (256,)), (256, 3), 1),
        ('conv3_fwd', ((4, 12, 12, 12, 128), (1589280,), (128,)), (128, 3), 1),
        ('conv3_fwd', ((4, 6, 6, 6, 256), (6357024,), (256,)), (256, 3), 1),
        ('conv3_fwd_stats', ((1, 12, 12, 12, 128), (1589280,), (128,)), (128, 3, 1), 1),
        ('conv3_fwd_stats', ((1, 24, 24, 24, 64), (397344,), (64,)), (64, 3, 1), 1),
        ('conv3_fwd_stats', ((1, 48, 48, 48, 32), (99360,), (32,)), (32, 3, 1), 1),
        ('conv3_fwd_stats', ((1, 6, 6, 6, 256), (6357024,), (256,)), (256, 3, 1), 1),
        ('conv3_fwd_stats', ((1, 96, 96, 96, 16), (24864,), (16,)), (16, 3, 1), 1),
        ('conv3_fwd_stats', ((4, 12, 12, 12, 128), (1589280,), (128,)), (128, 3, 4), 1),
        ('conv3_fwd_stats', ((4, 24, 24, 24, 64), (397344,), (64,)), (64, 3, 4), 1),
        ('conv3_fwd_stats', ((4, 48, 48, 48, 32), (99360,), (32,)), (32, 3, 4), 1),
        ('conv3_fwd_stats', ((4, 6, 6, 6, 256), (6357024,), (256,)), (256, 3, 4), 1),
        ('conv3_fwd_stats', ((4, 96, 96, 96, 16), (24864,), (16,)), (16, 3, 4), 1),
        ('conv3_pack_many', ((800,),), (20,), 0),
        ('down_fwd', ((1, 12, 12, 12, 128), (262144,), (256,)), (256,), 1),
        ('down_fwd', ((1, 24, 24, 24, 64), (65536,), (128,)), (128,), 1),
        ('down_fwd', ((1, 48, 48, 48, 32), (16384,), (64,)), (64,), 1),
        ('down_fwd', ((1, 96, 96, 96, 16), (4096,), (32,)), (32,), 1),
        ('down_fwd', ((4, 12, 12, 12, 128), (262144,), (256,)), (256,), 1),
        ('down_fwd', ((4, 24, 24, 24, 64), (65536,), (128,)), (128,), 1),
        ('down_fwd', ((4, 48, 48, 48, 32), (16384,), (64,)), (64,), 1),
        ('down_fwd', ((4, 96, 96, 96, 16), (4096,), (32,)), (32,), 1),
        ('k2_pack_many', ((512,),), (8,), 0),
        ('norm_fwd', ((1, 12, 12, 12, 128),), (1, 1), 0),
        ('norm_fwd', ((1, 24, 24, 24, 64),), (1, 1), 0),
        ('norm_fwd', ((1, 48, 48, 48, 32),), (1, 1), 0),
        ('norm_fwd', ((1, 6, 6, 6, 256),), (1, 1), 0),
        ('norm_fwd', ((1, 96, 96, 96, 16),), (1, 1), 0),
        ('norm_fwd', ((4, 12, 12, 12, 128),), (4, 1), 0),
        ('norm_fwd', ((4, 24, 24, 24, 64),), (4, 1), 0),
        ('norm_fwd', ((4, 48, 48, 48, 32),), (4, 1), 0),
        ('norm_fwd', ((4, 6, 6, 6, 256),), (4, 1), 0),
        ('norm_fwd', ((4, 96, 96, 96, 16),), (4, 1), 0),
        ('overlap_counts', ((96, 96, 112), (96, 96, 112)), (0,), 0),
        ('pw16_fwd', ((1, 96, 96, 96, 16), (2, 16, 1, 1, 1), (2,)), (2,), 1),
        ('pw16_fwd', ((4, 96, 96, 96, 16), (2, 16, 1, 1, 1), (2,)), (2,), 1),
        ('sw_accumulate', ((96, 96, 96, 2), (96, 96, 112), (96, 96, 112)), (), 0),
        ('sw_finish', ((96, 96, 112), (96, 96, 112)), (), 0),
        ('up_fwd', ((1, 12, 12, 12, 128), (65536,), (64,)), (64,), 1),
        ('up_fwd', ((1, 24, 24, 24, 64), (16384,), (32,)), (32,), 1),
        ('up_fwd', ((1, 48, 48, 48, 32), (4096,), (16,)), (16,), 1),
        ('up_fwd', ((1, 6, 6, 6, 256), (262144,), (128,)), (128,), 1),
        ('up_fwd', ((4, 12, 12, 12, 128), (65536,), (64,)), (64,), 1),
        ('up_fwd', ((4, 24, 24, 24, 64), (16384,), (32,)), (32,), 1),
        ('up_fwd', ((4, 48, 48, 48, 32), (4096,), (16,)), (16,), 1),
        ('up_fwd', ((4, 6, 6, 6, 256), (262144,), (128,)), (128,), 1),
    ),
    "acdc_val": (
        ('bilinear2x_fwd', ((1, 1, 128, 128, 16), (1, 1, 256, 256, 32)), (16,), 0),
        ('bilinear2x_fwd', ((1, 1, 16, 16, 128), (1, 1, 32, 32, 256)), (128,), 0),
        ('bilinear2x_fwd', ((1, 1, 32, 32, 64), (1, 1, 64, 64, 128)), (64,), 0),
        ('bilinear2x_fwd', ((1, 1, 64, 64, 32), (1, 1, 128, 128, 64)), (32,), 0),
        ('bilinear2x_fwd', ((16, 1, 128, 128, 16), (16, 1, 256, 256, 32)), (16,), 0),
        ('bilinear2x_fwd', ((16, 1, 16, 16, 128), (16, 1, 32, 32, 256)), (128,), 0),
        ('bilinear2x_fwd', ((16, 1, 32, 32, 64), (16, 1, 64, 64, 128)), (64,), 0),
        ('bilinear2x_fwd', ((16, 1, 64, 64, 32), (16, 1, 128, 128, 64)), (32,), 0),
        ('conv3_c1_fwd', ((1, 1, 256, 256, 1), (16, 1, 3, 3), (16,)), (1,), 0),
        ('conv3_c1_fwd', ((16, 1, 256, 256, 1), (16, 1, 3, 3), (16,)), (1,), 0),
        ('conv3_fwd', ((1, 1, 128, 128, 16), (17440,), (32,)), (32, 1), 0),
        ('conv3_fwd', ((1, 1, 128, 128, 32), (34848,), (32,)), (32, 1), 0),
        ('conv3_fwd', ((1, 1, 128, 128, 64), (69664,), (32,)), (32, 1), 0),
        ('conv3_fwd', ((1, 1, 16, 16, 128), (1114144,), (256,)), (256, 1), 0),
        ('conv3_fwd', ((1, 1, 16, 16, 256), (2228256,), (256,)), (256, 1), 0),
        ('conv3_fwd', ((1, 1, 256, 256, 16), (8736,), (16,)), (16, 1), 0),
        ('conv3_fwd', ((1, 1, 256, 256, 16), (8736,), (4,)), (4, 1), 0),
        ('conv3_fwd', ((1, 1, 256, 256, 32), (17440,), (16,)), (16, 1), 0),
        ('conv3_fwd', ((1, 1, 32, 32, 128), (557088,), (128,)), (128, 1), 0),
        ('conv3_fwd', ((1, 1, 32, 32, 256), (1114144,), (128,)), (128, 1), 0),
        ('conv3_fwd', ((1, 1, 32, 32, 64), (278560,), (128,)), (128, 1), 0),
        ('conv3_fwd', ((1, 1, 64, 64, 128), (278560,), (64,)), (64, 1), 0),
        ('conv3_fwd', ((1, 1, 64, 64, 32), (69664,), (64,)), (64, 1), 0),
        ('conv3_fwd', ((1, 1, 64, 64, 64), (139296,), (64,)), (64, 1), 0),
        ('conv3_fwd', ((16, 1, 128, 128, 16), (17440,), (32,)), (32, 1), 0),
        ('conv3_fwd', ((16, 1, 128, 128, 32), (34848,), (32,)), (32, 1), 0),
        ('conv3_fwd', ((16, 1, 128, 128, 64), (69664,), (32,)), (32, 1), 0),
        ('conv3_fwd', ((16, 1, 16, 16, 128), (1114144,), (256,)), (256, 1), 0),
        ('conv3_fwd', ((16, 1, 16, 16, 256), (2228256,), (256,)), (256, 1), 0),
        ('conv3_fwd', ((16, 1, 256, 256, 16), (8736,), (16,)), (16, 1), 0),
        ('conv3_fwd', ((16, 1, 256, 256, 16), (8736,), (4,)), (4, 1), 0),
        ('conv3_fwd', ((16, 1, 256, 256, 32), (17440,), (16,)), (16, 1), 0),
        ('conv3_fwd', ((16, 1, 32, 32, 128), (557088,), (128,)), (128, 1), 0),
        ('conv3_fwd', ((16, 1, 32, 32, 256), (1114144,), (128,)), (128, 1), 0),
        ('conv3_fwd', ((16, 1, 32, 32, 64), (278560,), (128,)), (128, 1), 0),
        ('conv3_fwd', ((16, 1, 64, 64, 128), (278560,), (64,)), (64, 1), 0),
        ('conv3_fwd', ((16, 1, 64, 64, 32), (69664,), (64,)), (64, 1), 0),
        ('conv3_fwd', ((16, 1, 64, 64, 64), (139296,), (64,)), (64, 1), 0),
        ('conv3_pack_many', ((720,),), (18,), 0),
        ('copy_channels', ((1, 1, 128, 128, 32), (1, 1, 128, 128, 64)), (32, 0, 0), 0),
        ('copy_channels', ((1, 1, 256, 256, 16), (1, 1, 256, 256, 32)), (16, 0, 0), 0),
        ('copy_channels', ((1, 1, 32, 32, 128), (1, 1, 32, 32, 256)), (128, 0, 0), 0),
        ('copy_channels', ((1, 1, 64, 64, 64), (1, 1, 64, 64, 128)), (64, 0, 0), 0),
        ('copy_channels', ((16, 1, 128, 128, 32), (16, 1, 128, 128, 64)), (32, 0, 0), 0),
        ('copy_channels', ((16, 1, 256, 256, 16), (16, 1, 256, 256, 32)), (16, 0, 0), 0),
        ('copy_channels', ((16, 1, 32, 32, 128), (16, 1, 32, 32, 256)), (128, 0, 0), 0),
        ('copy_channels', ((16, 1, 64, 64, 64), (16, 1, 64, 64, 128)), (64, 0, 0), 0),
        ('k2_pack_many', ((256,),), (4,), 0),
        ('maxpool2d_fwd', ((1, 1, 128, 128, 32),), (), 0),
        ('maxpool2d_fwd', ((1, 1, 256, 256, 16),), (), 0),
        ('maxpool2d_fwd', ((1, 1, 32, 32, 128),), (), 0),
        ('maxpool2d_fwd', ((1, 1, 64, 64, 64),), (), 0),
        ('maxpool2d_fwd', ((16, 1, 128, 128, 32),), (), 0),
        ('maxpool2d_fwd', ((16, 1, 256, 256, 16),), (), 0),
        ('maxpool2d_fwd', ((16, 1, 32, 32, 128),), (), 0),
        ('maxpool2d_fwd', ((16, 1, 64, 64, 64),), (), 0),
        ('norm_eval', ((1, 1, 128, 128, 32), (32,), (32,)), (2,), 0),
        ('norm_eval', ((1, 1, 16, 16, 256), (256,), (256,)), (2,), 0),
        ('norm_eval', ((1, 1, 256, 256, 16), (16,), (16,)), (2,), 0),
        ('norm_eval', ((1, 1, 32, 32, 128), (128,), (128,)), (2,), 0),
        ('norm_eval', ((1, 1, 64, 64, 64), (64,), (64,)), (2,), 0),
        ('norm_eval', ((16, 1, 128, 128, 32), (32,), (32,)), (2,), 0),
        ('norm_eval', ((16, 1, 16, 16, 256), (256,), (256,)), (2,), 0),
        ('norm_eval', ((16, 1, 256, 256, 16), (16,), (16,)), (2,), 0),
        ('norm_eval', ((16, 1, 32, 32, 128), (128,), (128,)), (2,), 0),
        ('norm_eval', ((16, 1, 64, 64, 64), (64,), (64,)), (2,), 0),
        ('overlap_counts', ((17, 256, 256), (17, 256, 256)), (1,), 0),
        ('overlap_counts', ((17, 256, 256), (17, 256, 256)), (2,), 0),
        ('overlap_counts', ((17, 256, 256), (17, 256, 256)), (3,), 0),
        ('plabel_argmax4', ((1, 1, 256, 256, 4),), (), 0),
        ('plabel_argmax4', ((16, 1, 256, 256, 4),), (), 0),
        ('pw_fwd', ((1, 1, 128, 128, 32), (512,), (16,)), (16,), 0),
        ('pw_fwd', ((1, 1, 16, 16, 256), (32768,), (128,)), (128,), 0),
        ('pw_fwd', ((1, 1, 32, 32, 128), (8192,), (64,)), (64,), 0),
        ('pw_fwd', ((1, 1, 64, 64, 64), (2048,), (32,)), (32,), 0),
        ('pw_fwd', ((16, 1, 128, 128, 32), (512,), (16,)), (16,), 0),
        ('pw_fwd', ((16, 1, 16, 16, 256), (32768,), (128,)), (128,), 0),
        ('pw_fwd', ((16, 1, 32, 32, 128), (8192,), (64,)), (64,), 0),
        ('pw_fwd', ((16, 1, 64, 64, 64), (2048,), (32,)), (32,), 0),
    ),
    "la8": (
        ('conv3_c1_norm_bwd_wgrad', ((4, 112, 112, 80, 1), (16, 1, 3, 3, 3), (16,)), (3, 2, 1), 0),
        ('conv3_c1_norm_fwd', ((4, 112, 112, 80, 1), (16, 1, 3, 3, 3), (16,)), (3, 2, 1), 0),
        ('conv3_dgrad_bwdstats', ((4, 28, 28, 20, 64), (397344,), (4, 28, 28, 20, 64)), (64, 3, 1), 1),
        ('conv3_dgrad_bwdstats', ((4, 56, 56, 40, 32), (99360,), (4, 56, 56, 40, 32)), (32, 3, 1), 1),
        ('conv3_fwd', ((4, 112, 112, 80, 16), (24864,)), (16, 3), 1),
        ('conv3_fwd_raw', ((4, 14, 14, 10, 128), (1589280,)), (128, 3, 2), 1),
        ('conv3_fwd_raw', ((4, 7, 7, 5, 256), (6357024,)), (256, 3, 8), 1),
        ('conv3_fwd_stats', ((4, 112, 112, 80, 16), (24864,), (16,)), (16, 3, 2), 1),
        ('conv3_fwd_stats', ((4, 28, 28, 20, 64), (397344,), (64,)), (64, 3, 2), 1),
        ('conv3_fwd_stats', ((4, 56, 56, 40, 32), (99360,), (32,)), (32, 3, 2), 1),
        ('conv3_pack_many', ((1600,),), (40,), 0),
        ('conv3_pack_many', ((800,),), (20,), 0),
        ('conv3_wgrad', ((4, 112, 112, 80, 16), (4, 112, 112, 80, 16), (16, 16, 3, 3, 3)), (3,), 2),
        ('conv3_wgrad', ((4, 14, 14, 10, 128), (4, 14, 14, 10, 128), (128, 128, 3, 3, 3)), (3,), 2),
        ('conv3_wgrad', ((4, 28, 28, 20, 64), (4, 28, 28, 20, 64), (64, 64, 3, 3, 3)), (3,), 2),
        ('conv3_wgrad', ((4, 56, 56, 40, 32), (4, 56, 56, 40, 32), (32, 32, 3, 3, 3)), (3,), 2),
        ('conv3_wgrad', ((4, 7, 7, 5, 256), (4, 7, 7, 5, 256), (256, 256, 3, 3, 3)), (3,), 2),
        ('down_dgrad', ((4, 14, 14, 10, 128), (65536,)), (64,), 1),
        ('down_dgrad', ((4, 28, 28, 20, 64), (16384,)), (32,), 1),
        ('down_dgrad', ((4, 56, 56, 40, 32), (4096,)), (16,), 1),
        ('down_dgrad', ((4, 7, 7, 5, 256), (262144,)), (128,), 1),
        ('down_fwd', ((4, 112, 112, 80, 16), (4096,), (32,)), (32,), 1),
        ('down_fwd', ((4, 14, 14, 10, 128), (262144,), (256,)), (256,), 1),
        ('down_fwd', ((4, 28, 28, 20, 64), (65536,), (128,)), (128,), 1),
        ('down_fwd', ((4, 56, 56, 40, 32), (16384,), (64,)), (64,), 1),
        ('ema', ((9457332,), (9457332,)), (), 0),
        ('k2_fwd_stats', ((4, 56, 56, 40, 32), (4096,), (16,)), (1, 16, 2), 1),
        ('k2_pack_many', ((1024,),), (16,), 0),
        ('k2_pack_many', ((512,),), (8,), 0),
        ('k2_wgrad', ((4, 112, 112, 80, 16), (4, 56, 56, 40, 32), (32, 16, 2, 2, 2)), (0,), 2),
        ('k2_wgrad', ((4, 14, 14, 10, 128), (4, 28, 28, 20, 64), (128, 64, 2, 2, 2)), (1,), 2),
        ('k2_wgrad', ((4, 14, 14, 10, 128), (4, 7, 7, 5, 256), (256, 128, 2, 2, 2)), (0,), 2),
        ('k2_wgrad', ((4, 28, 28, 20, 64), (4, 14, 14, 10, 128), (128, 64, 2, 2, 2)), (0,), 2),
        ('k2_wgrad', ((4, 28, 28, 20, 64), (4, 56, 56, 40, 32), (64, 32, 2, 2, 2)), (1,), 2),
        ('k2_wgrad', ((4, 56, 56, 40, 32), (4, 112, 112, 80, 16), (32, 16, 2, 2, 2)), (1,), 2),
        ('k2_wgrad', ((4, 56, 56, 40, 32), (4, 28, 28, 20, 64), (64, 32, 2, 2, 2)), (0,), 2),
        ('k2_wgrad', ((4, 7, 7, 5, 256), (4, 14, 14, 10, 128), (256, 128, 2, 2, 2)), (1,), 2),
        ('mix_box', ((2, 112, 112, 80, 1), (2, 112, 112, 80, 1)), (), 0),
        ('mixloss_pair_bwd', ((4, 112, 112, 80, 2), (2, 112, 112, 80), (2, 112, 112, 80)), (0,), 0),
        ('mixloss_pair_fwd', ((4, 112, 112, 80, 2), (2, 112, 112, 80), (2, 112, 112, 80)), (0,), 0),
        ('norm_bwd', ((4, 112, 112, 80, 16), (4, 112, 112, 80, 16), (5, 2, 16)), (2, 1, True), 0),
        ('norm_bwd', ((4, 14, 14, 10, 128), (4, 14, 14, 10, 128), (5, 2, 128)), (2, 1, True), 0),
        ('norm_bwd', ((4, 28, 28, 20, 64), (4, 28, 28, 20, 64), (5, 2, 64)), (2, 1, True), 0),
        ('norm_bwd', ((4, 56, 56, 40, 32), (4, 56, 56, 40, 32), (5, 2, 32)), (2, 1, True), 0),
        ('norm_bwd', ((4, 7, 7, 5, 256), (4, 7, 7, 5, 256), (5, 2, 256)), (2, 1, True), 0),
        ('norm_bwd_slabs', ((4, 14, 14, 10, 128), (2, 4, 14, 14, 10, 128), (5, 2, 128)), (2, 2, 1), 0),
        ('norm_bwd_slabs', ((4, 7, 7, 5, 256), (8, 4, 7, 7, 5, 256), (5, 2, 256)), (8, 2, 1), 0),
        ('norm_fwd', ((4, 112, 112, 80, 16), (16,), (16,)), (2, 1), 0),
        ('norm_fwd', ((4, 14, 14, 10, 128), (128,), (128,)), (2, 1), 0),
        ('norm_fwd', ((4, 28, 28, 20, 64), (64,), (64,)), (2, 1), 0),
        ('norm_fwd', ((4, 56, 56, 40, 32), (32,), (32,)), (2, 1), 0),
        ('norm_fwd', ((4, 7, 7, 5, 256), (256,), (256,)), (2, 1), 0),
        ('norm_fwd_slabs', ((2, 4, 14, 14, 10, 128), (128,), (128,)), (2, 2, 1), 0),
        ('norm_fwd_slabs', ((8, 4, 7, 7, 5, 256), (256,), (256,)), (8, 2, 1), 0),
        ('plabel_cc_largest', ((4, 112, 112, 80, 2),), (3,), 0),
        ('pw16_bwd_norm_bwd', ((4, 112, 112, 80, 16), (5, 2, 16), (4, 16)), (2, 1), 0),
        ('pw16_fwd_norm', ((4, 112, 112, 80, 16), (5, 2, 16), (4, 16)), (2, 1, 2), 0),
        ('sgd', ((9448868,), (9448868,), (9448868,)), (), 0),
        ('up_dgrad', ((4, 112, 112, 80, 16), (4096,)), (32,), 1),
        ('up_dgrad', ((4, 14, 14, 10, 128), (262144,)), (256,), 1),
        ('up_dgrad', ((4, 28, 28, 20, 64), (65536,)), (128,), 1),
        ('up_dgrad', ((4, 56, 56, 40, 32), (16384,)), (64,), 1),
        ('up_fwd', ((4, 14, 14, 10, 128), (65536,), (64,)), (64,), 1),
        ('up_fwd', ((4, 28, 28, 20, 64), (16384,), (32,)), (32,), 1),
        ('up_fwd', ((4, 7, 7, 5, 256), (262144,), (128,)), (128,), 1),
    ),
    # the residual V-Net (has_residual=True): la, la_pre, la_val with residual networks
    "lares": (
        ('axpy', ((2, 7, 7, 5, 256), (2, 7, 7, 5, 256)), (), 0),
        ('axpy', ((2, 14, 14, 10, 128), (2, 14, 14, 10, 128)), (), 0),
        ('axpy', ((2, 28, 28, 20, 64), (2, 28, 28, 20, 64)), (), 0),
        ('axpy', ((2, 56, 56, 40, 32), (2, 56, 56, 40, 32)), (), 0),
        ('axpy', ((2, 112, 112, 80, 16), (2, 112, 112, 80, 16)), (), 0),
        ('conv3_c1_fwd_stats', ((2, 112, 112, 80, 1), (16, 1, 3, 3, 3), (16,)), (3, 2), 0),
        ('conv3_c1_wgrad', ((2, 112, 112, 80, 1), (2, 112, 112, 80, 16), (16, 1, 3, 3, 3)), (3,), 1),
        ('conv3_dgrad_bwdstats', ((2, 28, 28, 20, 64), (397344,), (2, 28, 28, 20, 64)), (64, 3, 1), 1),
        ('conv3_dgrad_bwdstats', ((2, 56, 56, 40, 32), (99360,), (2, 56, 56, 40, 32)), (32, 3, 1), 1),
        ('conv3_fwd', ((2, 7, 7, 5, 256), (6357024,)), (256, 3), 1),
        ('conv3_fwd', ((2, 7, 7, 5, 256), (6357024,), (256,)), (256, 3), 1),
        ('conv3_fwd', ((2, 14, 14, 10, 128), (1589280,)), (128, 3), 1),
        ('conv3_fwd', ((2, 14, 14, 10, 128), (1589280,), (128,)), (128, 3), 1),
        ('conv3_fwd', ((2, 28, 28, 20, 64), (397344,)), (64, 3), 1),
        ('conv3_fwd', ((2, 56, 56, 40, 32), (99360,)), (32, 3), 1),
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
        ('norm_bwd_res', ((2, 7, 7, 5, 256), (2, 7, 7, 5, 256), (2, 7, 7, 5, 256)), (2, 1, True), 0),
        ('norm_bwd_res', ((2, 14, 14, 10, 128), (2, 14, 14, 10, 128), (2, 14, 14, 10, 128)), (2, 1, True), 0),
        ('norm_bwd_res', ((2, 28, 28, 20, 64), (2, 28, 28, 20, 64), (2, 28, 28, 20, 64)), (2, 1, True), 0),
        ('norm_bwd_res', ((2, 56, 56, 40, 32), (2, 56, 56, 40, 32), (2, 56, 56, 40, 32)), (2, 1, True), 0),
        ('norm_bwd_res', ((2, 112, 112, 80, 16), (2, 112, 112, 80, 16), (2, 112, 112, 80, 1)), (2, 1, True), 0),
        ('norm_bwd_res', ((2, 112, 112, 80, 16), (2, 112, 112, 80, 16), (2, 112, 112, 80, 16)), (2, 1, True), 0),
        ('norm_bwd_slabs', ((2, 7, 7, 5, 256), (8, 2, 7, 7, 5, 256), (5, 2, 256)), (8, 2, 1), 0),
        ('norm_bwd_slabs', ((2, 14, 14, 10, 128), (4, 2, 14, 14, 10, 128), (5, 2, 128)), (4, 2, 1), 0),
        ('norm_fwd', ((2, 7, 7, 5, 256), (256,), (256,)), (2, 1), 0),
        ('norm_fwd', ((2, 14, 14, 10, 128), (128,), (128,)), (2, 1), 0),
        ('norm_fwd', ((2, 28, 28, 20, 64), (64,), (64,)), (2, 1), 0),
        ('norm_fwd', ((2, 56, 56, 40, 32), (32,), (32,)), (2, 1), 0),
        ('norm_fwd', ((2, 112, 112, 80, 16), (16,), (16,)), (2, 1), 0),
        ('norm_fwd_res', ((2, 7, 7, 5, 256), (256,), (256,)), (2, 1), 0),
        ('norm_fwd_res', ((2, 14, 14, 10, 128), (128,), (128,)), (2, 1), 0),
        ('norm_fwd_res', ((2, 28, 28, 20, 64), (64,), (64,)), (2, 1), 0),
        ('norm_fwd_res', ((2, 56, 56, 40, 32), (32,), (32,)), (2, 1), 0),
        ('norm_fwd_res', ((2, 112, 112, 80, 16), (16,), (16,)), (2, 1), 0),
        ('norm_fwd_slabs', ((4, 2, 14, 14, 10, 128), (128,), (128,)), (4, 2, 1), 0),
        ('norm_fwd_slabs', ((8, 2, 7, 7, 5, 256), (256,), (256,)), (8, 2, 1), 0),
        ('plabel_cc_largest', ((2, 112, 112, 80, 2),), (3,), 0),
        ('pw16_bwd', ((2, 112, 112, 80, 16), (2, 112, 112, 80, 2), (2, 16, 1, 1, 1)), (), 1),
        ('pw16_fwd', ((2, 112, 112, 80, 16), (2, 16, 1, 1, 1), (2,)), (2,), 1),
        ('sgd', ((9448868,), (9448868,), (9448868,)), (), 0),
        ('up_dgrad', ((2, 14, 14, 10, 128), (262144,)), (256,), 1),
        ('up_dgrad', ((2, 28, 28, 20, 64), (65536,)), (128,), 1),
        ('up_dgrad', ((2, 56, 56, 40, 32), (16384,)), (64,), 1),
        ('up_dgrad', ((2, 112, 112, 80, 16), (4096,)), (32,), 1),
        ('up_fwd', ((2, 7, 7, 5, 256), (262144,), (128,)), (128,), 1),
        ('up_fwd', ((2, 14, 14, 10, 128), (65536,), (64,)), (64,), 1),
        ('up_fwd', ((2, 28, 28, 20, 64), (16384,), (32,)), (32,), 1),
    ),
    "lares_pre": (
        ('axpy', ((1, 7, 7, 5, 256), (1, 7, 7, 5, 256)), (), 0),
        ('axpy', ((1, 14, 14, 10, 128), (1, 14, 14, 10, 128)), (), 0),
        ('axpy', ((1, 28, 28, 20, 64), (1, 28, 28, 20, 64)), (), 0),
        ('axpy', ((1, 56, 56, 40, 32), (1, 56, 56, 40, 32)), (), 0),
        ('axpy', ((1, 112, 112, 80, 16), (1, 112, 112, 80, 16)), (), 0),
        ('conv3_c1_fwd_stats', ((1, 112, 112, 80, 1), (16, 1, 3, 3, 3), (16,)), (3, 1), 0),
        ('conv3_c1_wgrad', ((1, 112, 112, 80, 1), (1, 112, 112, 80, 16), (16, 1, 3, 3, 3)), (3,), 1),
        ('conv3_dgrad_bwdstats', ((1, 56, 56, 40, 32), (99360,), (1, 56, 56, 40, 32)), (32, 3, 1), 1),
        ('conv3_fwd', ((1, 7, 7, 5, 256), (6357024,)), (256, 3), 1),
        ('conv3_fwd', ((1, 7, 7, 5, 256), (6357024,), (256,)), (256, 3), 1),
        ('conv3_fwd', ((1, 14, 14, 10, 128), (1589280,)), (128, 3), 1),
        ('conv3_fwd', ((1, 14, 14, 10, 128), (1589280,), (128,)), (128, 3), 1),
        ('conv3_fwd', ((1, 28, 28, 20, 64), (397344,)), (64, 3), 1),
        ('conv3_fwd', ((1, 56, 56, 40, 32), (99360,)), (32, 3), 1),
        ('conv3_fwd', ((1, 112, 112, 80, 16), (24864,)), (16, 3), 1),
        ('conv3_fwd_raw', ((1, 14, 14, 10, 128), (1589280,)), (128, 3, 4), 1),
        ('conv3_fwd_stats', ((1, 28, 28, 20, 64), (397344,), (64,)), (64, 3, 1), 1),
        ('conv3_fwd_stats', ((1, 56, 56, 40, 32), (99360,), (32,)), (32, 3, 1), 1),
        ('conv3_fwd_stats', ((1, 112, 112, 80, 16), (24864,), (16,)), (16, 3, 1), 1),
        ('conv3_pack_many', ((1600,),), (40,), 0),
        ('conv3_wgrad', ((1, 7, 7, 5, 256), (1, 7, 7, 5, 256), (256, 256, 3, 3, 3)), (3,), 2),
        ('conv3_wgrad', ((1, 14, 14, 10, 128), (1, 14, 14, 10, 128), (128, 128, 3, 3, 3)), (3,), 2),
        ('conv3_wgrad', ((1, 28, 28, 20, 64), (1, 28, 28, 20, 64), (64, 64, 3, 3, 3)), (3,), 2),
        ('conv3_wgrad', ((1, 56, 56, 40, 32), (1, 56, 56, 40, 32), (32, 32, 3, 3, 3)), (3,), 2),
        ('conv3_wgrad', ((1, 112, 112, 80, 16), (1, 112, 112, 80, 16), (16, 16, 3, 3, 3)), (3,), 2),
        ('down_dgrad', ((1, 7, 7, 5, 256), (262144,)), (128,), 1),
        ('down_dgrad', ((1, 14, 14, 10, 128), (65536,)), (64,), 1),
        ('down_dgrad', ((1, 28, 28, 20, 64), (16384,)), (32,), 1),
        ('down_dgrad', ((1, 56, 56, 40, 32), (4096,)), (16,), 1),
        ('down_fwd', ((1, 14, 14, 10, 128), (262144,), (256,)), (256,), 1),
        ('down_fwd', ((1, 28, 28, 20, 64), (65536,), (128,)), (128,), 1),
        ('down_fwd', ((1, 56, 56, 40, 32), (16384,), (64,)), (64,), 1),
        ('down_fwd', ((1, 112, 112, 80, 16), (4096,), (32,)), (32,), 1),
        ('k2_pack_many', ((1024,),), (16,), 0),
        ('k2_wgrad', ((1, 7, 7, 5, 256), (1, 14, 14, 10, 128), (256, 128, 2, 2, 2)), (1,), 2),
        ('k2_wgrad', ((1, 14, 14, 10, 128), (1, 7, 7, 5, 256), (256, 128, 2, 2, 2)), (0,), 2),
        ('k2_wgrad', ((1, 14, 14, 10, 128), (1, 28, 28, 20, 64), (128, 64, 2, 2, 2)), (1,), 2),
        ('k2_wgrad', ((1, 28, 28, 20, 64), (1, 14, 14, 10, 128), (128, 64, 2, 2, 2)), (0,), 2),
        ('k2_wgrad', ((1, 28, 28, 20, 64), (1, 56, 56, 40, 32), (64, 32, 2, 2, 2)), (1,), 2),
        ('k2_wgrad', ((1, 56, 56, 40, 32), (1, 28, 28, 20, 64), (64, 32, 2, 2, 2)), (0,), 2),
        ('k2_wgrad', ((1, 56, 56, 40, 32), (1, 112, 112, 80, 16), (32, 16, 2, 2, 2)), (1,), 2),
        ('k2_wgrad', ((1, 112, 112, 80, 16), (1, 56, 56, 40, 32), (32, 16, 2, 2, 2)), (0,), 2),
        ('mix_box', ((1, 112, 112, 80, 1), (1, 112, 112, 80, 1)), (), 0),
        ('mixloss_bwd', ((1, 112, 112, 80, 2), (1, 112, 112, 80), (1, 112, 112, 80)), (0,), 0),
        ('mixloss_fwd', ((1, 112, 112, 80, 2), (1, 112, 112, 80), (1, 112, 112, 80)), (0,), 0),
        ('norm_bwd', ((1, 7, 7, 5, 256), (1, 7, 7, 5, 256), (5, 1, 256)), (1, 1, True), 0),
        ('norm_bwd', ((1, 14, 14, 10, 128), (1, 14, 14, 10, 128), (5, 1, 128)), (1, 1, True), 0),
        ('norm_bwd', ((1, 28, 28, 20, 64), (1, 28, 28, 20, 64), (5, 1, 64)), (1, 1, True), 0),
        ('norm_bwd', ((1, 56, 56, 40, 32), (1, 56, 56, 40, 32), (5, 1, 32)), (1, 1, True), 0),
        ('norm_bwd', ((1, 112, 112, 80, 16), (1, 112, 112, 80, 16), (5, 1, 16)), (1, 1, True), 0),
        ('norm_bwd_res', ((1, 7, 7, 5, 256), (1, 7, 7, 5, 256), (1, 7, 7, 5, 256)), (1, 1, True), 0),
        ('norm_bwd_res', ((1, 14, 14, 10, 128), (1, 14, 14, 10, 128), (1, 14, 14, 10, 128)), (1, 1, True), 0),
        ('norm_bwd_res', ((1, 28, 28, 20, 64), (1, 28, 28, 20, 64), (1, 28, 28, 20, 64)), (1, 1, True), 0),
        ('norm_bwd_res', ((1, 56, 56, 40, 32), (1, 56, 56, 40, 32), (1, 56, 56, 40, 32)), (1, 1, True), 0),
        ('norm_bwd_res', ((1, 112, 112, 80, 16), (1, 112, 112, 80, 16), (1, 112, 112, 80, 1)), (1, 1, True), 0),
        ('norm_bwd_res', ((1, 112, 112, 80, 16), (1, 112, 112, 80, 16), (1, 112, 112, 80, 16)), (1, 1, True), 0),
        ('norm_bwd_slabs', ((1, 14, 14, 10, 128), (4, 1, 14, 14, 10, 128), (5, 1, 128)), (4, 1, 1), 0),
        ('norm_fwd', ((1, 7, 7, 5, 256), (256,), (256,)), (1, 1), 0),
        ('norm_fwd', ((1, 14, 14, 10, 128), (128,), (128,)), (1, 1), 0),
        ('norm_fwd', ((1, 28, 28, 20, 64), (64,), (64,)), (1, 1), 0),
        ('norm_fwd', ((1, 56, 56, 40, 32), (32,), (32,)), (1, 1), 0),
        ('norm_fwd', ((1, 112, 112, 80, 16), (16,), (16,)), (1, 1), 0),
        ('norm_fwd_res', ((1, 7, 7, 5, 256), (256,), (256,)), (1, 1), 0),
        ('norm_fwd_res', ((1, 14, 14, 10, 128), (128,), (128,)), (1, 1), 0),
        ('norm_fwd_res', ((1, 28, 28, 20, 64), (64,), (64,)), (1, 1), 0),
        ('norm_fwd_res', ((1, 56, 56, 40, 32), (32,), (32,)), (1, 1), 0),
        ('norm_fwd_res', ((1, 112, 112, 80, 16), (16,), (16,)), (1, 1), 0),
        ('norm_fwd_slabs', ((4, 1, 14, 14, 10, 128), (128,), (128,)), (4, 1, 1), 0),
        ('pw16_bwd', ((1, 112, 112, 80, 16), (1, 112, 112, 80, 2), (2, 16, 1, 1, 1)), (), 1),
        ('pw16_fwd', ((1, 112, 112, 80, 16), (2, 16, 1, 1, 1), (2,)), (2,), 1),
        ('sgd', ((9448868,), (9448868,), (9448868,)), (), 0),
        ('up_dgrad', ((1, 14, 14, 10, 128), (262144,)), (256,), 1),
        ('up_dgrad', ((1, 28, 28, 20, 64), (65536,)), (128,), 1),
        ('up_dgrad', ((1, 56, 56, 40, 32), (16384,)), (64,), 1),
        ('up_dgrad', ((1, 112, 112, 80, 16), (4096,)), (32,), 1),
        ('up_fwd', ((1, 7, 7, 5, 256), (262144,), (128,)), (128,), 1),
        ('up_fwd', ((1, 14, 14, 10, 128), (65536,), (64,)), (64,), 1),
        ('up_fwd', ((1, 28, 28, 20, 64), (16384,), (32,)), (32,), 1),
        ('up_fwd', ((1, 56, 56, 40, 32), (4096,), (16,)), (16,), 1),
    ),
    "lares_val": (
        ('conv3_c1_fwd', ((1, 112, 112, 80, 1), (16, 1, 3, 3, 3), (16,)), (3,), 0),
        ('conv3_c1_fwd', ((4, 112, 112, 80, 1), (16, 1, 3, 3, 3), (16,)), (3,), 0),
        ('conv3_fwd', ((1, 7, 7, 5, 256), (6357024,), (256,)), (256, 3), 0),
        ('conv3_fwd', ((1, 14, 14, 10, 128), (1589280,), (128,)), (128, 3), 0),
        ('conv3_fwd', ((1, 28, 28, 20, 64), (397344,), (64,)), (64, 3), 0),
        ('conv3_fwd', ((1, 56, 56, 40, 32), (99360,), (32,)), (32, 3), 0),
        ('conv3_fwd', ((1, 112, 112, 80, 16), (24864,), (16,)), (16, 3), 0),
        ('conv3_fwd', ((4, 7, 7, 5, 256), (6357024,), (256,)), (256, 3), 0),
        ('conv3_fwd', ((4, 14, 14, 10, 128), (1589280,), (128,)), (128, 3), 0),
        ('conv3_fwd', ((4, 28, 28, 20, 64), (397344,), (64,)), (64, 3), 0),
        ('conv3_fwd', ((4, 56, 56, 40, 32), (99360,), (32,)), (32, 3), 0),
        ('conv3_fwd', ((4, 112, 112, 80, 16), (24864,), (16,)), (16, 3), 0),
        ('conv3_pack_many', ((800,),), (20,), 0),
        ('down_fwd', ((1, 14, 14, 10, 128), (262144,), (256,)), (256,), 0),
        ('down_fwd', ((1, 28, 28, 20, 64), (65536,), (128,)), (128,), 0),
        ('down_fwd', ((1, 56, 56, 40, 32), (16384,), (64,)), (64,), 0),
        ('down_fwd', ((1, 112, 112, 80, 16), (4096,), (32,)), (32,), 0),
        ('down_fwd', ((4, 14, 14, 10, 128), (262144,), (256,)), (256,), 0),
        ('down_fwd', ((4, 28, 28, 20, 64), (65536,), (128,)), (128,), 0),
        ('down_fwd', ((4, 56, 56, 40, 32), (16384,), (64,)), (64,), 0),
        ('down_fwd', ((4, 112, 112, 80, 16), (4096,), (32,)), (32,), 0),
        ('k2_pack_many', ((512,),), (8,), 0),
        ('norm_eval', ((1, 7, 7, 5, 256), (256,), (256,)), (1,), 0),
        ('norm_eval', ((1, 14, 14, 10, 128), (128,), (128,)), (1,), 0),
        ('norm_eval', ((1, 28, 28, 20, 64), (64,), (64,)), (1,), 0),
        ('norm_eval', ((1, 56, 56, 40, 32), (32,), (32,)), (1,), 0),
        ('norm_eval', ((1, 112, 112, 80, 16), (16,), (16,)), (1,), 0),
        ('norm_eval', ((4, 7, 7, 5, 256), (256,), (256,)), (1,), 0),
        ('norm_eval', ((4, 14, 14, 10, 128), (128,), (128,)), (1,), 0),
        ('norm_eval', ((4, 28, 28, 20, 64), (64,), (64,)), (1,), 0),
        ('norm_eval', ((4, 56, 56, 40, 32), (32,), (32,)), (1,), 0),
        ('norm_eval', ((4, 112, 112, 80, 16), (16,), (16,)), (1,), 0),
        ('norm_eval_res', ((1, 7, 7, 5, 256), (256,), (256,)), (1,), 0),
        ('norm_eval_res', ((1, 14, 14, 10, 128), (128,), (128,)), (1,), 0),
        ('norm_eval_res', ((1, 28, 28, 20, 64), (64,), (64,)), (1,), 0),
        ('norm_eval_res', ((1, 56, 56, 40, 32), (32,), (32,)), (1,), 0),
        ('norm_eval_res', ((1, 112, 112, 80, 16), (16,), (16,)), (1,), 0),
        ('norm_eval_res', ((4, 7, 7, 5, 256), (256,), (256,)), (1,), 0),
        ('norm_eval_res', ((4, 14, 14, 10, 128), (128,), (128,)), (1,), 0),
        ('norm_eval_res', ((4, 28, 28, 20, 64), (64,), (64,)), (1,), 0),
        ('norm_eval_res', ((4, 56, 56, 40, 32), (32,), (32,)), (1,), 0),
        ('norm_eval_res', ((4, 112, 112, 80, 16), (16,), (16,)), (1,), 0),
        ('overlap_counts', ((112, 112, 96), (112, 112, 96)), (0,), 0),
        ('pw16_fwd', ((1, 112, 112, 80, 16), (2, 16, 1, 1, 1), (2,)), (2,), 0),
        ('pw16_fwd', ((4, 112, 112, 80, 16), (2, 16, 1, 1, 1), (2,)), (2,), 0),
        ('sw_accumulate', ((112, 112, 80, 2), (112, 112, 96), (112, 112, 96)), (), 0),
        ('sw_finish', ((112, 112, 96), (112, 112, 96)), (), 0),
        ('up_fwd', ((1, 7, 7, 5, 256), (262144,), (128,)), (128,), 0),
        ('up_fwd', ((1, 14, 14, 10, 128), (65536,), (64,)), (64,), 0),
        ('up_fwd', ((1, 28, 28, 20, 64), (16384,), (32,)), (32,), 0),
        ('up_fwd', ((1, 56, 56, 40, 32), (4096,), (16,)), (16,), 0),
        ('up_fwd', ((4, 7, 7, 5, 256), (262144,), (128,)), (128,), 0),
        ('up_fwd', ((4, 14, 14, 10, 128), (65536,), (64,)), (64,), 0),
        ('up_fwd', ((4, 28, 28, 20, 64), (16384,), (32,)), (32,), 0),
        ('up_fwd', ((4, 56, 56, 40, 32), (4096,), (16,)), (16,), 0),
    ),
    "lagn": (
        ('conv3_c1_fwd_stats', ((2, 112, 112, 80, 1), (16, 1, 3, 3, 3), (16,)), (3, 2), 0),
        ('conv3_c1_wgrad', ((2, 112, 112, 80, 1), (2, 112, 112, 80, 16), (16, 1, 3, 3, 3)), (3,), 1),
        ('conv3_dgrad_bwdstats', ((2, 28, 28, 20, 64), (397344,), (2, 28, 28, 20, 64)), (64, 3, 1), 1),
        ('conv3_dgrad_bwdstats', ((2, 56, 56, 40, 32), (99360,), (2, 56, 56, 40, 32)), (32, 3, 1), 1),
        ('conv3_fwd', ((2, 7, 7, 5, 256), (6357024,)), (256, 3), 1),
        ('conv3_fwd', ((2, 7, 7, 5, 256), (6357024,), (256,)), (256, 3), 1),
        ('conv3_fwd', ((2, 14, 14, 10, 128), (1589280,)), (128, 3), 1),
        ('conv3_fwd', ((2, 14, 14, 10, 128), (1589280,), (128,)), (128, 3), 1),
        ('conv3_fwd', ((2, 112, 112, 80, 16), (24864,)), (16, 3), 1),
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
        ('gnorm_bwd', ((2, 7, 7, 5, 256), (2, 7, 7, 5, 256), (5, 2, 256)), (1, 1), 0),
        ('gnorm_bwd', ((2, 14, 14, 10, 128), (2, 14, 14, 10, 128), (5, 2, 128)), (1, 1), 0),
        ('gnorm_bwd', ((2, 28, 28, 20, 64), (2, 28, 28, 20, 64), (5, 2, 64)), (1, 1), 0),
        ('gnorm_bwd', ((2, 56, 56, 40, 32), (2, 56, 56, 40, 32), (5, 2, 32)), (1, 1), 0),
        ('gnorm_bwd', ((2, 112, 112, 80, 16), (2, 112, 112, 80, 16), (5, 2, 16)), (1, 1), 0),
        ('gnorm_fwd', ((2, 7, 7, 5, 256), (256,), (256,)), (1,), 0),
        ('gnorm_fwd', ((2, 14, 14, 10, 128), (128,), (128,)), (1,), 0),
        ('gnorm_fwd', ((2, 28, 28, 20, 64), (64,), (64,)), (1,), 0),
        ('gnorm_fwd', ((2, 56, 56, 40, 32), (32,), (32,)), (1,), 0),
        ('gnorm_fwd', ((2, 112, 112, 80, 16), (16,), (16,)), (1,), 0),
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
        ('plabel_cc_largest', ((2, 112, 112, 80, 2),), (3,), 0),
        ('pw16_bwd_norm', ((2, 112, 112, 80, 16), (5, 2, 16), (2, 16)), (2, 1), 0),
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
    "lagn_pre": (
        ('conv3_c1_fwd_stats', ((1, 112, 112, 80, 1), (16, 1, 3, 3, 3), (16,)), (3, 1), 0),
        ('conv3_c1_wgrad', ((1, 112, 112, 80, 1), (1, 112, 112, 80, 16), (16, 1, 3, 3, 3)), (3,), 1),
        ('conv3_dgrad_bwdstats', ((1, 56, 56, 40, 32), (99360,), (1, 56, 56, 40, 32)), (32, 3, 1), 1),
        ('conv3_fwd', ((1, 7, 7, 5, 256), (6357024,)), (256, 3), 1),
        ('conv3_fwd', ((1, 7, 7, 5, 256), (6357024,), (256,)), (256, 3), 1),
        ('conv3_fwd', ((1, 14, 14, 10, 128), (1589280,)), (128, 3), 1),
        ('conv3_fwd', ((1, 14, 14, 10, 128), (1589280,), (128,)), (128, 3), 1),
        ('conv3_fwd', ((1, 28, 28, 20, 64), (397344,)), (64, 3), 1),
        ('conv3_fwd', ((1, 112, 112, 80, 16), (24864,)), (16, 3), 1),
        ('conv3_fwd_stats', ((1, 28, 28, 20, 64), (397344,), (64,)), (64, 3, 1), 1),
        ('conv3_fwd_stats', ((1, 56, 56, 40, 32), (99360,), (32,)), (32, 3, 1), 1),
        ('conv3_fwd_stats', ((1, 112, 112, 80, 16), (24864,), (16,)), (16, 3, 1), 1),
        ('conv3_pack_many', ((1600,),), (40,), 0),
        ('conv3_wgrad', ((1, 7, 7, 5, 256), (1, 7, 7, 5, 256), (256, 256, 3, 3, 3)), (3,), 2),
        ('conv3_wgrad', ((1, 14, 14, 10, 128), (1, 14, 14, 10, 128), (128, 128, 3, 3, 3)), (3,), 2),
        ('conv3_wgrad', ((1, 28, 28, 20, 64), (1, 28, 28, 20, 64), (64, 64, 3, 3, 3)), (3,), 2),
        ('conv3_wgrad', ((1, 56, 56, 40, 32), (1, 56, 56, 40, 32), (32, 32, 3, 3, 3)), (3,), 2),
        ('conv3_wgrad', ((1, 112, 112, 80, 16), (1, 112, 112, 80, 16), (16, 16, 3, 3, 3)), (3,), 2),
        ('down_dgrad', ((1, 7, 7, 5, 256), (262144,)), (128,), 1),
        ('down_dgrad', ((1, 14, 14, 10, 128), (65536,)), (64,), 1),
        ('down_dgrad', ((1, 28, 28, 20, 64), (16384,)), (32,), 1),
        ('down_dgrad', ((1, 56, 56, 40, 32), (4096,)), (16,), 1),
        ('down_fwd', ((1, 14, 14, 10, 128), (262144,), (256,)), (256,), 1),
        ('down_fwd', ((1, 28, 28, 20, 64), (65536,), (128,)), (128,), 1),
        ('down_fwd', ((1, 56, 56, 40, 32), (16384,), (64,)), (64,), 1),
        ('down_fwd', ((1, 112, 112, 80, 16), (4096,), (32,)), (32,), 1),
        ('gnorm_bwd', ((1, 7, 7, 5, 256), (1, 7, 7, 5, 256), (5, 1, 256)), (1, 1), 0),
        ('gnorm_bwd', ((1, 14, 14, 10, 128), (1, 14, 14, 10, 128), (5, 1, 128)), (1, 1), 0),
        ('gnorm_bwd', ((1, 28, 28, 20, 64), (1, 28, 28, 20, 64), (5, 1, 64)), (1, 1), 0),
        ('gnorm_bwd', ((1, 56, 56, 40, 32), (1, 56, 56, 40, 32), (5, 1, 32)), (1, 1), 0),
        ('gnorm_bwd', ((1, 112, 112, 80, 16), (1, 112, 112, 80, 16), (5, 1, 16)), (1, 1), 0),
        ('gnorm_fwd', ((1, 7, 7, 5, 256), (256,), (256,)), (1,), 0),
        ('gnorm_fwd', ((1, 14, 14, 10, 128), (128,), (128,)), (1,), 0),
        ('gnorm_fwd', ((1, 28, 28, 20, 64), (64,), (64,)), (1,), 0),
        ('gnorm_fwd', ((1, 56, 56, 40, 32), (32,), (32,)), (1,), 0),
        ('gnorm_fwd', ((1, 112, 112, 80, 16), (16,), (16,)), (1,), 0),
        ('k2_pack_many', ((1024,),), (16,), 0),
        ('k2_wgrad', ((1, 7, 7, 5, 256), (1, 14, 14, 10, 128), (256, 128, 2, 2, 2)), (1,), 2),
        ('k2_wgrad', ((1, 14, 14, 10, 128), (1, 7, 7, 5, 256), (256, 128, 2, 2, 2)), (0,), 2),
        ('k2_wgrad', ((1, 14, 14, 10, 128), (1, 28, 28, 20, 64), (128, 64, 2, 2, 2)), (1,), 2),
        ('k2_wgrad', ((1, 28, 28, 20, 64), (1, 14, 14, 10, 128), (128, 64, 2, 2, 2)), (0,), 2),
        ('k2_wgrad', ((1, 28, 28, 20, 64), (1, 56, 56, 40, 32), (64, 32, 2, 2, 2)), (1,), 2),
        ('k2_wgrad', ((1, 56, 56, 40, 32), (1, 28, 28, 20, 64), (64, 32, 2, 2, 2)), (0,), 2),
        ('k2_wgrad', ((1, 56, 56, 40, 32), (1, 112, 112, 80, 16), (32, 16, 2, 2, 2)), (1,), 2),
        ('k2_wgrad', ((1, 112, 112, 80, 16), (1, 56, 56, 40, 32), (32, 16, 2, 2, 2)), (0,), 2),
        ('mix_box', ((1, 112, 112, 80, 1), (1, 112, 112, 80, 1)), (), 0),
        ('mixloss_bwd', ((1, 112, 112, 80, 2), (1, 112, 112, 80), (1, 112, 112, 80)), (0,), 0),
        ('mixloss_fwd', ((1, 112, 112, 80, 2), (1, 112, 112, 80), (1, 112, 112, 80)), (0,), 0),
        ('pw16_bwd_norm', ((1, 112, 112, 80, 16), (5, 1, 16), (1, 16)), (1, 1), 0),
        ('pw16_fwd_norm', ((1, 112, 112, 80, 16), (5, 1, 16), (1, 16)), (1, 1, 2), 0),
        ('sgd', ((9448868,), (9448868,), (9448868,)), (), 0),
        ('up_dgrad', ((1, 14, 14, 10, 128), (262144,)), (256,), 1),
        ('up_dgrad', ((1, 28, 28, 20, 64), (65536,)), (128,), 1),
        ('up_dgrad', ((1, 56, 56, 40, 32), (16384,)), (64,), 1),
        ('up_dgrad', ((1, 112, 112, 80, 16), (4096,)), (32,), 1),
        ('up_fwd', ((1, 7, 7, 5, 256), (262144,), (128,)), (128,), 1),
        ('up_fwd', ((1, 14, 14, 10, 128), (65536,), (64,)), (64,), 1),
        ('up_fwd', ((1, 28, 28, 20, 64), (16384,), (32,)), (32,), 1),
        ('up_fwd', ((1, 56, 56, 40, 32), (4096,), (16,)), (16,), 1),
    ),
    "lagn_val": (
        ('conv3_c1_fwd_stats', ((1, 112, 112, 80, 1), (16, 1, 3, 3, 3), (16,)), (3, 1), 0),
        ('conv3_c1_fwd_stats', ((4, 112, 112, 80, 1), (16, 1, 3, 3, 3), (16,)), (3, 4), 0),
        ('conv3_fwd', ((1, 7, 7, 5, 256), (6357024,), (256,)), (256, 3), 1),
        ('conv3_fwd', ((1, 14, 14, 10, 128), (1589280,), (128,)), (128, 3), 1),
        ('conv3_fwd', ((4, 7, 7, 5, 256), (6357024,), (256,)), (256, 3), 1),
        ('conv3_fwd', ((4, 14, 14, 10, 128), (1589280,), (128,)), (128, 3), 1),
        ('conv3_fwd_stats', ((1, 7, 7, 5, 256), (6357024,), (256,)), (256, 3, 1), 1),
        ('conv3_fwd_stats', ((1, 14, 14, 10, 128), (1589280,), (128,)), (128, 3, 1), 1),
        ('conv3_fwd_stats', ((1, 28, 28, 20, 64), (397344,), (64,)), (64, 3, 1), 1),
        ('conv3_fwd_stats', ((1, 56, 56, 40, 32), (99360,), (32,)), (32, 3, 1), 1),
        ('conv3_fwd_stats', ((1, 112, 112, 80, 16), (24864,), (16,)), (16, 3, 1), 1),
        ('conv3_fwd_stats', ((4, 7, 7, 5, 256), (6357024,), (256,)), (256, 3, 4), 1),
        ('conv3_fwd_stats', ((4, 14, 14, 10, 128), (1589280,), (128,)), (128, 3, 4), 1),
        ('conv3_fwd_stats', ((4, 28, 28, 20, 64), (397344,), (64,)), (64, 3, 4), 1),
        ('conv3_fwd_stats', ((4, 56, 56, 40, 32), (99360,), (32,)), (32, 3, 4), 1),
        ('conv3_fwd_stats', ((4, 112, 112, 80, 16), (24864,), (16,)), (16, 3, 4), 1),
        ('conv3_pack_many', ((800,),), (20,), 0),
        ('down_fwd', ((1, 14, 14, 10, 128), (262144,), (256,)), (256,), 1),
        ('down_fwd', ((1, 28, 28, 20, 64), (65536,), (128,)), (128,), 1),
        ('down_fwd', ((1, 56, 56, 40, 32), (16384,), (64,)), (64,), 1),
        ('down_fwd', ((1, 112, 112, 80, 16), (4096,), (32,)), (32,), 1),
        ('down_fwd', ((4, 14, 14, 10, 128), (262144,), (256,)), (256,), 1),
        ('down_fwd', ((4, 28, 28, 20, 64), (65536,), (128,)), (128,), 1),
        ('down_fwd', ((4, 56, 56, 40, 32), (16384,), (64,)), (64,), 1),
        ('down_fwd', ((4, 112, 112, 80, 16), (4096,), (32,)), (32,), 1),
        ('gnorm_fwd', ((1, 7, 7, 5, 256), (256,), (256,)), (1,), 0),
        ('gnorm_fwd', ((1, 14, 14, 10, 128), (128,), (128,)), (1,), 0),
        ('gnorm_fwd', ((1, 28, 28, 20, 64), (64,), (64,)), (1,), 0),
        ('gnorm_fwd', ((1, 56, 56, 40, 32), (32,), (32,)), (1,), 0),
        ('gnorm_fwd', ((1, 112, 112, 80, 16), (16,), (16,)), (1,), 0),
        ('gnorm_fwd', ((4, 7, 7, 5, 256), (256,), (256,)), (1,), 0),
        ('gnorm_fwd', ((4, 14, 14, 10, 128), (128,), (128,)), (1,), 0),
        ('gnorm_fwd', ((4, 28, 28, 20, 64), (64,), (64,)), (1,), 0),
        ('gnorm_fwd', ((4, 56, 56, 40, 32), (32,), (32,)), (1,), 0),
        ('gnorm_fwd', ((4, 112, 112, 80, 16), (16,), (16,)), (1,), 0),
        ('k2_fwd_stats', ((4, 56, 56, 40, 32), (4096,), (16,)), (1, 16, 4), 1),
        ('k2_pack_many', ((512,),), (8,), 0),
        ('overlap_counts', ((112, 112, 96), (112, 112, 96)), (0,), 0),
        ('pw16_fwd_norm', ((1, 112, 112, 80, 16), (5, 1, 16), (2, 16, 1, 1, 1)), (1, 1, 2), 0),
        ('pw16_fwd_norm', ((4, 112, 112, 80, 16), (5, 4, 16), (2, 16, 1, 1, 1)), (4, 1, 2), 0),
        ('sw_accumulate', ((112, 112, 80, 2), (112, 112, 96), (112, 112, 96)), (), 0),
        ('sw_finish', ((112, 112, 96), (112, 112, 96)), (), 0),
        ('up_fwd', ((1, 7, 7, 5, 256), (262144,), (128,)), (128,), 1),
        ('up_fwd', ((1, 14, 14, 10, 128), (65536,), (64,)), (64,), 1),
        ('up_fwd', ((1, 28, 28, 20, 64), (16384,), (32,)), (32,), 1),
        ('up_fwd', ((1, 56, 56, 40, 32), (4096,), (16,)), (16,), 1),
        ('up_fwd', ((4, 7, 7, 5, 256), (262144,), (128,)), (128,), 1),
        ('up_fwd', ((4, 14, 14, 10, 128), (65536,), (64,)), (64,), 1),
        ('up_fwd', ((4, 28, 28, 20, 64), (16384,), (32,)), (32,), 1),
    ),
    "pancreasgn": (
        ('adam', ((9448868,), (9448868,), (9448868,)), (3,), 0),
        ('conv3_c1_fwd_stats', ((2, 96, 96, 96, 1), (16, 1, 3, 3, 3), (16,)), (3, 2), 0),
        ('conv3_c1_wgrad', ((2, 96, 96, 96, 1), (2, 96, 96, 96, 16), (16, 1, 3, 3, 3)), (3,), 1),
        ('conv3_dgrad_bwdstats', ((2, 24, 24, 24, 64), (397344,), (2, 24, 24, 24, 64)), (64, 3, 1), 1),
        ('conv3_dgrad_bwdstats', ((2, 48, 48, 48, 32), (99360,), (2, 48, 48, 48, 32)), (32, 3, 1), 1),
        ('conv3_fwd', ((2, 6, 6, 6, 256), (6357024,)), (256, 3), 1),
        ('conv3_fwd', ((2, 6, 6, 6, 256), (6357024,), (256,)), (256, 3), 1),
        ('conv3_fwd', ((2, 12, 12, 12, 128), (1589280,)), (128, 3), 1),
        ('conv3_fwd', ((2, 12, 12, 12, 128), (1589280,), (128,)), (128, 3), 1),
        ('conv3_fwd', ((2, 96, 96, 96, 16), (24864,)), (16, 3), 1),
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
        ('ema', ((9448868,), (9448868,)), (), 0),
        ('gnorm_bwd', ((2, 6, 6, 6, 256), (2, 6, 6, 6, 256), (5, 2, 256)), (1, 1), 0),
        ('gnorm_bwd', ((2, 12, 12, 12, 128), (2, 12, 12, 12, 128), (5, 2, 128)), (1, 1), 0),
        ('gnorm_bwd', ((2, 24, 24, 24, 64), (2, 24, 24, 24, 64), (5, 2, 64)), (1, 1), 0),
        ('gnorm_bwd', ((2, 48, 48, 48, 32), (2, 48, 48, 48, 32), (5, 2, 32)), (1, 1), 0),
        ('gnorm_bwd', ((2, 96, 96, 96, 16), (2, 96, 96, 96, 16), (5, 2, 16)), (1, 1), 0),
        ('gnorm_fwd', ((2, 6, 6, 6, 256), (256,), (256,)), (1,), 0),
        ('gnorm_fwd', ((2, 12, 12, 12, 128), (128,), (128,)), (1,), 0),
        ('gnorm_fwd', ((2, 24, 24, 24, 64), (64,), (64,)), (1,), 0),
        ('gnorm_fwd', ((2, 48, 48, 48, 32), (32,), (32,)), (1,), 0),
        ('gnorm_fwd', ((2, 96, 96, 96, 16), (16,), (16,)), (1,), 0),
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
        ('plabel_cc_largest', ((2, 96, 96, 96, 2),), (2,), 0),
        ('pw16_bwd_norm', ((2, 96, 96, 96, 16), (5, 2, 16), (2, 96, 96, 96, 2)), (2, 1), 0),
        ('pw16_fwd_norm', ((2, 96, 96, 96, 16), (5, 2, 16), (2, 16, 1, 1, 1)), (2, 1, 2), 0),
        ('up_dgrad', ((2, 12, 12, 12, 128), (262144,)), (256,), 1),
        ('up_dgrad', ((2, 24, 24, 24, 64), (65536,)), (128,), 1),
        ('up_dgrad', ((2, 48, 48, 48, 32), (16384,)), (64,), 1),
        ('up_dgrad', ((2, 96, 96, 96, 16), (4096,)), (32,), 1),
        ('up_fwd', ((2, 6, 6, 6, 256), (262144,), (128,)), (128,), 1),
        ('up_fwd', ((2, 12, 12, 12, 128), (65536,), (64,)), (64,), 1),
        ('up_fwd', ((2, 24, 24, 24, 64), (16384,), (32,)), (32,), 1),
    ),
}

TAU = 2.0 ** -14            # elementwise bound for convolutions, GEMMs and norms: |out - ref64| <= TAU * cond
TAU_OPT = 2.0 ** -22        # optimiser / EMA updates: |out - ref64| <= TAU_OPT * (|p| + |update|)
TAU_ADAM = 2.0 ** -21       # Adam's update goes through six fp32 roundings (sqrt, / bc2, + eps, m / den, lr / bc1, the product): up to
                            # ~6 * 2^-24 of |update|; 1.3 * 2^-22 measured on the device and on the simulator (correctly rounded host math)
TAU_NORM_EVAL = 2.0 ** -20  # norm_eval: nine fp32 roundings (rv + eps, sqrt, 1 / ., gamma * ., y - rm, * scale, + beta, the LeakyReLU slope and
                            # its 0.01f, + residual): up to ~9.4 * 2^-24 of cond -> the power of two above
STEP_GROUPS = 2             # every self-training step runs its networks grouped 2 (norm statistics per group of samples)
EPS = 1e-5


def network_of(wl):
    """the workload whose network (and configuration) `wl` runs: la_pre, la_val, la8 -> la; lares_pre, lares_val -> lares (the residual
    V-Net); lagn_pre, lagn_val -> lagn (the GroupNorm V-Net, as pancreasgn)"""
    return "la" if wl == "la8" else wl.partition("_")[0]


GN_NETWORKS = ("lagn", "pancreasgn")
# ops whose key can repeat a plain workload's while the table behind or in front of the launch is a GroupNorm table (groups = samples)
GN_TABLE_OPS = ("conv3_dgrad_bwdstats", "pw16_fwd_norm", "k2_fwd_stats", "conv3_c1_fwd_stats")


def is_gn(wl):
    """whether `wl` runs GroupNorm V-Nets (normalization='groupnorm'): every norm table is per sample, its mean and rstd per group of C / 16
    adjacent channels"""
    return network_of(wl) in GN_NETWORKS


def stats_fused(wl, key):
    """whether `wl` feeds the norm behind the conv3_fwd_stats launch `key` from its fused partials: STEP_VARIANTS has a 'partial'
    epilogue at the norm key of the conv's output"""
    ys = tuple(key[1][0][:-1]) + (key[2][0],)
    return any(k[0] in ("norm_fwd", "norm_fwd_res", "gnorm_fwd") and tuple(k[1][0]) == ys and any("partial" in f for f in fl) for k, fl in STEP_VARIANTS.get(wl, {}).items())


def step_groups(wl):
    """norm groups of the workload's network calls: 2 in the self-training steps; pre-training calls the network without groups=.  (A
    GroupNorm network ignores them: its statistics groups are the samples, is_gn)"""
    return 1 if wl.endswith(("_pre", "_val")) else STEP_GROUPS


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


def drive_conv(ops, dev, key, g, groups=STEP_GROUPS, fused=True, gn=False):
    """conv3_fwd / conv3_fwd_stats / conv3_fwd_raw / conv3_dgrad_bwdstats: the output against sum over 27 (9) shifted matmuls in fp64,
    sample by sample (the reference of an N = 4 validation chunk is the cost of its row).  namax == 0 (the validation pass: norm_eval
    leaves no |max| on its output): the operand must reach the library without one and the launch must not take the two-plane fp16 instance.
    fused (conv3_fwd_stats): whether the pass feeds the norm behind from this launch's statistics partials (stats_fused) -- the
    pancreas validation pass calls conv3_fwd_stats at every level and gets none at the small ones, where the call is a plain conv.
    gn (conv3_dgrad_bwdstats of a GroupNorm workload): the table of the layer in front comes from gnorm_fwd with one group per sample,
    and the epilogue's backward-statistics rows are held against sums formed with GROUP statistics"""
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
        act, Gn = ints[2], xs[0] if gn else groups            # (the key's ints are Cin, KD, act: the groups argument comes fourth)
        C = yp.shape[-1]
        gam = (torch.rand(C, generator=g) + 0.5).to(dev)
        bet = (torch.rand(C, generator=g) - 0.5).to(dev)
        if gn:
            yp = _seam()._pre_norm(_np_rng(g), xs[0], tuple(shapes[2][1:4]), C).to(dev)      # (offsets of order 30, every sample its own)
            _, st = ops.gnorm_fwd(yp, gam, bet, act)
        else:
            _, st = ops.norm_fwd(yp, Gn, gam, bet, torch.zeros(C, device=dev), torch.ones(C, device=dev), act)
        res, part, rows = ops.conv3_dgrad_bwdstats(xd, wd, Cin, KD, yp, st, act, Gn)
        assert rows > 0 or dev.type == "cpu", f"{op} {xs}: no fused backward statistics at the step's shape"
        if rows:
            # the epilogue's (sum dz, sum dz * xhat) partials of the norm layer behind: fp64 sums of the kernel's own da
            _, z, xh, _, _, fcond = _seam().gn_ref64(yp.cpu(), gam.cpu(), bet.cpu(), act)[:6] if gn else norm_ref64(yp.cpu(), Gn, gam.cpu(), bet.cpu(), act)
            if gn and NEAR_MISS == "gn_channel_statistics":      # (test_product_ops_cpu: every channel its own statistics)
                _, z, xh, _, _, fcond = _seam().gn_ref64(yp.cpu(), gam.cpu(), bet.cpu(), act, how="channel")
                _near_miss_hit(C > 16)
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
            assert (rows > 0) == fused or dev.type == "cpu", f"{op} {xs}: {rows} rows of fused statistics at the step's shape, the pass {'uses' if fused else 'has none'}"
        elif op == "conv3_fwd_raw":
            nsl = ops.conv3_nslabs(xs, Cout, KD)          # (ints[2] at the in-step shape; the reduced simulator shapes may not be served raw)
            assert nsl == ints[2] or dev.type == "cpu", f"{op} {xs}: {nsl} split-K slabs, the step launches {ints[2]}"
            res = ops.conv3_fwd_raw(xd, wf, Cout, KD, nsl).double().sum(0) if nsl else ops.conv3_fwd(xd, wf, None, Cout, KD)
        else:
            raise KeyError(op)
        wk = w.double()
    if not namax:
        assert ops._amax_of(xd) is None, f"{op} {xs}: the operand carries a |max| the step's does not"
        sec = int(ops.b.call("bcp_conv3_last_section"))        # (4: the launch read the two-plane fp16 section of the pack)
        assert sec != 4, f"{op} {xs}: an operand without |max| took the two-plane fp16 instance"
    xc = x.double()
    if two_d:
        wk = wk.reshape(wk.shape[0], wk.shape[1], 3, 3)
    tile = (1, 16, 16) if two_d else (4, 8, 8)
    rc = res.cpu()
    worst = None
    for n in range(xs[0]):
        ref = conv3_cl64(xc[n:n + 1], wk)
        cond = conv3_cl64(xc[n:n + 1].abs(), wk.abs())
        if op in ("conv3_fwd", "conv3_fwd_stats") and b is not None:
            ref += b.double().cpu()
            cond += b.double().cpu().abs()
        r = check_elementwise(rc[n:n + 1], ref, cond, TAU, f"{op} {xs} sample {n}", tile)
        worst = r if worst is None or r[0] > worst[0] else worst
    out.append((op, worst))
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


def _running_check(tag, rm, rv, rm0, rv0, mu, var, n):
    """BatchNorm's running statistics after one grouped call (momentum 0.1, one update per group, unbiased variance over n voxels)"""
    m64, v64 = rm0.double(), rv0.double()
    for gi in range(mu.shape[0]):
        m64 = 0.9 * m64 + 0.1 * mu[gi, 0]
        v64 = 0.9 * v64 + 0.1 * var[gi, 0] * n / (n - 1)
    for t, r in ((rm, m64), (rv, v64)):
        e = float(((t.double().cpu() - r).abs() / (r.abs() + mu.abs().amax((0, 1)) + 1e-30)).max())
        assert e <= TAU, f"{tag}: running statistics off by {e:.3e}"


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
            _running_check(tag, rm, rv, rm0, rv0, mu, var, y.numel() // C // G)
    return out


def _kink(z, fcond):
    """elements whose pre-activation lies within 2^-18 of its magnitude of the activation's kink: the fp32 kernel computes z from fp32
    statistics (a few ulps of fcond off the fp64 value), so there it may take the other branch -- a whole |da| of difference, not a
    rounding error (one such element, z = 3.9e-8 at fcond 1.35, moved dbeta by 9e-5 of sum |dz| at 2 x 14 x 14 x 10 x 128)"""
    return z.abs() <= 2.0 ** -18 * fcond


def _norm_bwd_ref64(y, G, gam, bet, act, da64, mult, zcond=None, res=None):
    """fp64 backward of norm_ref64 for the incoming gradient da64 * mult -> (dy ref, its cond, dz, xhat, dk), the last three as
    [G, n, C]; dk: the terms of elements at the activation's kink (_kink), which may take either branch.  zcond: what else the kernel's
    pre-activation can move by per unit of rounding (a y it recomputes in fp32), added to the norm's own cond in the kink test.
    res: a residual in FRONT of the activation (norm_bwd_res): the pattern and the kink test are those of t = z + res, the kink band
    2^-18 * (fcond + |res|)"""
    ys = tuple(y.shape)
    C = ys[-1]
    _, z, xh, _, var, fcond = norm_ref64(y, G, gam, bet, act)
    t = z if res is None else z + res.double()
    kink = _kink(t, (fcond if zcond is None else fcond + zcond) + (0 if res is None else res.double().abs()))
    _, dact = _acts(act, t)
    dz = (da64 * mult * dact).reshape(G, -1, C)
    xg = xh.reshape(G, -1, C)
    dk = (da64 * mult * kink).abs().reshape(G, -1, C)      # (a kink element may take either branch: its whole term is allowed)
    rstd = 1.0 / torch.sqrt(var + EPS)
    gm = torch.ones(C, dtype=torch.float64) if gam is None else gam.double()
    m1, m2 = dz.mean(1, keepdim=True), (dz * xg).mean(1, keepdim=True)
    if res is not None and NEAR_MISS == "c1c2_from_z":       # (test_product_ops_cpu: the two means from the pattern of z alone)
        dzz = (da64 * mult * _acts(act, z)[1]).reshape(G, -1, C)
        m1, m2 = dzz.mean(1, keepdim=True), (dzz * xg).mean(1, keepdim=True)
        _near_miss_hit(not torch.equal(dzz, dz))
    ref = (gm * rstd * (dz - m1 - xg * m2)).reshape(ys)
    # the two means are fp32-staged reductions over n = voxels per group; their rounding grows with the reduction depth, ~log2(n).
    # Without the factor the pancreas InstanceNorm at 2 x 48^3 x 32 (n = 110 592) measured 2.1 x TAU, with it 0.32 x TAU at worst.
    kap = float(np.log2(dz.shape[1]))
    cond = (gm * rstd * (dz.abs() + kap * (dz.abs().mean(1, keepdim=True) + xg.abs() * (dz * xg).abs().mean(1, keepdim=True)))).reshape(ys)
    cond = torch.where(kink, torch.full_like(cond, float("inf")), cond)
    return ref, cond, dz, xg, dk


def _dgamma_dbeta_check(tag, dg, db, dg0, db0, dz, xg, dk, dzb=None):
    """the accumulated dgamma / dbeta against their fp64 sums (plus what they held), less the kink allowance; dzb: a bound on |dz| where
    dz is itself a rounded sum (the slab kernels), else |dz|"""
    sdb, sdg = dz.sum((0, 1)), (dz * xg).sum((0, 1))
    dzb = dz.abs() if dzb is None else dzb
    for name, t, base, s_, c, k in (("dbeta", db, db0, sdb, dzb.sum((0, 1)), dk.sum((0, 1))),
                                    ("dgamma", dg, dg0, sdg, (dzb * xg.abs()).sum((0, 1)), (dk * xg.abs()).sum((0, 1)))):
        err = ((t.double().cpu() - (base.double() + s_)).abs() - k).clamp_min(0)
        r, _ = elementwise_ratio(err, torch.zeros_like(err), base.double().abs() + c)
        assert r <= TAU, f"{tag}: {name} off by {r:.3e} x cond"


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
        part, rows = None, 0
        if "partial" in flags:
            dad, part, rows = _conv_partial_source(ops, dev, g, ys, G, fwd=False, yprev=yd, stats=st, act=act)
            assert rows > 0 or dev.type == "cpu", f"{tag}: conv3_dgrad_bwdstats left no partials at the step's shape"
            da = dad.cpu()
        else:
            da = gradient(g, ys)
            dad = da.to(dev)
        ref, cond, dz, xg, dk = _norm_bwd_ref64(y, G, gam, bet, act, da.double(), mult)
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
        out.append((op + ("" if not flags else " " + "+".join(flags)), check_elementwise(dx.cpu(), ref, cond, TAU, tag)))
        if affine:
            _dgamma_dbeta_check(tag, dg, db, dg0, db0, dz, xg, dk)
    return out


# -------------------------------------------------------------------------------------------------- the residual V-Net's norms and join
# NEAR_MISS names a reference that is wrong the way a plausible kernel bug would be (tests/test_product_ops_cpu.py sets it and expects the
# driver to raise on the very inputs and bound that pass with the right reference); NEAR_MISS_HITS counts the references it really changed.
NEAR_MISS = None
NEAR_MISS_HITS = 0
NEAR_MISSES = ("pattern_from_z", "residual_behind_activation", "neighbour_chan_scale", "bcast_row_off", "group_statistics_swapped",
               "dres_without_chan_scale", "c1c2_from_z", "eval_batch_statistics")
KINK_CAP = 1e-4                 # at most this share of a tensor's elements may be exempt as kink elements (asserted on the reference alone)
TAU_DRES = 2.0 ** -22           # dres = da * chan_scale * act'(t): two fp32 multiplications, each at most 2^-24 relative
KINK_SHARES = []                # (tag, share) of every residual / GroupNorm backward case run (the report of the largest share seen)


def _near_miss_hit(changed=True):
    global NEAR_MISS_HITS
    NEAR_MISS_HITS += int(bool(changed))


def _res_mult(cs, ys):
    """the Dropout3d channel scale [N, C] as a per-element factor (ones without one)"""
    mult = torch.ones(ys, dtype=torch.float64)
    if cs is not None:
        c = cs.double()
        if NEAR_MISS == "neighbour_chan_scale":
            c = torch.roll(c, 1, 0)
            _near_miss_hit(not torch.equal(c, cs.double()))
        mult = mult * c.view(ys[0], *([1] * (len(ys) - 2)), ys[-1])
    return mult


def _res64(res, ys):
    """the pre-activation residual as the reference adds it: [.., C], or [.., 1] broadcast"""
    r = res.double().cpu()
    if NEAR_MISS == "bcast_row_off" and r.shape[-1] == 1:
        r = torch.roll(r.reshape(-1), 1).reshape(r.shape)
        _near_miss_hit()
    return r.expand(ys)


def _res_norm64(y, G, gam, bet):
    """norm_ref64 without activation -> (z, xhat, mean, var, cond)"""
    if NEAR_MISS == "group_statistics_swapped" and G > 1:
        y = y.double().cpu()
        C = y.shape[-1]
        yg = y.reshape(G, -1, C)
        mu = yg.mean(1, keepdim=True)
        var = ((yg - mu) ** 2).mean(1, keepdim=True)
        mu_w, var_w = mu.clone(), var.clone()
        mu_w[0], var_w[0] = mu[1], var[1]
        xh = (yg - mu_w) / torch.sqrt(var_w + EPS)
        z = gam.double() * xh + bet.double()
        cond = gam.double().abs() * (xh.abs() + 1) + bet.double().abs()
        _near_miss_hit()
        return z.reshape(y.shape), xh.reshape(y.shape), mu, var, cond.reshape(y.shape)
    _, z, xh, mu, var, cond = norm_ref64(y, G, gam, bet, 0)
    return z, xh, mu, var, cond


def res_fwd_ref64(y, G, gam, bet, act, res, cs):
    """fp64 norm_fwd_res: a = act(norm(y) + r) * chan_scale -> (a, cond, mean, var); cond = (the norm's cond + |r|) * |chan_scale|"""
    ys = tuple(y.shape)
    z, _, mu, var, cond = _res_norm64(y, G, gam, bet)
    r = _res64(res, ys)
    mult = _res_mult(cs, ys)
    if NEAR_MISS == "residual_behind_activation":
        a = _acts(act, z)[0] + r
        _near_miss_hit()
    else:
        a = _acts(act, z + r)[0]
    return a * mult, (cond + r.abs()) * mult.abs(), mu, var


def res_bwd_ref64(y, G, gam, bet, act, res, cs, da):
    """fp64 norm_bwd_res -> (dy, its cond (inf at kink elements), dres, its cond, dz, xhat, dk, the kink share)"""
    ys = tuple(y.shape)
    r = _res64(res, ys)
    mult = _res_mult(cs, ys)
    da64 = da.double().cpu()
    if NEAR_MISS == "pattern_from_z":
        ref, cond, dz, xg, dk = _norm_bwd_ref64(y, G, gam, bet, act, da64, mult)
        _near_miss_hit()
    else:
        ref, cond, dz, xg, dk = _norm_bwd_ref64(y, G, gam, bet, act, da64, mult, res=r)
    kink = torch.isinf(cond)
    dres = dz.reshape(ys)
    dcond = (da64 * mult).abs()
    if NEAR_MISS == "dres_without_chan_scale" and cs is not None:
        z, _, _, _, _ = _res_norm64(y, G, gam, bet)
        dres = da64 * _acts(act, z + r)[1]
        _near_miss_hit()
    dcond = torch.where(kink, torch.full_like(dcond, float("inf")), dcond)
    return ref, cond, dres, dcond, dz, xg, dk, float(kink.double().mean())


def _res_source(ops, dev, g, ys, G, flags):
    """(y on the device, y, partial, rows, residual) as the step produces them for `flags`: partial: y and its statistics rows from a real
    conv3_fwd_stats launch; partial + bcast (block_one): from a real conv3_c1_fwd_stats launch on a 1-channel input, which is the residual"""
    C = ys[-1]
    bc = "bcast" in flags
    x1 = activation(g, tuple(ys[:-1]) + (1,)) if bc else None
    part, rows = None, 0
    if "partial" in flags and bc:
        assert C == 16, ys
        KD = 1 if ys[1] == 1 else 3
        yd, part, rows = ops.conv3_c1_fwd_stats(x1.to(dev), _conv_weight(g, 16, 1, KD).to(dev), (torch.randn(16, generator=g) * 0.1).to(dev), KD, G)
        y = yd.cpu()
    elif "partial" in flags:
        yd, part, rows = _conv_partial_source(ops, dev, g, ys, G)
        y = yd.cpu()
    else:
        y = _pre_norm(g, ys)
        yd = y.to(dev)
    res = x1 if bc else activation(g, ys)
    return yd, y, part, rows, res


def _res_params(g, C, N, flags):
    gam, bet = torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) - 0.5
    rm0, rv0 = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    cs = ((torch.rand(N, C, generator=g) < 0.5).float() * 2.0) if "chan_scale" in flags else None
    return gam, bet, rm0, rv0, cs


def drive_norm_fwd_res(ops, dev, key, g, variants=((),)):
    """norm_fwd_res (the closing layer of a residual block): a = act(norm(y) + r) * chan_scale with each flag set the step uses at this key --
    statistics from a real conv3_fwd_stats / conv3_c1_fwd_stats launch's partial rows, the Dropout3d channel scale, the full-width or the
    1-channel broadcast residual; statistics, running statistics, the published |max| exactly"""
    from bcp_amd import hip_ops as H
    op, shapes, ints, namax = key
    ys = tuple(shapes[0])
    G, act = ints[0], ints[1]
    N, C = ys[0], ys[-1]
    out = []
    for flags in variants:
        tag = f"{op} {ys} [{'+'.join(flags) or 'plain'}]"
        yd, y, part, rows, res = _res_source(ops, dev, g, ys, G, flags)
        if "partial" in flags:
            assert rows > 0 or dev.type == "cpu", f"{tag}: the producer left no statistics rows at the step's shape"
        gam, bet, rm0, rv0, cs = _res_params(g, C, N, flags)
        ref, cond, mu, var = res_fwd_ref64(y, G, gam, bet, act, res, cs)
        rm, rv = rm0.clone().to(dev), rv0.clone().to(dev)
        kw = dict(chan_scale=None if cs is None else cs.to(dev))
        if rows:
            kw.update(partial=part, nb=rows)
        a, st = ops.norm_fwd_res(yd, G, gam.to(dev), bet.to(dev), rm, rv, act, res.to(dev), **kw)
        _stats_check(st, mu, var, tag)
        out.append((op + ("" if not flags else " " + "+".join(flags)), check_elementwise(a.cpu(), ref, cond, TAU, tag)))
        _running_check(tag, rm, rv, rm0, rv0, mu, var, y.numel() // C // G)
        assert H.amax_value(a._bcp_amax) == float(a.abs().max()), f"{tag}: published |max| {H.amax_value(a._bcp_amax)!r} != {float(a.abs().max())!r}"
    return out


def drive_norm_bwd_res(ops, dev, key, g, variants=((),)):
    """norm_bwd_res: dy against the fp64 norm backward with the pattern of t = z + r (kink band 2^-18 * (cond + |r|), at most KINK_CAP of
    the elements, asserted on the reference before the device result is read), dgamma / dbeta accumulated as the step does, dres = da *
    chan_scale * act'(t) to TAU_DRES, the published |max| of dy exactly; want_dres=False where the step asks for none"""
    from bcp_amd import hip_ops as H
    op, shapes, ints, namax = key
    ys = tuple(shapes[0])
    G, act, accumulate = ints[0], ints[1], bool(ints[2])
    N, C = ys[0], ys[-1]
    out = []
    for flags in variants:
        bc = shapes[2][-1] == 1
        assert bc == ("bcast" in flags), (key, flags)
        tag = f"{op} {ys} [{'+'.join(flags) or 'plain'}]"
        yd, y, _, _, res = _res_source(ops, dev, g, ys, G, tuple(f for f in flags if f == "bcast"))
        gam, bet, _, _, cs = _res_params(g, C, N, flags)
        csd = None if cs is None else cs.to(dev)
        resd = res.to(dev)
        _, st = ops.norm_fwd_res(yd, G, gam.to(dev), bet.to(dev), torch.zeros(C, device=dev), torch.ones(C, device=dev), act, resd, chan_scale=csd)
        da = gradient(g, ys)
        ref, cond, dres_ref, dres_cond, dz, xg, dk, share = res_bwd_ref64(y, G, gam, bet, act, res, cs, da)
        KINK_SHARES.append((tag, share))
        print(f"[product-op] {tag}: {share:.2e} of the elements at the kink of z + r (cap {KINK_CAP:.0e})")
        assert share <= KINK_CAP, f"{tag}: {share:.2e} of the elements lie at the activation's kink (cap {KINK_CAP:.0e}): another seed or generator"
        dg0, db0 = (torch.randn(C, generator=g) * 1e-2, torch.randn(C, generator=g) * 1e-2) if accumulate else (torch.zeros(C), torch.zeros(C))
        dg, db = dg0.clone().to(dev), db0.clone().to(dev)
        want = "no_dres" not in flags
        dy, dres = ops.norm_bwd_res(yd, da.to(dev), resd, G, st, act, dg, db, accumulate, chan_scale=csd, want_dres=want)
        name = op + ("" if not flags else " " + "+".join(flags))
        out.append((name, check_elementwise(dy.cpu(), ref, cond, TAU, tag)))
        _dgamma_dbeta_check(tag, dg, db, dg0, db0, dz, xg, dk)
        if getattr(dy, "_bcp_amax", None) is not None:
            assert H.amax_value(dy._bcp_amax) == float(dy.abs().max()), f"{tag}: published |max| of dy"
        if want and not bc:
            out.append((name + " dres", check_elementwise(dres.cpu(), dres_ref, dres_cond, TAU_DRES, tag + " dres")))
        else:
            assert dres is None, f"{tag}: a dres nobody asked for"
    return out


def res_eval_ref64(y, gam, bet, rm, rv, act, res, eps=EPS):
    """fp64 norm_eval_res: act((y - rm) * gamma / sqrt(rv + eps) + beta + r) -> (a, cond); the activations are 1-Lipschitz, so the
    pre-activation's bound is the output's"""
    y64 = y.double().cpu()
    if NEAR_MISS == "eval_batch_statistics":
        C = y64.shape[-1]
        rm, rv = y64.reshape(-1, C).mean(0), y64.reshape(-1, C).var(0, unbiased=False)
        _near_miss_hit()
    _, z, _, zcond = norm_eval_ref64(y64, gam, bet, rm, rv, act, None, eps)
    r = _res64(res, tuple(y64.shape))
    return _acts(act, z + r)[0], zcond + r.abs()


def drive_norm_eval_res(ops, dev, key, g, variants=((),)):
    """norm_eval_res at the validation chunk's shape: one launch at the recorded N, the fp64 reference sample by sample; running
    variances over four decades; both residual widths as the pass uses them; the running statistics unchanged bit for bit; no |max|"""
    op, shapes, ints, namax = key
    ys, act = tuple(shapes[0]), ints[0]
    C = ys[-1]
    out = []
    for flags in variants:
        tag = f"{op} {ys} [{'+'.join(flags) or 'plain'}]"
        y = _pre_norm(g, ys)
        rm = (y.reshape(-1, C)[:4096].double().mean(0) + torch.randn(C, generator=g, dtype=torch.float64) * 0.1).float()
        rv = torch.pow(10.0, torch.rand(C, generator=g, dtype=torch.float64) * 4 - 2).float()
        gam, bet = torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) - 0.5
        res = activation(g, tuple(ys[:-1]) + (1 if "bcast" in flags else C,))
        rmd, rvd = rm.clone().to(dev), rv.clone().to(dev)
        a = ops.norm_eval_res(y.to(dev), gam.to(dev), bet.to(dev), rmd, rvd, act, res.to(dev))
        assert getattr(a, "_bcp_amax", None) is None, f"{tag}: the output carries a |max|"
        assert torch.equal(rmd.cpu().view(torch.int32), rm.view(torch.int32)) and torch.equal(rvd.cpu().view(torch.int32), rv.view(torch.int32)), \
            f"{tag}: eval mode changed the running statistics"
        ac = a.cpu()
        worst = None
        for n in range(ys[0]):
            ref, cond = res_eval_ref64(y[n:n + 1], gam, bet, rm, rv, act, res[n:n + 1])
            r = check_elementwise(ac[n:n + 1], ref, cond, TAU_NORM_EVAL, f"{tag} sample {n}")
            worst = r if worst is None or r[0] > worst[0] else worst
        out.append((op + ("" if not flags else " " + "+".join(flags)), worst))
    return out


def drive_axpy(ops, dev, key, g):
    """axpy, the join of a residual block's two gradients (y += a * x, a = 1 in the step): against y + a * x in fp64 on gradient() operands"""
    from bcp_amd import hip_ops as H
    op, shapes, ints, namax = key
    ys = tuple(shapes[0])
    assert tuple(shapes[1]) == ys, key
    out = []
    for a in (1.0, -0.375) if int(np.prod(ys)) <= 1 << 22 else (1.0,):      # (the step's a = 1 everywhere; another scalar where the row is cheap)
        y, x = gradient(g, ys), gradient(g, ys)
        yd, xd = y.clone().to(dev), x.to(dev)
        for t in (yd, xd)[:namax]:
            _amax(H, t, dev)
        r = ops.axpy(yd, xd, a)
        assert r.data_ptr() == yd.data_ptr(), f"{op} {ys}: the sum is formed in place"
        ref, cond = y.double() + a * x.double(), y.double().abs() + (a * x.double()).abs()
        out.append((f"{op} a={a:g}", check_elementwise(yd.cpu(), ref, cond, TAU_OPT, f"{op} {ys} a={a:g}")))
    return out


def drive_c1_stats(ops, dev, key, g, gn=False):
    """conv3_c1_fwd_stats, the first layer in front of a closing norm (block_one of the residual V-Net): the fp64 conv sample by sample,
    and the statistics rows of its epilogue against fp64 column sums of the kernel's own output, as drive_conv checks conv3_fwd_stats'"""
    op, shapes, ints, namax = key
    xs, ws = shapes[0], shapes[1]
    KD, G = ints[0], ints[1]
    x, w, b = activation(g, xs), _conv_weight(g, 16, 1, KD), torch.randn(16, generator=g) * 0.1
    assert tuple(w.shape) == tuple(ws), key
    yd, part, rows = ops.conv3_c1_fwd_stats(x.to(dev), w.to(dev), b.to(dev), KD, G)
    assert rows > 0 or dev.type == "cpu", f"{op} {xs}: no fused statistics at the step's shape"
    y = yd.cpu()
    tile = (1, 16, 16) if KD == 1 else (4, 8, 8)
    worst = None
    for n in range(xs[0]):
        ref = conv3_cl64(x[n:n + 1], w) + b.double()
        cond = conv3_cl64(x[n:n + 1].abs(), w.abs()) + b.double().abs()
        r = check_elementwise(y[n:n + 1], ref, cond, TAU, f"{op} {xs} sample {n}", tile)
        worst = r if worst is None or r[0] > worst[0] else worst
    if rows:
        pt = _partials(part, G, rows, 16)
        yg = y.double().reshape(G, -1, 16)
        for j, (s_, c) in enumerate(((yg.sum(1), yg.abs().sum(1)), ((yg * yg).sum(1), (yg * yg).sum(1)))):
            r = float(((pt[..., j] - s_).abs() / c.clamp_min(1e-300)).max())
            assert r <= 1e-12, f"{op} {xs}: fused statistics partial {j} off by {r:.3e} x sum|.|"
        if gn:
            _gn_table_from_rows(ops, dev, g, f"{op} {xs}", yd, part, rows, G)
    return [(op, worst)]


def drive_c1_wgrad(ops, dev, key, g, variants=((),)):
    """conv3_c1_wgrad, the first layer's weight gradient from a materialised dy (behind norm_bwd_res): fp64 sums over all voxels"""
    from bcp_amd import hip_ops as H
    op, shapes, ints, namax = key
    xs, dys, ws = shapes
    KD = ints[0]
    out = []
    for flags in variants:
        acc = "accumulate" in flags
        x, dy = activation(g, xs), gradient(g, dys)
        dw0 = gradient(g, ws, -4.0, 0.0) if acc else torch.zeros(ws)
        dwd = dw0.clone().to(dev) if acc else torch.full(ws, float("nan"), device=dev)
        xd, dyd = x.to(dev), dy.to(dev)
        for t in (xd, dyd)[2 - namax:]:           # (the step's dy comes out of norm_bwd_res with its |max|; the network input has none)
            _amax(H, t, dev)
        ops.conv3_c1_wgrad(xd, dyd, dwd, KD, accumulate=acc)
        ref = conv3_wgrad64(x, dy, 3, KD == 1) + dw0.double()
        cond = conv3_wgrad64(x.abs(), dy.abs(), 3, KD == 1) + dw0.double().abs()
        out.append((op + ("" if not flags else " " + "+".join(flags)), check_elementwise(dwd.cpu(), ref, cond, TAU, f"{op} {xs} -> {ws}")))
    return out


def drive_pw16_bwd(ops, dev, key, g, variants=((),)):
    """pw16_bwd, the 16 -> C head's backward on a materialised activation (the residual V-Net: block_nine closes a block, the fused head
    is off): dx = dy @ W elementwise, dw = dy^T @ x and db = sum dy as bounded sums, accumulated where the step accumulates"""
    from bcp_amd import hip_ops as H
    op, shapes, ints, namax = key
    xs, dys, ws = shapes
    Cout = dys[-1]
    out = []
    for flags in variants:
        acc = "accumulate" in flags
        tag = f"{op} {xs} [{'+'.join(flags) or 'plain'}]"
        x, dy, w = activation(g, xs), gradient(g, dys), _k2_weight(g, tuple(ws), 16)
        xd, dyd = x.to(dev), dy.to(dev)
        for t in (xd, dyd)[:namax]:
            _amax(H, t, dev)
        dw0, db0 = (gradient(g, tuple(ws), -4.0, 0.0), gradient(g, (Cout,), -4.0, 0.0)) if acc else (torch.zeros(ws), torch.zeros(Cout))
        dwd, dbd = ((dw0.clone().to(dev), db0.clone().to(dev)) if acc
                    else (torch.full(tuple(ws), float("nan"), device=dev), torch.full((Cout,), float("nan"), device=dev)))
        dx = ops.pw16_bwd(xd, dyd, w.to(dev), dwd, dbd, accumulate=acc)
        W = w.double().reshape(Cout, 16)
        d2, x2 = dy.double().reshape(-1, Cout), x.double().reshape(-1, 16)
        name = op + ("" if not flags else " " + "+".join(flags))
        out.append((name, check_elementwise(dx.cpu(), dy.double() @ W, dy.double().abs() @ W.abs(), TAU, tag)))
        out.append((name + " dw", check_elementwise(dwd.cpu().reshape(Cout, 16), d2.t() @ x2 + dw0.double().reshape(Cout, 16),
                                                    d2.abs().t() @ x2.abs() + dw0.double().abs().reshape(Cout, 16), TAU, tag + " dw")))
        out.append((name + " db", check_elementwise(dbd.cpu(), d2.sum(0) + db0.double(), d2.abs().sum(0) + db0.double().abs(), TAU, tag + " db")))
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


def _k2_weight(g, shape, fan_in):
    """a k2s2 / transposed / 1x1 conv weight drawn as _conv_weight draws the 3x3x3 ones, scaled for its fan-in"""
    return (torch.randn(shape, generator=g, dtype=torch.float64) * (2.0 / fan_in) ** 0.5).float()


# k2_fwd_stats: each partial row sums fp32 lane partials of the GEMM epilogue (<= 256 values each), the rows are summed in fp64: the
# 1e-12 of conv3_fwd_stats (fp64 throughout) does not hold.  Measured on the device, worst |partial sum - fp64 sum| / sum |.| over
# groups and channels: LA 2 x 56 x 56 x 40 x 32 -> 16 (980 rows) 2.81e-10 (sum) / 1.63e-9 (sum of squares), pancreas 2 x 48^3 x 32 -> 16
# (864 rows) 3.75e-10 / 1.89e-9.  The bound is twice the worst.
TAU_K2_STATS_MEASURED = 1.89e-9
TAU_K2_STATS = 2 * TAU_K2_STATS_MEASURED


def drive_k2(ops, dev, key, g, variants=((),), gn=False):
    """down_fwd / down_dgrad / up_fwd / up_dgrad / k2_fwd_stats / k2_wgrad / pw_fwd at the step's row counts, against the strided-view
    fp64 matmuls (down64, up64, k2_wgrad64).  The weights go through ops.k2_pack with the launch's PACK_* kind; the flags of `variants`
    (out given, accumulate) are the step's: down_dgrad adds into the skip gradient, every k2_wgrad into the flat gradient buffer."""
    from bcp_amd import hip_ops as H
    op, shapes, ints, namax = key
    xs = shapes[0]
    two_d = xs[1] == 1
    tile = (1, 16, 16) if two_d else (4, 8, 8)
    out = []
    for flags in variants:
        tag = f"{op} {xs} {ints} [{'+'.join(flags) or 'plain'}]"
        name = op + ("" if not flags else " " + "+".join(flags))
        acc = "accumulate" in flags
        if op == "k2_wgrad":
            _, dys, ws = shapes
            kind = ints[0]
            x, dy = activation(g, xs), gradient(g, dys)
            xd, dyd = x.to(dev), dy.to(dev)
            for t in (xd, dyd)[:namax]:
                _amax(H, t, dev)
            ref = k2_wgrad64(x, dy, kind).reshape(ws)
            cond = k2_wgrad64(x.abs(), dy.abs(), kind).reshape(ws)
            dw0 = gradient(g, ws, -4.0, 0.0)
            dwd = dw0.clone().to(dev) if acc else torch.full(ws, float("nan"), device=dev)
            res = ops.k2_wgrad(xd, dyd, dwd, kind, accumulate=acc)
            if acc:
                ref, cond = ref + dw0.double(), cond + dw0.double().abs()
            out.append((name, check_elementwise(res.cpu(), ref, cond, TAU, tag)))
            continue
        Cx = xs[-1]
        Co = ints[1] if op == "k2_fwd_stats" else ints[0]          # channels of the result
        kind = {"down_fwd": 0, "up_fwd": 1, "down_dgrad": 1, "up_dgrad": 0, "pw_fwd": 2}.get(op, ints[0])     # the reference: down64 / up64 / 1x1
        fwd = op in ("down_fwd", "up_fwd", "k2_fwd_stats") or (op == "pw_fwd" and len(shapes) > 2)
        x = activation(g, xs) if fwd else gradient(g, xs)
        xd = x.to(dev)
        if namax:
            _amax(H, xd, dev)
        else:
            assert ops._amax_of(xd) is None, f"{tag}: the operand carries a |max| the pass's does not"
        b = (torch.randn(Co, generator=g) * 0.1) if fwd else None
        bd = None if b is None else b.to(dev)
        # the layer's own weight: Conv3d [Cout, Cin, 2, 2, 2] (down, 1x1) or ConvTranspose3d [Cin, Cout, 2, 2, 2] (up); a dgrad maps Cout -> Cin
        Cin, Cout = (Cx, Co) if fwd else (Co, Cx)
        if op in ("down_fwd", "down_dgrad") or (op == "k2_fwd_stats" and kind == 0):
            w = _k2_weight(g, (Cout, Cin, 2, 2, 2), 8 * Cin)
            pk = H.PACK_DOWN_FWD if fwd else H.PACK_DOWN_DGRAD
        elif op == "pw_fwd":
            w = _k2_weight(g, (Cout, Cin, 1, 1), Cin)
            pk = H.PACK_PW_FWD if fwd else H.PACK_PW_DGRAD
        else:
            w = _k2_weight(g, (Cin, Cout, 2, 2, 2), 8 * Cin)
            pk = H.PACK_UP_FWD if fwd else H.PACK_UP_DGRAD
        bp = ops.k2_pack(w.to(dev), Cin, Cout, pk)
        assert tuple(bp.shape) == tuple(shapes[1]), (tag, bp.shape)
        if kind == 2:
            wm = w.double()[:, :, 0, 0]
            wm = wm.t() if fwd else wm                                   # [Cx, Co]
            ref, cond = x.double() @ wm, x.double().abs() @ wm.abs()
        else:
            f64 = down64 if kind == 0 else up64
            ref, cond = f64(x, w), f64(x.abs(), w.abs())
        if b is not None:
            ref, cond = ref + b.double(), cond + b.double().abs()
        ys = tuple(ref.shape)
        kw = {}
        if "out" in flags:
            out0 = gradient(g, ys)
            kw["out"] = out0.clone().to(dev)
            if acc:
                kw["accumulate"] = True
                ref, cond = ref + out0.double(), cond + out0.double().abs()
        else:
            assert not acc, tag
        if op == "k2_fwd_stats":
            G = ints[2]
            rows = ops.k2_stat_rows(kind, xs, Co, G)
            assert rows > 0 or dev.type == "cpu", f"{tag}: no fused statistics at the step's shape"
            plain = ops.down_fwd if kind == 0 else ops.up_fwd
            if rows:
                y0 = plain(xd, bp, bd, Co).clone()
                res, part, nb = ops.k2_fwd_stats(kind, xd, bp, bd, Co, G)
                assert nb == rows and torch.equal(res, y0), f"{tag}: y differs from the plain launch"
                pt = _partials(part, G, rows, Co)
                yg = res.cpu().double().reshape(G, -1, Co)
                worst = 0.0
                for j, (s_, c) in enumerate(((yg.sum(1), yg.abs().sum(1)), ((yg * yg).sum(1), (yg * yg).sum(1)))):
                    r = float(((pt[..., j] - s_).abs() / c.clamp_min(1e-300)).max())
                    print(f"[product-op] {tag}: fused statistics partial {j} off by {r:.3e} x sum|.| ({rows} rows)")
                    worst = max(worst, r)
                assert worst <= TAU_K2_STATS, f"{tag}: fused statistics partials off by {worst:.3e} x sum|.| (bound {TAU_K2_STATS:.3e})"
                if gn:
                    _gn_table_from_rows(ops, dev, g, tag, res, part, rows, G)
            else:
                res = plain(xd, bp, bd, Co)
        elif fwd or op == "pw_fwd":
            res = getattr(ops, op)(xd, bp, bd, Co, **kw)
        else:
            res = getattr(ops, op)(xd, bp, Co, **kw)
        out.append((name, check_elementwise(res.cpu(), ref, cond, TAU, tag, tile)))
    return out


def _raw_slabs(ops, dev, g, ys, nslab, x, fwd, tag):
    """the split-K slabs of a real conv3_fwd_raw launch (C -> C) on x at the row's shape, with the forward (activation x) or the dgrad
    (gradient x) pack -> (slabs on the device, float64 copy).  On the device the launch must write the key's slab count; the simulator's
    reduced shapes may not be served raw, there the conv's output is split into `nslab` signed parts"""
    from bcp_amd import hip_ops as H
    C = ys[-1]
    KD = 1 if ys[1] == 1 else 3
    w = _conv_weight(g, C, C, KD)
    wf, wd = ops.conv3_pack(w.to(dev), KD)
    xd = _amax(H, x.to(dev), dev)
    nsl = ops.conv3_nslabs(ys, C, KD)
    assert nsl == nslab or dev.type == "cpu", f"{tag}: {nsl} split-K slabs, the step launches {nslab}"
    if nsl == nslab:
        slabs = ops.conv3_fwd_raw(xd, wf if fwd else wd, C, KD, nsl)
    else:
        y = ops.conv3_fwd(xd, wf if fwd else wd, None, C, KD)
        parts = torch.randn((nslab - 1,) + tuple(ys), generator=g).to(dev) * y.abs().mean()
        slabs = torch.cat([parts, (y - parts.sum(0)).unsqueeze(0)]).contiguous()
    return slabs, slabs.cpu().double()


def drive_norm_slabs(ops, dev, key, g, variants=((),)):
    """norm_fwd_slabs / norm_bwd_slabs: the statistics pass sums the raw split-K slabs of a real conv3_fwd_raw launch (+ the conv bias)
    on its way in and writes the sum once.  Reference: the fp64 sum of the slabs fed to the fp64 norm references; the written sum
    (y, resp. da) against it elementwise; the epilogues of `variants` as in drive_norm_fwd / drive_norm_bwd"""
    op, shapes, ints, namax = key
    nslab, G, act = ints
    fwd = op == "norm_fwd_slabs"
    ys = tuple(shapes[0][1:] if fwd else shapes[0])
    assert tuple((shapes[0] if fwd else shapes[1])) == (nslab,) + ys, key
    C, N = ys[-1], ys[0]
    tile = (1, 16, 16) if ys[1] == 1 else (4, 8, 8)
    out = []
    for flags in variants:
        tag = f"{op} {ys} x{nslab} [{'+'.join(flags) or 'plain'}]"
        name = op + ("" if not flags else " " + "+".join(flags))
        if fwd:
            affine = len(shapes) > 2
            slabs, s64 = _raw_slabs(ops, dev, g, ys, nslab, activation(g, ys), True, tag)
            bias = torch.randn(C, generator=g) * 0.1
            gam = (torch.rand(C, generator=g) + 0.5) if affine else None
            bet = (torch.rand(C, generator=g) - 0.5) if affine else None
            rm0, rv0 = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
            rm, rv = (rm0.clone().to(dev), rv0.clone().to(dev)) if affine else (None, None)
            cs, sm, es, res, mult, H = _epilogue(ops, dev, g, ys, flags)
            a, st, y = ops.norm_fwd_slabs(slabs, nslab, bias.to(dev), G, *((gam.to(dev), bet.to(dev)) if affine else (None, None)), rm, rv, act,
                                          chan_scale=None if cs is None else cs.to(dev), elem_mask=sm, elem_scale=es,
                                          residual=None if res is None else res.to(dev))
            y64 = s64.sum(0) + bias.double()
            out.append((name + " y", check_elementwise(y.cpu(), y64, s64.abs().sum(0) + bias.double().abs(), TAU, tag + " slab sum", tile)))
            ar, z, xh, mu, var, _ = norm_ref64(y64, G, gam, bet, act)
            _stats_check(st, mu, var, tag)
            # cond composed as the op is: xhat = (sum of slabs + bias - mean) * rstd, each term by its magnitude (>= norm_ref64's own cond)
            S = (s64.abs().sum(0) + bias.double().abs()).reshape(G, -1, C)
            gm = torch.ones(C, dtype=torch.float64) if gam is None else gam.double().abs()
            cond = (gm * ((S + mu.abs()) / torch.sqrt(var + EPS) + 1) + (0 if bet is None else bet.double().abs())).reshape(ys)
            ref = ar * mult + (0 if res is None else res.double())
            cnd = cond * mult.abs() + (0 if res is None else res.double().abs())
            out.append((name, check_elementwise(a.cpu(), ref, cnd, TAU, tag, tile)))
            if rm is not None:
                _running_check(tag, rm, rv, rm0, rv0, mu, var, y64.numel() // C // G)
            continue
        accumulate = "accumulate" in flags
        affine = accumulate or G != N
        y = _pre_norm(g, ys)
        gam = (torch.rand(C, generator=g) + 0.5) if affine else None
        bet = (torch.rand(C, generator=g) - 0.5) if affine else None
        yd = y.to(dev)
        _, st = ops.norm_fwd(yd, G, *((gam.to(dev), bet.to(dev), torch.zeros(C, device=dev), torch.ones(C, device=dev)) if affine else (None,) * 4), act)
        cs, sm, es, _, mult, H = _epilogue(ops, dev, g, ys, flags)
        slabs, s64 = _raw_slabs(ops, dev, g, ys, nslab, gradient(g, ys), False, tag)
        da64 = s64.sum(0)
        ref, _, dz, xg, _ = _norm_bwd_ref64(y, G, gam, bet, act, da64, mult)
        # cond composed as the op is: the kernel forms da in fp32 from the slabs, so the bound is the norm backward's on sum |slab|
        _, cond, dzb, _, dk = _norm_bwd_ref64(y, G, gam, bet, act, s64.abs().sum(0), mult.abs())
        dg0, db0 = (torch.randn(C, generator=g) * 1e-2, torch.randn(C, generator=g) * 1e-2) if accumulate else (torch.zeros(C), torch.zeros(C))
        dg, db = (dg0.clone().to(dev), db0.clone().to(dev)) if affine else (None, None)
        dy, da = ops.norm_bwd_slabs(yd, slabs, nslab, G, st, act, dg, db, accumulate, chan_scale=None if cs is None else cs.to(dev),
                                    elem_mask=sm, elem_scale=es)
        out.append((name + " da", check_elementwise(da.cpu(), da64, s64.abs().sum(0), TAU, tag + " slab sum", tile)))
        out.append((name, check_elementwise(dy.cpu(), ref, cond, TAU, tag, tile)))
        if affine:
            _dgamma_dbeta_check(tag, dg, db, dg0, db0, dz, xg, dk, dzb)
    return out


def _boxes(sp, g):
    """two boxes (d, h, w, size_d, size_h, size_w) of context_mask's size rule (2/3 of each extent) in a volume of extents sp: one at a
    random position; one pushed against the three far faces, its sizes trimmed until neither they nor its origin are multiples of 4"""
    size = [max(1, int(e * 2 / 3)) if e > 1 else 1 for e in sp]
    rnd = tuple(int(torch.randint(0, e - s + 1, (1,), generator=g)) for e, s in zip(sp, size))
    odd = list(size)
    for i, e in enumerate(sp):
        while e > 4 and (odd[i] % 4 == 0 or (e - odd[i]) % 4 == 0):
            odd[i] -= 1
    return rnd + tuple(size), tuple(e - s for e, s in zip(sp, odd)) + tuple(odd)


def _in_box(sp, box6):
    m = torch.zeros(sp, dtype=torch.bool)
    d, h, w, sd, sh, sw = box6
    m[d:d + sd, h:h + sh, w:w + sw] = True
    return m


def drive_mix_box(ops, dev, key, g, variants=((),)):
    """mix_box at the step's shape, bit for bit against torch.where on the box, for a random box and one against three faces with ragged
    edges; then with NaN in b outside the box and in a inside it: the kernel reads b inside the box only, a outside only"""
    op, shapes, ints, namax = key
    xs = shapes[0]
    sp = tuple(xs[1:4])
    out = []
    for flags in variants:
        for bi, box6 in enumerate(_boxes(sp, g)):
            tag = f"{op} {xs} box {box6} [{'+'.join(flags) or 'plain'}]"
            a, b = activation(g, xs), activation(g, xs) + 3.0
            inb = _in_box(sp, box6).view((1,) + sp + (1,)).expand(xs)
            ref = torch.where(inb, b, a)
            nan = torch.full(xs, float("nan"))
            for poison in (False, True):
                ad, bd = (torch.where(inb, nan, a), torch.where(inb, b, nan)) if poison else (a, b)
                kw = {"out": torch.full(xs, -1.0, device=dev)} if "out" in flags else {}
                o = ops.mix_box(ad.to(dev), bd.to(dev), box6, **kw).cpu()
                assert not bool(torch.isnan(o).any()), f"{tag}: read outside its side of the box (NaN in the output)"
                assert torch.equal(o.view(torch.int32), ref.view(torch.int32)), f"{tag}: {int((o != ref).sum())} voxels differ from torch.where"
            out.append((f"{op} box{bi}", (0.0, "exact")))
    return out


_NETS = {}


def _step_network(wl, dev, ops):
    """the workload's student network as its factory builds it for make_step (net_factory / BCP_net / create_Vnet), on `dev`, bound to `ops`"""
    wl = network_of(wl)
    net = _NETS.get((wl, dev.type))
    if net is None:
        torch.manual_seed(1337)
        if wl in ("la", "lares", "lagn"):
            from bcp_amd.networks.VNet import VNet
            net = VNet(n_channels=1, n_classes=2, normalization="groupnorm" if wl == "lagn" else "batchnorm", has_dropout=True, has_residual=wl == "lares")
        elif wl == "acdc":
            from bcp_amd.networks.unet import UNet_2d
            net = UNet_2d(in_chns=1, class_num=4)
        else:
            from bcp_amd.pancreas.Vnet import VNet
            net = VNet(normalization="groupnorm" if wl == "pancreasgn" else "instancenorm")
        net = _NETS[(wl, dev.type)] = net.to(dev).flatten_()
    return net.set_ops(ops)


def drive_pack_many(ops, dev, key, g, wl):
    """conv3_pack_many / k2_pack_many: the network's own pack call (every layer in one launch, forward packs or forward + dgrad) over
    poisoned buffers; every layer's packed buffer bit for bit against the single-layer conv3_pack / k2_pack of the same weight -- the conv
    and GEMM drivers hold those single packs to fp64 through their consumers.  (descriptor bytes, n) must be the table's key."""
    op, shapes, ints, namax = key
    net = _step_network(wl, dev, ops)
    c3 = op == "conv3_pack_many"
    net._ensure_packed(False)                          # (builds the descriptor tables)
    layers = net._c3 if c3 else net._k2
    n = ints[0]
    assert n in (len(layers), 2 * len(layers)), f"{op}: the step packs {n} descriptors, the network has {len(layers)} layers"
    both = n == 2 * len(layers)
    desc = (net._desc_all if both else net._desc_fwd) if c3 else (net._k2_desc_all if both else net._k2_desc_fwd)
    assert tuple(desc.shape) == tuple(shapes[0]), f"{op}: descriptor table of {tuple(desc.shape)} bytes, the step's has {shapes[0]}"
    with torch.no_grad():                               # new weights, so that packs left by an earlier row cannot pass
        for w in (l[1] for l in layers):
            w.mul_(1.0 + 0.25 * float(torch.rand(1, generator=g)))
    (net._pack_buf if c3 else net._k2_buf).fill_(float("nan"))
    net._pack_state = net._k2_state = None
    net._ensure_packed(both)
    bad = []
    for l in layers:
        if c3:
            k, w, KD = l
            single = ops.conv3_pack(w.data, KD)
            views = net._pack_views[k]
        else:
            k, w, Cin, Cout, kf, kd = l
            single = (ops.k2_pack(w.data, Cin, Cout, kf), ops.k2_pack(w.data, Cin, Cout, kd))
            views = net._k2_views[k]
        for d in range(2 if both else 1):
            a, b = views[d].view(torch.int32), single[d].view(torch.int32)
            if c3:
                # the pack ends in a 32-word header: word 0 the weight's |max| (what the convs read), words 1 .. 16 the pack kernels' partial
                # maxima -- scratch, which a dgrad descriptor behind its forward twin leaves to the twin's header (csrc/conv3.hip k_wamax_many)
                h = a.numel() - 32
                a, b = torch.cat([a[:h + 1], a[h + 17:]]), torch.cat([b[:h + 1], b[h + 17:]])
            if not torch.equal(a, b):
                bad.append((k, "dgrad" if d else "fwd", int((a != b).sum())))
    assert not bad, f"{op} {n}: packed buffers differ from the single-layer pack: {bad[:6]}"
    return [(f"{op} {len(layers)} layers", (0.0, "exact"))]


def drive_c1(ops, dev, key, g, variants=((),)):
    """the fused first layer.  conv3_c1_norm_fwd: a = act(norm(conv(x, w) + b)) with y recomputed in fp32 and never stored, so cond is the
    norm's plus |gamma| * rstd * conv(|x|, |w|); statistics and running statistics as drive_norm_fwd.  conv3_c1_norm_bwd_wgrad: dw =
    wgrad(x, dy) with dy the fp64 norm backward (never written by the kernel), dgamma / dbeta as drive_norm_bwd; the flags (accumulate,
    dw_accumulate, the seeded dropout mask) are the step's.  The key does not say whether the norm is affine: the forward runs BatchNorm
    and, where G == N, InstanceNorm; the backward is affine where the step accumulates dgamma / dbeta."""
    op, shapes, ints, namax = key
    xs, ws = shapes[0], shapes[1]
    KD, G, act = ints
    two_d = KD == 1
    N, C = xs[0], 16
    ys = tuple(xs[:-1]) + (C,)
    tile = (1, 16, 16) if two_d else (4, 8, 8)
    fwd = op == "conv3_c1_norm_fwd"
    assert ops.conv3_c1_norm_ok(xs, KD, G), f"{op} {xs}: the fused first layer does not serve the step's shape"
    out = []
    for flags in variants:
        for affine in ((True, False) if G == N else (True,)) if fwd else ("accumulate" in flags or G != N,):
            tag = f"{op} {xs} [{'+'.join(flags) or 'plain'}{'' if affine else ' instance'}]"
            name = op + ("" if not flags else " " + "+".join(flags)) + ("" if affine else " in")
            x = activation(g, xs)
            w = _conv_weight(g, C, 1, KD)
            assert tuple(w.shape) == tuple(ws), key
            b = torch.randn(C, generator=g) * 0.1
            gam = (torch.rand(C, generator=g) + 0.5) if affine else None
            bet = (torch.rand(C, generator=g) - 0.5) if affine else None
            rm0, rv0 = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
            rm, rv = (rm0.clone().to(dev), rv0.clone().to(dev)) if affine else (None, None)
            _, sm, es, _, mult, H = _epilogue(ops, dev, g, ys, flags)
            xd, wd, bd = x.to(dev), w.to(dev), b.to(dev)
            a, st = ops.conv3_c1_norm_fwd(xd, wd, bd, KD, G, *((gam.to(dev), bet.to(dev)) if affine else (None, None)), rm, rv, act,
                                          elem_mask=sm, elem_scale=es)
            y64 = conv3_cl64(x, w) + b.double()
            cy = conv3_cl64(x.abs(), w.abs()) + b.double().abs()
            ar, z, xh, mu, var, ncond = norm_ref64(y64, G, gam, bet, act)
            gm = torch.ones(C, dtype=torch.float64) if gam is None else gam.double().abs()
            ycond = (gm / torch.sqrt(var + EPS) * cy.reshape(G, -1, C)).reshape(ys)       # what the fp32 recompute of y can move z by, per unit
            if fwd:
                _stats_check(st, mu, var, tag)
                out.append((name, check_elementwise(a.cpu(), ar * mult, (ncond + ycond) * mult.abs(), TAU, tag, tile)))
                if rm is not None:
                    _running_check(tag, rm, rv, rm0, rv0, mu, var, y64.numel() // C // G)
                continue
            da = gradient(g, ys)
            acc, dwacc = "accumulate" in flags, "dw_accumulate" in flags
            dy, dcond, dz, xg, dk = _norm_bwd_ref64(y64, G, gam, bet, act, da.double(), mult, ycond)
            wg = conv3_wgrad64(x, dy, 3, two_d)
            dw0 = gradient(g, ws, -4.0, 0.0) if dwacc else torch.zeros(ws)
            dg0, db0 = (torch.randn(C, generator=g) * 1e-2, torch.randn(C, generator=g) * 1e-2) if acc else (torch.zeros(C), torch.zeros(C))
            dg, db = (dg0.clone().to(dev), db0.clone().to(dev)) if affine else (None, None)
            dwd = dw0.clone().to(dev) if dwacc else torch.full(ws, float("nan"), device=dev)
            ops.conv3_c1_norm_bwd_wgrad(xd, wd, bd, KD, G, st, da.to(dev), act, dwd, dg, db, acc, dw_accumulate=dwacc, elem_mask=sm, elem_scale=es)
            # a kink element may take either branch: its own term and its share of the two means, through |x|, are allowed on top of the bound
            rstd = (gm / torch.sqrt(var + EPS))
            kdy = (rstd * (dk + dk.mean(1, keepdim=True) + xg.abs() * (dk * xg.abs()).mean(1, keepdim=True))).reshape(ys)
            dcond = torch.where(torch.isinf(dcond), torch.zeros_like(dcond), dcond)
            ref = wg + dw0.double()
            cond = conv3_wgrad64(x.abs(), dcond, 3, two_d) + dw0.double().abs()
            allow = conv3_wgrad64(x.abs(), kdy, 3, two_d)
            err = ((dwd.cpu().double() - ref).abs() - allow).clamp_min(0)
            out.append((name, check_elementwise(err, torch.zeros_like(err), cond, TAU, tag)))
            if affine:
                _dgamma_dbeta_check(tag, dg, db, dg0, db0, dz, xg, dk)
    return out


def drive_head(ops, dev, key, g, variants=((),)):
    """the fused 16 -> C head.  pw16_fwd_norm: logits = (act(norm(y)) * chan_scale) @ W^T + b from the raw conv output and the
    statistics of a real norm_fwd(stats_only) fed by conv3_fwd_stats partials, as the network runs it.  pw16_bwd_norm_bwd: dw / db of the
    head, dgamma / dbeta of the norm as bounded sums, the returned gradient w.r.t. y elementwise.  BatchNorm where the step passes a
    channel scale or accumulates the norm's gradients (LA), InstanceNorm otherwise (pancreas); the forward runs both."""
    op, shapes, ints, namax = key
    ys = shapes[0]
    G, act = ints[0], ints[1]
    N, C, Cout = ys[0], ys[-1], 2
    fwd = op == "pw16_fwd_norm"
    assert not fwd or ints[2] == Cout, key
    out = []
    for flags in variants:
        for affine in ((True, False) if G == N else (True,)) if fwd else ("norm_accumulate" in flags or G != N,):
            tag = f"{op} {ys} [{'+'.join(flags) or 'plain'}{'' if affine else ' instance'}]"
            name = op + ("" if not flags else " " + "+".join(flags)) + ("" if affine else " in")
            yd, part, rows = _conv_partial_source(ops, dev, g, ys, G)
            assert rows > 0 or dev.type == "cpu", f"{tag}: conv3_fwd_stats left no partials at the step's shape"
            y = yd.cpu()
            gam = (torch.rand(C, generator=g) + 0.5) if affine else None
            bet = (torch.rand(C, generator=g) - 0.5) if affine else None
            rm, rv = (torch.zeros(C, device=dev), torch.ones(C, device=dev)) if affine else (None, None)
            cs, _, _, _, mult, H = _epilogue(ops, dev, g, ys, tuple(f for f in flags if f == "chan_scale"))
            csd = None if cs is None else cs.to(dev)
            _, st = ops.norm_fwd(yd, G, *((gam.to(dev), bet.to(dev)) if affine else (None, None)), rm, rv, act, chan_scale=csd, stats_only=True,
                                 **({"partial": part, "nb": rows} if rows else {}))
            w = _k2_weight(g, (Cout, C, 1, 1, 1), C)
            b = torch.randn(Cout, generator=g) * 0.1
            wd, bd = w.to(dev), b.to(dev)
            W = w.double().reshape(Cout, C)
            ar, z, xh, mu, var, ncond = norm_ref64(y, G, gam, bet, act)
            _stats_check(st, mu, var, tag)
            if fwd:
                lg = ops.pw16_fwd_norm(yd, st, csd, G, act, wd, bd, Cout)
                ref = (ar * mult) @ W.t() + b.double()
                cond = (ncond * mult.abs()) @ W.abs().t() + b.double().abs()
                out.append((name, check_elementwise(lg.cpu(), ref, cond, TAU, tag)))
                continue
            acc, nacc = "accumulate" in flags, "norm_accumulate" in flags
            dy = gradient(g, tuple(ys[:-1]) + (Cout,))
            d2 = dy.double().reshape(-1, Cout)
            a2, c2 = (ar * mult).reshape(-1, C), (ncond * mult.abs()).reshape(-1, C)
            dwr, dcr = d2.t() @ a2, d2.sum(0)
            dw0, dc0 = (gradient(g, tuple(w.shape), -4.0, 0.0), gradient(g, (Cout,), -4.0, 0.0)) if acc else (torch.zeros(w.shape), torch.zeros(Cout))
            dg0, db0 = (torch.randn(C, generator=g) * 1e-2, torch.randn(C, generator=g) * 1e-2) if nacc else (torch.zeros(C), torch.zeros(C))
            dwd, dcd = ((dw0.clone().to(dev), dc0.clone().to(dev)) if acc
                        else (torch.full(tuple(w.shape), float("nan"), device=dev), torch.full((Cout,), float("nan"), device=dev)))
            dg, db = (dg0.clone().to(dev), db0.clone().to(dev)) if affine else (None, None)
            dyr = ops.pw16_bwd_norm_bwd(yd, st, csd, G, act, dy.to(dev), wd, dwd, dcd, dg, db, norm_accumulate=nacc, accumulate=acc)
            out.append((name + " dw", check_elementwise(dwd.cpu().reshape(Cout, C), dwr + dw0.double().reshape(Cout, C),
                                                        d2.abs().t() @ c2 + dw0.double().abs().reshape(Cout, C), TAU, tag + " dw")))
            out.append((name + " db", check_elementwise(dcd.cpu(), dcr + dc0.double(), d2.abs().sum(0) + dc0.double().abs(), TAU, tag + " db")))
            # the gradient entering the norm is dy @ W, formed in fp32: the bound is the norm backward's on |dy| @ |W|
            ref, _, dz, xg, _ = _norm_bwd_ref64(y, G, gam, bet, act, dy.double() @ W, mult)
            _, cond, dzb, _, dk = _norm_bwd_ref64(y, G, gam, bet, act, dy.double().abs() @ W.abs(), mult.abs())
            out.append((name, check_elementwise(dyr.cpu(), ref, cond, TAU, tag)))
            if affine:
                _dgamma_dbeta_check(tag, dg, db, dg0, db0, dz, xg, dk, dzb)
    return out


def mixloss_pair64(logits, labs, box6, flavour, weights, dtype=torch.float64):
    """closed form of the step's two mix_loss calls on channels-last logits [2N, D, H, W, C]: call h on samples hN .. hN + N - 1 with labels
    labs[h] = (img_l, patch_l) [N, D, H, W] and weights[h] = (w_img, w_patch); the image term outside the box, the patch term inside.
    flavour 0 (LA / pancreas, C = 2): masked soft Dice per (sample, class), smooth 1e-5, mean over N * C; loss = (dice + ce) / 2, out3 =
    {loss, ce, dice}, total = loss_1 + loss_2.  flavour 1 (ACDC, C = 4): Dice per class over the batch with squared denominators, smooth
    1e-10, mean over classes; out3 = {dice, ce, (dice + ce) / 2}, total = ((dice_2 + dice_1) + (ce_2 + ce_1)) / 2.  CE: region sum
    over region count + 1e-16.  -> (out6 [2, 3], total, d total / d logits, cond of that gradient: the sum of its terms' magnitudes),
    evaluated in `dtype` throughout (fp64: the reference; fp32: what plain fp32 arithmetic makes of the same expression)"""
    L = logits.to(dtype)
    N2, C = L.shape[0], L.shape[-1]
    N = N2 // 2
    sp = tuple(L.shape[1:4])
    inb = _in_box(sp, box6).reshape(1, -1)
    p = torch.softmax(L.reshape(N2, -1, C), dim=-1)
    lse = torch.logsumexp(L.reshape(N2, -1, C), dim=-1)
    out6 = torch.zeros(2, 3, dtype=dtype)
    grad, cond = torch.zeros_like(p), torch.zeros_like(p)
    for h in range(2):
        ph, Lh = p[h * N:(h + 1) * N], L.reshape(N2, -1, C)[h * N:(h + 1) * N]
        gp, gpa = torch.zeros_like(ph), torch.zeros_like(ph)            # d / d p of the dice term, and the magnitudes of its terms
        gl, gla = torch.zeros_like(ph), torch.zeros_like(ph)            # d / d logits of the ce term
        dice = ce = torch.zeros((), dtype=dtype)
        for lab, wgt, reg in ((labs[h][0], weights[h][0], ~inb), (labs[h][1], weights[h][1], inb)):
            r = reg.to(dtype).expand(N, -1).unsqueeze(-1)               # [N, V, 1]
            t = torch.nn.functional.one_hot(lab.reshape(N, -1).long(), C).to(dtype)
            if flavour == 0:
                s = 1e-5
                I, U = (ph * t * r).sum(1, keepdim=True), ((ph + t) * r).sum(1, keepdim=True)
                dice = dice + wgt * (1 - ((2 * I + s) / (U + s)).mean())
                k = wgt / (N * C) / (U + s) ** 2
                gp = gp - k * r * (2 * t * (U + s) - (2 * I + s))
                gpa = gpa + k * r * (2 * t * (U + s) + (2 * I + s))
            else:
                s = 1e-10
                I, Y, Z = (ph * t * r).sum((0, 1), keepdim=True), (t * r).sum((0, 1), keepdim=True), (ph * ph * r).sum((0, 1), keepdim=True)
                dice = dice + wgt * (1 - (2 * I + s) / (Z + Y + s)).sum() / C
                k = wgt / C / (Z + Y + s) ** 2
                gp = gp - k * r * (2 * t * (Z + Y + s) - (2 * I + s) * 2 * ph)
                gpa = gpa + k * r * (2 * t * (Z + Y + s) + (2 * I + s) * 2 * ph)
            cnt = r.sum() + 1e-16
            ce = ce + wgt * ((lse[h * N:(h + 1) * N].unsqueeze(-1) * t - Lh * t).sum(-1, keepdim=True) * r).sum() / cnt
            gl = gl + wgt / cnt * r * (ph - t)
            gla = gla + wgt / cnt * r * (ph + t)
        out6[h] = torch.stack([(dice + ce) / 2, ce, dice] if flavour == 0 else [dice, ce, (dice + ce) / 2])
        # softmax Jacobian on the dice part: dL_c = p_c * (gp_c - sum_k p_k gp_k); every term by its magnitude in cond
        dot, dota = (ph * gp).sum(-1, keepdim=True), (ph * gpa).sum(-1, keepdim=True)
        grad[h * N:(h + 1) * N] = 0.5 * (ph * (gp - dot) + gl)
        cond[h * N:(h + 1) * N] = 0.5 * (ph * (gpa + dota) + gla)
    total = out6[0, 0] + out6[1, 0] if flavour == 0 else ((out6[1, 0] + out6[0, 0]) + (out6[1, 1] + out6[0, 1])) / 2
    return out6, total, grad.reshape(L.shape), cond.reshape(L.shape)


# d total / d logits against the fp64 closed form, in units of cond (the sum of the closed form's term magnitudes).  The same closed form
# evaluated in fp32 by torch on the host differs from fp64 by at most TAU_LOSS_TORCH32 x cond over the drivers' inputs (all rows, both
# boxes); TAU_LOSS = 4 x that, rounded up to a power of two -- the kernel may order its few roundings differently.  The kernel itself
# measured TAU_LOSS_KERNEL x cond on the device.
TAU_LOSS_TORCH32 = 1.30e-6      # = 21.7 x 2^-24 (ACDC 12 x 256 x 256 x 4; LA 1.13e-6, pancreas 1.10e-6): exp() of a logit difference up to 24
TAU_LOSS_KERNEL = 1.24e-6       # ACDC, box against three faces; LA 1.07e-6, pancreas 1.09e-6; the simulator at the reduced LA shape 1.03e-6
TAU_LOSS = 2.0 ** -17           # 4 x 1.30e-6 = 5.2e-6 -> 7.63e-6


def _loss_inputs(g, ls, C):
    """logits spread over +-12 (some softmaxes saturate), blob-structured labels (cc_maps' smoothed noise, classes in bands for C = 4)"""
    N2 = ls[0]
    N, sp = N2 // 2, tuple(ls[1:4])
    logits = ((torch.rand(ls, generator=g, dtype=torch.float64) * 2 - 1) * 12).float()
    labs = []
    for _ in range(4):
        m = cc_maps((N,) + sp, g, two_d=sp[0] == 1)[0][1].long()
        if C == 4:
            m = (m * (1 + (torch.arange(sp[2]) * 3 // max(sp[2], 1)).view(1, 1, 1, -1))).clamp(max=3)
        labs.append(m.to(torch.uint8).contiguous())
    return logits, ((labs[0], labs[1]), (labs[2], labs[3]))


def drive_mixloss(ops, dev, key, g, variants=((),)):
    """mixloss_pair_fwd / mixloss_pair_bwd at the step's shape against the fp64 closed form (mixloss_pair64), for a random box and one
    against three faces with ragged edges: out6 and total to the project's gate |d| <= 1e-5, the gradient elementwise to TAU_LOSS x cond.
    The backward runs as the step's: written into a given buffer, the upstream gradient read from the device."""
    op, shapes, ints, namax = key
    ls, flavour = shapes[0], ints[0]
    C = ls[-1]
    sp = tuple(ls[1:4])
    weights = ((1.0, 0.5), (0.5, 1.0))                  # (labeled image + unlabeled patch, then the reverse: l_weight 1, u_weight 0.5)
    tile = (1, 16, 16) if sp[0] == 1 else (4, 8, 8)
    out = []
    for flags in variants:
        for bi, box6 in enumerate(_boxes(sp, g)):
            tag = f"{op} {ls} box {box6} [{'+'.join(flags) or 'plain'}]"
            logits, labs = _loss_inputs(g, ls, C)
            o64, t64, g64, c64 = mixloss_pair64(logits, labs, box6, flavour, weights)
            ld = logits.to(dev)
            lab = [t.to(dev) for pair in labs for t in pair]
            o6, total, ws = ops.mixloss_pair_fwd(ld, lab[0], lab[1], lab[2], lab[3], box6, flavour, weights[0], weights[1])
            d6 = float((o6.cpu().double() - o64).abs().max())
            dt = float((total.cpu().double() - t64).abs().max())
            print(f"[product-op] {tag}: out6 off by {d6:.3e} (relative {float(((o6.cpu().double() - o64).abs() / o64.abs()).max()):.3e}), "
                  f"total by {dt:.3e} (relative {dt / float(t64.abs()):.3e})")
            assert d6 <= 1e-5 and dt <= 1e-5, f"{tag}: out6 off by {d6:.3e}, total by {dt:.3e}"
            if op == "mixloss_pair_fwd":
                out.append((f"{op} box{bi}", (max(d6, dt) / 1e-5, "scalars")))
                continue
            up = 0.75
            kw = {}
            if "out" in flags:
                kw["out"] = torch.full(ls, float("nan"), device=dev)
            if "g_dev" in flags:
                kw["g_dev"] = torch.full((1,), up, device=dev)
            d = ops.mixloss_pair_bwd(ld, lab[0], lab[1], lab[2], lab[3], box6, flavour, ws, 0.5 * (1.0 if "g_dev" in flags else up),
                                     0.5 * (1.0 if "g_dev" in flags else up), **kw)
            _, _, g32, _ = mixloss_pair64(logits, labs, box6, flavour, weights, torch.float32)
            r32, _ = elementwise_ratio(g32.double(), g64, c64)
            print(f"[product-op] {tag}: the closed form in torch fp32 is off by {r32:.3e} x cond ({r32 / 2.0 ** -24:.2f} x 2^-24)")
            res = check_elementwise(d.cpu(), up * g64, up * c64, TAU_LOSS, tag, tile)
            print(f"[product-op] {tag}: the kernel is off by {res[0] * TAU_LOSS:.3e} x cond")
            out.append((f"{op} box{bi}", res))
    return out


# -------------------------------------------------------------------------------------------------- the validation passes' ops


def norm_eval_ref64(y, gamma, beta, rm, rv, act, residual=None, eps=EPS):
    """fp64 eval-mode BatchNorm: act((y - rm) * gamma / sqrt(rv + eps) + beta) [+ residual] -> (a, pre-activation z, cond, its part
    in front of the activation); eps as the kernel receives it (fp32)"""
    y, gamma, beta, rm, rv = (t.double().cpu() for t in (y, gamma, beta, rm, rv))
    sc = gamma / torch.sqrt(rv + float(np.float32(eps)))
    z = (y - rm) * sc + beta
    a, _ = _acts(act, z)
    zcond = (y - rm).abs() * sc.abs() + beta.abs()
    cond = zcond.clone()
    if residual is not None:
        a = a + residual.double().cpu()
        cond = cond + residual.double().cpu().abs()
    return a, z, cond, zcond


def drive_norm_eval(ops, dev, key, g, variants=((),)):
    """norm_eval at the chunk's shape: one launch at the recorded N, the fp64 reference sample by sample.  Running variances over four
    decades, gamma / beta as the norm drivers draw them, a residual where the pass adds a skip.  An element whose fp64 pre-activation
    lies within the bound of the activation's kink may take the other branch: there the two branches differ by less than |z|, which is
    allowed on top (the comparison is then the pre-activation's).  The output must carry no |max|: the convs behind take the
    three-plane instances."""
    op, shapes, ints, namax = key
    ys, act = shapes[0], ints[0]
    C = ys[-1]
    tile = (1, 16, 16) if ys[1] == 1 else (4, 8, 8)
    out = []
    for flags in variants:
        tag = f"{op} {ys} [{'+'.join(flags) or 'plain'}]"
        y = _pre_norm(g, ys)
        rm = (y.reshape(-1, C)[:4096].double().mean(0) + torch.randn(C, generator=g, dtype=torch.float64) * 0.1).float()
        rv = torch.pow(10.0, torch.rand(C, generator=g, dtype=torch.float64) * 4 - 2).float()
        gam, bet = torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) - 0.5
        res = activation(g, ys) if "residual" in flags else None
        a = ops.norm_eval(y.to(dev), gam.to(dev), bet.to(dev), rm.to(dev), rv.to(dev), act, residual=None if res is None else res.to(dev))
        assert getattr(a, "_bcp_amax", None) is None, f"{tag}: the output carries a |max|"
        ac = a.cpu()
        worst = None
        for n in range(ys[0]):
            ref, z, cond, zcond = norm_eval_ref64(y[n:n + 1], gam, bet, rm, rv, act, None if res is None else res[n:n + 1])
            kink = z.abs() <= TAU_NORM_EVAL * zcond
            err = ((ac[n:n + 1].double() - ref).abs() - torch.where(kink, z.abs(), torch.zeros_like(z))).clamp_min(0)
            r = check_elementwise(err, torch.zeros_like(err), cond, TAU_NORM_EVAL, f"{tag} sample {n}", tile)
            worst = r if worst is None or r[0] > worst[0] else worst
        out.append((op + ("" if not flags else " " + "+".join(flags)), worst))
    return out


def drive_c1_plain(ops, dev, key, g):
    """conv3_c1_fwd, the eval-mode first layer (1 -> 16, bias, no norm): fp64 conv sample by sample"""
    op, shapes, ints, namax = key
    xs, ws = shapes[0], shapes[1]
    KD = ints[0]
    x, w, b = activation(g, xs), _conv_weight(g, 16, 1, KD), torch.randn(16, generator=g) * 0.1
    assert tuple(w.shape) == tuple(ws), key
    y = ops.conv3_c1_fwd(x.to(dev), w.to(dev), b.to(dev), KD).cpu()
    tile = (1, 16, 16) if KD == 1 else (4, 8, 8)
    worst = None
    for n in range(xs[0]):
        ref = conv3_cl64(x[n:n + 1], w) + b.double()
        cond = conv3_cl64(x[n:n + 1].abs(), w.abs()) + b.double().abs()
        r = check_elementwise(y[n:n + 1], ref, cond, TAU, f"{op} {xs} sample {n}", tile)
        worst = r if worst is None or r[0] > worst[0] else worst
    return [(op, worst)]


def drive_pw16(ops, dev, key, g):
    """pw16_fwd, the eval-mode 16 -> C head on a materialised activation: x @ W^T + b in fp64"""
    from bcp_amd import hip_ops as H
    op, shapes, ints, namax = key
    xs, Cout = shapes[0], ints[0]
    x = activation(g, xs)
    w, b = _k2_weight(g, tuple(shapes[1]), 16), torch.randn(Cout, generator=g) * 0.1
    xd = x.to(dev)
    if namax:
        _amax(H, xd, dev)
    else:
        assert ops._amax_of(xd) is None, f"{op} {xs}: the operand carries a |max| the pass's does not"
    lg = ops.pw16_fwd(xd, w.to(dev), b.to(dev), Cout)
    W = w.double().reshape(Cout, 16)
    ref, cond = x.double() @ W.t() + b.double(), x.double().abs() @ W.abs().t() + b.double().abs()
    return [(op, check_elementwise(lg.cpu(), ref, cond, TAU, f"{op} {xs}"))]


def drive_copy_channels(ops, dev, key, g):
    """copy_channels as the eval-mode U-Net fills the skip half of a concat buffer: the first Cc channels bit for bit, the rest untouched"""
    op, shapes, ints, namax = key
    xs, ds = shapes[0], shapes[1]
    Cc, so, do = ints
    src = activation(g, xs)
    dst = torch.full(ds, 7.0, device=dev)
    ops.copy_channels(src.to(dev), dst, Cc, so, do, carry_amax=True)
    d = dst.cpu()
    assert torch.equal(d[..., do:do + Cc].contiguous().view(torch.int32), src[..., so:so + Cc].contiguous().view(torch.int32)), f"{op} {xs}: copied channels differ"
    keep = torch.ones(ds[-1], dtype=torch.bool)
    keep[do:do + Cc] = False
    assert bool((d[..., keep] == 7.0).all()), f"{op} {xs}: wrote outside its channels"
    assert getattr(dst, "_bcp_amax", None) is None, f"{op} {xs}: a source without |max| left one on the buffer"
    return [(op, (0.0, "exact"))]


def sw_origins(vol, patch, stride_xy=18, stride_z=4):
    """the patch origins of a sliding-window pass in stream order (test_3d_patch.sliding_window_scores: x, y, z nested, the last origin
    along an axis clamped to extent - patch) over a volume at least as large as the patch"""
    import math
    st = (stride_xy, stride_xy, stride_z)
    n = [math.ceil((v - p) / s) + 1 for v, p, s in zip(vol, patch, st)]
    return [tuple(min(s * i, v - p) for s, i, v, p in zip(st, ijk, vol, patch))
            for ijk in ((x, y, z) for x in range(n[0]) for y in range(n[1]) for z in range(n[2]))]


def _sw_logits(g, vol, patch, C, origins):
    """one patch of logits per origin: a volume-wide field uniform on +-12 (as _loss_inputs draws logits) cropped at the origin, plus a
    per-visit jitter of +-0.5 -- the overlapping patches of a real pass see the same voxels, so a voxel's visits agree up to the
    network's dependence on the patch position.  (Independent +-12 draws per visit would put a saturated 1 beside a saturated 0 on
    1.2 % of the twice-visited voxels: an average of exactly 0.5 that no real pass produces, and far over SW_BAND_CAP.)"""
    field = (torch.rand(vol + (C,), generator=g, dtype=torch.float64) * 2 - 1) * 12
    return [(field[x:x + patch[0], y:y + patch[1], z:z + patch[2]] + torch.rand(patch + (C,), generator=g, dtype=torch.float64) - 0.5).float()
            for x, y, z in origins]


def sw_ref(logits, origins, vol, cls, dtype=torch.float64):
    """sliding-window score of class `cls`: softmax per patch, summed over the visits in stream order, divided by the visit count, all in
    `dtype` (fp64: the reference; fp32: what plain torch arithmetic makes of the same expression) -> (score, integer counts)"""
    score, cnt = torch.zeros(vol, dtype=dtype), torch.zeros(vol, dtype=torch.int64)
    for lg, (x, y, z) in zip(logits, origins):
        px, py, pz = lg.shape[:3]
        score[x:x + px, y:y + py, z:z + pz] += torch.softmax(lg.to(dtype), -1)[..., cls]
        cnt[x:x + px, y:y + py, z:z + pz] += 1
    return score / cnt.to(dtype), cnt


# the sliding-window score against fp64, in units of the score itself (a sum of positive terms over a count: cond = the fp64 score).  The
# same expression in torch fp32 on the host is off by at most TAU_SW_TORCH32 x cond on the driver's inputs (logits uniform on +-12, five
# visits); TAU_SW = 4 x that, rounded up to a power of two (the rule that set TAU_LOSS).  The kernel: TAU_SW_KERNEL x cond on the device.
TAU_SW_TORCH32 = 1.09e-6        # = 18.3 x 2^-24 (LA 112 x 112 x 96, class 0; class 1 1.07e-6; pancreas 96 x 96 x 112 1.08e-6): exp() of a logit
                                # difference up to 25
TAU_SW_KERNEL = 1.10e-6         # pancreas 96 x 96 x 112, class 1 alone; LA 1.07e-6; the simulator at the reduced LA shape 1.02e-6
TAU_SW = 2.0 ** -17             # 4 x 1.09e-6 = 4.4e-6 -> 7.63e-6
SW_BAND_CAP = 1e-4              # at most this share of the voxels may lie within TAU_SW of the threshold (logit differences have density
                                # 1 / 24 at zero: about 1e-6 of them do)


def drive_sw(ops, dev, key, g):
    """sw_accumulate + sw_finish.  The sw_accumulate row replays a validation pass's origin list (strides 18 / 4: clamped last origins,
    overlapping patches, stream order) on logits spread over +-12, once with class 1 into one map (LA) and once with classes 0 and 1
    into two maps sharing the first one's counts (pancreas): counts exact, scores elementwise to TAU_SW x score, the label bit for bit
    `kernel score > 0.5` and equal to the fp64 label outside the band |ref - 0.5| <= TAU_SW.  The sw_finish row divides planted
    quotients: exact halves (label 0: the rule is >, not >=), their upper neighbours (label 1), zeros."""
    op, shapes, ints, namax = key
    vol = tuple(shapes[1] if op == "sw_accumulate" else shapes[0])
    out = []
    if op == "sw_finish":
        cnt = torch.randint(1, 6, vol, generator=g).float()
        score = (torch.rand(vol, generator=g, dtype=torch.float64) * cnt.double()).float()
        flat, cf = score.view(-1), cnt.view(-1)
        half = torch.arange(0, flat.numel(), 7)
        flat[half] = 0.5 * cf[half]                                                     # exact quotient 0.5 for every count
        up = half[: half.numel() // 2] + 1
        flat[up] = torch.nextafter(torch.tensor(0.5), torch.tensor(1.0)) * cf[up]
        flat[half[: half.numel() // 3] + 2] = 0.0
        ref = score.double() / cnt.double()
        sd = score.clone().to(dev)
        lab = ops.sw_finish(sd, cnt.to(dev), 0.5).cpu()
        sk = sd.cpu()
        res = check_elementwise(sk, ref, ref, 2.0 ** -24, f"{op} {vol} quotient")         # (one correctly rounded division)
        assert torch.equal(lab, (sk > 0.5).to(torch.uint8)), f"{op} {vol}: label differs from kernel score > 0.5"
        assert bool((sk.view(-1)[half] == 0.5).all()) and not bool(lab.view(-1)[half].any()), f"{op} {vol}: an exact 0.5 was labelled 1"
        far = (ref - 0.5).abs() > TAU_SW
        assert torch.equal(lab[far], (ref > 0.5).to(torch.uint8)[far]), f"{op} {vol}: label differs from the fp64 label outside the band"
        return [(op, res)]
    patch, C = tuple(shapes[0][:3]), shapes[0][3]
    origins = sw_origins(vol, patch)
    for classes in ((1,), (0, 1)):
        tag = f"{op} {vol} patch {patch} classes {classes}"
        logits = _sw_logits(g, vol, patch, C, origins)
        refs = [sw_ref(logits, origins, vol, c) for c in classes]
        for c, (r64, _) in zip(classes, refs):
            band = float(((r64 - 0.5).abs() <= TAU_SW).double().mean())
            assert band <= SW_BAND_CAP, f"{tag}: {band:.2e} of the fp64 scores of class {c} lie within the bound of the threshold"
        scores = [torch.zeros(vol, device=dev) for _ in classes]
        cnt = torch.zeros(vol, device=dev)
        scratch = torch.zeros(vol, device=dev)
        for lg, org in zip(logits, origins):
            ld = lg.to(dev)
            for ci, c in enumerate(classes):
                ops.sw_accumulate(ld, scores[ci], cnt if ci == 0 else scratch, org, cls=c)
        assert torch.equal(cnt.cpu().long(), refs[0][1]), f"{tag}: visit counts differ"
        for ci, c in enumerate(classes):
            r64 = refs[ci][0]
            lab = ops.sw_finish(scores[ci], cnt, 0.5).cpu()
            sk = scores[ci].cpu()
            r32, _ = elementwise_ratio(sw_ref(logits, origins, vol, c, torch.float32)[0].double(), r64, r64)
            res = check_elementwise(sk, r64, r64, TAU_SW, f"{tag} class {c}")
            print(f"[product-op] {tag} class {c}: torch fp32 is off by {r32:.3e} x cond ({r32 / 2.0 ** -24:.2f} x 2^-24), the kernel by "
                  f"{res[0] * TAU_SW:.3e} x cond")
            assert torch.equal(lab, (sk > 0.5).to(torch.uint8)), f"{tag} class {c}: label differs from kernel score > 0.5"
            far = (r64 - 0.5).abs() > TAU_SW
            assert torch.equal(lab[far], (r64 > 0.5).to(torch.uint8)[far]), f"{tag} class {c}: label differs from the fp64 label outside the band"
            out.append((f"{op} cls{c}/{len(classes)}", res))
    return out


def overlap_ref(pred, gt, cls):
    """{|A & B|, |A|, |B|} in numpy integers (A = pred != 0, or == cls where cls > 0; B = gt likewise)"""
    p, q = np.asarray(pred).reshape(-1), np.asarray(gt).reshape(-1)
    a, b = ((p == cls), (q == cls)) if cls else ((p != 0), (q != 0))
    return [int(np.count_nonzero(a & b)), int(np.count_nonzero(a)), int(np.count_nonzero(b))]


def drive_overlap(ops, dev, key, g):
    """overlap_counts on cc_maps pairs at the recorded size (binary maps for cls 0, three classes in bands for the ACDC classes), then on
    prefixes whose length is no multiple of 64 or 256, and lengths on both sides of the grid cap (2048 blocks of 256): exact"""
    op, shapes, ints, namax = key
    vol, cls = tuple(shapes[0]), ints[0]
    two_d = cls > 0                                                     # ACDC: [slices, H, W]
    maps = [m for _, m in cc_maps(((vol[0], 1) + vol[1:]) if two_d else ((1,) + vol), g, two_d=two_d)]
    if two_d:
        W = vol[2]
        maps = [(m.long() * (1 + (torch.arange(W) * 3 // max(W, 1)).view(1, 1, 1, W))).clamp(max=3).to(torch.uint8) for m in maps]
    maps = [m.reshape(vol).contiguous() for m in maps]
    n = maps[0].numel()
    cap = 2048 * 256
    lens = sorted({n - 1, n - vol[-1] - 37, 255, 257, cap - 1, cap + 1, cap + 257} & set(range(1, n)))
    for i, (p, q) in enumerate(((maps[0], maps[1]), (maps[1], maps[2]), (maps[2], maps[0]))):
        got = ops.overlap_counts(p.to(dev), q.to(dev), cls).tolist()
        assert got == overlap_ref(p, q, cls), f"{op} {vol} cls {cls} pair {i}: {got} != {overlap_ref(p, q, cls)}"
        for L in lens if i == 0 else ():
            pf, qf = p.reshape(-1)[:L].contiguous(), q.reshape(-1)[:L].contiguous()
            got = ops.overlap_counts(pf.to(dev), qf.to(dev), cls).tolist()
            assert got == overlap_ref(pf, qf, cls), f"{op} length {L} cls {cls}: {got} != {overlap_ref(pf, qf, cls)}"
    return [(op, (0.0, "exact"))]


def drive_argmax4(ops, dev, key, g):
    """plabel_argmax4 bit for bit against torch.argmax on the same fp32 logits, with planted exact ties (two, three and all four
    channels equal at the maximum): the first index wins"""
    op, shapes, ints, namax = key
    ls = shapes[0]
    lg = ((torch.rand(ls, generator=g, dtype=torch.float64) * 2 - 1) * 12).float()
    flat = lg.view(-1, 4)
    top = flat.max(1).values
    idx = torch.arange(0, flat.shape[0], 5)
    for j, sel in enumerate((idx[0::3], idx[1::3], idx[2::3])):
        ch = [(3, 1), (0, 2, 3), (0, 1, 2, 3)][j]
        for c in ch:
            flat[sel, c] = top[sel]
    ref = torch.argmax(lg, -1).to(torch.uint8)
    o = ops.plabel_argmax4(lg.to(dev)).cpu()
    assert torch.equal(o, ref), f"{op} {ls}: {int((o != ref).sum())} voxels differ from torch.argmax"
    return [(op, (0.0, "exact"))]


def mixloss64(logits, img_l, patch_l, box6, flavour, weights, dtype=torch.float64):
    """closed form of ONE mix_loss call (the pre-training loss): the first half of mixloss_pair64 on the batch doubled ->
    (out3, d ((dice + ce) / 2) / d logits, cond of that gradient)"""
    N = logits.shape[0]
    o6, _, gr, cond = mixloss_pair64(torch.cat([logits, logits]), ((img_l, patch_l), (img_l, patch_l)), box6, flavour, (weights, weights), dtype)
    return o6[0], gr[:N], cond[:N]


def drive_mixloss_single(ops, dev, key, g, variants=((),)):
    """mixloss_fwd / mixloss_bwd as the pre-training steps call them.  LA / pancreas (flavour 0, sup_loss_parts): both label arguments
    the same map, the all-zero box, weights (1, 0) -- CE and Dice over the whole volume.  ACDC (flavour 1, acdc_mix_loss(u_weight=1.0,
    unlab=True)): image and patch labels, a real box, weights (1, 1).  out3 to 1e-5, the gradient (upstream gradients on the device,
    0.5 each: loss = (dice + ce) / 2) elementwise to TAU_LOSS x cond."""
    op, shapes, ints, namax = key
    ls, flavour = shapes[0], ints[0]
    N, C = ls[0], ls[-1]
    sp = tuple(ls[1:4])
    tile = (1, 16, 16) if sp[0] == 1 else (4, 8, 8)
    out = []
    for flags in variants:
        cases = [((0,) * 6, (1.0, 0.0), True)] if flavour == 0 else [(b, (1.0, 1.0), False) for b in _boxes(sp, g)]
        for bi, (box6, wts, same) in enumerate(cases):
            tag = f"{op} {ls} box {box6} [{'+'.join(flags) or 'plain'}]"
            logits, labs = _loss_inputs(g, (2 * N,) + tuple(ls[1:]), C)
            logits = logits[:N].contiguous()
            img_l, patch_l = labs[0][0], (labs[0][0] if same else labs[0][1])
            o64, g64, c64 = mixloss64(logits, img_l, patch_l, box6, flavour, wts)
            ld, il, pl = logits.to(dev), img_l.to(dev), patch_l.to(dev)
            o3, ws = ops.mixloss_fwd(ld, il, pl, box6, flavour, wts[0], wts[1])
            d3 = float((o3.cpu().double() - o64).abs().max())
            print(f"[product-op] {tag}: out3 off by {d3:.3e}")
            assert d3 <= 1e-5, f"{tag}: out3 off by {d3:.3e}"
            if op == "mixloss_fwd":
                out.append((f"{op} box{bi}", (d3 / 1e-5, "scalars")))
                continue
            up = 0.75
            if "g_dev" in flags:
                d = ops.mixloss_bwd(ld, il, pl, box6, flavour, ws, 1.0, 1.0, g_dev=torch.full((2,), 0.5 * up, device=dev))
            else:
                d = ops.mixloss_bwd(ld, il, pl, box6, flavour, ws, 0.5 * up, 0.5 * up)
            res = check_elementwise(d.cpu(), up * g64, up * c64, TAU_LOSS, tag, tile)
            print(f"[product-op] {tag}: the kernel is off by {res[0] * TAU_LOSS:.3e} x cond")
            out.append((f"{op} box{bi}", res))
    return out


# -------------------------------------------------------------------------------------------------- the GroupNorm V-Nets
# lagn, lagn_pre, lagn_val, pancreasgn: normalization='groupnorm' (csrc/gnorm.hip).  The checks are those of tests/gnorm_seam_checks.py
# (gn_ref64, BwdRef, _table_check, dbias_closed64: the bound TAU * cond with the 2^-18 kink allowance, KINK_CAP on the reference before the
# device result is read, TAU_BIAS_CLOSED where the partial rows are visible), walked sample by sample -- a group never leaves its sample,
# so the reference of a 32 M element row is two of 16 M.  Inputs are the seam file's: per-channel offsets of order 30, per-sample offsets
# and scales that all differ.  Where the step feeds a layer's statistics from a producer's epilogue ('partial'), the driver asks the
# network's own planner which producers those are at the in-step shape (gn_routes) and launches each of them.
GN_PASSES = {"lagn": ("la", (112, 112, 80), ((2, "teacher"), (2, "student"))), "lagn_pre": ("la", (112, 112, 80), ((1, "student"),)),
             "lagn_val": ("la", (112, 112, 80), ((4, "eval"), (1, "eval"))), "pancreasgn": ("pancreas", (96, 96, 96), ((2, "teacher"), (2, "student")))}
GN_NEAR_MISSES = ("gn_channel_statistics", "gn_shifted_table", "gn_block_dropped", "gn_row4_flipped")
_GN_NETS = {}


def _seam():
    import gnorm_seam_checks as S        # (imports this module: not at load time)
    return S


def gn_routes(ops, wl, ys):
    """the planner (VNet.plan_forward: shape queries, no launch) for the passes of the GroupNorm workload `wl` -> {(producer, cin, flags)}
    of the layers whose gnorm_fwd reads a tensor of the in-step shape ys; producer: 'c1' / 'c3' / 'up' / 'down' (the seam file's names),
    flags: the epilogue as STEP_VARIANTS spells it ('partial' where the producer's row query answers > 0)"""
    from bcp_amd.networks.VNet import VNet
    variant, sp, passes = GN_PASSES[wl]
    net = _GN_NETS.get((variant, id(ops)))
    if net is None:
        net = _GN_NETS[(variant, id(ops))] = VNet(n_channels=1, n_classes=2, normalization="groupnorm", has_dropout=variant == "la", variant=variant).set_ops(ops)
    found = set()
    for N, mode in passes:
        train = mode != "eval"
        plan = net.plan_forward(N, *sp, 2, save=mode == "student", training=train, dropout=net.has_dropout and train)
        for L, r in zip(net._layers, plan.layers):
            if tuple(r.yshape) == tuple(ys) and r.norm == "gnorm_fwd":
                flags = tuple(f for f, on in (("chan_scale", r.dropout), ("partial", r.rows > 0), ("residual", L.skip_pop), ("stats_only", r.stats_only)) if on)
                found.add(({"c1": "c1", "c3": "c3", "dw": "down", "up": "up"}[L.kind], L.cin, flags))
    return found


def _np_rng(g):
    return np.random.default_rng(int(torch.randint(1, 1 << 31, (1,), generator=g)))


def _gn_producer(ops, dev, rng, prod, Cin, ys, tag):
    """the launch of the step's kind that leaves y of shape ys WITH its statistics rows (the seam file's _produce, the *_fwd_stats launch
    alone) -> (y on the device, partial, rows); rows == 0 where the reduced simulator shape is not served: the caller's own pass then"""
    S = _seam()
    N, C = ys[0], ys[-1]
    sp = tuple(ys[1:4])
    if prod == "up":
        if any(e % 2 for e in sp):
            return None, None, 0
        sp = tuple(e // 2 for e in sp)
    elif prod == "down":
        sp = tuple(2 * e for e in sp)
    if S.fwd_rows(ops, prod, (N,) + sp + (Cin,), C, N) <= 0:
        assert dev.type == "cpu", f"{tag}: the producer '{prod}' leaves no statistics rows at the step's shape"
        return None, None, 0
    return S._produce(ops, dev, rng, prod, N, Cin, C, sp, tag, verify=False)


def _gn_how(S, y, n, C):
    """the reference of sample n: GroupNorm's, or -- NEAR_MISS -- one that is wrong the way a plausible kernel would be: every channel its
    own statistics, sample n - 1's table, one block of the statistics pass left out -> (how, stats) for gn_ref64 / BwdRef"""
    N = y.shape[0]
    if NEAR_MISS == "gn_channel_statistics":
        _near_miss_hit(C > 16)
        return "channel", None
    if NEAR_MISS == "gn_shifted_table":
        _near_miss_hit(N > 1)
        return "group", S._stats64(y[(n - 1) % N:(n - 1) % N + 1].double().reshape(1, -1, C))
    if NEAR_MISS == "gn_block_dropped":
        rows = y[n].numel() // C
        chunk = -(-rows // max(2, S.own_geometry(rows, C)[0]))
        _near_miss_hit(chunk < rows)
        return ("drop", 0, chunk), None
    return "group", None


def _gn_mult(cs, n, shape):
    return None if cs is None else cs[n:n + 1].double().view(1, *([1] * (len(shape) - 2)), shape[-1])


def _worse(a, b):
    return b if a is None or b[0] > a[0] else a


def drive_gnorm_fwd(ops, dev, key, g, variants=((),), wl="lagn", table_key=None):
    """gnorm_fwd with each epilogue the step uses at this key: the statistics rows of every producer the planner names for it (or the
    kernel's own pass: hundreds of blocks per sample at these shapes), channel scale, the decoder's skip add, the table alone in front
    of the fused head.  The five table rows, a elementwise, the published |max|"""
    from bcp_amd import hip_ops as H
    S = _seam()
    op, shapes, ints, namax = key
    ys, act = tuple(shapes[0]), ints[0]
    N, C = ys[0], ys[-1]
    routes = gn_routes(ops, wl, tuple((table_key or key)[1][0]))
    out = []
    for flags in variants:
        srcs = [None]
        if "partial" in flags:
            srcs = sorted({(p, cin) for p, cin, f in routes if f == tuple(flags)})
            assert srcs, f"{op} {ys} {flags}: the planner names no producer for this epilogue"
        else:
            assert any(f == tuple(flags) for _, _, f in routes) or "stats_only" in flags, f"{op} {ys} {flags}: not an epilogue the planner emits here"
        for src in srcs:
            rng = _np_rng(g)
            tag = f"{op} {ys} [{'+'.join(flags) or 'plain'}{'' if src is None else f' {src[0]} {src[1]}->{C}'}]"
            name = op + ("" if not flags else " " + "+".join(flags)) + ("" if src is None else " " + src[0])
            yd, part, rows = _gn_producer(ops, dev, rng, src[0], src[1], ys, tag) if src else (None, None, 0)
            if yd is None:
                yd = S._pre_norm(rng, N, ys[1:4], C).to(dev)
            y = yd.cpu()
            gamma, beta = S._affine(rng, C)
            cs = S._chan_scale(rng, N, C) if "chan_scale" in flags else None
            res = torch.from_numpy(rng.standard_normal(ys, dtype=np.float32)) if "residual" in flags else None
            kw = dict(partial=part, nb=rows) if rows else {}
            a, st = ops.gnorm_fwd(yd, gamma.to(dev), beta.to(dev), act, chan_scale=None if cs is None else cs.to(dev),
                                  residual=None if res is None else res.to(dev), stats_only="stats_only" in flags, **kw)
            stc = st.cpu()
            worst = (0.0, "table") if a is None else None
            for n in range(N):
                sl = slice(n, n + 1)
                if NEAR_MISS is None:
                    S._table_check(f"{tag} sample {n}", stc[:, sl], y[sl], gamma, beta)
                if a is None:
                    continue
                how, stats = _gn_how(S, y, n, C)
                ar, _, _, _, _, cond = S.gn_ref64(y[sl], gamma, beta, act, how=how, stats=stats)
                mult = _gn_mult(cs, n, ys)
                if mult is not None:
                    ar, cond = ar * mult, cond * mult.abs()
                if res is not None:
                    ar, cond = ar + res[sl].double(), cond + res[sl].double().abs()
                worst = _worse(worst, check_elementwise(a[sl].cpu(), ar, cond, TAU, f"{tag} sample {n}"))
            if a is not None:
                assert H.amax_value(a._bcp_amax) == float(a.abs().max()), f"{tag}: |max| of a"
            out.append((name, worst))
    return out


def drive_gnorm_bwd(ops, dev, key, g, variants=((),), wl="lagn", table_key=None):
    """gnorm_bwd with each flag set the step uses at this key: the backward statistics from a real conv3_dgrad_bwdstats launch's rows
    ('partial') or from the kernel's own pass, channel scale, accumulation onto non-zero gradients, with and without the conv-bias gradient
    buffer.  dy elementwise, dgamma / dbeta, the conv-bias gradient (bias_chain; bias_closed from the producer's rows), the |max|"""
    from bcp_amd import hip_ops as H
    import kernel_checks as K
    S = _seam()
    op, shapes, ints, namax = key
    ys, act, accumulate = tuple(shapes[0]), ints[0], bool(ints[1])
    N, C = ys[0], ys[-1]
    sp, cg = ys[1:4], C // S.GROUPS
    out = []
    for flags in variants:
        assert ("accumulate" in flags) == accumulate, (key, flags)
        rng = _np_rng(g)
        tag = f"{op} {ys} [{'+'.join(flags) or 'plain'}]"
        y = S._pre_norm(rng, N, sp, C)
        gamma, beta = S._affine(rng, C)
        yd, gd = y.to(dev), gamma.to(dev)
        _, st = ops.gnorm_fwd(yd, gd, beta.to(dev), act)
        cs = S._chan_scale(rng, N, C) if "chan_scale" in flags else None
        part, rows = None, 0
        if "partial" in flags:
            rows = S.bwd_rows(ops, "c3", ys, C, N)
            assert rows > 0 or dev.type == "cpu", f"{tag}: conv3_dgrad_bwdstats leaves no rows at the step's shape"
        if rows:
            _, wd = ops.conv3_pack((K.R(rng, C, C, 3, 3, 3) * 0.1).to(dev).contiguous(), 3)
            dad, part, nb = ops.conv3_dgrad_bwdstats(_amax(H, K.to_cl(K.R(rng, N, C, *sp)).contiguous().to(dev), dev), wd, C, 3, yd, st, act, N)
            assert nb == rows, (tag, nb, rows)
            da = dad.cpu()
        else:
            da = (K.to_cl(K.R(rng, N, C, *sp)) + 5.0).contiguous()
            dad = da.to(dev)
        g0, gr = S._grad_start(rng, C, accumulate, dev)
        if "dbias" not in flags:
            gr[2] = None
        dy = ops.gnorm_bwd(yd, dad, st, gd, act, gr[0], gr[1], gr[2], accumulate, chan_scale=None if cs is None else cs.to(dev),
                           **(dict(partial=part, nb=rows) if rows else {}))
        worst = None
        acc = [torch.zeros(C, dtype=torch.float64) for _ in range(9)]      # sums, conds and kink allowances of dbeta, dgamma, dbias
        rstd, devs, closed = [], [], torch.zeros(C, dtype=torch.float64)
        refs = [S.BwdRef(y[n:n + 1], gamma, beta, act, da[n:n + 1].double(), _gn_mult(cs, n, ys), how=how, stats=stats)
                for n, (how, stats) in ((n, _gn_how(S, y, n, C)) for n in range(N))]
        S._kink_cap(tag, torch.cat([r_.kink for r_ in refs]))               # (on the reference, before the device result is read)
        KINK_SHARES.append((tag, sum(float(r_.kink.sum()) for r_ in refs) / y.numel()))
        print(f"[product-op] {tag}: {KINK_SHARES[-1][1]:.2e} of the elements at the activation's kink (cap {S.KINK_CAP:.0e})")
        for n in range(N):
            sl = slice(n, n + 1)
            ref, refs[n] = refs[n], None
            r = S._ratio(dy[sl], ref.dy, ref.cond, ref.allow)
            assert r <= TAU, f"{tag} sample {n}: dy off by {r:.3e} x cond (bound {TAU:.3e})"
            worst = _worse(worst, (r / TAU, f"sample {n}"))
            xa = ref.xg.abs()
            for i, t in enumerate((ref.dz.sum((0, 1)), ref.dz.abs().sum((0, 1)), ref.dk.sum((0, 1)),
                                   (ref.dz * ref.xg).sum((0, 1)), (ref.dz.abs() * xa).sum((0, 1)), (ref.dk * xa).sum((0, 1)),
                                   ref.dbias, ref.dbias_cond, ref.dbias_allow)):
                acc[i] += t
            if NEAR_MISS == "gn_row4_flipped":
                closed += S.dbias_closed64(ref.dz.sum(1), (ref.dz * ref.xg).sum(1), ref.gm, ref.rstd, ref.dev, ref.rows, flip=True)[0]
            rstd.append(ref.rstd)
            devs.append(ref.dev)
            del ref
        assert H.amax_value(dy._bcp_amax) == float(dy.abs().max()), f"{tag}: |max| of dy"
        for nm, t, base, i in (("dbeta", gr[1], g0[1], 0), ("dgamma", gr[0], g0[0], 3)):
            r = S._ratio(t, base.double() + acc[i], base.double().abs() + acc[i + 1], acc[i + 2])
            assert r <= TAU, f"{tag}: {nm} off by {r:.3e} x cond"
        if gr[2] is not None:
            assert cg > 1, key
            bias = acc[6]
            if NEAR_MISS == "gn_row4_flipped":
                bias = closed
                _near_miss_hit(True)
            rb = S._ratio(gr[2], g0[2].double() + bias, g0[2].double().abs() + acc[7], acc[8])
            assert rb <= TAU, f"{tag}: conv-bias gradient off by {rb:.3e} x cond (bias_chain, bound {TAU:.3e})"
            if rows and NEAR_MISS is None:      # bias_closed: the closed form in fp64 from the very rows the finalize read
                ps = _partials(part, N, rows, C)
                val, cc = S.dbias_closed64(ps[..., 0], ps[..., 1], gamma.double(), torch.cat(rstd), torch.cat(devs), y[0].numel() // C)
                rc = S._ratio(gr[2], g0[2].double() + val, g0[2].double().abs() + cc)
                assert rc <= S.TAU_BIAS_CLOSED, f"{tag}: conv-bias gradient off by {rc:.3e} x cond_c from the producer's own rows (bound 2^-22)"
        out.append((op + ("" if not flags else " " + "+".join(flags)), worst))
    return out


def drive_gn_head(ops, dev, key, g, variants=((),), wl="lagn", table_key=None):
    """the fused 16 -> C head on a GroupNorm table.  pw16_fwd_norm: logits from the raw conv output and the table gnorm_fwd(stats_only)
    makes from a real conv3_fwd_stats launch's rows, as the network runs it (groups = N).  pw16_bwd_norm: the gradient w.r.t. the
    activation elementwise, the head's weight and bias gradients as bounded sums, accumulated where the step accumulates"""
    import kernel_checks as K
    S = _seam()
    op, shapes, ints, namax = key
    ys = tuple(shapes[0])
    G, act = ints[0], ints[1]
    N, C, Cout = ys[0], ys[-1], 2
    assert G == N and C == 16, key
    fwd = op == "pw16_fwd_norm"
    out = []
    for flags in variants:
        rng = _np_rng(g)
        tag = f"{op} {ys} [{'+'.join(flags) or 'plain'}]"
        name = op + ("" if not flags else " " + "+".join(flags))
        yd, part, rows = _gn_producer(ops, dev, rng, "c3", C, ys, tag)
        if yd is None:
            yd = S._pre_norm(rng, N, ys[1:4], C).to(dev)
        y = yd.cpu()
        gamma, beta = S._affine(rng, C)
        cs = S._chan_scale(rng, N, C) if "chan_scale" in flags else None
        csd = None if cs is None else cs.to(dev)
        none, st = ops.gnorm_fwd(yd, gamma.to(dev), beta.to(dev), act, chan_scale=csd, stats_only=True, **(dict(partial=part, nb=rows) if rows else {}))
        assert none is None
        w = (K.R(rng, Cout, C, 1, 1, 1) * (2.0 / C) ** 0.5).contiguous()
        b = K.R(rng, Cout) * 0.1
        W = w.double().reshape(Cout, C)
        acc = "accumulate" in flags
        if fwd:
            res = ops.pw16_fwd_norm(yd, st, csd, G, act, w.to(dev), b.to(dev), Cout)
        else:
            dl = K.to_cl(K.R(rng, N, Cout, *ys[1:4])).contiguous()
            dw0, db0 = (K.R(rng, Cout, C, 1, 1, 1) * 0.5 + 1.0, K.R(rng, Cout) * 0.5 - 1.0) if acc else (torch.zeros(Cout, C, 1, 1, 1), torch.zeros(Cout))
            dwd, dbd = ((dw0.clone().contiguous().to(dev), db0.clone().to(dev)) if acc
                        else (torch.full((Cout, C, 1, 1, 1), float("nan"), device=dev), torch.full((Cout,), float("nan"), device=dev)))
            res = ops.pw16_bwd_norm(yd, st, csd, G, act, dl.to(dev), w.to(dev), dwd, dbd, accumulate=acc)
            dwr, dwc = dw0.double().reshape(Cout, C).clone(), dw0.double().abs().reshape(Cout, C).clone()
            dbr, dbc = db0.double().clone(), db0.double().abs().clone()
        stc = st.cpu()
        worst = None
        for n in range(N):
            sl = slice(n, n + 1)
            if NEAR_MISS is None:
                S._table_check(f"{tag} sample {n}", stc[:, sl], y[sl], gamma, beta)
            how, stats = _gn_how(S, y, n, C)
            ar, _, _, _, _, cond = S.gn_ref64(y[sl], gamma, beta, act, how=how, stats=stats)
            mult = _gn_mult(cs, n, ys)
            if mult is not None:
                ar, cond = ar * mult, cond * mult.abs()
            if fwd:
                worst = _worse(worst, check_elementwise(res[sl].cpu(), ar @ W.t() + b.double(), cond @ W.abs().t() + b.double().abs(), TAU, f"{tag} sample {n}"))
                continue
            d2 = dl[sl].double().reshape(-1, Cout)
            dwr += d2.t() @ ar.reshape(-1, C)
            dwc += d2.abs().t() @ cond.reshape(-1, C)
            dbr += d2.sum(0)
            dbc += d2.abs().sum(0)
            worst = _worse(worst, check_elementwise(res[sl].cpu(), dl[sl].double() @ W, dl[sl].double().abs() @ W.abs(), TAU, f"{tag} dh sample {n}"))
        out.append((name, worst))
        if not fwd:
            out.append((name + " dw", check_elementwise(dwd.cpu().reshape(Cout, C), dwr, dwc, TAU, tag + " dw")))
            out.append((name + " db", check_elementwise(dbd.cpu(), dbr, dbc, TAU, tag + " db")))
    return out


def _gn_table_from_rows(ops, dev, g, tag, yd, part, rows, G):
    """a producer row of a GroupNorm workload: the table gnorm_fwd (groups = N) makes from the launch's statistics rows, sample by sample"""
    S = _seam()
    N, C = yd.shape[0], yd.shape[-1]
    assert G == N, f"{tag}: a GroupNorm network asks for one statistics group per sample, the key says {G} for {N}"
    gamma, beta = S._affine(_np_rng(g), C)
    none, st = ops.gnorm_fwd(yd, gamma.to(dev), beta.to(dev), 1, partial=part, nb=rows, stats_only=True)
    assert none is None
    y, stc = yd.cpu(), st.cpu()
    for n in range(N):
        S._table_check(f"{tag}: gnorm_fwd from the launch's rows, sample {n}", stc[:, n:n + 1], y[n:n + 1], gamma, beta)


DRIVERS = {"conv3_fwd": drive_conv, "conv3_fwd_stats": drive_conv, "conv3_fwd_raw": drive_conv, "conv3_dgrad_bwdstats": drive_conv,
           "conv3_wgrad": drive_wgrad, "norm_fwd": drive_norm_fwd, "norm_bwd": drive_norm_bwd,
           "sgd": drive_optim, "ema": drive_optim, "adam": drive_optim,
           "maxpool2d_fwd": drive_pool, "maxpool2d_bwd": drive_pool, "bilinear2x_fwd": drive_pool, "bilinear2x_bwd": drive_pool,
           "plabel_cc_largest": drive_cc,
           "down_fwd": drive_k2, "down_dgrad": drive_k2, "up_fwd": drive_k2, "up_dgrad": drive_k2, "k2_fwd_stats": drive_k2,
           "k2_wgrad": drive_k2, "pw_fwd": drive_k2, "norm_fwd_slabs": drive_norm_slabs, "norm_bwd_slabs": drive_norm_slabs,
           "mix_box": drive_mix_box, "conv3_pack_many": drive_pack_many, "k2_pack_many": drive_pack_many,
           "conv3_c1_norm_fwd": drive_c1, "conv3_c1_norm_bwd_wgrad": drive_c1, "pw16_fwd_norm": drive_head, "pw16_bwd_norm_bwd": drive_head,
           "mixloss_pair_fwd": drive_mixloss, "mixloss_pair_bwd": drive_mixloss,
           "mixloss_fwd": drive_mixloss_single, "mixloss_bwd": drive_mixloss_single, "norm_eval": drive_norm_eval,
           "conv3_c1_fwd": drive_c1_plain, "pw16_fwd": drive_pw16, "copy_channels": drive_copy_channels,
           "sw_accumulate": drive_sw, "sw_finish": drive_sw, "overlap_counts": drive_overlap, "plabel_argmax4": drive_argmax4,
           "norm_fwd_res": drive_norm_fwd_res, "norm_bwd_res": drive_norm_bwd_res, "norm_eval_res": drive_norm_eval_res, "axpy": drive_axpy,
           "conv3_c1_fwd_stats": drive_c1_stats, "conv3_c1_wgrad": drive_c1_wgrad, "pw16_bwd": drive_pw16_bwd,
           "gnorm_fwd": drive_gnorm_fwd, "gnorm_bwd": drive_gnorm_bwd, "pw16_bwd_norm": drive_gn_head}


def table_rows():
    """[(workload, key)] in table order"""
    return [(wl, k) for wl, keys in STEP_KEYS.items() for k in keys]


def _row_ident(wl, k):
    """what makes a row a repeat of an earlier workload's: the key, the flags its calls pass, the norm groups a conv driver runs the
    layer behind with, -- for the pack rows, which drive a whole network -- the network, and for the ops that read or feed a norm table
    (GN_TABLE_OPS) whether that table is a GroupNorm table: the same key then means another thing"""
    return (k, tuple(variants_of(wl, k)), step_groups(wl) if k[0] == "conv3_dgrad_bwdstats" else stats_fused(wl, k) if k[0] == "conv3_fwd_stats" else None,
            network_of(wl) if k[0].endswith("pack_many") else None, "gn" if is_gn(wl) and k[0] in GN_TABLE_OPS else None)


def driven_rows():
    """table rows with a driver, plus norm keys only a statistics-only call uses (the profile does not record those); a key that
    already stands under an earlier workload with the same flags is driven once"""
    rows, seen = [], set()
    for wl, k in table_rows():
        if k[0] in DRIVERS and _row_ident(wl, k) not in seen:
            seen.add(_row_ident(wl, k))
            rows.append((wl, k))
    for wl, v in STEP_VARIANTS.items():
        for k in v:
            if k not in STEP_KEYS[wl] and _row_ident(wl, k) not in seen:
                seen.add(_row_ident(wl, k))
                rows.append((wl, k))
    return rows


def row_id(wl, key):
    """the row's parametrisation id: workload, op, first shape, int arguments (keys that differ only behind those -- a conv with and
    without bias -- share it, and pytest numbers them)"""
    op, shapes, ints, _ = key
    return f"{wl}-{op}-" + "x".join(str(v) for v in shapes[0]) + ("-" + "-".join(str(int(i)) for i in ints) if ints else "")


def reduce_key(key, f=8):
    """the key with every spatial extent divided by f (at least 2, even where a pool or a stride-2 conv needs it) and flat sizes by
    f^3: the host simulator's twin of an in-step shape"""
    op, shapes, ints, namax = key

    def red(s):
        if op in ("sw_accumulate", "sw_finish", "overlap_counts") and len(s) in (3, 4):      # a volume [X, Y, Z] / one patch's logits [px, py, pz, C]
            return tuple(max(2, e // f) for e in s[:3]) + tuple(s[3:])
        if len(s) == 5:
            N, D, H, W, C = s
            return (N, D if D == 1 else max(2, D // f), max(2, H // f) // 2 * 2, max(2, W // f) // 2 * 2, C)
        if len(s) == 6:
            return (s[0],) + red(s[1:])
        if len(s) == 1 and op in ("sgd", "ema", "adam"):
            return (max(64, s[0] // f ** 3),)
        return s
    def fine(s):
        """a k2s2 op's fine grid: every extent even, so that the coarse grid is exactly its half"""
        N, D, H, W, C = s
        return (N,) + tuple(max(2, e // f) // 2 * 2 for e in (D, H, W)) + (C,)

    def coarse(s):
        """the coarse grid of a k2s2 op, derived from its reduced fine grid (28 // 8 = 3 is no half of anything)"""
        N, D, H, W, C = s
        fs = fine((N, 2 * D, 2 * H, 2 * W, C))
        return (N, fs[1] // 2, fs[2] // 2, fs[3] // 2, C)
    # which of a k2s2 op's leading tensors live on the fine / coarse grid
    grids = {"down_fwd": (fine,), "up_dgrad": (fine,), "down_dgrad": (coarse,), "up_fwd": (coarse,),
             "k2_fwd_stats": ((fine,), (coarse,))[ints[0]] if op == "k2_fwd_stats" else None,
             "k2_wgrad": ((fine, coarse), (coarse, fine), (red, red))[ints[0]] if op == "k2_wgrad" else None}.get(op)
    if grids:
        shapes = tuple(grids[i](s) if i < len(grids) else s for i, s in enumerate(shapes))
        return op, shapes, ints, namax
    # shapes that stay: a weight gradient's, and the weights behind the input of the fused first layer and head
    first_only = op in ("conv3_c1_norm_fwd", "conv3_c1_norm_bwd_wgrad", "pw16_fwd_norm", "conv3_c1_fwd", "pw16_fwd", "conv3_c1_fwd_stats")
    shapes = tuple(s if (i > 0 and first_only) or (i == 2 and (op.endswith("wgrad") or op == "pw16_bwd")) else red(s) for i, s in enumerate(shapes))
    if op == "mix_box":                     # (the kernel takes W * C in fours)
        shapes = tuple(s[:3] + (max(4, s[3] // 4 * 4), s[4]) for s in shapes)
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
_VARIANT_OPS = ("norm_fwd", "norm_bwd", "down_fwd", "down_dgrad", "up_fwd", "up_dgrad", "k2_fwd_stats", "k2_wgrad", "pw_fwd",
                "norm_fwd_slabs", "norm_bwd_slabs", "mix_box", "conv3_c1_norm_fwd", "conv3_c1_norm_bwd_wgrad", "pw16_fwd_norm",
                "pw16_bwd_norm_bwd", "mixloss_pair_fwd", "mixloss_pair_bwd", "mixloss_fwd", "mixloss_bwd", "norm_eval",
                "norm_fwd_res", "norm_bwd_res", "norm_eval_res", "conv3_c1_wgrad", "pw16_bwd", "gnorm_fwd", "gnorm_bwd", "pw16_bwd_norm")
_FLAG_ORDER = ("chan_scale", "elem_mask", "partial", "bcast", "no_dres", "residual", "stats_only", "out_slab", "accumulate", "dw_accumulate",
               "norm_accumulate", "out", "mask", "g_dev", "dbias")


def _variant_flags(name, kw):
    """the flags of one call; kw: its arguments by parameter name (inspect.signature(...).bind: the networks pass some positionally)"""
    f = [n for n in ("chan_scale", "elem_mask", "partial") if kw.get(n) is not None]
    if name in ("norm_fwd_res", "norm_bwd_res", "norm_eval_res"):
        # the flags that pick a kernel instance or a branch of csrc/norm_res.hip: statistics rows from the producer, the per-sample channel
        # scale (segments per sample), the 1-channel broadcast residual (the RB instances), no dres store
        if kw["res"].shape[-1] == 1:
            f.append("bcast")
        if name == "norm_bwd_res" and not kw.get("want_dres", True):
            f.append("no_dres")
        return tuple(f)
    if kw.get("residual") is not None:
        f.append("residual")
    if kw.get("stats_only"):
        f.append("stats_only")
    out = kw.get("out")
    if name == "norm_fwd":
        if out is not None and out.dim() >= 2 and out.stride(-2) != out.shape[-1]:
            f.append("out_slab")
        out = None
    if name != "norm_bwd":                               # (norm_bwd's accumulate is the third int of its key already)
        f += [n for n in ("accumulate", "dw_accumulate", "norm_accumulate") if kw.get(n)]
    if out is not None:
        f.append("out")
    f += [n for n in ("mask", "g_dev") if kw.get(n) is not None]
    if name == "gnorm_bwd" and kw.get("dbias") is not None:      # the conv-bias gradient buffer (VNet._backward_impl: L.cout > 16)
        f.append("dbias")
    return tuple(f)


def _bound(fn, self, a, kw):
    import inspect
    return inspect.signature(fn).bind(self, *a, **kw).arguments


def variant_key(name, a):
    """the profile key of a call (hip_ops._profiled's arithmetic)"""
    ts = [t for t in a if isinstance(t, torch.Tensor)]
    return (name, tuple(tuple(t.shape) for t in ts[:3]), tuple(x for x in a if isinstance(x, int))[:3],
            sum(1 for t in ts[:2] if getattr(t, "_bcp_amax", None) is not None))


def record_step_variants(workload, names=None):
    """{key: set of flag tuples} of the calls of the ops `names` (_VARIANT_OPS) in one step of `workload` (its eager recording pass)"""
    from bcp_amd.hip_ops import Ops
    seen = {}
    names = _VARIANT_OPS if names is None else names
    saved = {n: getattr(Ops, n) for n in names}

    def wrap(name, fn):
        def w(self, *a, **kw):
            k = variant_key(name, a)
            k = (k[0], tuple(tuple(int(v) for v in s) for s in k[1]), tuple(int(v) for v in k[2]), k[3])
            seen.setdefault(k, set()).add(_variant_flags(name, _bound(fn, self, a, kw)))
            return fn(self, *a, **kw)
        return w
    for n in names:
        setattr(Ops, n, wrap(n, saved[n]))
    try:
        step = make_step(workload, torch.device("cuda:0"))
        for _ in range(max(1, setup_steps(workload))):
            step()
        torch.cuda.synchronize()
    finally:
        for n in names:
            setattr(Ops, n, saved[n])
    return seen


STEP_VARIANTS = {   # {workload: {key: flag sets the step uses}} (record_step_variants)
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
        ('down_dgrad', ((2, 7, 7, 5, 256), (262144,)), (128,), 1): (('accumulate', 'out'),),
        ('down_dgrad', ((2, 14, 14, 10, 128), (65536,)), (64,), 1): (('accumulate', 'out'),),
        ('down_dgrad', ((2, 28, 28, 20, 64), (16384,)), (32,), 1): (('accumulate', 'out'),),
        ('down_dgrad', ((2, 56, 56, 40, 32), (4096,)), (16,), 1): (('accumulate', 'out'),),
        ('k2_wgrad', ((2, 7, 7, 5, 256), (2, 14, 14, 10, 128), (256, 128, 2, 2, 2)), (1,), 2): (('accumulate',),),
        ('k2_wgrad', ((2, 14, 14, 10, 128), (2, 7, 7, 5, 256), (256, 128, 2, 2, 2)), (0,), 2): (('accumulate',),),
        ('k2_wgrad', ((2, 14, 14, 10, 128), (2, 28, 28, 20, 64), (128, 64, 2, 2, 2)), (1,), 2): (('accumulate',),),
        ('k2_wgrad', ((2, 28, 28, 20, 64), (2, 14, 14, 10, 128), (128, 64, 2, 2, 2)), (0,), 2): (('accumulate',),),
        ('k2_wgrad', ((2, 28, 28, 20, 64), (2, 56, 56, 40, 32), (64, 32, 2, 2, 2)), (1,), 2): (('accumulate',),),
        ('k2_wgrad', ((2, 56, 56, 40, 32), (2, 28, 28, 20, 64), (64, 32, 2, 2, 2)), (0,), 2): (('accumulate',),),
        ('k2_wgrad', ((2, 56, 56, 40, 32), (2, 112, 112, 80, 16), (32, 16, 2, 2, 2)), (1,), 2): (('accumulate',),),
        ('k2_wgrad', ((2, 112, 112, 80, 16), (2, 56, 56, 40, 32), (32, 16, 2, 2, 2)), (0,), 2): (('accumulate',),),
        ('mix_box', ((1, 112, 112, 80, 1), (1, 112, 112, 80, 1)), (), 0): (('out',),),
        ('norm_bwd_slabs', ((2, 7, 7, 5, 256), (8, 2, 7, 7, 5, 256), (5, 2, 256)), (8, 2, 1), 0): (('accumulate',),),
        ('norm_bwd_slabs', ((2, 14, 14, 10, 128), (4, 2, 14, 14, 10, 128), (5, 2, 128)), (4, 2, 1), 0): (('accumulate',),),
        ('norm_fwd_slabs', ((8, 2, 7, 7, 5, 256), (256,), (256,)), (8, 2, 1), 0): ((), ('chan_scale',)),
        ('conv3_c1_norm_bwd_wgrad', ((2, 112, 112, 80, 1), (16, 1, 3, 3, 3), (16,)), (3, 2, 1), 0): (('accumulate', 'dw_accumulate'),),
        ('pw16_bwd_norm_bwd', ((2, 112, 112, 80, 16), (5, 2, 16), (2, 16)), (2, 1), 0): (('chan_scale', 'accumulate', 'norm_accumulate'),),
        ('pw16_fwd_norm', ((2, 112, 112, 80, 16), (5, 2, 16), (2, 16)), (2, 1, 2), 0): (('chan_scale',),),
        ('mixloss_pair_bwd', ((2, 112, 112, 80, 2), (1, 112, 112, 80), (1, 112, 112, 80)), (0,), 0): (('out', 'g_dev'),),
        ('conv3_c1_norm_fwd', ((2, 112, 112, 80, 1), (16, 1, 3, 3, 3), (16,)), (3, 2, 1), 0): ((),),
        ('down_fwd', ((2, 14, 14, 10, 128), (262144,), (256,)), (256,), 1): ((),),
        ('down_fwd', ((2, 28, 28, 20, 64), (65536,), (128,)), (128,), 1): ((),),
        ('down_fwd', ((2, 56, 56, 40, 32), (16384,), (64,)), (64,), 1): ((),),
        ('down_fwd', ((2, 112, 112, 80, 16), (4096,), (32,)), (32,), 1): ((),),
        ('k2_fwd_stats', ((2, 56, 56, 40, 32), (4096,), (16,)), (1, 16, 2), 1): ((),),
        ('mixloss_pair_fwd', ((2, 112, 112, 80, 2), (1, 112, 112, 80), (1, 112, 112, 80)), (0,), 0): ((),),
        ('norm_fwd_slabs', ((4, 2, 14, 14, 10, 128), (128,), (128,)), (4, 2, 1), 0): ((),),
        ('up_dgrad', ((2, 14, 14, 10, 128), (262144,)), (256,), 1): ((),),
        ('up_dgrad', ((2, 28, 28, 20, 64), (65536,)), (128,), 1): ((),),
        ('up_dgrad', ((2, 56, 56, 40, 32), (16384,)), (64,), 1): ((),),
        ('up_dgrad', ((2, 112, 112, 80, 16), (4096,)), (32,), 1): ((),),
        ('up_fwd', ((2, 7, 7, 5, 256), (262144,), (128,)), (128,), 1): ((),),
        ('up_fwd', ((2, 14, 14, 10, 128), (65536,), (64,)), (64,), 1): ((),),
        ('up_fwd', ((2, 28, 28, 20, 64), (16384,), (32,)), (32,), 1): ((),),
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
        ('down_dgrad', ((2, 6, 6, 6, 256), (262144,)), (128,), 1): (('accumulate', 'out'),),
        ('down_dgrad', ((2, 12, 12, 12, 128), (65536,)), (64,), 1): (('accumulate', 'out'),),
        ('down_dgrad', ((2, 24, 24, 24, 64), (16384,)), (32,), 1): (('accumulate', 'out'),),
        ('down_dgrad', ((2, 48, 48, 48, 32), (4096,)), (16,), 1): (('accumulate', 'out'),),
        ('k2_wgrad', ((2, 6, 6, 6, 256), (2, 12, 12, 12, 128), (256, 128, 2, 2, 2)), (1,), 2): (('accumulate',),),
        ('k2_wgrad', ((2, 12, 12, 12, 128), (2, 6, 6, 6, 256), (256, 128, 2, 2, 2)), (0,), 2): (('accumulate',),),
        ('k2_wgrad', ((2, 12, 12, 12, 128), (2, 24, 24, 24, 64), (128, 64, 2, 2, 2)), (1,), 2): (('accumulate',),),
        ('k2_wgrad', ((2, 24, 24, 24, 64), (2, 12, 12, 12, 128), (128, 64, 2, 2, 2)), (0,), 2): (('accumulate',),),
        ('k2_wgrad', ((2, 24, 24, 24, 64), (2, 48, 48, 48, 32), (64, 32, 2, 2, 2)), (1,), 2): (('accumulate',),),
        ('k2_wgrad', ((2, 48, 48, 48, 32), (2, 24, 24, 24, 64), (64, 32, 2, 2, 2)), (0,), 2): (('accumulate',),),
        ('k2_wgrad', ((2, 48, 48, 48, 32), (2, 96, 96, 96, 16), (32, 16, 2, 2, 2)), (1,), 2): (('accumulate',),),
        ('k2_wgrad', ((2, 96, 96, 96, 16), (2, 48, 48, 48, 32), (32, 16, 2, 2, 2)), (0,), 2): (('accumulate',),),
        ('mix_box', ((1, 96, 96, 96, 1), (1, 96, 96, 96, 1)), (), 0): (('out',),),
        ('conv3_c1_norm_bwd_wgrad', ((2, 96, 96, 96, 1), (16, 1, 3, 3, 3), (16,)), (3, 2, 1), 0): (('dw_accumulate',),),
        ('pw16_bwd_norm_bwd', ((2, 96, 96, 96, 16), (5, 2, 16), (2, 96, 96, 96, 2)), (2, 1), 0): (('accumulate',),),
        ('mixloss_pair_bwd', ((2, 96, 96, 96, 2), (1, 96, 96, 96), (1, 96, 96, 96)), (0,), 0): (('out', 'g_dev'),),
        ('conv3_c1_norm_fwd', ((2, 96, 96, 96, 1), (16, 1, 3, 3, 3), (16,)), (3, 2, 1), 0): ((),),
        ('down_fwd', ((2, 12, 12, 12, 128), (262144,), (256,)), (256,), 1): ((),),
        ('down_fwd', ((2, 24, 24, 24, 64), (65536,), (128,)), (128,), 1): ((),),
        ('down_fwd', ((2, 48, 48, 48, 32), (16384,), (64,)), (64,), 1): ((),),
        ('down_fwd', ((2, 96, 96, 96, 16), (4096,), (32,)), (32,), 1): ((),),
        ('k2_fwd_stats', ((2, 48, 48, 48, 32), (4096,), (16,)), (1, 16, 2), 1): ((),),
        ('mixloss_pair_fwd', ((2, 96, 96, 96, 2), (1, 96, 96, 96), (1, 96, 96, 96)), (0,), 0): ((),),
        ('norm_bwd_slabs', ((2, 6, 6, 6, 256), (8, 2, 6, 6, 6, 256), (5, 2, 256)), (8, 2, 1), 0): ((),),
        ('norm_bwd_slabs', ((2, 12, 12, 12, 128), (4, 2, 12, 12, 12, 128), (5, 2, 128)), (4, 2, 1), 0): ((),),
        ('norm_fwd_slabs', ((4, 2, 12, 12, 12, 128), (128,)), (4, 2, 1), 0): ((),),
        ('norm_fwd_slabs', ((8, 2, 6, 6, 6, 256), (256,)), (8, 2, 1), 0): ((),),
        ('pw16_fwd_norm', ((2, 96, 96, 96, 16), (5, 2, 16), (2, 16, 1, 1, 1)), (2, 1, 2), 0): ((),),
        ('up_dgrad', ((2, 12, 12, 12, 128), (262144,)), (256,), 1): ((),),
        ('up_dgrad', ((2, 24, 24, 24, 64), (65536,)), (128,), 1): ((),),
        ('up_dgrad', ((2, 48, 48, 48, 32), (16384,)), (64,), 1): ((),),
        ('up_dgrad', ((2, 96, 96, 96, 16), (4096,)), (32,), 1): ((),),
        ('up_fwd', ((2, 6, 6, 6, 256), (262144,), (128,)), (128,), 1): ((),),
        ('up_fwd', ((2, 12, 12, 12, 128), (65536,), (64,)), (64,), 1): ((),),
        ('up_fwd', ((2, 24, 24, 24, 64), (16384,), (32,)), (32,), 1): ((),),
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
        ('k2_wgrad', ((12, 1, 16, 16, 256), (12, 1, 16, 16, 128), (128, 256, 1, 1)), (2,), 1): (('accumulate',),),
        ('k2_wgrad', ((12, 1, 32, 32, 128), (12, 1, 32, 32, 64), (64, 128, 1, 1)), (2,), 1): (('accumulate',),),
        ('k2_wgrad', ((12, 1, 64, 64, 64), (12, 1, 64, 64, 32), (32, 64, 1, 1)), (2,), 1): (('accumulate',),),
        ('k2_wgrad', ((12, 1, 128, 128, 32), (12, 1, 128, 128, 16), (16, 32, 1, 1)), (2,), 1): (('accumulate',),),
        ('mix_box', ((6, 1, 256, 256, 1), (6, 1, 256, 256, 1)), (), 0): (('out',),),
        ('norm_bwd_slabs', ((12, 1, 16, 16, 256), (4, 12, 1, 16, 16, 256), (5, 2, 256)), (4, 2, 2), 0): (('elem_mask', 'accumulate'),),
        ('norm_fwd_slabs', ((4, 12, 1, 16, 16, 256), (256,), (256,)), (4, 2, 2), 0): ((), ('elem_mask',)),
        ('conv3_c1_norm_bwd_wgrad', ((12, 1, 256, 256, 1), (16, 1, 3, 3), (16,)), (1, 2, 2), 0): (('elem_mask', 'accumulate', 'dw_accumulate'),),
        ('conv3_c1_norm_fwd', ((12, 1, 256, 256, 1), (16, 1, 3, 3), (16,)), (1, 2, 2), 0): (('elem_mask',),),
        ('mixloss_pair_bwd', ((12, 1, 256, 256, 4), (6, 1, 256, 256), (6, 1, 256, 256)), (1,), 0): (('out', 'g_dev'),),
        ('mixloss_pair_fwd', ((12, 1, 256, 256, 4), (6, 1, 256, 256), (6, 1, 256, 256)), (1,), 0): ((),),
        ('pw_fwd', ((12, 1, 16, 16, 128), (32768,)), (256,), 0): ((),),
        ('pw_fwd', ((12, 1, 16, 16, 256), (32768,), (128,)), (128,), 1): ((),),
        ('pw_fwd', ((12, 1, 32, 32, 64), (8192,)), (128,), 0): ((),),
        ('pw_fwd', ((12, 1, 32, 32, 128), (8192,), (64,)), (64,), 1): ((),),
        ('pw_fwd', ((12, 1, 64, 64, 32), (2048,)), (64,), 0): ((),),
        ('pw_fwd', ((12, 1, 64, 64, 64), (2048,), (32,)), (32,), 1): ((),),
        ('pw_fwd', ((12, 1, 128, 128, 16), (512,)), (32,), 0): ((),),
        ('pw_fwd', ((12, 1, 128, 128, 32), (512,), (16,)), (16,), 1): ((),),
    },
    "la_pre": {
        ('conv3_c1_norm_bwd_wgrad', ((1, 112, 112, 80, 1), (16, 1, 3, 3, 3), (16,)), (3, 1, 1), 0): (('accumulate', 'dw_accumulate'),),
        ('conv3_c1_norm_fwd', ((1, 112, 112, 80, 1), (16, 1, 3, 3, 3), (16,)), (3, 1, 1), 0): ((),),
        ('down_dgrad', ((1, 14, 14, 10, 128), (65536,)), (64,), 1): (('accumulate', 'out'),),
        ('down_dgrad', ((1, 28, 28, 20, 64), (16384,)), (32,), 1): (('accumulate', 'out'),),
        ('down_dgrad', ((1, 56, 56, 40, 32), (4096,)), (16,), 1): (('accumulate', 'out'),),
        ('down_dgrad', ((1, 7, 7, 5, 256), (262144,)), (128,), 1): (('accumulate', 'out'),),
        ('down_fwd', ((1, 112, 112, 80, 16), (4096,), (32,)), (32,), 1): ((),),
        ('down_fwd', ((1, 14, 14, 10, 128), (262144,), (256,)), (256,), 1): ((),),
        ('down_fwd', ((1, 28, 28, 20, 64), (65536,), (128,)), (128,), 1): ((),),
        ('down_fwd', ((1, 56, 56, 40, 32), (16384,), (64,)), (64,), 1): ((),),
        ('k2_wgrad', ((1, 112, 112, 80, 16), (1, 56, 56, 40, 32), (32, 16, 2, 2, 2)), (0,), 2): (('accumulate',),),
        ('k2_wgrad', ((1, 14, 14, 10, 128), (1, 28, 28, 20, 64), (128, 64, 2, 2, 2)), (1,), 2): (('accumulate',),),
        ('k2_wgrad', ((1, 14, 14, 10, 128), (1, 7, 7, 5, 256), (256, 128, 2, 2, 2)), (0,), 2): (('accumulate',),),
        ('k2_wgrad', ((1, 28, 28, 20, 64), (1, 14, 14, 10, 128), (128, 64, 2, 2, 2)), (0,), 2): (('accumulate',),),
        ('k2_wgrad', ((1, 28, 28, 20, 64), (1, 56, 56, 40, 32), (64, 32, 2, 2, 2)), (1,), 2): (('accumulate',),),
        ('k2_wgrad', ((1, 56, 56, 40, 32), (1, 112, 112, 80, 16), (32, 16, 2, 2, 2)), (1,), 2): (('accumulate',),),
        ('k2_wgrad', ((1, 56, 56, 40, 32), (1, 28, 28, 20, 64), (64, 32, 2, 2, 2)), (0,), 2): (('accumulate',),),
        ('k2_wgrad', ((1, 7, 7, 5, 256), (1, 14, 14, 10, 128), (256, 128, 2, 2, 2)), (1,), 2): (('accumulate',),),
        ('mix_box', ((1, 112, 112, 80, 1), (1, 112, 112, 80, 1)), (), 0): ((),),
        ('norm_bwd', ((1, 112, 112, 80, 16), (1, 112, 112, 80, 16), (5, 1, 16)), (1, 1, 1), 0): ((),),
        ('norm_bwd', ((1, 14, 14, 10, 128), (1, 14, 14, 10, 128), (5, 1, 128)), (1, 1, 1), 0): ((),),
        ('norm_bwd', ((1, 28, 28, 20, 64), (1, 28, 28, 20, 64), (5, 1, 64)), (1, 1, 1), 0): ((),),
        ('norm_bwd', ((1, 56, 56, 40, 32), (1, 56, 56, 40, 32), (5, 1, 32)), (1, 1, 1), 0): ((), ('partial',)),
        ('norm_bwd', ((1, 7, 7, 5, 256), (1, 7, 7, 5, 256), (5, 1, 256)), (1, 1, 1), 0): ((), ('chan_scale',)),
        ('norm_bwd_slabs', ((1, 14, 14, 10, 128), (4, 1, 14, 14, 10, 128), (5, 1, 128)), (4, 1, 1), 0): (('accumulate',),),
        ('norm_fwd', ((1, 112, 112, 80, 16), (16,), (16,)), (1, 1), 0): (('chan_scale', 'partial', 'stats_only'), ('residual',)),
        ('norm_fwd', ((1, 14, 14, 10, 128), (128,), (128,)), (1, 1), 0): ((), ('residual',)),
        ('norm_fwd', ((1, 28, 28, 20, 64), (64,), (64,)), (1, 1), 0): ((), ('partial',), ('residual',)),
        ('norm_fwd', ((1, 56, 56, 40, 32), (32,), (32,)), (1, 1), 0): ((), ('partial',), ('residual',)),
        ('norm_fwd', ((1, 7, 7, 5, 256), (256,), (256,)), (1, 1), 0): ((), ('chan_scale',)),
        ('norm_fwd_slabs', ((4, 1, 14, 14, 10, 128), (128,), (128,)), (4, 1, 1), 0): ((),),
        ('pw16_bwd_norm_bwd', ((1, 112, 112, 80, 16), (5, 1, 16), (1, 16)), (1, 1), 0): (('chan_scale', 'accumulate', 'norm_accumulate'),),
        ('pw16_fwd_norm', ((1, 112, 112, 80, 16), (5, 1, 16), (1, 16)), (1, 1, 2), 0): (('chan_scale',),),
        ('up_dgrad', ((1, 112, 112, 80, 16), (4096,)), (32,), 1): ((),),
        ('up_dgrad', ((1, 14, 14, 10, 128), (262144,)), (256,), 1): ((),),
        ('up_dgrad', ((1, 28, 28, 20, 64), (65536,)), (128,), 1): ((),),
        ('up_dgrad', ((1, 56, 56, 40, 32), (16384,)), (64,), 1): ((),),
        ('up_fwd', ((1, 14, 14, 10, 128), (65536,), (64,)), (64,), 1): ((),),
        ('up_fwd', ((1, 28, 28, 20, 64), (16384,), (32,)), (32,), 1): ((),),
        ('up_fwd', ((1, 56, 56, 40, 32), (4096,), (16,)), (16,), 1): ((),),
        ('up_fwd', ((1, 7, 7, 5, 256), (262144,), (128,)), (128,), 1): ((),),
        ('mixloss_fwd', ((1, 112, 112, 80, 2), (1, 112, 112, 80), (1, 112, 112, 80)), (0,), 0): ((),),
        ('mixloss_bwd', ((1, 112, 112, 80, 2), (1, 112, 112, 80), (1, 112, 112, 80)), (0,), 0): (('g_dev',),),
    },
    "pancreas_pre": {
        ('conv3_c1_norm_bwd_wgrad', ((1, 96, 96, 96, 1), (16, 1, 3, 3, 3), (16,)), (3, 1, 1), 0): (('dw_accumulate',),),
        ('conv3_c1_norm_fwd', ((1, 96, 96, 96, 1), (16, 1, 3, 3, 3), (16,)), (3, 1, 1), 0): ((),),
        ('down_dgrad', ((1, 12, 12, 12, 128), (65536,)), (64,), 1): (('accumulate', 'out'),),
        ('down_dgrad', ((1, 24, 24, 24, 64), (16384,)), (32,), 1): (('accumulate', 'out'),),
        ('down_dgrad', ((1, 48, 48, 48, 32), (4096,)), (16,), 1): (('accumulate', 'out'),),
        ('down_dgrad', ((1, 6, 6, 6, 256), (262144,)), (128,), 1): (('accumulate', 'out'),),
        ('down_fwd', ((1, 12, 12, 12, 128), (262144,), (256,)), (256,), 1): ((),),
        ('down_fwd', ((1, 24, 24, 24, 64), (65536,), (128,)), (128,), 1): ((),),
        ('down_fwd', ((1, 48, 48, 48, 32), (16384,), (64,)), (64,), 1): ((),),
        ('down_fwd', ((1, 96, 96, 96, 16), (4096,), (32,)), (32,), 1): ((),),
        ('k2_wgrad', ((1, 12, 12, 12, 128), (1, 24, 24, 24, 64), (128, 64, 2, 2, 2)), (1,), 2): (('accumulate',),),
        ('k2_wgrad', ((1, 12, 12, 12, 128), (1, 6, 6, 6, 256), (256, 128, 2, 2, 2)), (0,), 2): (('accumulate',),),
        ('k2_wgrad', ((1, 24, 24, 24, 64), (1, 12, 12, 12, 128), (128, 64, 2, 2, 2)), (0,), 2): (('accumulate',),),
        ('k2_wgrad', ((1, 24, 24, 24, 64), (1, 48, 48, 48, 32), (64, 32, 2, 2, 2)), (1,), 2): (('accumulate',),),
        ('k2_wgrad', ((1, 48, 48, 48, 32), (1, 24, 24, 24, 64), (64, 32, 2, 2, 2)), (0,), 2): (('accumulate',),),
        ('k2_wgrad', ((1, 48, 48, 48, 32), (1, 96, 96, 96, 16), (32, 16, 2, 2, 2)), (1,), 2): (('accumulate',),),
        ('k2_wgrad', ((1, 6, 6, 6, 256), (1, 12, 12, 12, 128), (256, 128, 2, 2, 2)), (1,), 2): (('accumulate',),),
        ('k2_wgrad', ((1, 96, 96, 96, 16), (1, 48, 48, 48, 32), (32, 16, 2, 2, 2)), (0,), 2): (('accumulate',),),
        ('mix_box', ((1, 96, 96, 96, 1), (1, 96, 96, 96, 1)), (), 0): ((),),
        ('norm_bwd', ((1, 12, 12, 12, 128), (1, 12, 12, 12, 128), (5, 1, 128)), (1, 1, 0), 0): ((),),
        ('norm_bwd', ((1, 24, 24, 24, 64), (1, 24, 24, 24, 64), (5, 1, 64)), (1, 1, 0), 0): ((),),
        ('norm_bwd', ((1, 48, 48, 48, 32), (1, 48, 48, 48, 32), (5, 1, 32)), (1, 1, 0), 0): ((), ('partial',)),
        ('norm_bwd', ((1, 6, 6, 6, 256), (1, 6, 6, 6, 256), (5, 1, 256)), (1, 1, 0), 0): ((),),
        ('norm_bwd', ((1, 96, 96, 96, 16), (1, 96, 96, 96, 16), (5, 1, 16)), (1, 1, 0), 0): ((),),
        ('norm_bwd_slabs', ((1, 12, 12, 12, 128), (4, 1, 12, 12, 12, 128), (5, 1, 128)), (4, 1, 1), 0): ((),),
        ('norm_fwd', ((1, 12, 12, 12, 128),), (1, 1), 0): ((), ('residual',)),
        ('norm_fwd', ((1, 24, 24, 24, 64),), (1, 1), 0): ((), ('residual',)),
        ('norm_fwd', ((1, 48, 48, 48, 32),), (1, 1), 0): ((), ('partial',), ('residual',)),
        ('norm_fwd', ((1, 6, 6, 6, 256),), (1, 1), 0): ((),),
        ('norm_fwd', ((1, 96, 96, 96, 16),), (1, 1), 0): (('partial', 'stats_only'), ('residual',)),
        ('norm_fwd_slabs', ((4, 1, 12, 12, 12, 128), (128,)), (4, 1, 1), 0): ((),),
        ('pw16_bwd_norm_bwd', ((1, 96, 96, 96, 16), (5, 1, 16), (1, 96, 96, 96, 2)), (1, 1), 0): (('accumulate',),),
        ('pw16_fwd_norm', ((1, 96, 96, 96, 16), (5, 1, 16), (2, 16, 1, 1, 1)), (1, 1, 2), 0): ((),),
        ('up_dgrad', ((1, 12, 12, 12, 128), (262144,)), (256,), 1): ((),),
        ('up_dgrad', ((1, 24, 24, 24, 64), (65536,)), (128,), 1): ((),),
        ('up_dgrad', ((1, 48, 48, 48, 32), (16384,)), (64,), 1): ((),),
        ('up_dgrad', ((1, 96, 96, 96, 16), (4096,)), (32,), 1): ((),),
        ('up_fwd', ((1, 12, 12, 12, 128), (65536,), (64,)), (64,), 1): ((),),
        ('up_fwd', ((1, 24, 24, 24, 64), (16384,), (32,)), (32,), 1): ((),),
        ('up_fwd', ((1, 48, 48, 48, 32), (4096,), (16,)), (16,), 1): ((),),
        ('up_fwd', ((1, 6, 6, 6, 256), (262144,), (128,)), (128,), 1): ((),),
        ('mixloss_fwd', ((1, 96, 96, 96, 2), (1, 96, 96, 96), (1, 96, 96, 96)), (0,), 0): ((),),
        ('mixloss_bwd', ((1, 96, 96, 96, 2), (1, 96, 96, 96), (1, 96, 96, 96)), (0,), 0): (('g_dev',),),
    },
    "acdc_pre": {
        ('conv3_c1_norm_bwd_wgrad', ((6, 1, 256, 256, 1), (16, 1, 3, 3), (16,)), (1, 1, 2), 0): (('elem_mask', 'accumulate', 'dw_accumulate'),),
        ('conv3_c1_norm_fwd', ((6, 1, 256, 256, 1), (16, 1, 3, 3), (16,)), (1, 1, 2), 0): (('elem_mask',),),
        ('k2_wgrad', ((6, 1, 128, 128, 32), (6, 1, 128, 128, 16), (16, 32, 1, 1)), (2,), 1): (('accumulate',),),
        ('k2_wgrad', ((6, 1, 16, 16, 256), (6, 1, 16, 16, 128), (128, 256, 1, 1)), (2,), 1): (('accumulate',),),
        ('k2_wgrad', ((6, 1, 32, 32, 128), (6, 1, 32, 32, 64), (64, 128, 1, 1)), (2,), 1): (('accumulate',),),
        ('k2_wgrad', ((6, 1, 64, 64, 64), (6, 1, 64, 64, 32), (32, 64, 1, 1)), (2,), 1): (('accumulate',),),
        ('mix_box', ((6, 1, 256, 256, 1), (6, 1, 256, 256, 1)), (), 0): ((),),
        ('norm_bwd', ((6, 1, 128, 128, 32), (6, 1, 128, 128, 32), (5, 1, 32)), (1, 2, 1), 0): ((), ('elem_mask',), ('partial',)),
        ('norm_bwd', ((6, 1, 16, 16, 256), (6, 1, 16, 16, 256), (5, 1, 256)), (1, 2, 1), 0): ((),),
        ('norm_bwd', ((6, 1, 256, 256, 16), (6, 1, 256, 256, 16), (5, 1, 16)), (1, 2, 1), 0): ((),),
        ('norm_bwd', ((6, 1, 32, 32, 128), (6, 1, 32, 32, 128), (5, 1, 128)), (1, 2, 1), 0): ((), ('elem_mask',)),
        ('norm_bwd', ((6, 1, 64, 64, 64), (6, 1, 64, 64, 64), (5, 1, 64)), (1, 2, 1), 0): ((), ('elem_mask',)),
        ('norm_bwd_slabs', ((6, 1, 16, 16, 256), (4, 6, 1, 16, 16, 256), (5, 1, 256)), (4, 1, 2), 0): (('elem_mask', 'accumulate'),),
        ('norm_fwd', ((6, 1, 128, 128, 32), (32,), (32,)), (1, 2), 0): (('elem_mask', 'partial'), ('partial',), ('partial', 'out_slab')),
        ('norm_fwd', ((6, 1, 256, 256, 16), (16,), (16,)), (1, 2), 0): (('partial',), ('partial', 'out_slab')),
        ('norm_fwd', ((6, 1, 32, 32, 128), (128,), (128,)), (1, 2), 0): ((), ('elem_mask',), ('out_slab',)),
        ('norm_fwd', ((6, 1, 64, 64, 64), (64,), (64,)), (1, 2), 0): (('elem_mask', 'partial'), ('partial',), ('partial', 'out_slab')),
        ('norm_fwd_slabs', ((4, 6, 1, 16, 16, 256), (256,), (256,)), (4, 1, 2), 0): ((), ('elem_mask',)),
        ('pw_fwd', ((6, 1, 128, 128, 16), (512,)), (32,), 0): ((),),
        ('pw_fwd', ((6, 1, 128, 128, 32), (512,), (16,)), (16,), 1): ((),),
        ('pw_fwd', ((6, 1, 16, 16, 128), (32768,)), (256,), 0): ((),),
        ('pw_fwd', ((6, 1, 16, 16, 256), (32768,), (128,)), (128,), 1): ((),),
        ('pw_fwd', ((6, 1, 32, 32, 128), (8192,), (64,)), (64,), 1): ((),),
        ('pw_fwd', ((6, 1, 32, 32, 64), (8192,)), (128,), 0): ((),),
        ('pw_fwd', ((6, 1, 64, 64, 32), (2048,)), (64,), 0): ((),),
        ('pw_fwd', ((6, 1, 64, 64, 64), (2048,), (32,)), (32,), 1): ((),),
        ('mixloss_fwd', ((6, 1, 256, 256, 4), (6, 1, 256, 256), (6, 1, 256, 256)), (1,), 0): ((),),
        ('mixloss_bwd', ((6, 1, 256, 256, 4), (6, 1, 256, 256), (6, 1, 256, 256)), (1,), 0): (('g_dev',),),
    },
    "la_val": {
        ('down_fwd', ((1, 112, 112, 80, 16), (4096,), (32,)), (32,), 0): ((),),
        ('down_fwd', ((1, 14, 14, 10, 128), (262144,), (256,)), (256,), 0): ((),),
        ('down_fwd', ((1, 28, 28, 20, 64), (65536,), (128,)), (128,), 0): ((),),
        ('down_fwd', ((1, 56, 56, 40, 32), (16384,), (64,)), (64,), 0): ((),),
        ('down_fwd', ((4, 112, 112, 80, 16), (4096,), (32,)), (32,), 0): ((),),
        ('down_fwd', ((4, 14, 14, 10, 128), (262144,), (256,)), (256,), 0): ((),),
        ('down_fwd', ((4, 28, 28, 20, 64), (65536,), (128,)), (128,), 0): ((),),
        ('down_fwd', ((4, 56, 56, 40, 32), (16384,), (64,)), (64,), 0): ((),),
        ('up_fwd', ((1, 14, 14, 10, 128), (65536,), (64,)), (64,), 0): ((),),
        ('up_fwd', ((1, 28, 28, 20, 64), (16384,), (32,)), (32,), 0): ((),),
        ('up_fwd', ((1, 56, 56, 40, 32), (4096,), (16,)), (16,), 0): ((),),
        ('up_fwd', ((1, 7, 7, 5, 256), (262144,), (128,)), (128,), 0): ((),),
        ('up_fwd', ((4, 14, 14, 10, 128), (65536,), (64,)), (64,), 0): ((),),
        ('up_fwd', ((4, 28, 28, 20, 64), (16384,), (32,)), (32,), 0): ((),),
        ('up_fwd', ((4, 56, 56, 40, 32), (4096,), (16,)), (16,), 0): ((),),
        ('up_fwd', ((4, 7, 7, 5, 256), (262144,), (128,)), (128,), 0): ((),),
        ('norm_eval', ((1, 112, 112, 80, 16), (16,), (16,)), (1,), 0): ((), ('residual',)),
        ('norm_eval', ((1, 14, 14, 10, 128), (128,), (128,)), (1,), 0): ((), ('residual',)),
        ('norm_eval', ((1, 28, 28, 20, 64), (64,), (64,)), (1,), 0): ((), ('residual',)),
        ('norm_eval', ((1, 56, 56, 40, 32), (32,), (32,)), (1,), 0): ((), ('residual',)),
        ('norm_eval', ((1, 7, 7, 5, 256), (256,), (256,)), (1,), 0): ((),),
        ('norm_eval', ((4, 112, 112, 80, 16), (16,), (16,)), (1,), 0): ((), ('residual',)),
        ('norm_eval', ((4, 14, 14, 10, 128), (128,), (128,)), (1,), 0): ((), ('residual',)),
        ('norm_eval', ((4, 28, 28, 20, 64), (64,), (64,)), (1,), 0): ((), ('residual',)),
        ('norm_eval', ((4, 56, 56, 40, 32), (32,), (32,)), (1,), 0): ((), ('residual',)),
        ('norm_eval', ((4, 7, 7, 5, 256), (256,), (256,)), (1,), 0): ((),),
    },
    "pancreas_val": {
        ('down_fwd', ((1, 12, 12, 12, 128), (262144,), (256,)), (256,), 1): ((),),
        ('down_fwd', ((1, 24, 24, 24, 64), (65536,), (128,)), (128,), 1): ((),),
        ('down_fwd', ((1, 48, 48, 48, 32), (16384,), (64,)), (64,), 1): ((),),
        ('down_fwd', ((1, 96, 96, 96, 16), (4096,), (32,)), (32,), 1): ((),),
        ('down_fwd', ((4, 12, 12, 12, 128), (262144,), (256,)), (256,), 1): ((),),
        ('down_fwd', ((4, 24, 24, 24, 64), (65536,), (128,)), (128,), 1): ((),),
        ('down_fwd', ((4, 48, 48, 48, 32), (16384,), (64,)), (64,), 1): ((),),
        ('down_fwd', ((4, 96, 96, 96, 16), (4096,), (32,)), (32,), 1): ((),),
        ('norm_fwd', ((1, 12, 12, 12, 128),), (1, 1), 0): ((), ('residual',)),
        ('norm_fwd', ((1, 24, 24, 24, 64),), (1, 1), 0): ((), ('residual',)),
        ('norm_fwd', ((1, 48, 48, 48, 32),), (1, 1), 0): ((), ('partial',), ('residual',)),
        ('norm_fwd', ((1, 6, 6, 6, 256),), (1, 1), 0): ((),),
        ('norm_fwd', ((1, 96, 96, 96, 16),), (1, 1), 0): ((), ('partial',), ('residual',)),
        ('norm_fwd', ((4, 12, 12, 12, 128),), (4, 1), 0): ((), ('residual',)),
        ('norm_fwd', ((4, 24, 24, 24, 64),), (4, 1), 0): ((), ('partial',), ('residual',)),
        ('norm_fwd', ((4, 48, 48, 48, 32),), (4, 1), 0): ((), ('partial',), ('residual',)),
        ('norm_fwd', ((4, 6, 6, 6, 256),), (4, 1), 0): ((),),
        ('norm_fwd', ((4, 96, 96, 96, 16),), (4, 1), 0): ((), ('partial',), ('residual',)),
        ('up_fwd', ((1, 12, 12, 12, 128), (65536,), (64,)), (64,), 1): ((),),
        ('up_fwd', ((1, 24, 24, 24, 64), (16384,), (32,)), (32,), 1): ((),),
        ('up_fwd', ((1, 48, 48, 48, 32), (4096,), (16,)), (16,), 1): ((),),
        ('up_fwd', ((1, 6, 6, 6, 256), (262144,), (128,)), (128,), 1): ((),),
        ('up_fwd', ((4, 12, 12, 12, 128), (65536,), (64,)), (64,), 1): ((),),
        ('up_fwd', ((4, 24, 24, 24, 64), (16384,), (32,)), (32,), 1): ((),),
        ('up_fwd', ((4, 48, 48, 48, 32), (4096,), (16,)), (16,), 1): ((),),
        ('up_fwd', ((4, 6, 6, 6, 256), (262144,), (128,)), (128,), 1): ((),),
    },
    "acdc_val": {
        ('pw_fwd', ((1, 1, 128, 128, 32), (512,), (16,)), (16,), 0): ((),),
        ('pw_fwd', ((1, 1, 16, 16, 256), (32768,), (128,)), (128,), 0): ((),),
        ('pw_fwd', ((1, 1, 32, 32, 128), (8192,), (64,)), (64,), 0): ((),),
        ('pw_fwd', ((1, 1, 64, 64, 64), (2048,), (32,)), (32,), 0): ((),),
        ('pw_fwd', ((16, 1, 128, 128, 32), (512,), (16,)), (16,), 0): ((),),
        ('pw_fwd', ((16, 1, 16, 16, 256), (32768,), (128,)), (128,), 0): ((),),
        ('pw_fwd', ((16, 1, 32, 32, 128), (8192,), (64,)), (64,), 0): ((),),
        ('pw_fwd', ((16, 1, 64, 64, 64), (2048,), (32,)), (32,), 0): ((),),
        ('norm_eval', ((1, 1, 128, 128, 32), (32,), (32,)), (2,), 0): ((),),
        ('norm_eval', ((1, 1, 16, 16, 256), (256,), (256,)), (2,), 0): ((),),
        ('norm_eval', ((1, 1, 256, 256, 16), (16,), (16,)), (2,), 0): ((),),
        ('norm_eval', ((1, 1, 32, 32, 128), (128,), (128,)), (2,), 0): ((),),
        ('norm_eval', ((1, 1, 64, 64, 64), (64,), (64,)), (2,), 0): ((),),
        ('norm_eval', ((16, 1, 128, 128, 32), (32,), (32,)), (2,), 0): ((),),
        ('norm_eval', ((16, 1, 16, 16, 256), (256,), (256,)), (2,), 0): ((),),
        ('norm_eval', ((16, 1, 256, 256, 16), (16,), (16,)), (2,), 0): ((),),
        ('norm_eval', ((16, 1, 32, 32, 128), (128,), (128,)), (2,), 0): ((),),
        ('norm_eval', ((16, 1, 64, 64, 64), (64,), (64,)), (2,), 0): ((),),
    },
    "la8": {
        ('conv3_c1_norm_bwd_wgrad', ((4, 112, 112, 80, 1), (16, 1, 3, 3, 3), (16,)), (3, 2, 1), 0): (('accumulate', 'dw_accumulate'),),
        ('conv3_c1_norm_fwd', ((4, 112, 112, 80, 1), (16, 1, 3, 3, 3), (16,)), (3, 2, 1), 0): ((),),
        ('down_dgrad', ((4, 14, 14, 10, 128), (65536,)), (64,), 1): (('accumulate', 'out'),),
        ('down_dgrad', ((4, 28, 28, 20, 64), (16384,)), (32,), 1): (('accumulate', 'out'),),
        ('down_dgrad', ((4, 56, 56, 40, 32), (4096,)), (16,), 1): (('accumulate', 'out'),),
        ('down_dgrad', ((4, 7, 7, 5, 256), (262144,)), (128,), 1): (('accumulate', 'out'),),
        ('down_fwd', ((4, 112, 112, 80, 16), (4096,), (32,)), (32,), 1): ((),),
        ('down_fwd', ((4, 14, 14, 10, 128), (262144,), (256,)), (256,), 1): ((),),
        ('down_fwd', ((4, 28, 28, 20, 64), (65536,), (128,)), (128,), 1): ((),),
        ('down_fwd', ((4, 56, 56, 40, 32), (16384,), (64,)), (64,), 1): ((),),
        ('k2_fwd_stats', ((4, 56, 56, 40, 32), (4096,), (16,)), (1, 16, 2), 1): ((),),
        ('k2_wgrad', ((4, 112, 112, 80, 16), (4, 56, 56, 40, 32), (32, 16, 2, 2, 2)), (0,), 2): (('accumulate',),),
        ('k2_wgrad', ((4, 14, 14, 10, 128), (4, 28, 28, 20, 64), (128, 64, 2, 2, 2)), (1,), 2): (('accumulate',),),
        ('k2_wgrad', ((4, 14, 14, 10, 128), (4, 7, 7, 5, 256), (256, 128, 2, 2, 2)), (0,), 2): (('accumulate',),),
        ('k2_wgrad', ((4, 28, 28, 20, 64), (4, 14, 14, 10, 128), (128, 64, 2, 2, 2)), (0,), 2): (('accumulate',),),
        ('k2_wgrad', ((4, 28, 28, 20, 64), (4, 56, 56, 40, 32), (64, 32, 2, 2, 2)), (1,), 2): (('accumulate',),),
        ('k2_wgrad', ((4, 56, 56, 40, 32), (4, 112, 112, 80, 16), (32, 16, 2, 2, 2)), (1,), 2): (('accumulate',),),
        ('k2_wgrad', ((4, 56, 56, 40, 32), (4, 28, 28, 20, 64), (64, 32, 2, 2, 2)), (0,), 2): (('accumulate',),),
        ('k2_wgrad', ((4, 7, 7, 5, 256), (4, 14, 14, 10, 128), (256, 128, 2, 2, 2)), (1,), 2): (('accumulate',),),
        ('mix_box', ((2, 112, 112, 80, 1), (2, 112, 112, 80, 1)), (), 0): (('out',),),
        ('mixloss_pair_bwd', ((4, 112, 112, 80, 2), (2, 112, 112, 80), (2, 112, 112, 80)), (0,), 0): (('out', 'g_dev'),),
        ('mixloss_pair_fwd', ((4, 112, 112, 80, 2), (2, 112, 112, 80), (2, 112, 112, 80)), (0,), 0): ((),),
        ('norm_bwd', ((4, 112, 112, 80, 16), (4, 112, 112, 80, 16), (5, 2, 16)), (2, 1, 1), 0): ((),),
        ('norm_bwd', ((4, 14, 14, 10, 128), (4, 14, 14, 10, 128), (5, 2, 128)), (2, 1, 1), 0): ((),),
        ('norm_bwd', ((4, 28, 28, 20, 64), (4, 28, 28, 20, 64), (5, 2, 64)), (2, 1, 1), 0): ((), ('partial',)),
        ('norm_bwd', ((4, 56, 56, 40, 32), (4, 56, 56, 40, 32), (5, 2, 32)), (2, 1, 1), 0): ((), ('partial',)),
        ('norm_bwd', ((4, 7, 7, 5, 256), (4, 7, 7, 5, 256), (5, 2, 256)), (2, 1, 1), 0): (('chan_scale',),),
        ('norm_bwd_slabs', ((4, 14, 14, 10, 128), (2, 4, 14, 14, 10, 128), (5, 2, 128)), (2, 2, 1), 0): (('accumulate',),),
        ('norm_bwd_slabs', ((4, 7, 7, 5, 256), (8, 4, 7, 7, 5, 256), (5, 2, 256)), (8, 2, 1), 0): (('accumulate',),),
        ('norm_fwd', ((4, 112, 112, 80, 16), (16,), (16,)), (2, 1), 0): (('chan_scale', 'partial', 'stats_only'), ('partial', 'residual')),
        ('norm_fwd', ((4, 14, 14, 10, 128), (128,), (128,)), (2, 1), 0): ((), ('residual',)),
        ('norm_fwd', ((4, 28, 28, 20, 64), (64,), (64,)), (2, 1), 0): ((), ('partial',), ('residual',)),
        ('norm_fwd', ((4, 56, 56, 40, 32), (32,), (32,)), (2, 1), 0): ((), ('partial',), ('residual',)),
        ('norm_fwd', ((4, 7, 7, 5, 256), (256,), (256,)), (2, 1), 0): ((),),
        ('norm_fwd_slabs', ((2, 4, 14, 14, 10, 128), (128,), (128,)), (2, 2, 1), 0): ((),),
        ('norm_fwd_slabs', ((8, 4, 7, 7, 5, 256), (256,), (256,)), (8, 2, 1), 0): ((), ('chan_scale',)),
        ('pw16_bwd_norm_bwd', ((4, 112, 112, 80, 16), (5, 2, 16), (4, 16)), (2, 1), 0): (('chan_scale', 'accumulate', 'norm_accumulate'),),
        ('pw16_fwd_norm', ((4, 112, 112, 80, 16), (5, 2, 16), (4, 16)), (2, 1, 2), 0): (('chan_scale',),),
        ('up_dgrad', ((4, 112, 112, 80, 16), (4096,)), (32,), 1): ((),),
        ('up_dgrad', ((4, 14, 14, 10, 128), (262144,)), (256,), 1): ((),),
        ('up_dgrad', ((4, 28, 28, 20, 64), (65536,)), (128,), 1): ((),),
        ('up_dgrad', ((4, 56, 56, 40, 32), (16384,)), (64,), 1): ((),),
        ('up_fwd', ((4, 14, 14, 10, 128), (65536,), (64,)), (64,), 1): ((),),
        ('up_fwd', ((4, 28, 28, 20, 64), (16384,), (32,)), (32,), 1): ((),),
        ('up_fwd', ((4, 7, 7, 5, 256), (262144,), (128,)), (128,), 1): ((),),
    },
    "lares": {
        ('conv3_c1_wgrad', ((2, 112, 112, 80, 1), (2, 112, 112, 80, 16), (16, 1, 3, 3, 3)), (3,), 1): (('accumulate',),),
        ('down_dgrad', ((2, 7, 7, 5, 256), (262144,)), (128,), 1): (('accumulate', 'out'),),
        ('down_dgrad', ((2, 14, 14, 10, 128), (65536,)), (64,), 1): (('accumulate', 'out'),),
        ('down_dgrad', ((2, 28, 28, 20, 64), (16384,)), (32,), 1): (('accumulate', 'out'),),
        ('down_dgrad', ((2, 56, 56, 40, 32), (4096,)), (16,), 1): (('accumulate', 'out'),),
        ('down_fwd', ((2, 14, 14, 10, 128), (262144,), (256,)), (256,), 1): ((),),
        ('down_fwd', ((2, 28, 28, 20, 64), (65536,), (128,)), (128,), 1): ((),),
        ('down_fwd', ((2, 56, 56, 40, 32), (16384,), (64,)), (64,), 1): ((),),
        ('down_fwd', ((2, 112, 112, 80, 16), (4096,), (32,)), (32,), 1): ((),),
        ('k2_fwd_stats', ((2, 56, 56, 40, 32), (4096,), (16,)), (1, 16, 2), 1): ((),),
        ('k2_wgrad', ((2, 7, 7, 5, 256), (2, 14, 14, 10, 128), (256, 128, 2, 2, 2)), (1,), 2): (('accumulate',),),
        ('k2_wgrad', ((2, 14, 14, 10, 128), (2, 7, 7, 5, 256), (256, 128, 2, 2, 2)), (0,), 2): (('accumulate',),),
        ('k2_wgrad', ((2, 14, 14, 10, 128), (2, 28, 28, 20, 64), (128, 64, 2, 2, 2)), (1,), 2): (('accumulate',),),
        ('k2_wgrad', ((2, 28, 28, 20, 64), (2, 14, 14, 10, 128), (128, 64, 2, 2, 2)), (0,), 2): (('accumulate',),),
        ('k2_wgrad', ((2, 28, 28, 20, 64), (2, 56, 56, 40, 32), (64, 32, 2, 2, 2)), (1,), 2): (('accumulate',),),
        ('k2_wgrad', ((2, 56, 56, 40, 32), (2, 28, 28, 20, 64), (64, 32, 2, 2, 2)), (0,), 2): (('accumulate',),),
        ('k2_wgrad', ((2, 56, 56, 40, 32), (2, 112, 112, 80, 16), (32, 16, 2, 2, 2)), (1,), 2): (('accumulate',),),
        ('k2_wgrad', ((2, 112, 112, 80, 16), (2, 56, 56, 40, 32), (32, 16, 2, 2, 2)), (0,), 2): (('accumulate',),),
        ('mix_box', ((1, 112, 112, 80, 1), (1, 112, 112, 80, 1)), (), 0): (('out',),),
        ('mixloss_pair_bwd', ((2, 112, 112, 80, 2), (1, 112, 112, 80), (1, 112, 112, 80)), (0,), 0): (('out', 'g_dev'),),
        ('mixloss_pair_fwd', ((2, 112, 112, 80, 2), (1, 112, 112, 80), (1, 112, 112, 80)), (0,), 0): ((),),
        ('norm_bwd', ((2, 7, 7, 5, 256), (2, 7, 7, 5, 256), (5, 2, 256)), (2, 1, 1), 0): ((),),
        ('norm_bwd', ((2, 14, 14, 10, 128), (2, 14, 14, 10, 128), (5, 2, 128)), (2, 1, 1), 0): ((),),
        ('norm_bwd', ((2, 28, 28, 20, 64), (2, 28, 28, 20, 64), (5, 2, 64)), (2, 1, 1), 0): ((), ('partial',)),
        ('norm_bwd', ((2, 56, 56, 40, 32), (2, 56, 56, 40, 32), (5, 2, 32)), (2, 1, 1), 0): ((), ('partial',)),
        ('norm_bwd', ((2, 112, 112, 80, 16), (2, 112, 112, 80, 16), (5, 2, 16)), (2, 1, 1), 0): ((),),
        ('norm_bwd_res', ((2, 7, 7, 5, 256), (2, 7, 7, 5, 256), (2, 7, 7, 5, 256)), (2, 1, 1), 0): (('chan_scale',),),
        ('norm_bwd_res', ((2, 14, 14, 10, 128), (2, 14, 14, 10, 128), (2, 14, 14, 10, 128)), (2, 1, 1), 0): ((),),
        ('norm_bwd_res', ((2, 28, 28, 20, 64), (2, 28, 28, 20, 64), (2, 28, 28, 20, 64)), (2, 1, 1), 0): ((),),
        ('norm_bwd_res', ((2, 56, 56, 40, 32), (2, 56, 56, 40, 32), (2, 56, 56, 40, 32)), (2, 1, 1), 0): ((),),
        ('norm_bwd_res', ((2, 112, 112, 80, 16), (2, 112, 112, 80, 16), (2, 112, 112, 80, 1)), (2, 1, 1), 0): (('bcast', 'no_dres'),),
        ('norm_bwd_res', ((2, 112, 112, 80, 16), (2, 112, 112, 80, 16), (2, 112, 112, 80, 16)), (2, 1, 1), 0): (('chan_scale',),),
        ('norm_bwd_slabs', ((2, 7, 7, 5, 256), (8, 2, 7, 7, 5, 256), (5, 2, 256)), (8, 2, 1), 0): (('accumulate',),),
        ('norm_bwd_slabs', ((2, 14, 14, 10, 128), (4, 2, 14, 14, 10, 128), (5, 2, 128)), (4, 2, 1), 0): (('accumulate',),),
        ('norm_fwd', ((2, 7, 7, 5, 256), (256,), (256,)), (2, 1), 0): ((),),
        ('norm_fwd', ((2, 14, 14, 10, 128), (128,), (128,)), (2, 1), 0): ((), ('residual',)),
        ('norm_fwd', ((2, 28, 28, 20, 64), (64,), (64,)), (2, 1), 0): ((), ('partial',), ('residual',)),
        ('norm_fwd', ((2, 56, 56, 40, 32), (32,), (32,)), (2, 1), 0): ((), ('partial',), ('residual',)),
        ('norm_fwd', ((2, 112, 112, 80, 16), (16,), (16,)), (2, 1), 0): (('partial', 'residual'),),
        ('norm_fwd_res', ((2, 7, 7, 5, 256), (256,), (256,)), (2, 1), 0): (('chan_scale',),),
        ('norm_fwd_res', ((2, 14, 14, 10, 128), (128,), (128,)), (2, 1), 0): ((),),
        ('norm_fwd_res', ((2, 28, 28, 20, 64), (64,), (64,)), (2, 1), 0): (('partial',),),
        ('norm_fwd_res', ((2, 56, 56, 40, 32), (32,), (32,)), (2, 1), 0): (('partial',),),
        ('norm_fwd_res', ((2, 112, 112, 80, 16), (16,), (16,)), (2, 1), 0): (('chan_scale', 'partial'), ('partial', 'bcast')),
        ('norm_fwd_slabs', ((4, 2, 14, 14, 10, 128), (128,), (128,)), (4, 2, 1), 0): ((),),
        ('norm_fwd_slabs', ((8, 2, 7, 7, 5, 256), (256,), (256,)), (8, 2, 1), 0): ((),),
        ('pw16_bwd', ((2, 112, 112, 80, 16), (2, 112, 112, 80, 2), (2, 16, 1, 1, 1)), (), 1): (('accumulate',),),
        ('up_dgrad', ((2, 14, 14, 10, 128), (262144,)), (256,), 1): ((),),
        ('up_dgrad', ((2, 28, 28, 20, 64), (65536,)), (128,), 1): ((),),
        ('up_dgrad', ((2, 56, 56, 40, 32), (16384,)), (64,), 1): ((),),
        ('up_dgrad', ((2, 112, 112, 80, 16), (4096,)), (32,), 1): ((),),
        ('up_fwd', ((2, 7, 7, 5, 256), (262144,), (128,)), (128,), 1): ((),),
        ('up_fwd', ((2, 14, 14, 10, 128), (65536,), (64,)), (64,), 1): ((),),
        ('up_fwd', ((2, 28, 28, 20, 64), (16384,), (32,)), (32,), 1): ((),),
    },
    "lares_pre": {
        ('conv3_c1_wgrad', ((1, 112, 112, 80, 1), (1, 112, 112, 80, 16), (16, 1, 3, 3, 3)), (3,), 1): (('accumulate',),),
        ('down_dgrad', ((1, 7, 7, 5, 256), (262144,)), (128,), 1): (('accumulate', 'out'),),
        ('down_dgrad', ((1, 14, 14, 10, 128), (65536,)), (64,), 1): (('accumulate', 'out'),),
        ('down_dgrad', ((1, 28, 28, 20, 64), (16384,)), (32,), 1): (('accumulate', 'out'),),
        ('down_dgrad', ((1, 56, 56, 40, 32), (4096,)), (16,), 1): (('accumulate', 'out'),),
        ('down_fwd', ((1, 14, 14, 10, 128), (262144,), (256,)), (256,), 1): ((),),
        ('down_fwd', ((1, 28, 28, 20, 64), (65536,), (128,)), (128,), 1): ((),),
        ('down_fwd', ((1, 56, 56, 40, 32), (16384,), (64,)), (64,), 1): ((),),
        ('down_fwd', ((1, 112, 112, 80, 16), (4096,), (32,)), (32,), 1): ((),),
        ('k2_wgrad', ((1, 7, 7, 5, 256), (1, 14, 14, 10, 128), (256, 128, 2, 2, 2)), (1,), 2): (('accumulate',),),
        ('k2_wgrad', ((1, 14, 14, 10, 128), (1, 7, 7, 5, 256), (256, 128, 2, 2, 2)), (0,), 2): (('accumulate',),),
        ('k2_wgrad', ((1, 14, 14, 10, 128), (1, 28, 28, 20, 64), (128, 64, 2, 2, 2)), (1,), 2): (('accumulate',),),
        ('k2_wgrad', ((1, 28, 28, 20, 64), (1, 14, 14, 10, 128), (128, 64, 2, 2, 2)), (0,), 2): (('accumulate',),),
        ('k2_wgrad', ((1, 28, 28, 20, 64), (1, 56, 56, 40, 32), (64, 32, 2, 2, 2)), (1,), 2): (('accumulate',),),
        ('k2_wgrad', ((1, 56, 56, 40, 32), (1, 28, 28, 20, 64), (64, 32, 2, 2, 2)), (0,), 2): (('accumulate',),),
        ('k2_wgrad', ((1, 56, 56, 40, 32), (1, 112, 112, 80, 16), (32, 16, 2, 2, 2)), (1,), 2): (('accumulate',),),
        ('k2_wgrad', ((1, 112, 112, 80, 16), (1, 56, 56, 40, 32), (32, 16, 2, 2, 2)), (0,), 2): (('accumulate',),),
        ('mix_box', ((1, 112, 112, 80, 1), (1, 112, 112, 80, 1)), (), 0): ((),),
        ('mixloss_bwd', ((1, 112, 112, 80, 2), (1, 112, 112, 80), (1, 112, 112, 80)), (0,), 0): (('g_dev',),),
        ('mixloss_fwd', ((1, 112, 112, 80, 2), (1, 112, 112, 80), (1, 112, 112, 80)), (0,), 0): ((),),
        ('norm_bwd', ((1, 7, 7, 5, 256), (1, 7, 7, 5, 256), (5, 1, 256)), (1, 1, 1), 0): ((),),
        ('norm_bwd', ((1, 14, 14, 10, 128), (1, 14, 14, 10, 128), (5, 1, 128)), (1, 1, 1), 0): ((),),
        ('norm_bwd', ((1, 28, 28, 20, 64), (1, 28, 28, 20, 64), (5, 1, 64)), (1, 1, 1), 0): ((),),
        ('norm_bwd', ((1, 56, 56, 40, 32), (1, 56, 56, 40, 32), (5, 1, 32)), (1, 1, 1), 0): ((), ('partial',)),
        ('norm_bwd', ((1, 112, 112, 80, 16), (1, 112, 112, 80, 16), (5, 1, 16)), (1, 1, 1), 0): ((),),
        ('norm_bwd_res', ((1, 7, 7, 5, 256), (1, 7, 7, 5, 256), (1, 7, 7, 5, 256)), (1, 1, 1), 0): (('chan_scale',),),
        ('norm_bwd_res', ((1, 14, 14, 10, 128), (1, 14, 14, 10, 128), (1, 14, 14, 10, 128)), (1, 1, 1), 0): ((),),
        ('norm_bwd_res', ((1, 28, 28, 20, 64), (1, 28, 28, 20, 64), (1, 28, 28, 20, 64)), (1, 1, 1), 0): ((),),
        ('norm_bwd_res', ((1, 56, 56, 40, 32), (1, 56, 56, 40, 32), (1, 56, 56, 40, 32)), (1, 1, 1), 0): ((),),
        ('norm_bwd_res', ((1, 112, 112, 80, 16), (1, 112, 112, 80, 16), (1, 112, 112, 80, 1)), (1, 1, 1), 0): (('bcast', 'no_dres'),),
        ('norm_bwd_res', ((1, 112, 112, 80, 16), (1, 112, 112, 80, 16), (1, 112, 112, 80, 16)), (1, 1, 1), 0): (('chan_scale',),),
        ('norm_bwd_slabs', ((1, 14, 14, 10, 128), (4, 1, 14, 14, 10, 128), (5, 1, 128)), (4, 1, 1), 0): (('accumulate',),),
        ('norm_fwd', ((1, 7, 7, 5, 256), (256,), (256,)), (1, 1), 0): ((),),
        ('norm_fwd', ((1, 14, 14, 10, 128), (128,), (128,)), (1, 1), 0): ((), ('residual',)),
        ('norm_fwd', ((1, 28, 28, 20, 64), (64,), (64,)), (1, 1), 0): ((), ('partial',), ('residual',)),
        ('norm_fwd', ((1, 56, 56, 40, 32), (32,), (32,)), (1, 1), 0): ((), ('partial',), ('residual',)),
        ('norm_fwd', ((1, 112, 112, 80, 16), (16,), (16,)), (1, 1), 0): (('residual',),),
        ('norm_fwd_res', ((1, 7, 7, 5, 256), (256,), (256,)), (1, 1), 0): (('chan_scale',),),
        ('norm_fwd_res', ((1, 14, 14, 10, 128), (128,), (128,)), (1, 1), 0): ((),),
        ('norm_fwd_res', ((1, 28, 28, 20, 64), (64,), (64,)), (1, 1), 0): (('partial',),),
        ('norm_fwd_res', ((1, 56, 56, 40, 32), (32,), (32,)), (1, 1), 0): (('partial',),),
        ('norm_fwd_res', ((1, 112, 112, 80, 16), (16,), (16,)), (1, 1), 0): (('chan_scale', 'partial'), ('partial', 'bcast')),
        ('norm_fwd_slabs', ((4, 1, 14, 14, 10, 128), (128,), (128,)), (4, 1, 1), 0): ((),),
        ('pw16_bwd', ((1, 112, 112, 80, 16), (1, 112, 112, 80, 2), (2, 16, 1, 1, 1)), (), 1): (('accumulate',),),
        ('up_dgrad', ((1, 14, 14, 10, 128), (262144,)), (256,), 1): ((),),
        ('up_dgrad', ((1, 28, 28, 20, 64), (65536,)), (128,), 1): ((),),
        ('up_dgrad', ((1, 56, 56, 40, 32), (16384,)), (64,), 1): ((),),
        ('up_dgrad', ((1, 112, 112, 80, 16), (4096,)), (32,), 1): ((),),
        ('up_fwd', ((1, 7, 7, 5, 256), (262144,), (128,)), (128,), 1): ((),),
        ('up_fwd', ((1, 14, 14, 10, 128), (65536,), (64,)), (64,), 1): ((),),
        ('up_fwd', ((1, 28, 28, 20, 64), (16384,), (32,)), (32,), 1): ((),),
        ('up_fwd', ((1, 56, 56, 40, 32), (4096,), (16,)), (16,), 1): ((),),
    },
    "lares_val": {
        ('down_fwd', ((1, 14, 14, 10, 128), (262144,), (256,)), (256,), 0): ((),),
        ('down_fwd', ((1, 28, 28, 20, 64), (65536,), (128,)), (128,), 0): ((),),
        ('down_fwd', ((1, 56, 56, 40, 32), (16384,), (64,)), (64,), 0): ((),),
        ('down_fwd', ((1, 112, 112, 80, 16), (4096,), (32,)), (32,), 0): ((),),
        ('down_fwd', ((4, 14, 14, 10, 128), (262144,), (256,)), (256,), 0): ((),),
        ('down_fwd', ((4, 28, 28, 20, 64), (65536,), (128,)), (128,), 0): ((),),
        ('down_fwd', ((4, 56, 56, 40, 32), (16384,), (64,)), (64,), 0): ((),),
        ('down_fwd', ((4, 112, 112, 80, 16), (4096,), (32,)), (32,), 0): ((),),
        ('norm_eval', ((1, 7, 7, 5, 256), (256,), (256,)), (1,), 0): ((),),
        ('norm_eval', ((1, 14, 14, 10, 128), (128,), (128,)), (1,), 0): ((), ('residual',)),
        ('norm_eval', ((1, 28, 28, 20, 64), (64,), (64,)), (1,), 0): ((), ('residual',)),
        ('norm_eval', ((1, 56, 56, 40, 32), (32,), (32,)), (1,), 0): ((), ('residual',)),
        ('norm_eval', ((1, 112, 112, 80, 16), (16,), (16,)), (1,), 0): (('residual',),),
        ('norm_eval', ((4, 7, 7, 5, 256), (256,), (256,)), (1,), 0): ((),),
        ('norm_eval', ((4, 14, 14, 10, 128), (128,), (128,)), (1,), 0): ((), ('residual',)),
        ('norm_eval', ((4, 28, 28, 20, 64), (64,), (64,)), (1,), 0): ((), ('residual',)),
        ('norm_eval', ((4, 56, 56, 40, 32), (32,), (32,)), (1,), 0): ((), ('residual',)),
        ('norm_eval', ((4, 112, 112, 80, 16), (16,), (16,)), (1,), 0): (('residual',),),
        ('norm_eval_res', ((1, 7, 7, 5, 256), (256,), (256,)), (1,), 0): ((),),
        ('norm_eval_res', ((1, 14, 14, 10, 128), (128,), (128,)), (1,), 0): ((),),
        ('norm_eval_res', ((1, 28, 28, 20, 64), (64,), (64,)), (1,), 0): ((),),
        ('norm_eval_res', ((1, 56, 56, 40, 32), (32,), (32,)), (1,), 0): ((),),
        ('norm_eval_res', ((1, 112, 112, 80, 16), (16,), (16,)), (1,), 0): ((), ('bcast',)),
        ('norm_eval_res', ((4, 7, 7, 5, 256), (256,), (256,)), (1,), 0): ((),),
        ('norm_eval_res', ((4, 14, 14, 10, 128), (128,), (128,)), (1,), 0): ((),),
        ('norm_eval_res', ((4, 28, 28, 20, 64), (64,), (64,)), (1,), 0): ((),),
        ('norm_eval_res', ((4, 56, 56, 40, 32), (32,), (32,)), (1,), 0): ((),),
        ('norm_eval_res', ((4, 112, 112, 80, 16), (16,), (16,)), (1,), 0): ((), ('bcast',)),
        ('up_fwd', ((1, 7, 7, 5, 256), (262144,), (128,)), (128,), 0): ((),),
        ('up_fwd', ((1, 14, 14, 10, 128), (65536,), (64,)), (64,), 0): ((),),
        ('up_fwd', ((1, 28, 28, 20, 64), (16384,), (32,)), (32,), 0): ((),),
        ('up_fwd', ((1, 56, 56, 40, 32), (4096,), (16,)), (16,), 0): ((),),
        ('up_fwd', ((4, 7, 7, 5, 256), (262144,), (128,)), (128,), 0): ((),),
        ('up_fwd', ((4, 14, 14, 10, 128), (65536,), (64,)), (64,), 0): ((),),
        ('up_fwd', ((4, 28, 28, 20, 64), (16384,), (32,)), (32,), 0): ((),),
        ('up_fwd', ((4, 56, 56, 40, 32), (4096,), (16,)), (16,), 0): ((),),
    },
    "lagn": {
        ('down_fwd', ((2, 14, 14, 10, 128), (262144,), (256,)), (256,), 1): ((),),
        ('down_fwd', ((2, 28, 28, 20, 64), (65536,), (128,)), (128,), 1): ((),),
        ('down_fwd', ((2, 56, 56, 40, 32), (16384,), (64,)), (64,), 1): ((),),
        ('down_fwd', ((2, 112, 112, 80, 16), (4096,), (32,)), (32,), 1): ((),),
        ('down_dgrad', ((2, 7, 7, 5, 256), (262144,)), (128,), 1): (('accumulate', 'out'),),
        ('down_dgrad', ((2, 14, 14, 10, 128), (65536,)), (64,), 1): (('accumulate', 'out'),),
        ('down_dgrad', ((2, 28, 28, 20, 64), (16384,)), (32,), 1): (('accumulate', 'out'),),
        ('down_dgrad', ((2, 56, 56, 40, 32), (4096,)), (16,), 1): (('accumulate', 'out'),),
        ('up_fwd', ((2, 7, 7, 5, 256), (262144,), (128,)), (128,), 1): ((),),
        ('up_fwd', ((2, 14, 14, 10, 128), (65536,), (64,)), (64,), 1): ((),),
        ('up_fwd', ((2, 28, 28, 20, 64), (16384,), (32,)), (32,), 1): ((),),
        ('up_dgrad', ((2, 14, 14, 10, 128), (262144,)), (256,), 1): ((),),
        ('up_dgrad', ((2, 28, 28, 20, 64), (65536,)), (128,), 1): ((),),
        ('up_dgrad', ((2, 56, 56, 40, 32), (16384,)), (64,), 1): ((),),
        ('up_dgrad', ((2, 112, 112, 80, 16), (4096,)), (32,), 1): ((),),
        ('k2_fwd_stats', ((2, 56, 56, 40, 32), (4096,), (16,)), (1, 16, 2), 1): ((),),
        ('k2_wgrad', ((2, 7, 7, 5, 256), (2, 14, 14, 10, 128), (256, 128, 2, 2, 2)), (1,), 2): (('accumulate',),),
        ('k2_wgrad', ((2, 14, 14, 10, 128), (2, 7, 7, 5, 256), (256, 128, 2, 2, 2)), (0,), 2): (('accumulate',),),
        ('k2_wgrad', ((2, 14, 14, 10, 128), (2, 28, 28, 20, 64), (128, 64, 2, 2, 2)), (1,), 2): (('accumulate',),),
        ('k2_wgrad', ((2, 28, 28, 20, 64), (2, 14, 14, 10, 128), (128, 64, 2, 2, 2)), (0,), 2): (('accumulate',),),
        ('k2_wgrad', ((2, 28, 28, 20, 64), (2, 56, 56, 40, 32), (64, 32, 2, 2, 2)), (1,), 2): (('accumulate',),),
        ('k2_wgrad', ((2, 56, 56, 40, 32), (2, 28, 28, 20, 64), (64, 32, 2, 2, 2)), (0,), 2): (('accumulate',),),
        ('k2_wgrad', ((2, 56, 56, 40, 32), (2, 112, 112, 80, 16), (32, 16, 2, 2, 2)), (1,), 2): (('accumulate',),),
        ('k2_wgrad', ((2, 112, 112, 80, 16), (2, 56, 56, 40, 32), (32, 16, 2, 2, 2)), (0,), 2): (('accumulate',),),
        ('mix_box', ((1, 112, 112, 80, 1), (1, 112, 112, 80, 1)), (), 0): (('out',),),
        ('pw16_fwd_norm', ((2, 112, 112, 80, 16), (5, 2, 16), (2, 16)), (2, 1, 2), 0): (('chan_scale',),),
        ('mixloss_pair_fwd', ((2, 112, 112, 80, 2), (1, 112, 112, 80), (1, 112, 112, 80)), (0,), 0): ((),),
        ('mixloss_pair_bwd', ((2, 112, 112, 80, 2), (1, 112, 112, 80), (1, 112, 112, 80)), (0,), 0): (('out', 'g_dev'),),
        ('conv3_c1_wgrad', ((2, 112, 112, 80, 1), (2, 112, 112, 80, 16), (16, 1, 3, 3, 3)), (3,), 1): (('accumulate',),),
        ('gnorm_fwd', ((2, 7, 7, 5, 256), (256,), (256,)), (1,), 0): ((), ('chan_scale',)),
        ('gnorm_fwd', ((2, 14, 14, 10, 128), (128,), (128,)), (1,), 0): ((), ('residual',)),
        ('gnorm_fwd', ((2, 28, 28, 20, 64), (64,), (64,)), (1,), 0): ((), ('partial',), ('residual',)),
        ('gnorm_fwd', ((2, 56, 56, 40, 32), (32,), (32,)), (1,), 0): ((), ('partial',), ('residual',)),
        ('gnorm_fwd', ((2, 112, 112, 80, 16), (16,), (16,)), (1,), 0): (('chan_scale', 'partial', 'stats_only'), ('partial',), ('partial', 'residual')),
        ('gnorm_bwd', ((2, 7, 7, 5, 256), (2, 7, 7, 5, 256), (5, 2, 256)), (1, 1), 0): (('chan_scale', 'accumulate', 'dbias'), ('accumulate', 'dbias')),
        ('gnorm_bwd', ((2, 14, 14, 10, 128), (2, 14, 14, 10, 128), (5, 2, 128)), (1, 1), 0): (('accumulate', 'dbias'),),
        ('gnorm_bwd', ((2, 28, 28, 20, 64), (2, 28, 28, 20, 64), (5, 2, 64)), (1, 1), 0): (('partial', 'accumulate', 'dbias'), ('accumulate', 'dbias')),
        ('gnorm_bwd', ((2, 56, 56, 40, 32), (2, 56, 56, 40, 32), (5, 2, 32)), (1, 1), 0): (('partial', 'accumulate', 'dbias'), ('accumulate', 'dbias')),
        ('gnorm_bwd', ((2, 112, 112, 80, 16), (2, 112, 112, 80, 16), (5, 2, 16)), (1, 1), 0): (('chan_scale', 'accumulate'), ('accumulate',)),
        ('pw16_bwd_norm', ((2, 112, 112, 80, 16), (5, 2, 16), (2, 16)), (2, 1), 0): (('chan_scale', 'accumulate'),),
    },
    "lagn_pre": {
        ('down_fwd', ((1, 14, 14, 10, 128), (262144,), (256,)), (256,), 1): ((),),
        ('down_fwd', ((1, 28, 28, 20, 64), (65536,), (128,)), (128,), 1): ((),),
        ('down_fwd', ((1, 56, 56, 40, 32), (16384,), (64,)), (64,), 1): ((),),
        ('down_fwd', ((1, 112, 112, 80, 16), (4096,), (32,)), (32,), 1): ((),),
        ('down_dgrad', ((1, 7, 7, 5, 256), (262144,)), (128,), 1): (('accumulate', 'out'),),
        ('down_dgrad', ((1, 14, 14, 10, 128), (65536,)), (64,), 1): (('accumulate', 'out'),),
        ('down_dgrad', ((1, 28, 28, 20, 64), (16384,)), (32,), 1): (('accumulate', 'out'),),
        ('down_dgrad', ((1, 56, 56, 40, 32), (4096,)), (16,), 1): (('accumulate', 'out'),),
        ('up_fwd', ((1, 7, 7, 5, 256), (262144,), (128,)), (128,), 1): ((),),
        ('up_fwd', ((1, 14, 14, 10, 128), (65536,), (64,)), (64,), 1): ((),),
        ('up_fwd', ((1, 28, 28, 20, 64), (16384,), (32,)), (32,), 1): ((),),
        ('up_fwd', ((1, 56, 56, 40, 32), (4096,), (16,)), (16,), 1): ((),),
        ('up_dgrad', ((1, 14, 14, 10, 128), (262144,)), (256,), 1): ((),),
        ('up_dgrad', ((1, 28, 28, 20, 64), (65536,)), (128,), 1): ((),),
        ('up_dgrad', ((1, 56, 56, 40, 32), (16384,)), (64,), 1): ((),),
        ('up_dgrad', ((1, 112, 112, 80, 16), (4096,)), (32,), 1): ((),),
        ('k2_wgrad', ((1, 7, 7, 5, 256), (1, 14, 14, 10, 128), (256, 128, 2, 2, 2)), (1,), 2): (('accumulate',),),
        ('k2_wgrad', ((1, 14, 14, 10, 128), (1, 7, 7, 5, 256), (256, 128, 2, 2, 2)), (0,), 2): (('accumulate',),),
        ('k2_wgrad', ((1, 14, 14, 10, 128), (1, 28, 28, 20, 64), (128, 64, 2, 2, 2)), (1,), 2): (('accumulate',),),
        ('k2_wgrad', ((1, 28, 28, 20, 64), (1, 14, 14, 10, 128), (128, 64, 2, 2, 2)), (0,), 2): (('accumulate',),),
        ('k2_wgrad', ((1, 28, 28, 20, 64), (1, 56, 56, 40, 32), (64, 32, 2, 2, 2)), (1,), 2): (('accumulate',),),
        ('k2_wgrad', ((1, 56, 56, 40, 32), (1, 28, 28, 20, 64), (64, 32, 2, 2, 2)), (0,), 2): (('accumulate',),),
        ('k2_wgrad', ((1, 56, 56, 40, 32), (1, 112, 112, 80, 16), (32, 16, 2, 2, 2)), (1,), 2): (('accumulate',),),
        ('k2_wgrad', ((1, 112, 112, 80, 16), (1, 56, 56, 40, 32), (32, 16, 2, 2, 2)), (0,), 2): (('accumulate',),),
        ('mix_box', ((1, 112, 112, 80, 1), (1, 112, 112, 80, 1)), (), 0): ((),),
        ('pw16_fwd_norm', ((1, 112, 112, 80, 16), (5, 1, 16), (1, 16)), (1, 1, 2), 0): (('chan_scale',),),
        ('mixloss_fwd', ((1, 112, 112, 80, 2), (1, 112, 112, 80), (1, 112, 112, 80)), (0,), 0): ((),),
        ('mixloss_bwd', ((1, 112, 112, 80, 2), (1, 112, 112, 80), (1, 112, 112, 80)), (0,), 0): (('g_dev',),),
        ('conv3_c1_wgrad', ((1, 112, 112, 80, 1), (1, 112, 112, 80, 16), (16, 1, 3, 3, 3)), (3,), 1): (('accumulate',),),
        ('gnorm_fwd', ((1, 7, 7, 5, 256), (256,), (256,)), (1,), 0): ((), ('chan_scale',)),
        ('gnorm_fwd', ((1, 14, 14, 10, 128), (128,), (128,)), (1,), 0): ((), ('residual',)),
        ('gnorm_fwd', ((1, 28, 28, 20, 64), (64,), (64,)), (1,), 0): ((), ('partial',), ('residual',)),
        ('gnorm_fwd', ((1, 56, 56, 40, 32), (32,), (32,)), (1,), 0): ((), ('partial',), ('residual',)),
        ('gnorm_fwd', ((1, 112, 112, 80, 16), (16,), (16,)), (1,), 0): (('chan_scale', 'partial', 'stats_only'), ('partial',), ('residual',)),
        ('gnorm_bwd', ((1, 7, 7, 5, 256), (1, 7, 7, 5, 256), (5, 1, 256)), (1, 1), 0): (('chan_scale', 'accumulate', 'dbias'), ('accumulate', 'dbias')),
        ('gnorm_bwd', ((1, 14, 14, 10, 128), (1, 14, 14, 10, 128), (5, 1, 128)), (1, 1), 0): (('accumulate', 'dbias'),),
        ('gnorm_bwd', ((1, 28, 28, 20, 64), (1, 28, 28, 20, 64), (5, 1, 64)), (1, 1), 0): (('accumulate', 'dbias'),),
        ('gnorm_bwd', ((1, 56, 56, 40, 32), (1, 56, 56, 40, 32), (5, 1, 32)), (1, 1), 0): (('partial', 'accumulate', 'dbias'), ('accumulate', 'dbias')),
        ('gnorm_bwd', ((1, 112, 112, 80, 16), (1, 112, 112, 80, 16), (5, 1, 16)), (1, 1), 0): (('chan_scale', 'accumulate'), ('accumulate',)),
        ('pw16_bwd_norm', ((1, 112, 112, 80, 16), (5, 1, 16), (1, 16)), (1, 1), 0): (('chan_scale', 'accumulate'),),
    },
    "lagn_val": {
        ('down_fwd', ((1, 14, 14, 10, 128), (262144,), (256,)), (256,), 1): ((),),
        ('down_fwd', ((1, 28, 28, 20, 64), (65536,), (128,)), (128,), 1): ((),),
        ('down_fwd', ((1, 56, 56, 40, 32), (16384,), (64,)), (64,), 1): ((),),
        ('down_fwd', ((1, 112, 112, 80, 16), (4096,), (32,)), (32,), 1): ((),),
        ('down_fwd', ((4, 14, 14, 10, 128), (262144,), (256,)), (256,), 1): ((),),
        ('down_fwd', ((4, 28, 28, 20, 64), (65536,), (128,)), (128,), 1): ((),),
        ('down_fwd', ((4, 56, 56, 40, 32), (16384,), (64,)), (64,), 1): ((),),
        ('down_fwd', ((4, 112, 112, 80, 16), (4096,), (32,)), (32,), 1): ((),),
        ('up_fwd', ((1, 7, 7, 5, 256), (262144,), (128,)), (128,), 1): ((),),
        ('up_fwd', ((1, 14, 14, 10, 128), (65536,), (64,)), (64,), 1): ((),),
        ('up_fwd', ((1, 28, 28, 20, 64), (16384,), (32,)), (32,), 1): ((),),
        ('up_fwd', ((1, 56, 56, 40, 32), (4096,), (16,)), (16,), 1): ((),),
        ('up_fwd', ((4, 7, 7, 5, 256), (262144,), (128,)), (128,), 1): ((),),
        ('up_fwd', ((4, 14, 14, 10, 128), (65536,), (64,)), (64,), 1): ((),),
        ('up_fwd', ((4, 28, 28, 20, 64), (16384,), (32,)), (32,), 1): ((),),
        ('k2_fwd_stats', ((4, 56, 56, 40, 32), (4096,), (16,)), (1, 16, 4), 1): ((),),
        ('pw16_fwd_norm', ((1, 112, 112, 80, 16), (5, 1, 16), (2, 16, 1, 1, 1)), (1, 1, 2), 0): ((),),
        ('pw16_fwd_norm', ((4, 112, 112, 80, 16), (5, 4, 16), (2, 16, 1, 1, 1)), (4, 1, 2), 0): ((),),
        ('gnorm_fwd', ((1, 7, 7, 5, 256), (256,), (256,)), (1,), 0): ((),),
        ('gnorm_fwd', ((1, 14, 14, 10, 128), (128,), (128,)), (1,), 0): ((), ('residual',)),
        ('gnorm_fwd', ((1, 28, 28, 20, 64), (64,), (64,)), (1,), 0): ((), ('partial',), ('residual',)),
        ('gnorm_fwd', ((1, 56, 56, 40, 32), (32,), (32,)), (1,), 0): ((), ('partial',), ('residual',)),
        ('gnorm_fwd', ((1, 112, 112, 80, 16), (16,), (16,)), (1,), 0): (('partial',), ('partial', 'stats_only'), ('residual',)),
        ('gnorm_fwd', ((4, 7, 7, 5, 256), (256,), (256,)), (1,), 0): ((),),
        ('gnorm_fwd', ((4, 14, 14, 10, 128), (128,), (128,)), (1,), 0): ((), ('residual',)),
        ('gnorm_fwd', ((4, 28, 28, 20, 64), (64,), (64,)), (1,), 0): ((), ('partial',), ('residual',)),
        ('gnorm_fwd', ((4, 56, 56, 40, 32), (32,), (32,)), (1,), 0): ((), ('partial',), ('residual',)),
        ('gnorm_fwd', ((4, 112, 112, 80, 16), (16,), (16,)), (1,), 0): (('partial',), ('partial', 'residual'), ('partial', 'stats_only')),
    },
    "pancreasgn": {
        ('down_fwd', ((2, 12, 12, 12, 128), (262144,), (256,)), (256,), 1): ((),),
        ('down_fwd', ((2, 24, 24, 24, 64), (65536,), (128,)), (128,), 1): ((),),
        ('down_fwd', ((2, 48, 48, 48, 32), (16384,), (64,)), (64,), 1): ((),),
        ('down_fwd', ((2, 96, 96, 96, 16), (4096,), (32,)), (32,), 1): ((),),
        ('down_dgrad', ((2, 6, 6, 6, 256), (262144,)), (128,), 1): (('accumulate', 'out'),),
        ('down_dgrad', ((2, 12, 12, 12, 128), (65536,)), (64,), 1): (('accumulate', 'out'),),
        ('down_dgrad', ((2, 24, 24, 24, 64), (16384,)), (32,), 1): (('accumulate', 'out'),),
        ('down_dgrad', ((2, 48, 48, 48, 32), (4096,)), (16,), 1): (('accumulate', 'out'),),
        ('up_fwd', ((2, 6, 6, 6, 256), (262144,), (128,)), (128,), 1): ((),),
        ('up_fwd', ((2, 12, 12, 12, 128), (65536,), (64,)), (64,), 1): ((),),
        ('up_fwd', ((2, 24, 24, 24, 64), (16384,), (32,)), (32,), 1): ((),),
        ('up_dgrad', ((2, 12, 12, 12, 128), (262144,)), (256,), 1): ((),),
        ('up_dgrad', ((2, 24, 24, 24, 64), (65536,)), (128,), 1): ((),),
        ('up_dgrad', ((2, 48, 48, 48, 32), (16384,)), (64,), 1): ((),),
        ('up_dgrad', ((2, 96, 96, 96, 16), (4096,)), (32,), 1): ((),),
        ('k2_fwd_stats', ((2, 48, 48, 48, 32), (4096,), (16,)), (1, 16, 2), 1): ((),),
        ('k2_wgrad', ((2, 6, 6, 6, 256), (2, 12, 12, 12, 128), (256, 128, 2, 2, 2)), (1,), 2): (('accumulate',),),
        ('k2_wgrad', ((2, 12, 12, 12, 128), (2, 6, 6, 6, 256), (256, 128, 2, 2, 2)), (0,), 2): (('accumulate',),),
        ('k2_wgrad', ((2, 12, 12, 12, 128), (2, 24, 24, 24, 64), (128, 64, 2, 2, 2)), (1,), 2): (('accumulate',),),
        ('k2_wgrad', ((2, 24, 24, 24, 64), (2, 12, 12, 12, 128), (128, 64, 2, 2, 2)), (0,), 2): (('accumulate',),),
        ('k2_wgrad', ((2, 24, 24, 24, 64), (2, 48, 48, 48, 32), (64, 32, 2, 2, 2)), (1,), 2): (('accumulate',),),
        ('k2_wgrad', ((2, 48, 48, 48, 32), (2, 24, 24, 24, 64), (64, 32, 2, 2, 2)), (0,), 2): (('accumulate',),),
        ('k2_wgrad', ((2, 48, 48, 48, 32), (2, 96, 96, 96, 16), (32, 16, 2, 2, 2)), (1,), 2): (('accumulate',),),
        ('k2_wgrad', ((2, 96, 96, 96, 16), (2, 48, 48, 48, 32), (32, 16, 2, 2, 2)), (0,), 2): (('accumulate',),),
        ('mix_box', ((1, 96, 96, 96, 1), (1, 96, 96, 96, 1)), (), 0): (('out',),),
        ('pw16_fwd_norm', ((2, 96, 96, 96, 16), (5, 2, 16), (2, 16, 1, 1, 1)), (2, 1, 2), 0): ((),),
        ('mixloss_pair_fwd', ((2, 96, 96, 96, 2), (1, 96, 96, 96), (1, 96, 96, 96)), (0,), 0): ((),),
        ('mixloss_pair_bwd', ((2, 96, 96, 96, 2), (1, 96, 96, 96), (1, 96, 96, 96)), (0,), 0): (('out', 'g_dev'),),
        ('conv3_c1_wgrad', ((2, 96, 96, 96, 1), (2, 96, 96, 96, 16), (16, 1, 3, 3, 3)), (3,), 1): (('accumulate',),),
        ('gnorm_fwd', ((2, 6, 6, 6, 256), (256,), (256,)), (1,), 0): ((),),
        ('gnorm_fwd', ((2, 12, 12, 12, 128), (128,), (128,)), (1,), 0): ((), ('residual',)),
        ('gnorm_fwd', ((2, 24, 24, 24, 64), (64,), (64,)), (1,), 0): ((), ('partial',), ('residual',)),
        ('gnorm_fwd', ((2, 48, 48, 48, 32), (32,), (32,)), (1,), 0): ((), ('partial',), ('residual',)),
        ('gnorm_fwd', ((2, 96, 96, 96, 16), (16,), (16,)), (1,), 0): (('partial',), ('partial', 'residual'), ('partial', 'stats_only')),
        ('gnorm_bwd', ((2, 6, 6, 6, 256), (2, 6, 6, 6, 256), (5, 2, 256)), (1, 1), 0): (('accumulate', 'dbias'),),
        ('gnorm_bwd', ((2, 12, 12, 12, 128), (2, 12, 12, 12, 128), (5, 2, 128)), (1, 1), 0): (('accumulate', 'dbias'),),
        ('gnorm_bwd', ((2, 24, 24, 24, 64), (2, 24, 24, 24, 64), (5, 2, 64)), (1, 1), 0): (('partial', 'accumulate', 'dbias'), ('accumulate', 'dbias')),
        ('gnorm_bwd', ((2, 48, 48, 48, 32), (2, 48, 48, 48, 32), (5, 2, 32)), (1, 1), 0): (('partial', 'accumulate', 'dbias'), ('accumulate', 'dbias')),
        ('gnorm_bwd', ((2, 96, 96, 96, 16), (2, 96, 96, 96, 16), (5, 2, 16)), (1, 1), 0): (('accumulate',),),
        ('pw16_bwd_norm', ((2, 96, 96, 96, 16), (5, 2, 16), (2, 96, 96, 96, 2)), (2, 1), 0): (('accumulate',),),
    },
}


def variants_of(wl, key):
    """the epilogues the step uses at a norm key (STEP_VARIANTS); other ops: one plain call"""
    return STEP_VARIANTS.get(wl, {}).get(key, ((),))


def run_row(ops, dev, wl, key, g, table_key=None):
    """one row through its driver; table_key: the STEP_KEYS row whose variants apply where `key` is its reduced twin"""
    fn = DRIVERS[key[0]]
    gn = is_gn(wl)
    if gn and fn is drive_head:
        fn = drive_gn_head
    if fn in (drive_gnorm_fwd, drive_gnorm_bwd, drive_gn_head):
        return fn(ops, dev, key, g, variants_of(wl, table_key or key), wl=wl, table_key=table_key or key)
    if key[0] in _VARIANT_OPS:
        return fn(ops, dev, key, g, variants_of(wl, table_key or key), **({"gn": True} if gn and fn is drive_k2 else {}))
    if fn is drive_pack_many:
        return fn(ops, dev, key, g, wl)
    if fn is drive_conv:
        return fn(ops, dev, key, g, step_groups(wl), stats_fused(wl, table_key or key) if key[0] == "conv3_fwd_stats" else True, gn=gn)
    if fn is drive_c1_stats:
        return fn(ops, dev, key, g, gn=gn)
    return fn(ops, dev, key, g)
