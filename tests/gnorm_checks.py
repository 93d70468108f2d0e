"""GroupNorm checks (normalization='groupnorm' of the V-Nets): the kernels of bcp_amd/csrc/gnorm.hip against torch fp64 on the CPU, and the
GroupNorm networks against the oracle with its norm patched to F.group_norm.  Shared by tests/test_emu_gnorm.py (host simulator) and
tests/test_gpu_gnorm.py (-m gpu).

Tolerances are the project's own: forward kernel_checks.close's default (rtol 1e-4); dy, dgamma, dbeta and the conv-bias gradient rtol 2e-4
(check_norm); logits rel-L2 < 1e-4, loss |d| < 1e-5, gradient tensors rel-L2 < 1e-4 (check_vnet_pattern_grads)."""
import ctypes

import numpy as np
import torch
import torch.nn.functional as F

import kernel_checks as K
from bcp_amd import hip_ops as H

GROUPS = 16


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------ kernels
class _Case:
    """one seeded GroupNorm layer: inputs, the fp64 reference (autograd) and the device tensors"""

    def __init__(self, rng, dev, N, Cc, sp, use_cs=False, use_res=False, offsets=False):
        self.N, self.C, self.sp, self.dev = N, Cc, sp, dev
        y = K.R(rng, N, Cc, *sp) * 1.7 + 0.4
        if offsets:      # per-channel offsets of order 30, spread 1: the group variance is dominated by the differences BETWEEN channels
            y = K.R(rng, N, Cc, *sp) + (30.0 + K.R(rng, Cc)).view(1, Cc, 1, 1, 1)
        self.y = y
        self.gamma = torch.from_numpy(rng.uniform(0.5, 1.5, Cc).astype(np.float32))
        self.beta = torch.from_numpy(rng.uniform(-0.3, 0.3, Cc).astype(np.float32))
        self.cs = torch.from_numpy(((rng.random((N, Cc)) < 0.5) * 2.0).astype(np.float32)) if use_cs else None
        self.res = K.R(rng, N, Cc, *sp) if use_res else None
        self.da = K.R(rng, N, Cc, *sp)
        # reference: torch on the CPU in fp64, gradients from autograd
        yd = y.double().requires_grad_(True)
        gd, bd = self.gamma.double().requires_grad_(True), self.beta.double().requires_grad_(True)
        a = F.relu(F.group_norm(yd, GROUPS, gd, bd, 1e-5))
        if self.cs is not None:
            a = a * self.cs.double().view(N, Cc, 1, 1, 1)
        if self.res is not None:
            a = a + self.res.double()
        a.backward(self.da.double())
        self.a_ref, self.dy_ref, self.dg_ref, self.db_ref = a.detach(), yd.grad, gd.grad, bd.grad
        self.dbias_ref = yd.grad.sum((0, 2, 3, 4))
        self.ycl, self.dacl = K.to_cl(y).to(dev), K.to_cl(self.da).to(dev)
        self.gd, self.bd = self.gamma.to(dev), self.beta.to(dev)
        self.csd = None if self.cs is None else self.cs.to(dev)
        self.resd = None if self.res is None else K.to_cl(self.res).to(dev)

    def fwd(self, ops, **kw):
        res = None if kw.get("stats_only") else self.resd      # (statistics only: no apply pass, so no residual)
        return ops.gnorm_fwd(self.ycl, self.gd, self.bd, H.ACT_RELU, chan_scale=self.csd, residual=res, **kw)

    def bwd(self, ops, stats, dg=None, db=None, dbias=None, accumulate=False, **kw):
        return ops.gnorm_bwd(self.ycl, self.dacl, stats, self.gd, H.ACT_RELU, dg, db, dbias, accumulate, chan_scale=self.csd, **kw)


def _check_case(ops, c, tag):
    N, Cc, dev = c.N, c.C, c.dev
    cg = Cc // GROUPS
    a, stats = c.fwd(ops)
    K.close(K.from_cl(a), c.a_ref, msg=f"gnorm fwd {tag}")
    # the table: mean / rstd constant within a group, scale == gamma * rstd, shift == beta
    st = stats.cpu()
    for row in (0, 1):
        g = st[row].view(N, GROUPS, cg)
        assert torch.equal(g, g[:, :, :1].expand_as(g)), f"{tag}: table row {row} must repeat over a group's channels"
    yg = c.y.double().view(N, GROUPS, -1)
    K.close(st[0].view(N, GROUPS, cg)[:, :, 0], yg.mean(2), rtol=1e-6, msg=f"{tag} mean")
    K.close(st[1].view(N, GROUPS, cg)[:, :, 0], 1.0 / torch.sqrt(yg.var(2, unbiased=False) + 1e-5), rtol=1e-5, msg=f"{tag} rstd")
    K.close(st[2], st[1] * c.gamma, rtol=1e-6, atol_scale=0.0, msg=f"{tag} scale == gamma * rstd")
    assert torch.equal(st[3], c.beta.expand(N, Cc)), f"{tag}: shift == beta"
    # |max| slots after the apply pass reduce to exactly max |a|
    assert H.amax_value(a._bcp_amax) == float(a.abs().max()), f"{tag}: |max| of a"
    # out = NULL: statistics only, the same table bit for bit
    none, stats0 = c.fwd(ops, stats_only=True)
    assert none is None and torch.equal(_bits(stats0), _bits(stats)), f"{tag}: statistics-only table"
    # backward
    dg, db, dbias = (torch.full((Cc,), 7.0).to(dev) for _ in range(3))
    dy = c.bwd(ops, stats, dg, db, dbias, False)
    K.close(K.from_cl(dy), c.dy_ref, rtol=2e-4, msg=f"gnorm dy {tag}")
    K.close(dg, c.dg_ref, rtol=2e-4, msg=f"gnorm dgamma {tag}")
    K.close(db, c.db_ref, rtol=2e-4, msg=f"gnorm dbeta {tag}")
    assert H.amax_value(dy._bcp_amax) == float(dy.abs().max()), f"{tag}: |max| of dy"
    l1 = float(c.dy_ref.abs().sum())

    def bias_ok(t, k, what):
        if cg > 1:
            K.close(t, k * c.dbias_ref, rtol=2e-4, msg=f"gnorm conv-bias gradient {what} {tag}")
        else:      # one channel per group: the gradient is rounding noise; exact zero is allowed
            assert float(t.abs().max()) <= 1e-6 * l1, f"{tag}: conv-bias gradient at C=16 {what}"
    bias_ok(dbias, 1, "=")
    dy2 = c.bwd(ops, stats, dg, db, dbias, True)
    assert torch.equal(_bits(dy2), _bits(dy))
    K.close(dg, 2 * c.dg_ref, rtol=2e-4, msg=f"gnorm dgamma accumulate {tag}")
    K.close(db, 2 * c.db_ref, rtol=2e-4, msg=f"gnorm dbeta accumulate {tag}")
    bias_ok(dbias, 2, "+=")
    # no parameter gradients asked for: dy alone, the same bits
    assert torch.equal(_bits(c.bwd(ops, stats)), _bits(dy))
    return a, stats, dy


WIDTH_CASES = ((3, 16, (3, 5, 7)), (3, 32, (3, 5, 7)), (3, 64, (3, 5, 7)), (3, 128, (3, 5, 7)), (3, 256, (1, 3, 5)))


def check_gnorm_widths(ops, dev):
    """all five group widths (cg = 1, 2, 4, 8, 16), N = 3, ragged rows per sample; sample independence bit for bit"""
    rng = np.random.default_rng(31)
    for (N, Cc, sp) in WIDTH_CASES:
        c = _Case(rng, dev, N, Cc, sp)
        a, stats, dy = _check_case(ops, c, f"C={Cc}")
        # a, the table rows and dy of sample n equal those of the same sample run alone: the partition invariance the feature exists for
        for n in range(N):
            y1, da1 = c.ycl[n:n + 1].contiguous(), c.dacl[n:n + 1].contiguous()
            a1, st1 = ops.gnorm_fwd(y1, c.gd, c.bd, H.ACT_RELU)
            dy1 = ops.gnorm_bwd(y1, da1, st1, c.gd, H.ACT_RELU)
            assert torch.equal(_bits(a1[0]), _bits(a[n])), f"C={Cc}: a of sample {n} depends on the batch"
            assert torch.equal(_bits(st1[:, 0]), _bits(stats[:, n])), f"C={Cc}: table rows of sample {n} depend on the batch"
            assert torch.equal(_bits(dy1[0]), _bits(dy[n])), f"C={Cc}: dy of sample {n} depends on the batch"


def check_gnorm_epilogues(ops, dev):
    """ReLU with the Dropout3d channel scale, with a residual, with both; per-channel offsets of order 30; more than one partial row per
    sample (rows per sample >= 2 * (256 / (C / 4)) * 16)"""
    rng = np.random.default_rng(32)
    for (N, Cc, sp, cs, res, off) in ((3, 32, (3, 5, 7), True, False, False), (3, 32, (3, 5, 7), False, True, False), (2, 64, (2, 5, 3), True, True, False),
                                     (3, 64, (3, 5, 7), False, False, True), (2, 16, (3, 5, 7), True, False, True),
                                     (3, 16, (12, 16, 11), False, False, False), (3, 32, (8, 12, 11), True, True, False)):
        _check_case(ops, _Case(rng, dev, N, Cc, sp, cs, res, off), f"C={Cc} sp={sp} cs={cs} res={res} offsets={off}")


def check_gnorm_partial_in(ops, dev):
    """statistics taken from the partial rows a conv epilogue left (bcp_conv3_fwd_stats forward, bcp_conv3_dgrad_bwdstats backward,
    groups = N) against the kernel's own passes: both within tolerance of the reference"""
    rng = np.random.default_rng(33)
    for (N, Cin, Cout, sp) in ((2, 32, 32, (8, 12, 20)), (2, 16, 16, (6, 5, 9))):
        x = K.R(rng, N, Cin, *sp)
        w = K.R(rng, Cout, Cin, 3, 3, 3) * 0.1
        b = K.R(rng, Cout) * 0.1
        gamma = torch.from_numpy(rng.uniform(0.5, 1.5, Cout).astype(np.float32))
        beta = torch.from_numpy(rng.uniform(-0.3, 0.3, Cout).astype(np.float32))
        wf, _ = ops.conv3_pack(w.to(dev).contiguous(), 3)
        y, part, rows = ops.conv3_fwd_stats(K.to_cl(x).to(dev), wf, b.to(dev), Cout, 3, N)
        assert rows > 0, "these shapes must support fused statistics"
        a_ref = F.relu(F.group_norm(K.from_cl(y).cpu().double(), GROUPS, gamma.double(), beta.double(), 1e-5))
        a1, st1 = ops.gnorm_fwd(y, gamma.to(dev), beta.to(dev), H.ACT_RELU, partial=part, nb=rows)
        a2, st2 = ops.gnorm_fwd(y, gamma.to(dev), beta.to(dev), H.ACT_RELU)
        K.close(K.from_cl(a1), a_ref, msg=f"gnorm from the conv epilogue's rows C={Cout}")
        K.close(K.from_cl(a2), a_ref, msg=f"gnorm own statistics C={Cout}")
        K.close(st1[:4], st2[:4], rtol=1e-6, msg="the two tables")
    # backward: the (sum dz, sum dz * xhat) rows a dgrad epilogue leaves for a GroupNorm table (bcp_conv3_dgrad_bwdstats reads mean / rstd /
    # scale / shift per (sample, channel), groups = N) against the kernel's own backward-statistics pass
    # (N, channels of dy, channels of da, extents, rows per sample the epilogue must leave): the row query answers the same on the
    # simulator and on the device for all four -- a case that stops being served is a failure, not a case to pass over
    for (N, Cdy, Cda, sp, want) in ((2, 32, 32, (8, 16, 16), 8), (3, 32, 32, (5, 9, 11), 12), (2, 16, 32, (6, 10, 12), 12), (2, 64, 64, (16, 16, 40), 160)):
        w = K.R(rng, Cdy, Cda, 3, 3, 3) * 0.1
        _, wd = ops.conv3_pack(w.to(dev).contiguous(), 3)
        dy = torch.from_numpy(rng.standard_normal((N,) + sp + (Cdy,), dtype=np.float32)).to(dev)
        yprev = (torch.from_numpy(rng.standard_normal((N,) + sp + (Cda,), dtype=np.float32)) * 1.3 + 0.2).to(dev)
        gam = torch.from_numpy(rng.uniform(0.5, 1.5, Cda).astype(np.float32)).to(dev)
        bet = torch.from_numpy(rng.uniform(-0.3, 0.3, Cda).astype(np.float32)).to(dev)
        _, st = ops.gnorm_fwd(yprev, gam, bet, H.ACT_RELU)
        da, part, rows = ops.conv3_dgrad_bwdstats(dy, wd, Cda, 3, yprev, st, H.ACT_RELU, N)
        asked = ops._ws_bytes("bcp_conv3_bwdstat_rows", N, *sp, Cdy, Cda, 3, N)
        assert asked == rows, f"bcp_conv3_bwdstat_rows answers {asked} for {Cdy}->{Cda} {sp} N={N}, the launch left {rows} rows"
        assert rows == want, f"conv3_dgrad_bwdstats {Cdy}->{Cda} {sp} N={N}: {rows} rows of fused backward statistics, expected {want}"
        g1 = [torch.zeros(Cda).to(dev) for _ in range(3)]
        g2 = [torch.zeros(Cda).to(dev) for _ in range(3)]
        d1 = ops.gnorm_bwd(yprev, da, st, gam, H.ACT_RELU, *g1, False, partial=part, nb=rows)
        d2 = ops.gnorm_bwd(yprev, da, st, gam, H.ACT_RELU, *g2, False)
        yd = K.from_cl(yprev).cpu().double().requires_grad_(True)
        gd = gam.cpu().double().requires_grad_(True)
        bd = bet.cpu().double().requires_grad_(True)
        F.relu(F.group_norm(yd, GROUPS, gd, bd, 1e-5)).backward(K.from_cl(da).cpu().double())
        for d, g, how in ((d1, g1, "the dgrad epilogue's rows"), (d2, g2, "own pass")):
            K.close(K.from_cl(d), yd.grad, rtol=2e-4, msg=f"gnorm dy from {how} {Cdy}->{Cda} {sp}")
            K.close(g[0], gd.grad, rtol=2e-4, msg=f"gnorm dgamma from {how}")
            K.close(g[1], bd.grad, rtol=2e-4, msg=f"gnorm dbeta from {how}")
            K.close(g[2], yd.grad.sum((0, 2, 3, 4)), rtol=2e-4, msg=f"gnorm conv-bias gradient from {how}")


def check_gnorm_refusals(binding):
    """bad arguments are refused with BCP_EINVAL and a bcp_last_error() text before any launch (no device needed)"""
    N, rows, Cc = 1, 8, 32
    buf = (ctypes.c_ubyte * (1 << 16))()
    base = (ctypes.addressof(buf) + 15) & ~15
    y, out, stats, ws = base, base + 4096, base + 8192, base + 16384
    fwd, bwd, err = binding.cdll.bcp_gnorm_fwd, binding.cdll.bcp_gnorm_bwd, binding.cdll.bcp_last_error

    def f(y=y, N=N, rows=rows, C=Cc, groups=GROUPS, stats=stats, ws=ws, out=out, res=None, part=None, nb=0):
        return fwd(y, N, rows, C, groups, None, None, 1e-5, 1, None, res, stats, ws, part, nb, out, None, None)

    def g(y=y, da=out, N=N, rows=rows, C=Cc, groups=GROUPS, stats=stats, ws=ws, dy=out + 2048, dg=None, db=None, part=None, nb=0, cs=None):
        return bwd(y, da, N, rows, C, groups, stats, None, 1, cs, dg, db, None, 0, ws, part, nb, dy, None, None)
    for call in (f, g):
        assert call(y=None) == -1 and b"null" in err()
        assert call(stats=None) == -1 and b"null" in err()
        assert call(ws=None) == -1 and b"null" in err()
        assert call(y=y + 4) == -1 and b"alignment" in err()
        assert call(stats=stats + 8) == -1 and b"alignment" in err()
        assert call(groups=3) == -1 and b"no multiple of groups" in err()
        assert call(groups=0) == -1 and b"groups" in err()
        assert call(groups=8) == -1 and b"unsupported" in err()            # 8 groups of 4 channels: not nn.GroupNorm(16, C)
        assert call(C=512) == -1 and b"unsupported" in err()               # 16 groups of 32 channels: wider than a finalize chunk
        assert call(C=8) == -1 and b"unsupported" in err()                 # the extents bcp_norm_fwd refuses
        assert call(C=48) == -1 and b"unsupported" in err()
        assert call(N=0) == -1 and b"extents" in err()
        assert call(rows=0) == -1 and b"extents" in err()
        assert call(part=ws, nb=0) == -1 and b"partial_in" in err()
    assert f(out=out + 4) == -1 and b"alignment" in err()
    assert f(out=None, res=out) == -1 and b"statistics-only" in err()
    assert g(dy=None) == -1 and b"null" in err()
    assert g(da=None) == -1 and b"null" in err()
    assert g(dy=out + 2052) == -1 and b"alignment" in err()
    assert g(dg=out) == -1 and b"pair" in err()
    assert g(part=ws, nb=2, cs=out) == -1 and b"partial_in" in err()
    assert binding.cdll.bcp_gnorm_workspace_bytes(1, 8, 8) == 0 and binding.cdll.bcp_gnorm_workspace_bytes(3, 105, 64) > 0
    assert not any(buf), "a refused call must not write"


# ------------------------------------------------------------------------------------------ networks
import collections  # noqa: E402

import bcp_oracle as O  # noqa: E402
import net_checks as NC  # noqa: E402
from bcp_amd.utils import BCP_utils as BU  # noqa: E402

NET_SHAPE = (32, 32, 16)


def gn_norm_act(y, P, bn_prefix, norm, train, momentum=0.1, eps=1e-5):
    """what bcp_oracle._norm_act is patched to: nn.GroupNorm(16, C) with the layer's weight / bias (train and eval alike)"""
    return F.group_norm(y, GROUPS, P[bn_prefix + ".weight"], P[bn_prefix + ".bias"], eps)


def patch_oracle(monkeypatch):
    monkeypatch.setattr(O, "_norm_act", gn_norm_act)


def _is_block_conv_bias(k, P):
    return k.endswith(".bias") and P[k[:-5] + ".weight"].dim() == 5 and "out_conv" not in k and not k.startswith("branchs.0.1")


def gn_params(variant, seed):
    """the oracle's parameter dictionary of a GroupNorm V-Net: the LA dictionary has weight / bias at every norm index already (its
    running statistics are simply unused); the pancreas one gets them added here, random like the LA ones"""
    P = O.init_params(O.vnet_param_shapes(variant=variant), seed=seed, random_affine=True)
    if variant == "la":
        return P
    rng = np.random.default_rng(seed + 1)
    Q = collections.OrderedDict()
    for k, v in P.items():
        Q[k] = v
        if _is_block_conv_bias(k, P):
            pre = O._next(k[:-5])
            Q[pre + ".weight"] = torch.from_numpy(rng.uniform(0.5, 1.5, v.shape).astype(np.float32))
            Q[pre + ".bias"] = torch.from_numpy(rng.uniform(-0.2, 0.2, v.shape).astype(np.float32))
    return Q


def make_gn_vnet(P, dev, ops, variant="la", has_dropout=True, normalization="groupnorm"):
    """net_checks.make_vnet for normalization='groupnorm' (keys P does not hold keep the constructor's values)"""
    from bcp_amd.networks.VNet import VNet
    net = VNet(n_channels=1, n_classes=2, normalization=normalization, has_dropout=has_dropout and variant == "la", variant=variant).to(dev)
    net.load_state_dict({k: (P[k].clone() if k in P else v) for k, v in net.state_dict().items()})
    net.flatten_()
    if dev.type == "cpu":
        net.set_ops(ops)
        BU.set_test_ops(ops)
    net.train()
    return net


def check_gn_keys(dev):
    """state_dict() keys, shapes and counts (172 / 118) and parameters() order, built from the default networks' own key lists; a round
    trip through state_dict() / load_state_dict() keeps the bits; a checkpoint of the other normalisation fails loudly"""
    import pytest
    from bcp_amd.networks.VNet import VNet
    track = ("running_mean", "running_var", "num_batches_tracked")
    for variant, default, nkeys, nparams in (("la", "batchnorm", 172, 154), ("pancreas", "instancenorm", 118, None)):
        la = variant == "la"
        base = VNet(n_channels=1, n_classes=2, normalization=default, has_dropout=la, variant=variant)
        gn = VNet(n_channels=1, n_classes=2, normalization="groupnorm", has_dropout=la, variant=variant)
        bsd, gsd = base.state_dict(), gn.state_dict()
        if la:
            exp = [(k, tuple(v.shape)) for k, v in bsd.items() if not (k.rsplit(".", 1)[-1] in track and k.startswith(("encoder.", "decoder.")))]
            assert [n for n, _ in gn.named_parameters()] == [n for n, _ in base.named_parameters()]
            assert [tuple(p.shape) for p in gn.parameters()] == [tuple(p.shape) for p in base.parameters()]
            assert len(list(gn.parameters())) == nparams
            assert sum(1 for k in gsd if k.rsplit(".", 1)[-1] in track) == 3 * 6      # the contrastive heads' BatchNorm1d buffers stay
        else:
            exp = []
            for k, v in bsd.items():
                exp.append((k, tuple(v.shape)))
                if _is_block_conv_bias(k, bsd):
                    exp += [(O._next(k[:-5]) + ".weight", tuple(v.shape)), (O._next(k[:-5]) + ".bias", tuple(v.shape))]
            names = [n for n, _ in gn.named_parameters()]
            assert names == [k for k, _ in exp] and len(list(gn.buffers())) == 0
        assert [(k, tuple(v.shape)) for k, v in gsd.items()] == exp and len(gsd) == nkeys, (variant, len(gsd))
        for k, v in gsd.items():      # GroupNorm weight = ones, bias = zeros
            if (k, tuple(v.shape)) not in [(k2, tuple(v2.shape)) for k2, v2 in bsd.items()]:
                assert torch.equal(v, torch.ones_like(v) if k.endswith(".weight") else torch.zeros_like(v)), k
        # round trip, through the flat buffer on the device
        rng = np.random.default_rng(3)
        src = {k: (torch.from_numpy(rng.standard_normal(tuple(v.shape)).astype(np.float32)) if v.is_floating_point() else v.clone()) for k, v in gsd.items()}
        gn2 = VNet(n_channels=1, n_classes=2, normalization="groupnorm", has_dropout=la, variant=variant).to(dev)
        gn2.load_state_dict(src)
        gn2.flatten_()
        back = gn2.state_dict()
        assert list(back) == list(src)
        for k in src:
            assert torch.equal(back[k].cpu(), src[k]) if not src[k].is_floating_point() else torch.equal(_bits(back[k]), _bits(src[k])), k
        with pytest.raises(RuntimeError):
            gn2.load_state_dict(bsd)
        with pytest.raises(RuntimeError):
            base.load_state_dict(gsd)
    # what stays refused, with the present message
    for kw in (dict(normalization="none"), dict(normalization="groupnorm", has_residual=True), dict(normalization="groupnorm", n_filters=32),
               dict(normalization="instancenorm"), dict(normalization="batchnorm", variant="pancreas")):
        with pytest.raises(AssertionError):
            VNet(n_channels=1, n_classes=2, **kw)


def check_gn_pattern_grads(ops, dev, monkeypatch, variant="la", seed=11, N=2, bound=1e-4):
    """net_checks.check_vnet_pattern_grads for the GroupNorm nets: every gradient tensor against the fp64 oracle linearised on the
    activation pattern the HIP forward took -- INCLUDING the pre-norm conv biases of every layer with >= 32 channels, whose gradient
    GroupNorm does not cancel (16-channel layers: one channel per group, exact zeros here, rounding noise in the reference)"""
    patch_oracle(monkeypatch)
    rng = np.random.default_rng(seed)
    P = gn_params(variant, seed + 200)
    x = torch.from_numpy(rng.standard_normal((N, 1) + NET_SHAPE, dtype=np.float32))
    tgt = torch.from_numpy(rng.integers(0, 2, (N,) + NET_SHAPE))
    dm = None
    if variant == "la":
        dm = {"x5": torch.from_numpy((rng.random((N, 256)) < 0.5).astype(np.float32)), "x9": torch.from_numpy((rng.random((N, 16)) < 0.5).astype(np.float32))}
    net = make_gn_vnet(P, dev, ops, variant)
    net.drop_masks = dm
    net._keep_saved = True
    out = net(x.to(dev))[0]
    loss = BU.sup_loss(out, tgt.to(dev))
    loss.backward()
    saved = net._last_saved
    masks = [NC._pattern(s.y, s.stats, saved.G) for s in saved.layers]
    Pd = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in P.items()}
    Q = O._with_grad(Pd, set(O.trainable_keys(Pd)))
    o64 = O.vnet_forward(Q, x.double(), dm, True, variant, act_masks=masks)
    l64 = O.sup_loss_la(o64, tgt)
    l64.backward()
    assert K.rel_l2(out, o64.detach()) < 1e-4 and abs(float(loss.detach()) - float(l64.detach())) < 1e-5
    params = dict(net.named_parameters())
    worst, n, nbias = ("", 0.0), 0, 0
    for k in Q:
        gref = getattr(Q[k], "grad", None)
        if gref is None or k not in params:
            continue
        if NC.is_prenorm_bias(k, params) and params[k].numel() < 32:
            assert float(params[k].grad.abs().max()) == 0.0, (k, "one channel per group: exact zeros")
            continue
        if float(gref.norm()) < 1e-9:
            continue
        r = K.rel_l2(params[k].grad, gref)
        n += 1
        nbias += int(NC.is_prenorm_bias(k, params))
        if r > worst[1]:
            worst = (k, r)
        assert r < bound, (variant, k, r)
    assert n >= 25 and nbias >= 20, (n, nbias)
    return worst


def check_gn_eval(ops, dev, monkeypatch, variants=("la", "pancreas"), sliding_window=True):
    """model.eval() is the train-mode function (dropout off) bit for bit and within rtol 2e-4 of the oracle; one var_all_case_LA case
    through the sliding window with a GroupNorm model"""
    patch_oracle(monkeypatch)
    rng = np.random.default_rng(17)
    for variant in variants:
        P = gn_params(variant, 301)
        net = make_gn_vnet(P, dev, ops, variant)
        x = torch.from_numpy(rng.standard_normal((2, 1) + NET_SHAPE, dtype=np.float32))
        ot = net(x.to(dev), turnoff_drop=True)[0].detach().clone()      # (autograd node: the forward that saves for a backward pass)
        with torch.no_grad():
            on = net(x.to(dev), turnoff_drop=True)[0].clone()
        net.eval()
        with torch.no_grad():
            oe = net(x.to(dev))[0].clone()
        net.train()
        assert torch.equal(_bits(ot), _bits(oe)) and torch.equal(_bits(on), _bits(oe)), (variant, "eval() != train() with dropout off")
        with torch.no_grad():
            ref = O.vnet_forward(P, x, None, False, variant, has_dropout=False)
        K.close(oe, ref, rtol=2e-4, msg=f"GroupNorm eval forward {variant}")
    if not sliding_window:
        return
    from bcp_amd.utils import test_3d_patch as T3
    P = gn_params("la", 302)
    net = make_gn_vnet(P, dev, ops, "la")
    vol, lab = O.synth_la_batch(1, shape=(40, 32, 20), seed=303)
    image, gt = vol[0, 0].numpy(), lab[0].numpy()
    label, _ = O.sliding_window_la(P, image, 8, 4, NET_SHAPE)
    mean_dice = T3.var_all_case_LA(net, 2, NET_SHAPE, 8, 4, cases=[(image, gt)])
    assert abs(mean_dice - O.dice_binary(label, gt)) < 1e-3, (mean_dice, O.dice_binary(label, gt))
    assert net.training


def check_gn_batch_split(ops, dev):
    """a forward of [a, b] against forwards of [a] and [b], dropout off: the GroupNorm logits agree within rtol 2e-4, the BatchNorm
    net's must not -- what GroupNorm buys"""
    rng = np.random.default_rng(19)
    P = gn_params("la", 311)
    x = torch.from_numpy(rng.standard_normal((2, 1) + NET_SHAPE, dtype=np.float32)).to(dev)
    err = {}
    for norm in ("groupnorm", "batchnorm"):
        net = make_gn_vnet(P, dev, ops, "la", normalization=norm)
        with torch.no_grad():
            both = net(x, turnoff_drop=True)[0].clone()
            one = torch.cat([net(x[i:i + 1], turnoff_drop=True)[0].clone() for i in range(2)])
        scale = float(one.abs().max())
        err[norm] = float((both - one).abs().max()) / scale
    assert err["groupnorm"] <= 2e-4 + 1e-5, err
    assert err["batchnorm"] > 2e-4 + 1e-5, err
    return err


def check_gn_step(ops, dev, monkeypatch, variant="la"):
    """the self-training step (sub-batches of two, a fixed box, dropout masks: net_checks.check_la_step_batch8) against the fp32 oracle
    step with the patched norm; then two optimiser steps move the student's GroupNorm weight / bias and, through the EMA, the teacher's"""
    from bcp_amd import train_step
    patch_oracle(monkeypatch)
    la = variant == "la"
    rng = np.random.default_rng(5)
    sub = 2
    P = gn_params(variant, 81)
    vol, lab = O.synth_la_batch(4 * sub, shape=NET_SHAPE, seed=82)
    drops = {k: {"x5": torch.from_numpy((rng.random((sub, 256)) < 0.5).astype(np.float32)),
                 "x9": torch.from_numpy((rng.random((sub, 16)) < 0.5).astype(np.float32))} for k in ("t_a", "t_b", "s_l", "s_u")} if la else {}
    box = (3, 5, 2, 21, 21, 10)
    conn = None if la else 2
    ro = O.la_self_train_step({k: v.clone() for k, v in P.items()}, {k: v.clone() for k, v in P.items()}, vol, lab, box, drops, sub,
                              variant=variant, connectivity=conn)
    model, ema = make_gn_vnet(P, dev, ops, variant), make_gn_vnet(P, dev, ops, variant)
    for p in ema.parameters():
        p.detach_()
    kw = dict(box=box, drops=drops, variant=variant, connect_mode=conn)
    r = train_step.la_self_train_step(model, ema, None, vol.to(dev), lab.to(dev), 2 * sub, **kw)
    dl = abs(float(r["loss"]) - float(ro["loss"]))
    dpl = int((r["plab_a"].cpu().float() != ro["plab_a"]).sum() + (r["plab_b"].cpu().float() != ro["plab_b"]).sum())
    params = dict(model.named_parameters())
    names = (("decoder.out_conv.weight", "decoder.block_nine.conv.0.weight", "encoder.block_one.conv.0.weight") if la else
             ("branchs.0.1.weight", "branchs.0.0.conv.0.weight", "block_one.conv.0.weight"))
    gerr = {k: K.rel_l2(params[k].grad, ro["grads"][k]) for k in names}
    print(f"[gnorm step {variant}] |dloss| {dl:.2e}  pseudo-label voxels differing {dpl}  gradients {gerr}")
    assert dl < 1e-5, (variant, float(r["loss"]), float(ro["loss"]))
    assert dpl <= 4, (variant, dpl)
    for k, e in gerr.items():
        assert e < 3e-2, (variant, k, e)
    # two optimiser steps
    opt = train_step.FlatSGD(model, lr=0.01) if la else train_step.FlatAdam(model, lr=1e-3)
    gk = [k for k in model.state_dict() if k.rsplit(".", 2)[-2] in ("1", "4", "7") and "conv." in k and k.endswith((".weight", ".bias"))]
    assert len(gk) == 58
    s0, t0 = ({k: v.clone() for k, v in m.state_dict().items()} for m in (model, ema))
    for _ in range(2):
        r = train_step.la_self_train_step(model, ema, opt, vol.to(dev), lab.to(dev), 2 * sub, **kw)
        assert bool(torch.isfinite(r["loss"]))
    s1, t1 = model.state_dict(), ema.state_dict()
    for k in gk:
        assert not torch.equal(s1[k], s0[k]), (variant, "student", k)
        assert not torch.equal(t1[k], t0[k]), (variant, "teacher", k)
    for sd in (s1, t1):
        assert all(bool(torch.isfinite(v.float()).all()) for v in sd.values())


def check_gn_launch_plans(ops, dev, monkeypatch, cases=(("la", True), ("pancreas", True)), **kw):
    """net_checks.check_launch_plans with GroupNorm networks: recorded launch plans / C replay / graphs == the eager path, bit for bit"""
    monkeypatch.setattr(NC, "make_vnet", lambda P, dev_, ops_, variant="la", has_dropout=True: make_gn_vnet(_gn_like(P, variant), dev_, ops_, variant, has_dropout))
    NC.check_launch_plans(ops, dev, cases=cases, **kw)


def _gn_like(P, variant):
    """random GroupNorm weight / bias for the parameter dictionaries net_checks builds for the default pancreas net"""
    if variant == "la" or any(k.endswith("conv.1.weight") for k in P):
        return P
    rng = np.random.default_rng(7)
    Q = dict(P)
    for k, v in P.items():
        if _is_block_conv_bias(k, P):
            Q[O._next(k[:-5]) + ".weight"] = torch.from_numpy(rng.uniform(0.5, 1.5, v.shape).astype(np.float32))
            Q[O._next(k[:-5]) + ".bias"] = torch.from_numpy(rng.uniform(-0.2, 0.2, v.shape).astype(np.float32))
    return Q
