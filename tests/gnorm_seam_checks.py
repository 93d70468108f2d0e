"""Every producer -> GroupNorm seam of the V-Nets, elementwise against fp64.  Shared by tests/test_emu_gnorm_seams.py (host simulator) and
tests/test_gpu_gnorm_seams.py (-m gpu).

With normalization='groupnorm' the networks take the statistics of a norm layer from the epilogue of the launch that produced its input
wherever that launch offers them (networks/VNet.py: conv3_c1_fwd_stats, conv3_fwd_stats, k2_fwd_stats forward; conv3_dgrad_bwdstats
backward) and hand the partial rows to gnorm_fwd / gnorm_bwd with groups = N.  tests/gnorm_checks.py holds the kernels of csrc/gnorm.hip to
normwise bounds (max |diff| against rtol * max |ref|); here every element is held to the product-op table's bound

    |out - ref64| <= TAU * cond,    TAU = 2^-14,    cond = |gamma| (|xhat| + 1) + |beta|    (forward)

with the helpers of tests/product_ops.py (check_elementwise, _kink, _partials, _stats_check, _dgamma_dbeta_check).  Elements whose
pre-activation lies within 2^-18 of its condition of the ReLU kink are exempt, their terms are allowed in every sum that holds them, and a
case may have at most KINK_CAP of its elements there.

  A  check_finalize_rows     k_gnorm_finalize / k_gnorm_bwd_finalize fed host-made fp64 partial tables of 1 .. 980 rows (the product feeds
                             245 .. 980; the kernels' own passes leave 1 or 2 at test shapes): the table to one fp32 rounding of the fp64
                             formulas, dgamma / dbeta / the closed-form conv-bias gradient to their rounding counts
  B  check_fwd_seams         producer launch -> gnorm_fwd(partial=) -> apply, for every (producer, channels) pair the networks can fuse
  C  check_bwd_seams         conv3_dgrad_bwdstats (and, with the option on, the k2 dgrad epilogues) -> gnorm_bwd(partial=)
  D  check_head              gnorm_fwd(stats_only) -> pw16_fwd_norm / pw16_bwd_norm on a GroupNorm table
  E  check_own_pass_edges    1, 2, 3 rows per sample, N = 1, no activation, accumulate onto non-zero gradients, da with a common offset
  F  every one of A .. E evaluates near-miss fp64 variants (per-channel in place of per-group statistics, sample n reading sample n-1's
     table, the k2 term dropped from dy, row 4's sign flipped in the conv-bias gradient, a neighbour channel's scale) against the SAME
     bound and asserts that it rejects them: no bound here can be vacuous
  G  route_census            the network's planner (VNet.plan_forward / plan_backward, launch-free) for both V-Nets at the product shapes: every (producer, channels)
                             pair the product fuses has a case in B or C
  H  check_own_blocks        the kernels' OWN statistics passes at 2 .. 130 blocks per sample (A .. E leave 1 or 2): ragged last chunk, a
     check_apply_past_cap    block with one row, a block with none; reduce_partials' four-way walk and tail on kernel-made rows at N > 1;
                             the workspace layout partial | terms | coef with more than one row; the apply passes' unrolled trips and
                             remainder loops.  (a) elementwise against fp64 as B / C / E, ReLU and none, accumulate both ways; (b) the
                             scratch buffer filled with 0x7f bytes in front of both calls: every output keeps its bits; (c) sample 1 alone
                             changed: the other samples' a, table and dy keep their bits; (d) statistics that miss one whole block are
                             rejected by the same bound; (e) norm_apply_cap = 2 (one workgroup per sample: hundreds of unrolled trips, then
                             the remainder loop): bit for bit the default launch, and -- device only -- N = 4 at 52 x 52 x 50 x 16, a sample
                             longer than one unrolled trip of the library's own grid cap; (f) KINK_CAP on every reference.  The simulator
                             runs every case of OWN_BLOCK_CASES; check_apply_past_cap (8.7 M elements) is left to the device

Inputs: a per-channel offset of order 30 with spread ~1 (the group variance of a layer with several channels per group is then dominated
by the differences BETWEEN channels, and a channel reading its neighbour's statistics is off by whole units), per-channel scales, and
per-sample offsets AND scales that all differ (mean, rstd and row 4 of the table all differ between samples), N = 3 wherever the route
allows it, ReLU and no activation in every part.  A hands its calls tensors that are NOT the ones the partial rows were summed from (y +
100 forward, another da backward): there the route through partial_in is asserted by the result, not only by the row query.

The conv-bias gradient has two checks.  bias_chain: against the fp64 sum of the reference dy with TAU * cond, cond = sum_n r (|gamma| sum
|dz| + rows mean_g |gamma dz| + rows |dev r| mean_g |gamma dz xhat|) -- the errors the statistics partials may carry (TAU of their sum
|.|, as dgamma / dbeta) pushed through the closed form; it must reject row 4's sign flipped and sample n - 1's table.  bias_closed
(wherever the partial rows are visible: A, and the seam path of C): the closed form evaluated in fp64 FROM THE SAME partial sums, bound
2^-22 * cond_c, cond_c = sum_n r (|a1| + rows |k1| + rows |k2 dev r|): r enters the last term twice and dev once, each one fp32 rounding
(2^-24) of the fp64 value, and the final store is the fourth.  That bound counts the finalize's roundings only.  Held against the fp64
sum of the REFERENCE dy instead it is a measurement, not an assertion (printed: "against the fp64 sum of dy"): the statistics pass forms
xhat from the fp32 table, whose mean is off by up to 2^-24 |mean| for a whole (sample, group), so s2 = sum dz xhat carries ~2^-24 |mean| /
sigma of s1 -- at |mean| = 30, sigma = 1.4 and a da with a common offset (s1 does not cancel) that alone is ~3 x 2^-22 cond_c.  Measured,
simulator and MI355X alike: 0.55 .. 1.5 (C), 2.9 (E).  The same absolute error of xhat is why E's dgamma has one more term in its cond
(_dgamma_dbeta_edges); C keeps product_ops._dgamma_dbeta_check as it is.

Worst measured ratio to the bound, per seam (recorded, not tuned to; every test run prints its own as [gnorm-seam] lines).  The simulator's
figures; an MI355X gave the same to two digits except where a second figure stands behind "dev":
  A  table rows 0 .. 2   0.50 x 2^-23        row 4  0.49 x (2^-23 |row 4| + 2^-40 |mean|)
     dgamma / dbeta      0.50 x 2^-23        bias_closed  0.17 x 2^-22
  B  seam / own pass, x TAU:   c1 ->16  0.021 / 0.021     c3 ->16 .. 256  0.0033 .. 0.010 / the same
                               up ->16  0.35 / 0.025      up ->32  0.082 / 0.017      up ->128  0.021 / 0.0087
                               down ->32  0.19 / 0.011    down ->128  0.040 / 0.0049  down ->256  0.012 / 0.0039
     (the k2 epilogues' fp32 lane sums of y^2 under a bias of 30: ~15 x the own pass, inherent, and inside TAU)
     partials: conv3 / c1 4.8e-16 of sum |.| (bound 1e-12), k2 6.6e-8 (bound 1e-6)
  C  dy 0.0008 x TAU both paths (dev 0.0006); partials 0.012 x TAU; bias_chain 0.0002 x TAU; bias_closed 0.23 x 2^-22
  D  logits 0.011, dh 0.0016, dw 0.0013, db 0.00007 x TAU
  E  forward 0.28, dy 0.28, dgamma 0.46, dbeta 0.001, bias_chain 0.011 x TAU (worst: one or two rows per sample)
  B on the device only: up 32 -> 16 at coarse 16 x 32 x 32 (row blocks per workgroup R > 1) stays below the 0.35 of the small case.
  H  forward 0.024, dy 0.0018, bias_chain 0.0058 x TAU; bias against the fp64 sum of dy 2.3 x 2^-22 cond_c (measured only, as in E); past the
     apply cap (device) forward 0.030, dy 0.0019 x TAU; largest kink share 5.0e-6 (cap 1e-4).  One whole block left out of the statistics
     (measured on the fp64 reference alone): 3.6e-4 .. 6.9e-4 x cond at the three 129- / 130-block shapes, 5.1e-4 .. 4.7e-2 at the others,
     against TAU = 6.1e-5.  Leaving out only the one-row block of the 130-block shape is inside the bound (5.2e-5): (b) is what catches it.
"""
import numpy as np
import torch

import kernel_checks as K
import product_ops as PO
from bcp_amd import hip_ops as H
from product_ops import EPS, TAU, _acts, _dgamma_dbeta_check, _kink, _partials, _stats_check, check_elementwise, elementwise_ratio

GROUPS = 16
KINK_CAP = 1e-4                 # at most this share of a case's elements may lie at the activation's kink
TAU_PART_FP64 = 1e-12           # conv3_fwd_stats / conv3_c1_fwd_stats: fp64 lane sums of the stored y (product_ops.drive_conv's bound)
TAU_PART_K2 = 1e-6              # k2_fwd_stats: fp32 lane sums of <= 256 values, fp64 behind (kernel_checks._check_k2_stats' bound)
TAU_ROUND = 2.0 ** -23          # one fp32 rounding of an fp64 result, doubled
TAU_BIAS_CLOSED = 2.0 ** -22    # closed-form conv-bias gradient from given partial sums: four fp32 roundings (module docstring)
NB_CASES = (1, 31, 32, 33, 96, 97, 128, 129, 245, 490, 980)

WORST = {}                      # {seam: worst measured ratio / bound} of this process, printed by the tests


def _note(seam, r):
    WORST[seam] = max(WORST.get(seam, 0.0), float(r))
    return r


def report(target):
    for k in sorted(WORST):
        print(f"[gnorm-seam] {target}: {k}: worst {WORST[k]:.3g} x bound")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _uni(rng, lo, hi, n):
    return torch.from_numpy(rng.uniform(lo, hi, n).astype(np.float32))


# ------------------------------------------------------------------------------------------ fp64 references
def _group_mean(t, cg):
    """mean over the voxels and the cg adjacent channels of each group of a [N, n, C] tensor -> [N, 1, C] (repeated over a group)"""
    N, n, C = t.shape
    return t.reshape(N, n, GROUPS, cg).mean((1, 3)).repeat_interleave(cg, 1).unsqueeze(1)


def _stats64(y3, how="group"):
    """(mean, var) as [N, 1, C] of a [N, n, C] fp64 tensor.  how: 'group' -- nn.GroupNorm(16, C); the near-misses 'channel' (every
    channel its own statistics), 'shift' (sample n reads sample n - 1's) and ('drop', r0, r1) (rows r0 .. r1 - 1, one block of the
    statistics pass, left out of every sum and of the count)"""
    N, n, C = y3.shape
    cg = C // GROUPS
    if isinstance(how, tuple):
        yk = torch.cat((y3[:, :how[1]], y3[:, how[2]:]), 1)
        mu = _group_mean(yk, cg)
        return mu, _group_mean((yk - mu) ** 2, cg)
    if how == "channel":
        mu = y3.mean(1, keepdim=True)
        return mu, ((y3 - mu) ** 2).mean(1, keepdim=True)
    mu = _group_mean(y3, cg)
    var = _group_mean((y3 - mu) ** 2, cg)
    if how == "shift":
        mu, var = mu.roll(1, 0), var.roll(1, 0)
    return mu, var


def gn_ref64(y, gamma, beta, act, eps=EPS, how="group", stats=None):
    """fp64 nn.GroupNorm(16, C) + activation of a channels-last tensor [N, ..., C]: product_ops.norm_ref64 with groups of C / 16 adjacent
    channels per sample -> (a, z, xhat, mean_g [N, 16], var_g [N, 16], cond), cond = |gamma| (|xhat| + 1) + |beta|.  stats: (mean, var) as
    _stats64 returns them, in place of y's own (a caller that walks the samples one by one and wants a neighbour's)"""
    y = y.detach().double().cpu()
    N, C = y.shape[0], y.shape[-1]
    cg = C // GROUPS
    y3 = y.reshape(N, -1, C)
    mu, var = _stats64(y3, how) if stats is None else stats
    xh = ((y3 - mu) / torch.sqrt(var + eps)).reshape(y.shape)
    gm = torch.ones(C, dtype=torch.float64) if gamma is None else gamma.detach().double().cpu()
    bt = torch.zeros(C, dtype=torch.float64) if beta is None else beta.detach().double().cpu()
    z = gm * xh + bt
    a, _ = _acts(act, z)
    cond = gm.abs() * (xh.abs() + 1) + bt.abs()
    return a, z, xh, mu[:, 0, ::cg], var[:, 0, ::cg], cond


class BwdRef:
    """fp64 backward of gn_ref64 for the incoming gradient da64 * mult (product_ops._norm_bwd_ref64 for GroupNorm): dy, its cond (kappa =
    log2(cg * rows) on the two group means; inf at kink elements), the allowance a kink element's term has in every other element's
    group means, dz / xhat / dk as [N, n, C], and the conv-bias gradient with its chain cond and kink allowance"""

    def __init__(self, y, gamma, beta, act, da64, mult=None, how="group", drop_k2=False, eps=EPS, stats=None):
        ys = tuple(y.shape)
        N, C = ys[0], ys[-1]
        cg = C // GROUPS
        _, z, xh, _, _, fcond = gn_ref64(y, gamma, beta, act, eps, how, stats)
        y3 = y.detach().double().cpu().reshape(N, -1, C)
        rows = y3.shape[1]
        mu, var = _stats64(y3, how) if stats is None else stats
        rstd = 1.0 / torch.sqrt(var + eps)
        kink = _kink(z, fcond) if act else torch.zeros_like(z, dtype=torch.bool)      # (no activation: no branch to flip)
        _, dact = _acts(act, z)
        dam = da64.double() if mult is None else da64.double() * mult
        gm = gamma.detach().double().cpu()
        dz = (dam * dact).reshape(N, -1, C)
        xg = xh.reshape(N, -1, C)
        dk = (dam * kink).abs().reshape(N, -1, C)
        k1, k2 = _group_mean(gm * dz, cg), _group_mean(gm * dz * xg, cg)
        if drop_k2:
            k2 = torch.zeros_like(k2)
        dy = rstd * (gm * dz - k1 - xg * k2)
        kap = float(np.log2(cg * rows))
        a1, a2 = _group_mean((gm * dz).abs(), cg), _group_mean((gm * dz * xg).abs(), cg)
        cond = rstd * ((gm * dz).abs() + kap * (a1 + xg.abs() * a2))
        g1, g2 = _group_mean(gm.abs() * dk, cg), _group_mean(gm.abs() * dk * xg.abs(), cg)
        self.allow = (rstd * (g1 + xg.abs() * g2)).reshape(ys)
        self.dy = dy.reshape(ys)
        self.cond = torch.where(kink, torch.full_like(z, float("inf")), cond.reshape(ys))
        self.kink, self.dz, self.xg, self.dk = kink, dz, xg, dk
        self.rows, self.cg, self.gm = rows, cg, gm
        self.rstd, self.dev = rstd[:, 0], (y3.mean(1, keepdim=True) - mu)[:, 0]        # [N, C]: row 1 and row 4 of the table in fp64
        # conv-bias gradient: sum over samples and voxels of dy; what the statistics' errors may move it by (module docstring)
        self.dbias = dy.sum((0, 1))
        r, dv = self.rstd, self.dev
        self.dbias_cond = (r * (gm.abs() * dz.abs().sum(1) + rows * a1[:, 0] + rows * (dv * r).abs() * a2[:, 0])).sum(0)
        self.dbias_allow = (r * (gm.abs() * dk.sum(1) + rows * g1[:, 0] + rows * (dv * r).abs() * g2[:, 0])).sum(0)


def dbias_closed64(s1, s2, gm, r, dev, rows, flip=False):
    """k_gnorm_bwd_finalize's closed form in fp64 from per-(sample, channel) sums s1 = sum dz, s2 = sum dz xhat [N, C]:
    sum_n r (a1 - rows k1 - rows k2 dev r), a = gamma s, k = group means of a -> (value [C], cond_c [C]).  flip: row 4's sign flipped"""
    N, C = s1.shape
    cg = C // GROUPS
    a1, a2 = gm * s1, gm * s2
    k1 = a1.reshape(N, GROUPS, cg).sum(2).repeat_interleave(cg, 1) / (cg * rows)
    k2 = a2.reshape(N, GROUPS, cg).sum(2).repeat_interleave(cg, 1) / (cg * rows)
    t3 = rows * k2 * dev * r
    val = (r * (a1 - rows * k1 - (-t3 if flip else t3))).sum(0)
    return val, (r * (a1.abs() + rows * k1.abs() + t3.abs())).sum(0)


def _dgamma_dbeta_edges(tag, seam, dg, db, dg0, db0, ref, y):
    """product_ops._dgamma_dbeta_check with one more term in dgamma's cond, for the own-pass edges (E).  There a channel's dgamma can be
    ONE element's dz * xhat, and sum |dz xhat| does not bound what an fp32 table does to it: the statistics pass forms xhat = (y - mean) *
    rstd from the table's fp32 mean, off by up to 2^-24 |mean| for the whole (sample, group), so xhat carries an ABSOLUTE error of 2^-24
    |mean| rstd however small it is itself -- in units of TAU = 2^-14 that is 2^-10 |mean| rstd (0.016 at |mean| = 33, rstd = 0.5), the
    term added to |xhat| below.  Measured without it, C = 256 at one row per sample: 1.0002 x TAU, a channel whose only active element
    has |xhat| = 0.02.  dbeta has no xhat and keeps its cond."""
    N, C = y.shape[0], y.shape[-1]
    mu, _ = _stats64(y.detach().double().cpu().reshape(N, -1, C))
    xabs = ref.xg.abs() + 2.0 ** -10 * mu.abs() * ref.rstd.unsqueeze(1)
    for name, t, base, s_, c, k in (("dbeta", db, db0, ref.dz.sum((0, 1)), ref.dz.abs().sum((0, 1)), ref.dk.sum((0, 1))),
                                    ("dgamma", dg, dg0, (ref.dz * ref.xg).sum((0, 1)), (ref.dz.abs() * xabs).sum((0, 1)), (ref.dk * xabs).sum((0, 1)))):
        r = _ratio(t, base.double() + s_, base.double().abs() + c, k)
        assert r <= TAU, f"{tag}: {name} off by {r:.3e} x cond"
        _note(f"{seam} {name}", r / TAU)


def _ratio(out, ref, cond, allow=None):
    """worst |out - ref| (less `allow`) / cond"""
    err = (out.detach().double().cpu() - ref).abs()
    if allow is not None:
        err = (err - allow).clamp_min(0)
    return elementwise_ratio(err, torch.zeros_like(err), cond)[0]


def _kink_cap(tag, kink):
    n = int(kink.sum())
    assert n <= KINK_CAP * kink.numel(), f"{tag}: {n} of {kink.numel()} elements at the activation's kink (cap {KINK_CAP:g}): change the seed"
    return n


def _rejects(tag, what, r, tau=TAU):
    assert r > tau, f"{tag}: the bound accepts the near-miss '{what}' ({r:.3e} x cond, bound {tau:.3e}): it is vacuous here"


# ------------------------------------------------------------------------------------------ inputs
SAMPLE_OFF = (0.0, 1.7, -2.3, 3.1)
SAMPLE_SCALE = (1.0, 1.4, 0.7, 1.9)       # (rstd and row 4 of the table then differ between the samples too, not only the mean)


def _pre_norm(rng, N, sp, C):
    """a pre-norm tensor [N, *sp, C]: per-channel offset 30 + N(0, 1) and scale in [0.5, 1.5], a different offset per sample and a
    different scale per sample on everything but the common 30"""
    y = K.to_cl(K.R(rng, N, C, *sp)) * _uni(rng, 0.5, 1.5, C) + K.R(rng, C)
    return (y * torch.tensor(SAMPLE_SCALE[:N]).view(N, 1, 1, 1, 1) + 30.0 + torch.tensor(SAMPLE_OFF[:N]).view(N, 1, 1, 1, 1)).contiguous()


def _affine(rng, C):
    return _uni(rng, 0.5, 1.5, C), _uni(rng, -0.3, 0.3, C)


def _chan_scale(rng, N, C):
    return torch.from_numpy(((rng.random((N, C)) < 0.5) * 2.0).astype(np.float32))


def _mult(cs, shape):
    N, C = shape[0], shape[-1]
    return None if cs is None else cs.double().view(N, *([1] * (len(shape) - 2)), C).expand(shape)


# ------------------------------------------------------------------------------------------ shared checks
def _table_check(tag, st, y, gamma, beta, eps=EPS):
    """the table float[5][N][C] of a forward call against fp64: product_ops._stats_check on rows 0 / 1 (mean to TAU * sqrt(var), rstd
    relative), rows 0 / 1 constant over a group, row 2 = gamma * rstd to TAU, row 3 == beta bit for bit, row 4 = mean_c - mean_g"""
    st = st.detach().cpu()
    N, C = y.shape[0], y.shape[-1]
    cg = C // GROUPS
    y3 = y.detach().double().cpu().reshape(N, -1, C)
    mu, var = _stats64(y3, "group")
    _stats_check(st, mu, var, tag)
    for row in (0, 1):
        g = st[row].view(N, GROUPS, cg)
        assert torch.equal(_bits(g), _bits(g[:, :, :1].expand_as(g).contiguous())), f"{tag}: table row {row} must repeat over a group's channels"
    rs = 1.0 / torch.sqrt(var[:, 0] + eps)
    assert _ratio(st[2], gamma.double().cpu() * rs, (gamma.double().cpu() * rs).abs()) <= TAU, f"{tag}: table row 2 != gamma * rstd"
    assert torch.equal(_bits(st[3]), _bits(beta.cpu().expand(N, C).contiguous())), f"{tag}: table row 3 != beta"
    dev = (y3.mean(1) - mu[:, 0])
    r4 = _ratio(st[4], dev, var[:, 0].sqrt())
    assert r4 <= TAU, f"{tag}: table row 4 (mean_c - mean_g) off by {r4:.3e} x sqrt(var)"


def _fwd_check(ops, dev, tag, seam, y, gamma, beta, act, cs=None, res=None, partial=None, nb=0, nearmiss=True):
    """gnorm_fwd (statistics from `partial` or the kernel's own pass) + apply against fp64, elementwise; -> (a, table).  nearmiss: the
    bound must reject per-channel statistics (cg > 1), sample n - 1's table (N > 1) and the neighbour channel's scale / shift"""
    N, C = y.shape[0], y.shape[-1]
    cg = C // GROUPS
    yd, gd, bd = y.to(dev), gamma.to(dev), beta.to(dev)
    csd = None if cs is None else cs.to(dev)
    resd = None if res is None else res.to(dev)
    kw = dict(partial=partial, nb=nb) if partial is not None else {}
    a, st = ops.gnorm_fwd(yd, gd, bd, act, chan_scale=csd, residual=resd, **kw)
    _table_check(tag, st, y, gamma, beta)
    mult = _mult(cs, tuple(y.shape))
    r64 = 0.0 if res is None else res.double()

    def full(ar, cond):
        if mult is not None:
            ar, cond = ar * mult, cond * mult.abs()
        return ar + r64, cond + (0.0 if res is None else res.double().abs())
    ar, _, _, _, _, cond = gn_ref64(y, gamma, beta, act)
    ref, cnd = full(ar, cond)
    _note(seam, check_elementwise(a.cpu(), ref, cnd, TAU, tag)[0])
    assert H.amax_value(a._bcp_amax) == float(a.abs().max()), f"{tag}: |max| of a"
    if nearmiss:
        miss = []
        if cg > 1:
            miss.append(("per-channel statistics", gn_ref64(y, gamma, beta, act, how="channel")[0]))
        if N > 1:
            miss.append(("sample n - 1's table", gn_ref64(y, gamma, beta, act, how="shift")[0]))
        miss.append(("the neighbour channel's scale and shift", gn_ref64(y, gamma.roll(1), beta.roll(1), act)[0]))
        assert len(miss) >= 2 or (N == 1 and cg == 1), tag
        for what, am in miss:
            _rejects(tag, what, _ratio(full(am, cond)[0], ref, cnd))
    return a, st


def _grad_start(rng, C, accumulate, dev):
    """(dgamma, dbeta, dbias) before a backward call -> (the values the result adds to, the device buffers).  accumulate: non-zero
    starting values that differ per channel; otherwise the kernel must overwrite whatever the buffers held"""
    if accumulate:
        g0 = [torch.from_numpy((rng.standard_normal(C) * s + o).astype(np.float32)) for s, o in ((3.0, 1.0), (3.0, -2.0), (3.0, 0.5))]
    else:
        g0 = [torch.zeros(C) for _ in range(3)]
    return g0, [t.clone().to(dev) if accumulate else torch.full((C,), 7.0).to(dev) for t in g0]


def _bwd_check(ops, dev, tag, seam, y, gamma, beta, act, da, st, cs=None, partial=None, nb=0, accumulate=False, rng=None, nearmiss=True,
               ref=None, edges=False):
    """gnorm_bwd (backward statistics from `partial` or the kernel's own pass) against fp64: dy elementwise, dgamma / dbeta as
    product_ops._dgamma_dbeta_check, the conv-bias gradient (bias_chain; exact zeros for C = 16).  accumulate: onto non-zero starting
    values that differ per channel.  -> (dy, BwdRef, (dgamma, dbeta, dbias))"""
    N, C = y.shape[0], y.shape[-1]
    cg = C // GROUPS
    ref = BwdRef(y, gamma, beta, act, da.double().cpu(), _mult(cs, tuple(y.shape))) if ref is None else ref
    _kink_cap(tag, ref.kink)
    g0, gr = _grad_start(rng, C, accumulate, dev)
    csd = None if cs is None else cs.to(dev)
    kw = dict(partial=partial, nb=nb) if partial is not None else {}
    dy = ops.gnorm_bwd(y.to(dev), da.to(dev), st, gamma.to(dev), act, gr[0], gr[1], gr[2], accumulate, chan_scale=csd, **kw)
    r = _ratio(dy, ref.dy, ref.cond, ref.allow)
    assert r <= TAU, f"{tag}: dy off by {r:.3e} x cond (bound {TAU:.3e})"
    _note(seam + " dy", r / TAU)
    assert H.amax_value(dy._bcp_amax) == float(dy.abs().max()), f"{tag}: |max| of dy"
    if edges:
        _dgamma_dbeta_edges(tag, seam, gr[0], gr[1], g0[0], g0[1], ref, y)
    else:
        _dgamma_dbeta_check(tag, gr[0], gr[1], g0[0], g0[1], ref.dz, ref.xg, ref.dk)
    if cg == 1:      # one channel per group: exact zeros, as behind BatchNorm
        assert torch.equal(_bits(gr[2]), _bits(g0[2])), f"{tag}: the conv-bias gradient at C = 16 must stay exact zeros"
    else:
        rb = _ratio(gr[2], g0[2].double() + ref.dbias, g0[2].double().abs() + ref.dbias_cond, ref.dbias_allow)
        assert rb <= TAU, f"{tag}: conv-bias gradient off by {rb:.3e} x cond (bias_chain, bound {TAU:.3e})"
        _note(seam + " bias_chain", rb / TAU)
        # the same bound must reject the closed form with row 4's sign flipped and with sample n - 1's table (fp64, the reference's sums)
        s1, s2 = ref.dz.sum(1), (ref.dz * ref.xg).sum(1)
        miss = [("row 4's sign flipped", dbias_closed64(s1, s2, ref.gm, ref.rstd, ref.dev, ref.rows, flip=True)[0])]
        if N > 1:
            miss.append(("sample n - 1's table", dbias_closed64(s1, s2, ref.gm, ref.rstd.roll(1, 0), ref.dev.roll(1, 0), ref.rows)[0]))
        for what, vm in miss:
            _rejects(tag + " bias_chain", what, _ratio(g0[2].double() + vm, g0[2].double() + ref.dbias, g0[2].double().abs() + ref.dbias_cond, ref.dbias_allow))
        cc = dbias_closed64(s1, s2, ref.gm, ref.rstd, ref.dev, ref.rows)[1]
        rc = _ratio(gr[2], g0[2].double() + ref.dbias, g0[2].double().abs() + cc, ref.dbias_allow)
        print(f"[gnorm-seam] {tag}: conv-bias gradient against the fp64 sum of dy: {rc / TAU_BIAS_CLOSED:.3g} x 2^-22 cond_c")
        _note(seam + " bias vs fp64 dy (x 2^-22 cond_c, measured only)", rc / TAU_BIAS_CLOSED)
    if nearmiss:
        mult = _mult(cs, tuple(y.shape))
        miss = [("the k2 term dropped from dy", BwdRef(y, gamma, beta, act, da.double().cpu(), mult, drop_k2=True))]
        if N > 1:
            miss.append(("sample n - 1's table", BwdRef(y, gamma, beta, act, da.double().cpu(), mult, how="shift")))
        if cg > 1:
            miss.append(("per-channel statistics", BwdRef(y, gamma, beta, act, da.double().cpu(), mult, how="channel")))
        assert len(miss) >= 2 or (N == 1 and cg == 1), tag
        for what, m in miss:
            _rejects(tag, what, _ratio(m.dy, ref.dy, ref.cond, ref.allow))
    return dy, ref, gr


# ------------------------------------------------------------------------------------------ A. finalizes at product row counts
def _host_partials(v1, v2, nb):
    """fp64 partial table [N][nb][C][2] of per-row values v1, v2 [N, rows, C]: the rows cut into min(nb, rows) chunks, spread evenly over
    the nb slots; the other slots are zero rows"""
    N, rows, C = v1.shape
    nch = min(nb, rows)
    P = torch.zeros(N, nb, C, 2, dtype=torch.float64)
    bounds = np.linspace(0, rows, nch + 1).astype(int)
    for i in range(nch):
        b = (i * nb) // nch
        P[:, b, :, 0] = v1[:, bounds[i]:bounds[i + 1]].sum(1)
        P[:, b, :, 1] = v2[:, bounds[i]:bounds[i + 1]].sum(1)
    return P


def _table64(P, gm, bt, rows, eps=EPS, how="group"):
    """k_gnorm_finalize's formulas in fp64 from the partial table P [N, nb, C, 2] -> the five rows [5, N, C]"""
    S = P.sum(1)
    N, C = S.shape[:2]
    cg = C // GROUPS
    s1, s2 = S[..., 0], S[..., 1]
    if how == "channel":
        m, q = s1 / rows, s2 / rows
    else:
        m = s1.reshape(N, GROUPS, cg).sum(2).repeat_interleave(cg, 1) / (cg * rows)
        q = s2.reshape(N, GROUPS, cg).sum(2).repeat_interleave(cg, 1) / (cg * rows)
    r = 1.0 / torch.sqrt((q - m * m).clamp_min(0) + eps)
    if how == "shift":
        m, r = m.roll(1, 0), r.roll(1, 0)
    return torch.stack([m, r, gm * r, bt.expand(N, C), s1 / rows - m])


def _table_ratio(t, T):
    """worst error of table rows 0, 1, 2 in units of their own magnitude, and of row 4 in units of 2^-23 |row 4| + 2^-40 |mean|"""
    t = t.double()
    r012 = max(_ratio(t[i], T[i], T[i].abs()) for i in range(3))
    r4 = _ratio(t[4], T[4], TAU_ROUND * T[4].abs() + 2.0 ** -40 * T[0].abs())
    return r012, r4


def check_finalize_rows(ops, dev):
    """A.  N = 3, 105 rows per sample, all five group widths, every row count of NB_CASES (the 32-slot tree, its tail loop, the
    four-loads-in-flight loop of reduce_partials that runs only for nb > 96, and the product's 245 / 490 / 980)"""
    rng = np.random.default_rng(41)
    N, rows = 3, 105
    for C in (16, 32, 64, 128, 256):
        cg = C // GROUPS
        y = _pre_norm(rng, N, (rows, 1, 1), C).reshape(N, rows, C).contiguous()
        gamma, beta = _affine(rng, C)
        gm, bt = gamma.double(), beta.double()
        da = (K.R(rng, N, rows, C) + 5.0).contiguous()          # a common offset: the terms of the conv-bias gradient cancel
        yd, dad, gd, bd = y.to(dev), da.to(dev), gamma.to(dev), beta.to(dev)
        y64 = y.double()
        # the tensors the calls are handed beside the partial rows are NOT the ones the rows were summed from: a call that ignored
        # partial_in and made its own statistics pass would fail every assertion below
        y_poison = (y + 100.0).contiguous().to(dev)
        da_rows = (K.R(rng, N, rows, C) * 1.5 + 5.0).double()
        act = H.ACT_RELU
        for nb in NB_CASES:
            tag = f"finalize C={C} nb={nb}"
            P = _host_partials(y64, y64 * y64, nb)
            Pd = P.to(dev)
            none, st = ops.gnorm_fwd(y_poison, gd, bd, act, partial=Pd, nb=nb, stats_only=True)
            assert none is None
            t = st.cpu()
            T = _table64(P, gm, bt, rows)
            r012, r4 = _table_ratio(t, T)
            assert r012 <= TAU_ROUND, f"{tag}: table rows 0 .. 2 off by {r012:.3e} relative (bound 2^-23)"
            assert torch.equal(_bits(t[3]), _bits(beta.expand(N, C).contiguous())), f"{tag}: row 3 != beta"
            assert r4 <= 1.0, f"{tag}: row 4 off by {r4:.3e} x (2^-23 |row 4| + 2^-40 |mean|)"
            _note("A table rows 0-2 (x 2^-23)", r012 / TAU_ROUND)
            _note("A table row 4", r4)
            for row in (0, 1):
                g = t[row].view(N, GROUPS, cg)
                assert torch.equal(_bits(g), _bits(g[:, :, :1].expand_as(g).contiguous())), f"{tag}: row {row} must repeat over a group's channels"
            for n in range(N):      # sample n alone: the same bits
                _, s1 = ops.gnorm_fwd(y_poison[n:n + 1].contiguous(), gd, bd, act, partial=P[n:n + 1].contiguous().to(dev), nb=nb, stats_only=True)
                assert torch.equal(_bits(s1[:, 0]), _bits(st[:, n])), f"{tag}: the table of sample {n} depends on the other samples"
            # near-misses, rounded to fp32 as the kernel would have stored them
            miss = [("sample n - 1's table", _table64(P, gm, bt, rows, how="shift"))]
            if cg > 1:
                miss.append(("per-channel statistics", _table64(P, gm, bt, rows, how="channel")))
            Tn = T.clone()
            Tn[2] = T[2].roll(1, 1)
            miss.append(("the neighbour channel's scale", Tn))
            for what, Tm in miss:
                m012, m4 = _table_ratio(Tm.float(), T)
                _rejects(tag, what, max(m012 / TAU_ROUND, m4), 1.0)
            # ---- backward finalize: partials of dz and dz * xhat, xhat and the activation pattern from the fp32 table the kernel wrote
            t64 = t.double()
            xh = (y64 - t64[0].unsqueeze(1)) * t64[1].unsqueeze(1)
            z = (y64 - t64[0].unsqueeze(1)) * t64[2].unsqueeze(1) + t64[3].unsqueeze(1)
            for bact, accumulate in ((H.ACT_RELU, False), (H.ACT_RELU, True), (0, False), (0, True)):
                btag = f"{tag} act={bact} accumulate={accumulate}"
                dz = da_rows * (z > 0) if bact else da_rows          # (no activation: no pattern, dz = da)
                Pb = _host_partials(dz, dz * xh, nb)
                g0 = [torch.from_numpy((rng.standard_normal(C) * 50.0 + 10.0).astype(np.float32)) if accumulate else torch.zeros(C) for _ in range(3)]
                gr = [g.clone().to(dev) if accumulate else torch.full((C,), 7.0).to(dev) for g in g0]
                ops.gnorm_bwd(yd, dad, st, gd, bact, gr[0], gr[1], gr[2], accumulate, partial=Pb.to(dev), nb=nb)
                S = Pb.sum(1)
                for name, out, base, j in (("dbeta", gr[1], g0[1], 0), ("dgamma", gr[0], g0[0], 1)):
                    rr = _ratio(out, base.double() + S[..., j].sum(0), base.double().abs() + Pb[..., j].abs().sum((0, 1)))
                    assert rr <= TAU_ROUND, f"{btag}: {name} off by {rr:.3e} x sum|.| (bound 2^-23)"
                    _note("A dgamma / dbeta (x 2^-23)", rr / TAU_ROUND)
                if cg == 1:
                    assert torch.equal(_bits(gr[2]), _bits(g0[2])), f"{btag}: the conv-bias gradient at C = 16 must stay exact zeros"
                    continue
                val, cc = dbias_closed64(S[..., 0], S[..., 1], gm, T[1], T[4], rows)
                rb = _ratio(gr[2], g0[2].double() + val, g0[2].double().abs() + cc)
                assert rb <= TAU_BIAS_CLOSED, f"{btag}: conv-bias gradient off by {rb:.3e} x cond_c (bound 2^-22)"
                _note("A bias_closed (x 2^-22)", rb / TAU_BIAS_CLOSED)
                Ts = _table64(P, gm, bt, rows, how="shift")
                for what, vm in (("row 4's sign flipped", dbias_closed64(S[..., 0], S[..., 1], gm, T[1], T[4], rows, flip=True)[0]),
                                 ("sample n - 1's table", dbias_closed64(S[..., 0], S[..., 1], gm, Ts[1], Ts[4], rows)[0])):
                    _rejects(btag, what, _ratio(g0[2].double() + vm, g0[2].double() + val, g0[2].double().abs() + cc), TAU_BIAS_CLOSED)


# ------------------------------------------------------------------------------------------ B. forward seams
# (producer, N, Cin, Cout, spatial extents of the producer's INPUT, epilogues): every case must be served -- the row query is asserted
FWD_SEAMS = (
    ("up", 2, 32, 16, (4, 4, 4), ("plain", "res")),
    ("up", 3, 64, 32, (4, 4, 4), ("plain", "res")),
    ("up", 2, 256, 128, (4, 4, 4), ("res",)),
    ("down", 2, 16, 32, (8, 8, 8), ("plain",)),
    ("down", 2, 64, 128, (8, 8, 8), ("plain",)),
    ("down", 2, 128, 256, (8, 8, 8), ("plain",)),
    ("c1", 3, 1, 16, (3, 5, 7), ("plain",)),
    ("c3", 2, 16, 16, (6, 5, 9), ("plain", "cs")),
    ("c3", 3, 16, 16, (6, 5, 9), ("plain", "cs")),
    ("c3", 2, 32, 32, (8, 8, 8), ("plain",)),
    ("c3", 3, 32, 32, (8, 8, 8), ("plain",)),
    # from 64 channels on a conv this small runs split-K when it is handed a workspace, and split-K leaves no statistics: the networks
    # reach the fused route where the output exceeds the split-K limit (LA batch 8: no workspace).  Here the limit is set to 0 instead.
    ("c3-nows", 2, 64, 64, (8, 8, 4), ("plain",)),
    ("c3-nows", 3, 64, 64, (8, 8, 4), ("plain",)),
    ("c3-nows", 2, 128, 128, (4, 4, 2), ("plain",)),
    ("c3-nows", 3, 128, 128, (4, 4, 2), ("plain",)),
    ("c3-nows", 2, 256, 256, (2, 2, 1), ("plain", "cs")),
    ("c3-nows", 3, 256, 256, (2, 2, 1), ("cs",)),
)
FWD_SEAMS_GPU = (("up", 2, 32, 16, (16, 32, 32), ("res",)),)      # thousands of row blocks: stat_plan picks R > 1


def fwd_rows(ops, prod, xshape, Cout, G):
    """the row query of the producer's fused forward statistics (host only, launches nothing)"""
    if prod == "c1":
        return ops.conv3_c1_stat_rows(xshape, 3, G)
    if prod == "c3":
        return ops.conv3_stat_rows(xshape, Cout, 3, G)
    return ops.k2_stat_rows(0 if prod == "down" else 1, xshape, Cout, G)


def _produce(ops, dev, rng, prod, N, Cin, Cout, sp, tag, verify=True):
    """the producer's plain launch and its *_fwd_stats launch on one input, bias of order 30 per channel -> (y, partial, rows).  verify
    False (the product-op drivers, whose producer rows have checks of their own): the *_fwd_stats launch alone"""
    x = K.to_cl(K.R(rng, N, Cin, *sp)) * torch.tensor(SAMPLE_SCALE[:N]).view(N, 1, 1, 1, 1) + torch.tensor(SAMPLE_OFF[:N]).view(N, 1, 1, 1, 1)
    xd = PO._amax(H, x.contiguous().to(dev), dev)             # (the networks' operands carry their |max|)
    b = (K.R(rng, Cout) * 0.1 + 30.0 * (1.0 + 0.03 * K.R(rng, Cout))).to(dev)
    rows = fwd_rows(ops, prod, tuple(xd.shape), Cout, N)
    assert rows > 0, f"{tag}: the row query serves no fused statistics here ({rows}): the seam is not covered"
    if prod == "c1":
        w = (K.R(rng, 16, 1, 3, 3, 3) * 0.2).to(dev)
        y0 = ops.conv3_c1_fwd(xd, w, b, 3).clone() if verify else None
        y, part, nb = ops.conv3_c1_fwd_stats(xd, w, b, 3, N)
    elif prod == "c3":
        wf, _ = ops.conv3_pack((K.R(rng, Cout, Cin, 3, 3, 3) * 0.1).to(dev).contiguous(), 3)
        y0 = ops.conv3_fwd(xd, wf, b, Cout, 3).clone() if verify else None
        y, part, nb = ops.conv3_fwd_stats(xd, wf, b, Cout, 3, N)
    else:
        kind = 0 if prod == "down" else 1
        w = (K.R(rng, Cout, Cin, 2, 2, 2) if kind == 0 else K.R(rng, Cin, Cout, 2, 2, 2)) * 0.1
        bp = ops.k2_pack(w.to(dev), Cin, Cout, H.PACK_DOWN_FWD if kind == 0 else H.PACK_UP_FWD)
        y0 = (ops.down_fwd if kind == 0 else ops.up_fwd)(xd, bp, b, Cout).clone() if verify else None
        y, part, nb = ops.k2_fwd_stats(kind, xd, bp, b, Cout, N)
    assert nb == rows, (tag, nb, rows)
    if not verify:
        return y, part, rows
    assert torch.equal(_bits(y), _bits(y0)), f"{tag}: y differs from the plain launch"
    # the partial rows against fp64 sums of the kernel's own y, per (sample, channel)
    pt = _partials(part, N, rows, Cout)
    yg = y.cpu().double().reshape(N, -1, Cout)
    bound = TAU_PART_K2 if prod in ("up", "down") else TAU_PART_FP64
    for j, (s_, c) in enumerate(((yg.sum(1), yg.abs().sum(1)), ((yg * yg).sum(1), (yg * yg).sum(1)))):
        r = float(((pt[..., j] - s_).abs() / c.clamp_min(1e-300)).max())
        assert r <= bound, f"{tag}: fused statistics partial {j} off by {r:.3e} x sum|.| (bound {bound:.1e}, {rows} rows)"
        _note(f"B {prod} partials (x {bound:.0e})", r / bound)
    return y, part, rows


def check_fwd_seam(ops, dev, case):
    prod, N, Cin, Cout, sp, epis = case
    if prod == "c3-nows":
        ops.set_option("conv3_sk_elems", 0)
        try:
            assert ops._ws_bytes("bcp_conv3_fwd_workspace_bytes", N, *sp, Cin, Cout, 3) == 0
            return check_fwd_seam(ops, dev, ("c3",) + tuple(case[1:]))
        finally:
            ops.set_option("conv3_sk_elems")
    rng = np.random.default_rng(1000 + 7 * Cin + Cout + N)
    tag = f"{prod} {Cin}->{Cout} N={N} sp={sp}"
    y, part, rows = _produce(ops, dev, rng, prod, N, Cin, Cout, sp, tag)
    yc = y.cpu()
    gamma, beta = _affine(rng, Cout)
    seam = f"B {prod} ->{Cout}"
    variants = [(H.ACT_RELU, e) for e in epis] + [(0, "plain")]
    for act, epi in variants:
        cs = _chan_scale(rng, N, Cout) if epi == "cs" else None
        res = torch.from_numpy(rng.standard_normal(tuple(yc.shape), dtype=np.float32)) if epi == "res" else None
        t = f"{tag} act={act} {epi}"
        # (`part` stays valid across the variants: no launch in this loop writes the producer's statistics workspace)
        _fwd_check(ops, dev, t + " [producer's rows]", seam + " seam", yc, gamma, beta, act, cs, res, partial=part, nb=rows)
        _fwd_check(ops, dev, t + " [own pass]", seam + " own", yc, gamma, beta, act, cs, res, nearmiss=False)
    return rows


def check_fwd_seams(ops, dev, cases=FWD_SEAMS):
    ops.set_option("k2_stats", 1)       # (the product default, 2, keeps the k2 epilogues to outputs of >= 2^24 elements)
    try:
        for case in cases:
            check_fwd_seam(ops, dev, case)
    finally:
        ops.set_option("k2_stats")


# ------------------------------------------------------------------------------------------ C. backward seams
BWD_SEAMS = tuple(("c3", 2, C, C, sp, act) for C, sp in ((32, (8, 8, 8)), (64, (16, 16, 40))) for act in (H.ACT_RELU, 0))
# the k2 dgrad epilogues (option k2_bwd_stats, off in the product): (kind, N, Cin, Cout, dy extents); kind 0: dgrad of the down conv
# Cin -> Cout (dy coarse, the norm in front has Cin channels on the fine grid), 1: of the transposed conv (dy fine)
BWD_SEAMS_K2 = ((0, 2, 16, 32, (4, 8, 8)), (1, 2, 32, 16, (8, 16, 16)))


def bwd_rows(ops, prod, dyshape, Cin, G):
    if prod == "c3":
        return ops.conv3_bwdstat_rows(dyshape, Cin, 3, G)
    return ops.k2_bwdstat_rows(0 if prod == "down" else 1, dyshape, Cin, G)


def check_bwd_seam(ops, dev, prod, N, Cin, Cout, sp, act=H.ACT_RELU):
    """a dgrad launch whose epilogue leaves the backward statistics of the GroupNorm layer in front of it (Cin channels), then gnorm_bwd
    from those rows and from its own pass"""
    rng = np.random.default_rng(2000 + 3 * Cin + Cout + (0 if prod == "c3" else 50) + 500 * (act == 0))
    tag = f"{prod} dgrad {Cout}->{Cin} N={N} dy sp={sp} act={act}"
    dy = K.to_cl(K.R(rng, N, Cout, *sp)).contiguous().to(dev)
    rows = bwd_rows(ops, prod, tuple(dy.shape), Cin, N)
    assert rows > 0, f"{tag}: the row query serves no fused backward statistics here: the seam is not covered"
    osp = sp if prod == "c3" else (tuple(2 * e for e in sp) if prod == "down" else tuple(e // 2 for e in sp))
    yprev = _pre_norm(rng, N, osp, Cin)
    gamma, beta = _affine(rng, Cin)
    ypd, gd, bd = yprev.to(dev), gamma.to(dev), beta.to(dev)
    _, st = ops.gnorm_fwd(ypd, gd, bd, act)
    if prod == "c3":
        _, wd = ops.conv3_pack((K.R(rng, Cout, Cin, 3, 3, 3) * 0.1).to(dev).contiguous(), 3)
        da, part, nb = ops.conv3_dgrad_bwdstats(PO._amax(H, dy, dev), wd, Cin, 3, ypd, st, act, N)
    else:
        kind = 0 if prod == "down" else 1
        w = (K.R(rng, Cout, Cin, 2, 2, 2) if kind == 0 else K.R(rng, Cin, Cout, 2, 2, 2)) * 0.1
        bp = ops.k2_pack(w.to(dev), Cin, Cout, H.PACK_DOWN_DGRAD if kind == 0 else H.PACK_UP_DGRAD)
        d0 = (ops.down_dgrad if kind == 0 else ops.up_dgrad)(dy, bp, Cin).clone()
        da, part, nb = ops.k2_dgrad_bwdstats(kind, dy, bp, Cin, ypd, st, act, N)
        assert torch.equal(_bits(da), _bits(d0)), f"{tag}: da differs from the plain dgrad"
    assert nb == rows, (tag, nb, rows)
    dac = da.cpu()
    ref = BwdRef(yprev, gamma, beta, act, dac.double())
    _kink_cap(tag, ref.kink)
    # the epilogue's partial rows, as product_ops.drive_norm_bwd checks them: fp64 sums of the kernel's own da, less the kink allowance
    ps = _partials(part, N, rows, Cin)
    for j, (s_, c, k) in enumerate(((ref.dz.sum(1), ref.dz.abs().sum(1), ref.dk.sum(1)),
                                    ((ref.dz * ref.xg).sum(1), (ref.dz * ref.xg).abs().sum(1), (ref.dk * ref.xg.abs()).sum(1)))):
        r = _ratio(ps[..., j], s_, c, k)
        assert r <= TAU, f"{tag}: the dgrad epilogue's backward-statistics partial {j} off by {r:.3e} x sum|.|"
        _note(f"C {prod} {Cin} partials", r / TAU)
    seam = f"C {prod} {Cin}"
    _, _, gr = _bwd_check(ops, dev, tag + " [producer's rows]", seam + " seam", yprev, gamma, beta, act, dac, st, partial=part, nb=rows, ref=ref)
    if Cin > GROUPS:
        # bias_closed: the closed form in fp64 from the SAME partial sums the finalize read
        val, cc = dbias_closed64(ps[..., 0], ps[..., 1], ref.gm, ref.rstd, ref.dev, ref.rows)
        rb = _ratio(gr[2], val, cc)
        print(f"[gnorm-seam] {tag}: conv-bias gradient from the epilogue's rows {rb / TAU_BIAS_CLOSED:.3g} x 2^-22 cond_c")
        assert rb <= TAU_BIAS_CLOSED, f"{tag}: conv-bias gradient off by {rb:.3e} x cond_c from the epilogue's own partial sums (bound 2^-22)"
        _note(seam + " bias_closed (x 2^-22)", rb / TAU_BIAS_CLOSED)
        sh = BwdRef(yprev, gamma, beta, act, dac.double(), how="shift")
        for what, vm in (("row 4's sign flipped", dbias_closed64(ps[..., 0], ps[..., 1], ref.gm, ref.rstd, ref.dev, ref.rows, flip=True)[0]),
                         ("sample n - 1's table", dbias_closed64(ps[..., 0], ps[..., 1], ref.gm, sh.rstd, sh.dev, ref.rows)[0])):
            _rejects(tag, what, _ratio(vm, val, cc), TAU_BIAS_CLOSED)
    _bwd_check(ops, dev, tag + " [own pass]", seam + " own", yprev, gamma, beta, act, dac, st, nearmiss=False, ref=ref)
    return rows


def check_bwd_seams(ops, dev, cases=BWD_SEAMS):
    for prod, N, Cin, Cout, sp, act in cases:
        check_bwd_seam(ops, dev, prod, N, Cin, Cout, sp, act)


def check_bwd_seams_k2(ops, dev):
    ops.set_option("k2_bwd_stats", 1)
    try:
        for kind, N, Cin, Cout, sp in BWD_SEAMS_K2:
            for act in (H.ACT_RELU, 0):
                check_bwd_seam(ops, dev, "down" if kind == 0 else "up", N, Cin, Cout, sp, act)
    finally:
        ops.set_option("k2_bwd_stats")


# ------------------------------------------------------------------------------------------ D. the fused head on a GroupNorm table
def check_head(ops, dev):
    """gnorm_fwd(stats_only, chan_scale) at C = 16, N = 3 -> pw16_fwd_norm / pw16_bwd_norm with G = N: logits, the gradient w.r.t. the
    activation, the head's weight and bias gradients, with product_ops.drive_head's bounds"""
    for act in (H.ACT_RELU, 0):
        _check_head(ops, dev, act)


def _check_head(ops, dev, act):
    rng = np.random.default_rng(51 + act)
    N, C, Cout, sp = 3, 16, 2, (6, 5, 9)
    y = _pre_norm(rng, N, sp, C)
    gamma, beta = _affine(rng, C)
    cs = _chan_scale(rng, N, C)
    cs[:, 0], cs[:, 1] = torch.tensor([2.0, 0.0, 2.0]), torch.tensor([0.0, 2.0, 0.0])      # (samples differ whatever the draw)
    yd, csd = y.to(dev), cs.to(dev)
    tag = f"head N={N} sp={sp} act={act}"
    none, st = ops.gnorm_fwd(yd, gamma.to(dev), beta.to(dev), act, chan_scale=csd, stats_only=True)
    assert none is None
    _table_check(tag, st, y, gamma, beta)
    w = (K.R(rng, Cout, C, 1, 1, 1) * (2.0 / C) ** 0.5).contiguous()
    b = K.R(rng, Cout) * 0.1
    W = w.double().reshape(Cout, C)
    mult = _mult(cs, tuple(y.shape))
    ar, _, _, _, _, ncond = gn_ref64(y, gamma, beta, act)
    lg = ops.pw16_fwd_norm(yd, st, csd, N, act, w.to(dev), b.to(dev), Cout)
    ref, cond = (ar * mult) @ W.t() + b.double(), (ncond * mult) @ W.abs().t() + b.double().abs()
    _note("D head logits", check_elementwise(lg.cpu(), ref, cond, TAU, tag + " logits")[0])
    dl = K.to_cl(K.R(rng, N, Cout, *sp)).contiguous()
    d2 = dl.double().reshape(-1, Cout)
    dw0, db0 = K.R(rng, Cout, C, 1, 1, 1) * 0.5 + 1.0, K.R(rng, Cout) * 0.5 - 1.0
    dwd, dbd = dw0.clone().contiguous().to(dev), db0.clone().to(dev)
    dh = ops.pw16_bwd_norm(yd, st, csd, N, act, dl.to(dev), w.to(dev), dwd, dbd, accumulate=True)
    a2, c2 = (ar * mult).reshape(-1, C), (ncond * mult).reshape(-1, C)
    dwr, dwc = d2.t() @ a2 + dw0.double().reshape(Cout, C), d2.abs().t() @ c2 + dw0.double().abs().reshape(Cout, C)
    _note("D head dw", check_elementwise(dwd.cpu().reshape(Cout, C), dwr, dwc, TAU, tag + " dw")[0])
    _note("D head db", check_elementwise(dbd.cpu(), d2.sum(0) + db0.double(), d2.abs().sum(0) + db0.double().abs(), TAU, tag + " db")[0])
    _note("D head dh", check_elementwise(dh.cpu(), dl.double() @ W, dl.double().abs() @ W.abs(), TAU, tag + " dh")[0])
    # near-misses: sample n - 1's table, sample n - 1's channel scale, the neighbour channel's scale and shift
    multm = _mult(cs.roll(1, 0), tuple(y.shape))
    for what, am in (("sample n - 1's table", gn_ref64(y, gamma, beta, act, how="shift")[0] * mult),
                     ("sample n - 1's channel scale", ar * multm),
                     ("the neighbour channel's scale and shift", gn_ref64(y, gamma.roll(1), beta.roll(1), act)[0] * mult)):
        _rejects(tag + " logits", what, _ratio(am @ W.t() + b.double(), ref, cond))
        _rejects(tag + " dw", what, _ratio(d2.t() @ am.reshape(-1, C) + dw0.double().reshape(Cout, C), dwr, dwc))


# ------------------------------------------------------------------------------------------ E. edges of the kernels' own passes
def check_own_pass_edges(ops, dev):
    """rows per sample 1, 2, 3 at C = 256 and C = 16; N = 1; no activation; accumulate onto non-zero gradients that differ per channel;
    da with a common offset -- the elementwise bounds of B and C on the kernels' own statistics passes"""
    rng = np.random.default_rng(61)
    cases = [(3, C, (1, 1, r), act, False) for C in (256, 16) for r in (1, 2, 3) for act in (H.ACT_RELU,)]
    cases += [(3, 256, (1, 1, 2), 0, False), (3, 16, (1, 1, 3), 0, True)]
    cases += [(1, C, (3, 5, 7), act, acc) for C, act, acc in ((16, H.ACT_RELU, False), (64, 0, True), (256, H.ACT_RELU, True))]
    cases += [(3, C, (3, 5, 7), act, True) for C, act in ((32, H.ACT_RELU), (64, 0), (128, H.ACT_RELU))]
    for N, C, sp, act, cs_on in cases:
        tag = f"own pass N={N} C={C} sp={sp} act={act} cs={cs_on}"
        y = _pre_norm(rng, N, sp, C)
        gamma, beta = _affine(rng, C)
        cs = _chan_scale(rng, N, C) if cs_on else None
        nm = (C // GROUPS) * sp[0] * sp[1] * sp[2] > 1        # (one element per group: xhat = 0, a = act(beta) and dy = 0 whatever the table)
        _, st = _fwd_check(ops, dev, tag, "E own fwd", y, gamma, beta, act, cs, nearmiss=nm)
        da = (K.to_cl(K.R(rng, N, C, *sp)) + 5.0).contiguous()
        for accumulate in (False, True):
            _bwd_check(ops, dev, tag + f" accumulate={accumulate}", "E own bwd", y, gamma, beta, act, da, st, cs=cs, accumulate=accumulate, rng=rng, nearmiss=nm, edges=True)


# ------------------------------------------------------------------------------------------ H. the own passes at many blocks per sample
def own_geometry(rows, C):
    """the launch geometry of the kernels' own statistics passes, from csrc/norm.hip: norm_blocks = clamp(rows C / 16384, 1, 1024) blocks
    per sample, k_col_partial's chunk = ceil(rows / nb) rows per block -> (nb, chunk, rows of the ragged block behind the full ones or 0,
    trailing blocks without a row)"""
    nb = max(1, min(1024, rows * C // 16384))
    chunk = -(-rows // nb)
    full, last = divmod(rows, chunk)
    return nb, chunk, last, nb - full - (1 if last else 0)


def apply_blocks(rows, C, N, cap=2048):
    """apply_grid of csrc/norm.hip for one sample's rows C / 4 float4: 1024 float4 per block and unrolled trip, at most cap / N blocks"""
    return max(1, min(-(-(rows * (C // 4)) // 1024), max(1, cap // N)))


# (N, C, spatial extents, nb, rows of the ragged block, blocks without a row, also run with norm_apply_cap = 2): nb hits 2, 33, 97 (the
# 32-slot tree alone; its tail; ONE slot in the four-way loop of reduce_partials), 129 and 130 (every slot in the four-way loop, one / two
# slots in its tail), every width 16 .. 256.  rows = nb 16384 / C plus an odd remainder
OWN_BLOCK_CASES = (
    (3, 256, (1, 53, 157), 130, 1, 1, True),        # block 128 has exactly one row, block 129 none
    (2, 16, (1, 1, 132133), 129, 933, 0, True),
    (3, 64, (1, 7, 4733), 129, 235, 0, False),
    (2, 32, (1, 1, 1061), 2, 530, 0, False),
    (2, 32, (1, 3, 5645), 33, 487, 0, False),
    (2, 32, (1, 1, 49795), 97, 451, 0, False),
    (2, 128, (1, 1, 309), 2, 154, 0, False),
    (2, 128, (1, 11, 391), 33, 109, 0, False),
    (2, 128, (1, 5, 2503), 97, 35, 0, False),
)
# the simulator runs every case (the largest takes it about as long as its fp64 references take the host)
PAST_CAP_CASE = (4, 16, (52, 52, 50))       # device only: 8.7 M elements


class _Scratch:
    """ops whose gnorm_fwd / gnorm_bwd find the grow-only scratch buffer they are about to use filled with `byte`.  0x7f: every double of
    the partial rows, the terms and every float of the coefficients is finite and huge (1.4e306 / 3.4e38) -- a trailing block that leaves
    its row unwritten, or a finalize that reads past the rows of its sample, shows in every output"""

    def __init__(self, ops, byte):
        self.ops, self.byte = ops, byte

    def _fill(self, y):
        N, C = y.shape[0], y.shape[-1]
        nbytes = self.ops._ws_bytes("bcp_gnorm_workspace_bytes", N, y.numel() // (N * C), C)
        self.ops.workspace("gnorm", nbytes, y).fill_(self.byte)

    def gnorm_fwd(self, y, *a, **kw):
        self._fill(y)
        return self.ops.gnorm_fwd(y, *a, **kw)

    def gnorm_bwd(self, y, *a, **kw):
        self._fill(y)
        return self.ops.gnorm_bwd(y, *a, **kw)


def _amax_of(t):
    """the published |max| of a tensor (the slots between the strided values are not the kernels' to define)"""
    return torch.tensor([H.amax_value(t._bcp_amax)])


def _same_bits(tag, what, got, want):
    assert torch.equal(_bits(got), _bits(want)), f"{tag}: {what} changed its bits"


def _raw_step(ops, dev, y, da, gamma, beta, act, accumulate, cs=None):
    """gnorm_fwd + gnorm_bwd on their own passes, no reference -> every output, for the bit comparisons of H.  The gradients start from
    the values _bwd_check starts them from"""
    g0, gr = _grad_start(np.random.default_rng(72), y.shape[-1], accumulate, dev)
    yd, gd, csd = y.to(dev), gamma.to(dev), None if cs is None else cs.to(dev)
    a, st = ops.gnorm_fwd(yd, gd, beta.to(dev), act, chan_scale=csd)
    dy = ops.gnorm_bwd(yd, da.to(dev), st, gd, act, gr[0], gr[1], gr[2], accumulate, chan_scale=csd)
    return dict(a=a, table=st, a_amax=_amax_of(a), dy=dy, dy_amax=_amax_of(dy), dgamma=gr[0], dbeta=gr[1], dbias=gr[2])


def check_own_blocks(ops, dev, case):
    """H (a) .. (f) for one shape of OWN_BLOCK_CASES: no partial= anywhere, every row is the kernels' own"""
    N, C, sp, nb_x, last_x, empty_x, wrap = case
    rows = sp[0] * sp[1] * sp[2]
    nb, chunk, last, empty = own_geometry(rows, C)
    assert (nb, last, empty) == (nb_x, last_x, empty_x), (case, nb, chunk, last, empty)
    # the library sizes partial | terms | coef for this many rows per sample
    assert ops._ws_bytes("bcp_gnorm_workspace_bytes", N, rows, C) == (N * nb * C * 2 + 3 * N * C) * 8 + 2 * N * C * 4, case
    rng = np.random.default_rng(71)
    y = _pre_norm(rng, N, sp, C)
    gamma, beta = _affine(rng, C)
    da = (K.to_cl(K.R(rng, N, C, *sp)) + 5.0).contiguous()
    y1, da1 = y.clone(), da.clone()         # (c): sample 1 alone changed
    y1[1] = y[1].flip(0, 1, 2) * 1.25 - 3.0
    da1[1] = -da[1].flip(2)
    full = (rows // chunk)
    drops = (("block 0 left out of the statistics", ("drop", 0, chunk)),
             ("the last full block left out of the statistics", ("drop", (full - 1) * chunk, full * chunk)))
    zero, poison = _Scratch(ops, 0x00), _Scratch(ops, 0x7f)
    for act in (H.ACT_RELU, 0):
        tag = f"own blocks N={N} C={C} rows={rows} nb={nb} act={act}"
        nm = act != 0                       # (the near-misses of the shared checks once per shape: they are the references' cost)
        a, st = _fwd_check(zero, dev, tag, "H fwd", y, gamma, beta, act, nearmiss=nm)
        # (d) the same bound, the same inputs: statistics that miss one whole block
        ar, _, _, _, _, cond = gn_ref64(y, gamma, beta, act)
        for what, how in drops:
            r = _ratio(gn_ref64(y, gamma, beta, act, how=how)[0], ar, cond)
            _rejects(tag, what, r)
            print(f"[gnorm-seam] {tag}: {what}: {r:.3g} x cond (TAU {TAU:.3g})")
        del ar, cond
        ref = BwdRef(y, gamma, beta, act, da.double())
        print(f"[gnorm-seam] {tag}: kink share {float(ref.kink.sum()) / ref.kink.numel():.3g}")
        _note("H kink share (of KINK_CAP)", float(ref.kink.sum()) / ref.kink.numel() / KINK_CAP)
        for accumulate in (False, True):
            t = f"{tag} accumulate={accumulate}"
            dy, _, gr = _bwd_check(zero, dev, t, "H bwd", y, gamma, beta, act, da, st, accumulate=accumulate, rng=np.random.default_rng(72),
                                   nearmiss=nm and not accumulate, ref=ref)
            base = dict(a=a, table=st, a_amax=_amax_of(a), dy=dy, dy_amax=_amax_of(dy), dgamma=gr[0], dbeta=gr[1], dbias=gr[2])
            # (b) the scratch buffer full of 0x7f bytes in front of both calls
            for k, v in _raw_step(poison, dev, y, da, gamma, beta, act, accumulate).items():
                _same_bits(t + " [scratch poisoned]", k, v, base[k])
            # (e) the apply passes in one or two workgroups: hundreds of unrolled trips per thread, then the remainder loop
            if wrap:
                assert apply_blocks(rows, C, N) > 4 * apply_blocks(rows, C, N, 2), case
                ops.set_option("norm_apply_cap", "2")
                try:
                    wrapped = _raw_step(ops, dev, y, da, gamma, beta, act, accumulate)
                finally:
                    ops.set_option("norm_apply_cap", "")
                for k, v in wrapped.items():
                    _same_bits(t + " [norm_apply_cap = 2]", k, v, base[k])
        # (c) the other samples keep their bits when sample 1 changes
        other = _raw_step(ops, dev, y1, da1, gamma, beta, act, False)
        base = _raw_step(ops, dev, y, da, gamma, beta, act, False)
        assert not torch.equal(_bits(other["table"][:2, 1]), _bits(base["table"][:2, 1])), tag
        for n in range(N):
            if n != 1:
                _same_bits(tag + f" [sample 1 changed] sample {n}", "a", other["a"][n], base["a"][n])
                _same_bits(tag + f" [sample 1 changed] sample {n}", "table", other["table"][:, n], base["table"][:, n])
                _same_bits(tag + f" [sample 1 changed] sample {n}", "dy", other["dy"][n], base["dy"][n])


def check_apply_past_cap(ops, dev):
    """H (e), second half: a sample longer than one unrolled trip of the library's own grid cap.  N = 4: 2048 / 4 = 512 blocks, 512 * 256 * 4
    = 524 288 float4 per unrolled trip against 540 800 per sample -- every thread makes one unrolled trip, 16 512 of them one more in the
    remainder loop, in k_norm_apply and in k_gnorm_bwd_apply; 132 statistics blocks per sample, with a channel scale"""
    N, C, sp = PAST_CAP_CASE
    rows = sp[0] * sp[1] * sp[2]
    nv, grid = rows * (C // 4), apply_blocks(rows, C, N)
    assert grid == 2048 // N and 4 * grid * 256 < nv < 5 * grid * 256, (nv, grid)
    rng = np.random.default_rng(73)
    y = _pre_norm(rng, N, sp, C)
    gamma, beta = _affine(rng, C)
    cs = _chan_scale(rng, N, C)
    da = (K.to_cl(K.R(rng, N, C, *sp)) + 5.0).contiguous()
    for act, accumulate in ((H.ACT_RELU, False), (0, True)):
        tag = f"past the apply cap N={N} C={C} rows={rows} act={act} accumulate={accumulate}"
        _, st = _fwd_check(ops, dev, tag, "H past cap fwd", y, gamma, beta, act, cs, nearmiss=act != 0)
        _bwd_check(ops, dev, tag, "H past cap bwd", y, gamma, beta, act, da, st, cs=cs, accumulate=accumulate, rng=rng, nearmiss=False)


# ------------------------------------------------------------------------------------------ G. route census
CENSUS_SHAPES = {"la": ((2, 4), (112, 112, 80)), "la8": ((4, 8), (112, 112, 80)), "pancreas": ((2, 4), (96, 96, 96))}
# what the census finds at the product shapes with the product's options: (route, channels of the normalised tensor) -> rows per sample
# in the order la N=2, la N=4, la8 N=4, la8 N=8, pancreas N=2, pancreas N=4 (0: not fused there).  check_route_census asserts equality, so
# a route the product gains or loses changes this table, and with it the cases of B and C
CENSUS_ORDER = (("la", 2), ("la", 4), ("la8", 4), ("la8", 8), ("pancreas", 2), ("pancreas", 4))
CENSUS_EXPECT = {
    ("conv3_c1_fwd_stats", 16): (490, 490, 490, 490, 432, 432),
    ("conv3_fwd_stats", 16): (496, 512, 512, 512, 496, 512),
    ("conv3_fwd_stats", 32): (490, 490, 490, 490, 432, 432),
    ("conv3_fwd_stats", 64): (245, 245, 245, 245, 216, 216),
    ("conv3_fwd_stats", 128): (0, 0, 0, 31, 0, 0),
    ("up_fwd_stats", 16): (980, 980, 980, 980, 864, 864),
    ("up_fwd_stats", 32): (0, 0, 0, 980, 0, 0),
    ("down_fwd_stats", 32): (0, 0, 0, 980, 0, 0),
    ("conv3_dgrad_bwdstats", 32): (490, 490, 490, 490, 432, 432),
    ("conv3_dgrad_bwdstats", 64): (245, 245, 245, 245, 216, 216),
}


def covered_routes():
    """the (route, channels of the normalised tensor) pairs B and C drive"""
    fw = {({"up": "up_fwd_stats", "down": "down_fwd_stats", "c1": "conv3_c1_fwd_stats", "c3": "conv3_fwd_stats"}[c[0].partition("-")[0]], c[3]) for c in FWD_SEAMS}
    bw = {("conv3_dgrad_bwdstats", c[2]) for c in BWD_SEAMS}
    bw |= {("down_dgrad_bwdstats" if c[0] == 0 else "up_dgrad_bwdstats", c[2]) for c in BWD_SEAMS_K2}
    return fw | bw


def route_census(ops, verbose=True):
    """ask the network's own planner (networks/VNet.py plan_forward / plan_backward: shape queries of the library, no launch) for the routes
    of the GroupNorm V-Nets' training step at the product shapes -> {(route, C): {(workload, N): rows}} of the producers that leave
    statistics rows: a forward producer for its own norm (C = its output channels), a dgrad for the norm of the layer in front (its input
    channels)"""
    from bcp_amd.networks.VNet import VNet
    found = {}
    for wl, (Ns, sp0) in CENSUS_SHAPES.items():
        variant = "pancreas" if wl == "pancreas" else "la"
        net = VNet(n_channels=1, n_classes=2, normalization="groupnorm", has_dropout=variant == "la", variant=variant).set_ops(ops)
        for N in Ns:
            plan = net.plan_forward(N, *sp0, groups=1, save=True, training=True, dropout=net.has_dropout)
            for L, r, b in zip(net._layers, plan.layers, net.plan_backward(plan)[1]):
                k2 = {"dw": "down", "up": "up"}.get(L.kind)           # (Ops.k2_fwd_stats / k2_dgrad_bwdstats: one wrapper, two kernels)
                if r.rows > 0:
                    found.setdefault((k2 + "_fwd_stats" if k2 else r.producer, L.cout), {})[(wl, N)] = r.rows
                if b.rows > 0:
                    found.setdefault((k2 + "_dgrad_bwdstats" if k2 else b.dgrad, L.cin), {})[(wl, N)] = b.rows
    if verbose:
        for k in sorted(found):
            print(f"[gnorm-seam census] {k[0]} C={k[1]}: " + ", ".join(f"{wl} N={n}: {r}" for (wl, n), r in sorted(found[k].items())))
    return found


def check_route_census(ops):
    found = route_census(ops)
    missing = sorted(set(found) - covered_routes())
    assert not missing, f"the product fuses these (route, channels) pairs into a GroupNorm layer and no case of B / C drives them: {missing}"
    table = {k: tuple(v.get(c, 0) for c in CENSUS_ORDER) for k, v in found.items()}
    assert table == CENSUS_EXPECT, ("the fused routes of the product shapes changed: update CENSUS_EXPECT and the cases of B / C",
                                    {k: (table.get(k), CENSUS_EXPECT.get(k)) for k in set(table) | set(CENSUS_EXPECT) if table.get(k) != CENSUS_EXPECT.get(k)})
    return found
