"""Host side of tests/test_gpu_product_ops.py: the elementwise comparator's own test (no kernel), and the same drivers and fp64
references on the host simulator at the in-step shapes divided by 8."""
import pytest
import torch

import product_ops as P
from test_emu_kernels import emu_ops  # noqa: F401  (fixture)


def _exact_output(g):
    """a level-2-sized fp64 'output' (2 M elements) and a conv-like per-element bound magnitude"""
    ref = P.activation(g, (1, 56, 56, 40, 16)).double() * 10
    cond = ref.abs() + 0.1 * float(ref.abs().mean())
    return ref, cond


def test_comparator_rejects_local_errors():
    """an fp64-exact output passes; one wrong corner voxel, one tile-seam plane off by 1e-4 relative, one interior 4x8x8 brick off by
    1e-3 each fail the elementwise bound -- while a rel-L2 bound of 1e-4 accepts the last two"""
    g = torch.Generator().manual_seed(11)
    ref, cond = _exact_output(g)
    assert P.check_elementwise(ref.clone(), ref, cond, P.TAU, "exact")[0] == 0.0
    assert P.check_elementwise(ref.float(), ref, cond, P.TAU, "fp32 rounding")[0] <= 2.0 ** -23 / P.TAU
    corner = ref.clone()
    corner[0, 0, 0, 0, 0] += 1e-2 * cond[0, 0, 0, 0, 0]
    seam = ref.clone()
    seam[:, 4] *= 1 + 1e-4                          # the plane d = 4: a 4x8x8 tile border
    brick = ref.clone()
    brick[:, 20:24, 24:32, 16:24] *= 1 + 1e-3       # one interior 4x8x8 tile
    for name, bad, loc in (("corner", corner, "face"), ("seam", seam, None), ("brick", brick, None)):
        with pytest.raises(AssertionError, match=name):
            P.check_elementwise(bad, ref, cond, P.TAU, name)
        r, k = P.elementwise_ratio(bad, ref, cond)
        assert r > P.TAU
        if loc:
            import numpy as np
            assert P.where(np.unravel_index(k, tuple(ref.shape)), tuple(ref.shape)) == loc, name
    for bad in (seam, brick):
        assert P.rel_l2(bad, ref) < 1e-4, "a rel-L2 1e-4 test accepts this error (that is the gap the elementwise bound closes)"


def test_conv3_cl64_matches_torch():
    g = torch.Generator().manual_seed(12)
    x = torch.randn(2, 5, 6, 7, 3, generator=g, dtype=torch.float64)
    w = torch.randn(4, 3, 3, 3, 3, generator=g, dtype=torch.float64)
    ref = torch.nn.functional.conv3d(x.permute(0, 4, 1, 2, 3), w, padding=1).permute(0, 2, 3, 4, 1)
    assert torch.allclose(P.conv3_cl64(x, w), ref, rtol=1e-12, atol=1e-12)
    w2 = torch.randn(4, 3, 3, 3, generator=g, dtype=torch.float64)
    x2 = x[:, :1]
    ref2 = torch.nn.functional.conv2d(x2[:, 0].permute(0, 3, 1, 2), w2, padding=1).permute(0, 2, 3, 1).unsqueeze(1)
    assert torch.allclose(P.conv3_cl64(x2, w2), ref2, rtol=1e-12, atol=1e-12)
    dy = torch.randn(2, 5, 6, 7, 4, generator=g, dtype=torch.float64)
    gw = torch.nn.grad.conv3d_weight(x.permute(0, 4, 1, 2, 3), w.shape, dy.permute(0, 4, 1, 2, 3), padding=1)
    assert torch.allclose(P.conv3_wgrad64(x, dy), gw, rtol=1e-12, atol=1e-10)


def _reduced_rows():
    seen, rows = set(), []
    for wl, k in P.driven_rows():
        rk = P.reduce_key(k)
        if (rk, wl if k[0].endswith("pack_many") else None) not in seen:        # (a pack row is its workload's network, whatever the key)
            seen.add((rk, wl if k[0].endswith("pack_many") else None))
            rows.append((wl, k, rk))
    return rows


# the LA rows (self-training, pre-training, validation; plain, residual and GroupNorm V-Net) run in the default CPU suite; the pancreas /
# ACDC / batch-8 rows (same drivers, other shapes; pancreasgn among them) with BCP_EXTENDED=1.
# At the reduced shapes the dispatch may differ from the in-step one: a conv3_fwd_raw row falls back to conv3_fwd where the shape is
# not served raw, and where a conv leaves no fused statistics (rows == 0) the fwd_stats / dgrad_bwdstats rows and the norm rows' "partial"
# epilogue run without them.  These rows check the drivers and references on the simulator; the route itself is asserted on the device
# (tests/test_gpu_product_ops.py: each row must launch its key, and the drivers require the fused routes there).
@pytest.mark.parametrize("wl,key,rkey", [pytest.param(*r, marks=() if r[0] in ("la", "la_pre", "la_val", "lares", "lares_pre", "lares_val", "lagn", "lagn_pre", "lagn_val") else pytest.mark.extended) for r in _reduced_rows()],
                         ids=[P.row_id(r[0], r[1]) for r in _reduced_rows()])
def test_product_op_reduced_on_simulator(emu_ops, wl, key, rkey):  # noqa: F811
    g = torch.Generator().manual_seed(5)
    P.run_row(emu_ops, torch.device("cpu"), wl, rkey, g, table_key=key)


# -------------------------------------------------------------------------------------------------- the new references' own tests


def test_k2_references_match_torch():
    """down64 / up64 / k2_wgrad64 against torch's fp64 conv3d(stride=2), conv_transpose3d and torch.nn.grad weight gradients"""
    F = torch.nn.functional
    g = torch.Generator().manual_seed(13)
    cf = lambda t: t.permute(0, 4, 1, 2, 3)          # noqa: E731  (channels-last -> NCDHW view)
    cl = lambda t: t.permute(0, 2, 3, 4, 1)          # noqa: E731
    x = torch.randn(2, 4, 6, 10, 3, generator=g, dtype=torch.float64)
    w = torch.randn(5, 3, 2, 2, 2, generator=g, dtype=torch.float64)
    y = cl(F.conv3d(cf(x), w, stride=2))
    assert torch.allclose(P.down64(x, w), y, rtol=1e-12, atol=1e-12)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    assert torch.allclose(P.up64(dy, w), cl(F.conv_transpose3d(cf(dy), w, stride=2)), rtol=1e-12, atol=1e-12)       # = the down conv's dgrad
    gw = torch.nn.grad.conv3d_weight(cf(x), w.shape, cf(dy), stride=2)
    assert torch.allclose(P.k2_wgrad64(x, dy, 0), gw, rtol=1e-12, atol=1e-12)
    # transposed conv: coarse xt [.., 5] -> fine [.., 3] with the weight [5, 3, 2, 2, 2]; its weight gradient is the twin conv's
    xt = torch.randn(2, 2, 3, 5, 5, generator=g, dtype=torch.float64)
    yt = cl(F.conv_transpose3d(cf(xt), w, stride=2))
    assert torch.allclose(P.up64(xt, w), yt, rtol=1e-12, atol=1e-12)
    dyt = torch.randn(yt.shape, generator=g, dtype=torch.float64)
    assert torch.allclose(P.down64(dyt, w), cl(F.conv3d(cf(dyt), w, stride=2)), rtol=1e-12, atol=1e-12)             # = the transposed conv's dgrad
    gwt = torch.nn.grad.conv3d_weight(cf(dyt), w.shape, cf(xt), stride=2)
    assert torch.allclose(P.k2_wgrad64(xt, dyt, 1), gwt, rtol=1e-12, atol=1e-12)
    # 1x1 conv on a D == 1 tensor
    x2 = torch.randn(3, 1, 4, 5, 6, generator=g, dtype=torch.float64)
    dy2 = torch.randn(3, 1, 4, 5, 7, generator=g, dtype=torch.float64)
    gw2 = torch.nn.grad.conv2d_weight(x2[:, 0].permute(0, 3, 1, 2), (7, 6, 1, 1), dy2[:, 0].permute(0, 3, 1, 2))
    assert torch.allclose(P.k2_wgrad64(x2, dy2, 2), gw2, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("flavour,ls", [(0, (4, 6, 8, 8, 2)), (1, (4, 1, 12, 12, 4))], ids=["la", "acdc"])
def test_mixloss_closed_form_matches_oracle_autograd(flavour, ls):
    """mixloss_pair64 (terms, total and d total / d logits in closed form) against fp64 autograd of the oracle's mix_loss_la /
    mix_loss_acdc, for both boxes of the drivers: <= 1e-12; and its cond bounds its gradient"""
    import bcp_oracle as O
    g = torch.Generator().manual_seed(3)
    sp, C = ls[1:4], ls[-1]
    N = ls[0] // 2
    w = ((1.0, 0.5), (0.5, 1.0))
    for box6 in P._boxes(sp, g):
        logits, labs = P._loss_inputs(g, ls, C)
        o, t, gr, cond = P.mixloss_pair64(logits, labs, box6, flavour, w)
        L = logits.double().requires_grad_(True)
        nc = L.permute(0, 4, 1, 2, 3)
        mask = (~P._in_box(sp, box6)).double().unsqueeze(0).expand(N, *sp)
        terms = []
        for h in range(2):
            xh = nc[h * N:(h + 1) * N]
            if flavour == 0:
                terms.append(O.mix_loss_la(xh, labs[h][0], labs[h][1], mask, l_weight=w[h][0], u_weight=w[h][1]))
            else:
                terms.append(O.mix_loss_acdc(xh[:, :, 0], labs[h][0][:, 0], labs[h][1][:, 0], mask[:, 0], l_weight=w[h][0], u_weight=w[h][1]))
        if flavour == 0:
            tot = terms[0] + terms[1]
            d = max(abs(float(terms[h].detach()) - float(o[h, 0])) for h in range(2))
        else:
            tot = ((terms[1][0] + terms[0][0]) + (terms[1][1] + terms[0][1])) / 2
            d = max(abs(float(terms[h][j].detach()) - float(o[h, j])) for h in range(2) for j in range(2))
        tot.backward()
        assert d <= 1e-12 and abs(float(tot.detach()) - float(t)) <= 1e-12, (box6, d)
        assert float((L.grad - gr).abs().max()) <= 1e-12 and P.elementwise_ratio(L.grad, gr, cond)[0] <= 1e-12, box6
        assert bool((cond >= gr.abs() * (1 - 1e-12)).all())


UNDRIVEN = {}        # {op: reason} -- ops of the table that are left without a driver on purpose (none)


def test_every_step_op_has_a_driver():
    """a new op in a step, a pre-training step or a validation pass cannot go undriven: every op of STEP_KEYS has a driver, every table
    row is driven under its own workload or is the repeat of a row driven under an earlier one (same key, same flags), and the only
    rows outside the table are the keys a statistics-only norm call uses"""
    assert sorted(P.STEP_KEYS) == sorted(["la", "pancreas", "acdc", "la_pre", "pancreas_pre", "acdc_pre", "la_val", "pancreas_val", "acdc_val", "la8",
                                          "lares", "lares_pre", "lares_val", "lagn", "lagn_pre", "lagn_val", "pancreasgn"])
    assert {k[0] for _, k in P.table_rows()} - set(UNDRIVEN) <= set(P.DRIVERS)
    rows = P.driven_rows()
    assert len(P.table_rows()) == 671 + 221 + 234 and len(set(rows)) == len(rows)    # (221: the three residual workloads, 234: the four GroupNorm ones)
    assert len([1 for wl, _ in P.table_rows() if not wl.startswith("lares") and not P.is_gn(wl)]) == 671
    assert [len(P.STEP_KEYS[wl]) for wl in ("lagn", "lagn_pre", "lagn_val", "pancreasgn")] == [63, 59, 49, 63]
    first = [(wl, k) for wl, k in P.table_rows() if wl in ("la", "pancreas", "acdc")]
    assert len(first) == 223 and set(first) <= set(rows)                      # (the self-training table is driven as before)
    driven = {P._row_ident(wl, k) for wl, k in rows}
    assert all(P._row_ident(wl, k) in driven for wl, k in P.table_rows() if k[0] not in UNDRIVEN)
    extra = [k for _, k in rows if (_, k) not in set(P.table_rows())]
    assert all(k[0] == "norm_fwd" for k in extra), extra
    for op in ("norm_fwd_res", "norm_bwd_res", "norm_eval_res", "axpy", "conv3_c1_fwd_stats", "conv3_c1_wgrad", "pw16_bwd"):      # the residual V-Net's
        assert any(k[0] == op and wl.startswith("lares") for wl, k in rows), op
    for op in ("gnorm_fwd", "gnorm_bwd", "pw16_bwd_norm", "pw16_fwd_norm", "conv3_dgrad_bwdstats", "k2_fwd_stats", "conv3_c1_fwd_stats"):      # the GroupNorm V-Nets'
        assert any(k[0] == op and P.is_gn(wl) for wl, k in rows), op
    gn_keys = {(wl, k) for wl, k in P.table_rows() if P.is_gn(wl) and k[0] in ("gnorm_fwd", "gnorm_bwd", "pw16_bwd_norm", "pw16_fwd_norm")}
    gn_driven = {P._row_ident(wl, k) for wl, k in rows if P.is_gn(wl)}     # (every GroupNorm launch a step records is driven under a GroupNorm workload)
    assert len(gn_keys) == 48 and all(P._row_ident(wl, k) in gn_driven for wl, k in gn_keys)
    for op in ("norm_eval", "sw_accumulate", "sw_finish", "overlap_counts", "plabel_argmax4", "mixloss_fwd", "mixloss_bwd", "conv3_c1_fwd", "pw16_fwd",
               "copy_channels"):
        assert any(k[0] == op for _, k in rows), op


def test_norm_eval_reference_matches_torch():
    """norm_eval_ref64 against F.batch_norm(training=False) + activation + residual in fp64; its cond bounds the result"""
    import numpy as np
    F = torch.nn.functional
    g = torch.Generator().manual_seed(14)
    y = torch.randn(2, 3, 4, 5, 8, generator=g, dtype=torch.float64) * 3 + 1
    gam, bet = torch.rand(8, generator=g, dtype=torch.float64) + 0.5, torch.rand(8, generator=g, dtype=torch.float64) - 0.5
    rm, rv = torch.randn(8, generator=g, dtype=torch.float64), torch.pow(10.0, torch.rand(8, generator=g, dtype=torch.float64) * 4 - 2)
    res = torch.randn(y.shape, generator=g, dtype=torch.float64)
    bn = F.batch_norm(y.permute(0, 4, 1, 2, 3), rm, rv, gam, bet, training=False, eps=float(np.float32(1e-5))).permute(0, 2, 3, 4, 1)
    for act, fn in ((1, torch.relu), (2, lambda t: F.leaky_relu(t, 0.01))):
        for r in (None, res):
            a, z, cond, zcond = P.norm_eval_ref64(y, gam, bet, rm, rv, act, r)
            assert torch.allclose(z, bn, rtol=1e-12, atol=1e-12)
            assert torch.allclose(a, fn(bn) + (0 if r is None else r), rtol=1e-12, atol=1e-12)
            assert bool((cond >= a.abs() * (1 - 1e-12)).all()) and bool((zcond >= z.abs() * (1 - 1e-12)).all())


def test_sliding_window_reference_matches_a_plain_loop():
    """sw_origins against the clamped grid written out, sw_ref against a voxel-by-voxel Python loop (math.exp, fp64)"""
    import math
    vol, patch = (5, 4, 7), (3, 4, 4)
    org = P.sw_origins(vol, patch, 2, 2)
    assert org == [(0, 0, 0), (0, 0, 2), (0, 0, 3), (2, 0, 0), (2, 0, 2), (2, 0, 3)]           # (z: 0, 2, then 4 clamped to 7 - 4)
    assert P.sw_origins((112, 112, 96), (112, 112, 80)) == [(0, 0, z) for z in (0, 4, 8, 12, 16)]
    assert len(P.sw_origins((96, 96, 112), (96, 96, 96))) == 5 and len(P.sw_origins((112, 112, 80), (112, 112, 80))) == 1
    g = torch.Generator().manual_seed(15)
    for C in (2, 4):
        logits = P._sw_logits(g, vol, patch, C, org)
        for cls in range(C):
            score = [[[0.0] * vol[2] for _ in range(vol[1])] for _ in range(vol[0])]
            cnt = [[[0] * vol[2] for _ in range(vol[1])] for _ in range(vol[0])]
            for lg, (x0, y0, z0) in zip(logits, org):
                for i in range(patch[0]):
                    for j in range(patch[1]):
                        for k in range(patch[2]):
                            e = [math.exp(float(v)) for v in lg[i, j, k]]
                            score[x0 + i][y0 + j][z0 + k] += e[cls] / sum(e)
                            cnt[x0 + i][y0 + j][z0 + k] += 1
            ref, rc = P.sw_ref(logits, org, vol, cls)
            assert torch.equal(rc, torch.tensor(cnt))
            assert torch.allclose(ref, torch.tensor(score, dtype=torch.float64) / torch.tensor(cnt, dtype=torch.float64), rtol=1e-13, atol=0)


@pytest.mark.parametrize("flavour,ls", [(0, (2, 6, 8, 8, 2)), (1, (3, 1, 12, 12, 4))], ids=["la", "acdc"])
def test_mixloss_single_closed_form_matches_oracle_autograd(flavour, ls):
    """mixloss64 as the pre-training steps use it -- LA: one label map, the all-zero box, weights (1, 0); ACDC: two label maps, a real
    box, weights (1, 1) -- against fp64 autograd of the oracle's mix_loss_la / mix_loss_acdc: <= 1e-12"""
    import bcp_oracle as O
    g = torch.Generator().manual_seed(4)
    sp, C, N = ls[1:4], ls[-1], ls[0]
    for box6, w, same in ([((0,) * 6, (1.0, 0.0), True)] if flavour == 0 else [(b, (1.0, 1.0), False) for b in P._boxes(sp, g)]):
        logits, labs = P._loss_inputs(g, (2 * N,) + tuple(ls[1:]), C)
        logits = logits[:N]
        img_l, patch_l = labs[0][0], labs[0][0] if same else labs[0][1]
        o3, gr, cond = P.mixloss64(logits, img_l, patch_l, box6, flavour, w)
        L = logits.double().requires_grad_(True)
        nc = L.permute(0, 4, 1, 2, 3)
        mask = (~P._in_box(sp, box6)).double().unsqueeze(0).expand(N, *sp)
        if flavour == 0:
            loss = O.mix_loss_la(nc, img_l, patch_l, mask, l_weight=w[0], u_weight=w[1])
            d = abs(float(loss.detach()) - float(o3[0]))
        else:
            dice, ce = O.mix_loss_acdc(nc[:, :, 0], img_l[:, 0], patch_l[:, 0], mask[:, 0], l_weight=w[0], u_weight=w[1])
            loss = (dice + ce) / 2
            d = max(abs(float(dice.detach()) - float(o3[0])), abs(float(ce.detach()) - float(o3[1])))
        loss.backward()
        assert d <= 1e-12, (box6, d)
        assert float((L.grad - gr).abs().max()) <= 1e-12 and P.elementwise_ratio(L.grad, gr, cond)[0] <= 1e-12, box6


# -------------------------------------------------------------------------------------------------- would the drivers notice?


class _Corrupt:
    """the simulator's ops with one op replaced by fn(orig, *args, **kw): a driver run on it must raise.  `pairs` keeps (clean, corrupted)
    results for the note on what a max-scaled close() or a rel-L2 1e-4 test would have said"""

    def __init__(self, ops, name, fn):
        self._ops, self._name, self._fn, self.pairs = ops, name, fn, []

    def __getattr__(self, n):
        v = getattr(self._ops, n)
        if n != self._name:
            return v
        return lambda *a, **k: self._fn(self, v, *a, **k)


def _first(r):
    return r if isinstance(r, torch.Tensor) else r[0]


def _scaled(sel, factor):
    """corruption: the op's (first) result with the elements sel(result) selects scaled by `factor` (0: zeroed)"""
    def fn(c, orig, *a, **k):
        r = orig(*a, **k)
        t = _first(r)
        clean = t.clone()
        sel(t).mul_(factor)
        c.pairs.append((clean, t.clone()))
        return r
    return fn


def _rerun(change):
    """corruption: the op run on changed arguments (change(args) -> args)"""
    def fn(c, orig, *a, **k):
        clean = _first(orig(*a, **k)).clone()
        r = orig(*change(list(a)), **k)
        c.pairs.append((clean, _first(r).clone()))
        return r
    return fn


def _drop_last_slab(i):
    def change(a):
        a[i] = torch.cat([a[i][:-1], torch.zeros_like(a[i][-1:])])
        return a
    return change


def _shift_box(a):
    b = list(a[2])
    b[2] += 1                                        # the box's w origin: two faces move by one voxel
    a[2] = tuple(b)
    return a


def _ragged_tail(t):
    rows = t.reshape(-1, t.shape[-1])
    return rows[(rows.shape[0] - 1) // 64 * 64:]


def _la_row(op, pick=0, wl="la"):
    return [(w, k) for w, k in P.table_rows() if w == wl and k[0] == op][pick]


def _smallest_variance_without_eps(a):
    rv = a[4].clone()
    rv[int(torch.argmin(rv))] -= 1e-5                # one channel: 1 / sqrt(rv) instead of 1 / sqrt(rv + eps)
    a[4] = rv
    return a


def _sw_last_origin_shifted(c, orig, lg, score, cnt, origin, cls=1):
    """the clamped last origin one voxel off along z (towards the volume: the run stays inside the maps)"""
    s0, c0 = score.clone(), cnt.clone()
    orig(lg, s0, c0, origin, cls=cls)
    bad = (origin[0], origin[1], origin[2] - 1) if origin[2] + lg.shape[2] == score.shape[2] and origin[2] > 0 else origin
    orig(lg, score, cnt, bad, cls=cls)
    if bad != origin:
        c.pairs.append((s0, score.clone()))


def _sw_visit_counted_twice(c, orig, lg, score, cnt, origin, cls=1):
    orig(lg, score, cnt, origin, cls=cls)
    if tuple(origin) == (0, 0, 0):
        clean = cnt.clone()
        cnt[:lg.shape[0], :lg.shape[1], :lg.shape[2]] += 1
        c.pairs.append((clean, cnt.clone()))


def _sw_finish_ge(c, orig, score, cnt, thres=0.5):
    lab = orig(score, cnt, thres)
    bad = (score >= thres).to(torch.uint8)
    c.pairs.append((lab.float(), bad.float()))
    return bad


def _overlap_tail_dropped(c, orig, pred, gt, cls=0):
    n = pred.numel() // 256 * 256
    clean = orig(pred, gt, cls)
    bad = orig(pred.reshape(-1)[:n].contiguous(), gt.reshape(-1)[:n].contiguous(), cls) if n else torch.zeros_like(clean)
    c.pairs.append((clean.float(), bad.float()))
    return bad


def _zero_box_as_full_volume(a):
    if not any(a[3]):
        a[3] = (0, 0, 0) + tuple(a[0].shape[1:4])
    return a


def _stale_amax(a):
    from bcp_amd import hip_ops as H
    x = a[0].clone()
    x._bcp_amax = H.amax_slots(float(x.abs().max()) / 4096, x.device)        # a |max| left over from a far smaller tensor
    a[0] = x
    return a


# case: (op of the LA row driven, op corrupted, corruption[, which of the op's rows[, its workload[, the divisor of the reduced shape]]]).  What the older comparators say of the same
# outputs at these reduced shapes (the test prints it): kernel_checks.close(), scaled by the tensor's largest element, accepts only the
# conv pack's changed word; a rel-L2 1e-4 test accepts the scaled first-layer channel (9.6e-5) and both pack words, and is within 4x of
# accepting every 1 + 2^-10 / 2^-12 scaling (1.2e-4 .. 6.7e-4).
SENSITIVITY = {
    "up-subposition": ("up_fwd", "up_fwd", _scaled(lambda t: t[:, 1::2, 0::2, 1::2], 1 + 2.0 ** -10), -1),
    "down-ragged-block": ("down_fwd", "down_fwd", _scaled(_ragged_tail, 0.0), -1),             # (2 x 7 x 7 x 5 = 490 rows: 7 blocks of 64 + 42)
    "wgrad-subposition": ("k2_wgrad", "k2_wgrad", _scaled(lambda t: t[:, :, 1, 0, 1], 1 + 2.0 ** -10)),
    "fwd-slab-dropped": ("norm_fwd_slabs", "norm_fwd_slabs", _rerun(_drop_last_slab(0))),
    "bwd-slab-dropped": ("norm_bwd_slabs", "norm_bwd_slabs", _rerun(_drop_last_slab(1))),
    "loss-class-gradient": ("mixloss_pair_bwd", "mixloss_pair_bwd", _scaled(lambda t: t[..., 1], 1 + 2.0 ** -12)),
    "box-face-shifted": ("mix_box", "mix_box", _rerun(_shift_box)),
    "c1-activation-channel": ("conv3_c1_norm_fwd", "conv3_c1_norm_fwd", _scaled(lambda t: t[..., 5], 1 + 2.0 ** -10)),
    # (the weight gradient's bound carries the log2(n) allowance for the norm backward's two means over every voxel: a 2^-10 scaling of a
    #  tap is inside it, a dropped tap -- a tap loop one short -- is not)
    "c1-wgrad-tap": ("conv3_c1_norm_bwd_wgrad", "conv3_c1_norm_bwd_wgrad", _scaled(lambda t: t[:, :, 0, 1, 2], 0.0)),
    "head-logit-class": ("pw16_fwd_norm", "pw16_fwd_norm", _scaled(lambda t: t[..., 1], 1 + 2.0 ** -10)),
    "head-gradient-channel": ("pw16_bwd_norm_bwd", "pw16_bwd_norm_bwd", _scaled(lambda t: t[..., 3], 1 + 2.0 ** -10)),
    "pack-one-word": ("conv3_pack_many", "conv3_pack", _scaled(lambda t: t[7:8], 1 + 2.0 ** -10)),
    "k2-pack-one-word": ("k2_pack_many", "k2_pack", _scaled(lambda t: t[7:8], 1 + 2.0 ** -10)),
    # the pre-training and validation rows (the LA workloads la_pre / la_val)
    "norm-eval-variance-without-eps": ("norm_eval", "norm_eval", _rerun(_smallest_variance_without_eps), 0, "la_val"),
    "sw-last-origin-off-by-one": ("sw_accumulate", "sw_accumulate", _sw_last_origin_shifted, 0, "la_val"),
    "sw-visit-counted-twice": ("sw_accumulate", "sw_accumulate", _sw_visit_counted_twice, 0, "la_val"),
    "sw-finish-greater-or-equal": ("sw_finish", "sw_finish", _sw_finish_ge, 0, "la_val"),
    "overlap-tail-dropped": ("overlap_counts", "overlap_counts", _overlap_tail_dropped, 0, "la_val"),
    "mixloss-zero-box-as-full-volume": ("mixloss_fwd", "mixloss_fwd", _rerun(_zero_box_as_full_volume), 0, "la_pre"),
    # (the row 1 x 28 x 28 x 20 x 64 at half its extents: the reduced shape at which the simulator's library has a two-plane fp16 instance)
    "conv-stale-amax": ("conv3_fwd", "conv3_fwd", _rerun(_stale_amax), 2, "la_val", 2),
}


@pytest.mark.parametrize("case", sorted(SENSITIVITY))
def test_driver_rejects_corruption(emu_ops, case):  # noqa: F811
    """each new driver, on the simulator at the reduced LA shape, with its op corrupted the way a real bug would: one (a, b, c)
    sub-position of a transposed conv scaled by 1 + 2^-10, the last ragged 64-row block of a down conv zeroed, one slab dropped from a
    slab sum, one class's loss gradient scaled by 1 + 2^-12, one box face shifted by a voxel, ... -- the driver must raise.  The printed
    note says whether kernel_checks.close() (max-scaled) or a rel-L2 1e-4 test would have accepted the same output."""
    import kernel_checks as K
    row_op, bad_op, fn, *pick = SENSITIVITY[case]
    wl, key = _la_row(row_op, *pick[:2])
    rkey = P.reduce_key(key, *pick[2:])
    g = torch.Generator().manual_seed(5)
    P.run_row(emu_ops, torch.device("cpu"), wl, rkey, g, table_key=key)                  # the clean op passes
    bad = _Corrupt(emu_ops, bad_op, fn)
    with pytest.raises(AssertionError):
        P.run_row(bad, torch.device("cpu"), wl, rkey, torch.Generator().manual_seed(5), table_key=key)
    assert bad.pairs, "the corrupted op was not called"
    clean, corrupt = bad.pairs[0]
    try:
        K.close(corrupt, clean)
        closes = True
    except AssertionError:
        closes = False
    print(f"[sensitivity] {case}: close() {'accepts' if closes else 'rejects'} it, rel-L2 {P.rel_l2(corrupt, clean):.2e} "
          f"({'accepted' if P.rel_l2(corrupt, clean) < 1e-4 else 'rejected'} at 1e-4)")


# -------------------------------------------------------------------------------------------------- can the residual drivers fail?
# (near-miss, the op of the residual row driven, its workload, the channel count of the row): the 16-channel rows carry every flag set --
# block_nine's channel scale, block_one's broadcast residual from conv3_c1_fwd_stats rows, two norm groups
RES_NEAR_MISSES = [("pattern_from_z", "norm_bwd_res", "lares"), ("residual_behind_activation", "norm_fwd_res", "lares"),
                   ("neighbour_chan_scale", "norm_fwd_res", "lares"), ("neighbour_chan_scale", "norm_bwd_res", "lares"),
                   ("bcast_row_off", "norm_fwd_res", "lares"), ("bcast_row_off", "norm_bwd_res", "lares"), ("bcast_row_off", "norm_eval_res", "lares_val"),
                   ("group_statistics_swapped", "norm_fwd_res", "lares"), ("dres_without_chan_scale", "norm_bwd_res", "lares"),
                   ("c1c2_from_z", "norm_bwd_res", "lares"), ("eval_batch_statistics", "norm_eval_res", "lares_val")]


def test_near_misses_cover_the_list():
    assert {n for n, _, _ in RES_NEAR_MISSES} == set(P.NEAR_MISSES)


@pytest.mark.parametrize("miss,op,wl", RES_NEAR_MISSES, ids=[f"{m}-{o}" for m, o, _ in RES_NEAR_MISSES])
def test_residual_driver_rejects_near_miss_reference(emu_ops, miss, op, wl):  # noqa: F811
    """each residual driver on the simulator at the reduced 16-channel shape of its workload: with the right fp64 reference every row
    passes; with a reference that is wrong the way a plausible kernel would be -- the ReLU pattern taken from z alone, relu(z) + r, the
    neighbouring sample's channel scale, the broadcast residual one row off, group 0 normalised with group 1's statistics, dres without the
    channel scale, the backward's two means from the z-only pattern, eval with batch statistics -- the same bound on the same inputs must
    reject the (correct) kernel output"""
    rows = [(w, k) for w, k in P.table_rows() if w == wl and k[0] == op and k[1][0][-1] == 16 and k[1][0][0] == 2 - (wl == "lares_val")]
    assert rows, (op, wl)
    n = 0
    for w, key in rows:                       # (norm_bwd_res has two 16-channel rows: the full and the broadcast residual)
        rkey = P.reduce_key(key)
        P.run_row(emu_ops, torch.device("cpu"), w, rkey, torch.Generator().manual_seed(5), table_key=key)
        P.NEAR_MISS, P.NEAR_MISS_HITS = miss, 0
        try:
            try:
                P.run_row(emu_ops, torch.device("cpu"), w, rkey, torch.Generator().manual_seed(5), table_key=key)
                assert P.NEAR_MISS_HITS == 0, f"{miss}: the near-miss reference was accepted at {rkey}"
            except AssertionError as e:
                assert P.NEAR_MISS_HITS > 0 and "accepted" not in str(e), e
                n += 1
        finally:
            P.NEAR_MISS = None
    assert n >= 1, f"{miss}: no {op} row applies it"


# -------------------------------------------------------------------------------------------------- can the GroupNorm drivers fail?
# (near-miss, the op of the GroupNorm row driven, its workload, the channel count of the row)
GN_NEAR_MISSES = [("gn_channel_statistics", "gnorm_fwd", "lagn", 32), ("gn_channel_statistics", "gnorm_bwd", "lagn", 32),
                  ("gn_channel_statistics", "conv3_dgrad_bwdstats", "lagn", 32),
                  ("gn_shifted_table", "gnorm_fwd", "lagn", 16), ("gn_shifted_table", "gnorm_bwd", "lagn", 16),
                  ("gn_shifted_table", "pw16_fwd_norm", "lagn", 16), ("gn_shifted_table", "pw16_bwd_norm", "lagn", 16),
                  ("gn_block_dropped", "gnorm_fwd", "lagn", 16), ("gn_block_dropped", "gnorm_bwd", "lagn", 32),
                  ("gn_row4_flipped", "gnorm_bwd", "lagn", 32)]


def test_gn_near_misses_cover_the_list():
    assert {n for n, _, _, _ in GN_NEAR_MISSES} == set(P.GN_NEAR_MISSES)


@pytest.mark.parametrize("miss,op,wl,C", GN_NEAR_MISSES, ids=[f"{m}-{o}" for m, o, _, _ in GN_NEAR_MISSES])
def test_gn_driver_rejects_near_miss_reference(emu_ops, miss, op, wl, C):  # noqa: F811
    """each GroupNorm driver on the simulator at the reduced shape of its row: with the right fp64 reference the row passes; with one that
    is wrong the way a plausible kernel would be -- every channel normalised with its own statistics, sample n with sample n - 1's table,
    one block of the statistics pass left out, row 4's sign flipped in the conv-bias gradient -- the driver's own bound on the driver's
    own inputs must reject the (correct) kernel output"""
    rows = [(w, k) for w, k in P.table_rows() if w == wl and k[0] == op and k[1][0][-1] == C]
    assert rows, (op, wl)
    n = 0
    for w, key in rows:
        rkey = P.reduce_key(key)
        P.run_row(emu_ops, torch.device("cpu"), w, rkey, torch.Generator().manual_seed(5), table_key=key)
        P.NEAR_MISS, P.NEAR_MISS_HITS = miss, 0
        try:
            try:
                P.run_row(emu_ops, torch.device("cpu"), w, rkey, torch.Generator().manual_seed(5), table_key=key)
                assert P.NEAR_MISS_HITS == 0, f"{miss}: the near-miss reference was accepted at {rkey}"
            except AssertionError as e:
                assert P.NEAR_MISS_HITS > 0 and "accepted" not in str(e), e
                n += 1
        finally:
            P.NEAR_MISS = None
    assert n >= 1, f"{miss}: no {op} row applies it"
