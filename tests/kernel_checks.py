"""Per-kernel parity checks: every C-ABI entry point against the oracle / plain torch fp32 on the same
seeded inputs.  Shared by tests/test_emu_kernels.py (host simulator, CPU tensors; debugging aid for
the kernel logic) and tests/test_gpu_kernels.py (-m gpu: the real libbcp_hip.so on an MI355X).

Tolerances: integer / byte outputs bit-exact; fp32 outputs rtol 1e-4 (atol scaled to the tensor's
magnitude) -- different but equally valid fp32 summation orders; loss scalars 1e-5 (north_star)."""
import numpy as np
import torch
import torch.nn.functional as F

import bcp_oracle as O
from bcp_amd import hip_ops as H


def to_cl(x):
    """NCDHW / NCHW -> physical [N,D,H,W,C]"""
    if x.dim() == 4:
        x = x.unsqueeze(2)
    return x.permute(0, 2, 3, 4, 1).contiguous()


def from_cl(x, two_d=False):
    y = x.permute(0, 4, 1, 2, 3)
    return y.squeeze(2) if two_d else y


def close(a, b, rtol=1e-4, atol_scale=1e-5, msg=""):
    a = a.detach().cpu().double()
    b = b.detach().cpu().double()
    scale = max(float(b.abs().max()), 1e-30)
    err = float((a - b).abs().max())
    tol = atol_scale * scale + rtol * scale
    assert a.shape == b.shape, f"{msg}: shape {tuple(a.shape)} vs {tuple(b.shape)}"
    assert err <= tol, f"{msg}: max|diff| {err:.3e} > {tol:.3e} (ref max {scale:.3e})"


def rel_l2(a, b):
    a = a.detach().cpu().double().reshape(-1)
    b = b.detach().cpu().double().reshape(-1)
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def R(rng, *shape):
    return torch.from_numpy(rng.standard_normal(shape, dtype=np.float32))


# ----------------------------------------------------------------------------------------------
def check_mix_box(ops, dev):
    rng = np.random.default_rng(0)
    # (single-channel shapes take k_mix_box_c1 when W % 4 == 0: box edges off the float4 grid, boxes touching every border, an empty box,
    #  the whole volume, a row length that is not a power of two; W = 6 and C = 16 take the general kernel)
    for shape, box in (((2, 6, 8, 12, 1), (1, 2, 3, 4, 5, 6)), ((1, 1, 16, 16, 1), (0, 3, 4, 1, 10, 9)), ((2, 4, 4, 8, 16), (0, 0, 0, 2, 2, 4)),
                       ((2, 5, 7, 20, 1), (0, 0, 0, 5, 7, 20)), ((2, 5, 7, 20, 1), (4, 6, 17, 1, 1, 3)), ((1, 3, 9, 80, 1), (1, 2, 5, 2, 6, 70)),
                       ((3, 1, 32, 32, 1), (0, 9, 13, 1, 21, 18)), ((1, 2, 4, 8, 1), (0, 0, 0, 0, 0, 0)), ((1, 2, 3, 6, 2), (1, 1, 1, 1, 2, 3)),
                       ((2, 3, 5, 4, 1), (1, 1, 1, 2, 3, 2))):
        a, b = R(rng, *shape).to(dev), R(rng, *shape).to(dev)
        out = ops.mix_box(a, b, box)
        m = torch.ones(shape[1:4])
        m[box[0]:box[0] + box[3], box[1]:box[1] + box[4], box[2]:box[2] + box[5]] = 0
        m = m.view(1, *shape[1:4], 1)
        ref = a.cpu() * m + b.cpu() * (1 - m)
        assert torch.equal(out.cpu(), ref), "mix_box must be bit-exact"


def check_plabel(ops, dev, golden_dir):
    g = np.load(f"{golden_dir}/plabel_cc.npz")
    lo = torch.from_numpy(g["logits3d"])
    out = ops.plabel_bin(to_cl(lo).to(dev))
    ref = O.get_cut_mask(lo)
    diff = int((out.cpu().long() != ref).sum())
    assert diff <= 2, f"plabel_bin differs from the oracle in {diff} voxels (expf ulp ties only)"
    assert out[0, 0, 0, :4].tolist() == [1, 1, 1, 1], "exact tie p == 0.5 must give 1"
    lo2 = torch.from_numpy(g["logits2d"])
    out2 = ops.plabel_argmax4(to_cl(lo2).to(dev))
    assert int((out2.cpu()[:, 0].long() != O.get_acdc_argmax(lo2)).sum()) <= 2
    # first-max-wins on exact ties
    t = torch.zeros(1, 1, 1, 4, 4)
    t[0, 0, 0, 1] = torch.tensor([1., 1., 0., 0.])
    t[0, 0, 0, 2] = torch.tensor([0., 2., 2., 2.])
    assert ops.plabel_argmax4(t.to(dev)).cpu().view(-1).tolist() == [0, 0, 1, 0]


def check_cc(ops, dev, golden_dir):
    g = np.load(f"{golden_dir}/plabel_cc.npz")
    cut = torch.from_numpy(g["cut"])
    for conn, key in ((3, "cc26"), (2, "cc18"), (1, "cc6")):
        out, outf = ops.cc_largest(cut.to(dev).contiguous(), 1, conn, want_f32=True)
        assert np.array_equal(out.cpu().numpy(), g[key]), f"cc {key} must be bit-exact"
        assert np.array_equal(outf.cpu().numpy().astype(np.uint8), g[key])
    am = torch.from_numpy(g["argmax"]).unsqueeze(1).contiguous()  # [N,1,H,W]
    out = ops.cc_largest(am.to(dev), 3, 2)
    assert np.array_equal(out.cpu().numpy()[:, 0], g["argmax_cc"]), "ACDC per-class 8-conn CC must be bit-exact"
    # empty input passes through; tie between equal-size components -> first in raster order
    z = torch.zeros(1, 4, 4, 4, dtype=torch.uint8)
    assert int(ops.cc_largest(z.to(dev), 1, 3).sum()) == 0
    z[0, 0, 0, 0] = 1
    z[0, 3, 3, 3] = 1
    o = ops.cc_largest(z.to(dev), 1, 3).cpu()
    assert int(o[0, 0, 0, 0]) == 1 and int(o[0, 3, 3, 3]) == 0
    # random blobs vs the oracle
    rng = np.random.default_rng(3)
    seg = (F.avg_pool3d(R(rng, 2, 1, 20, 24, 28), 3, 1, 1)[:, 0] > 0.15).to(torch.uint8).contiguous()
    for conn, oc in ((3, None), (2, 2), (1, 1)):
        ref = O.largest_cc(seg.long(), oc)
        assert torch.equal(ops.cc_largest(seg.to(dev), 1, conn).cpu().float(), ref)
    # noise maps (what a random-init teacher emits): one percolating component chained through every tile + thousands of specks
    noise = torch.from_numpy((rng.random((2, 20, 40, 36)) < 0.5).astype(np.uint8))
    for conn, oc in ((3, None), (2, 2), (1, 1)):
        assert torch.equal(ops.cc_largest(noise.to(dev), 1, conn).cpu().float(), O.largest_cc(noise.long(), oc)), f"noise cc conn={conn}"
    # the big-tile variant (8x16x16 / 32x64 local tiles, chosen automatically for large volumes) must give the same answers
    ops.set_option("cc_tile", 2)
    try:
        for conn, oc in ((3, None), (1, 1)):
            assert torch.equal(ops.cc_largest(noise.to(dev), 1, conn).cpu().float(), O.largest_cc(noise.long(), oc)), f"big-tile noise cc conn={conn}"
        for conn, oc in ((3, None), (2, 2), (1, 1)):
            assert torch.equal(ops.cc_largest(seg.to(dev), 1, conn).cpu().float(), O.largest_cc(seg.long(), oc))
        for conn, key in ((3, "cc26"), (2, "cc18"), (1, "cc6")):
            assert np.array_equal(ops.cc_largest(cut.to(dev).contiguous(), 1, conn).cpu().numpy(), g[key]), f"big-tile cc {key}"
        assert np.array_equal(ops.cc_largest(am.to(dev), 3, 2).cpu().numpy()[:, 0], g["argmax_cc"])
    finally:
        ops.set_option("cc_tile")
    # (round 6) the two-launch count + select (cc_fuse_select = 0) against the fused kernel that everything above ran through
    # ... and the fused kernel with one atomic per tile-local root (cc_count_tile = 0) against the per-tile LDS table of the default
    for fuse, tile_tab in ((0, 0), (1, 0)):
        ops.set_option("cc_fuse_select", fuse)
        ops.set_option("cc_count_tile", tile_tab)
        try:
            for conn, key in ((3, "cc26"), (2, "cc18"), (1, "cc6")):
                assert np.array_equal(ops.cc_largest(cut.to(dev).contiguous(), 1, conn).cpu().numpy(), g[key]), f"select {fuse} / {tile_tab} cc {key}"
            assert np.array_equal(ops.cc_largest(am.to(dev), 3, 2).cpu().numpy()[:, 0], g["argmax_cc"])
            for conn, oc in ((3, None), (1, 1)):
                assert torch.equal(ops.cc_largest(noise.to(dev), 1, conn).cpu().float(), O.largest_cc(noise.long(), oc))
        finally:
            ops.set_option("cc_fuse_select")
            ops.set_option("cc_count_tile")
    # a checkerboard under 6-connectivity: every foreground voxel its own component (the most tile-local roots a tile can hold: half its
    # voxels -- the LDS table's worst case); the first voxel in raster order wins the tie
    cb = torch.zeros(1, 16, 32, 32, dtype=torch.uint8)
    idx = torch.arange(16).view(16, 1, 1) + torch.arange(32).view(1, 32, 1) + torch.arange(32).view(1, 1, 32)
    cb[0][(idx % 2) == 1] = 1
    for tile in (1, 2):
        ops.set_option("cc_tile", tile)
        try:
            o = ops.cc_largest(cb.to(dev), 1, 1).cpu()
        finally:
            ops.set_option("cc_tile")
        assert int(o.sum()) == 1 and int(o[0, 0, 0, 1]) == 1, f"checkerboard (tile option {tile}): {int(o.sum())} voxels kept"
    # (round 6) pseudo-label + largest-CC as one chain from the logits (bcp_plabel_cc_largest) == the two calls, bit for bit: the golden
    # logits (values at the threshold's expf ties included), noise logits (a random-init teacher), both tile sizes, 3-D two-channel and 2-D
    # four-channel
    rl = np.random.default_rng(5)
    cases2 = [to_cl(torch.from_numpy(g["logits3d"])).to(dev), to_cl(R(rl, 2, 2, 20, 40, 36)).to(dev), to_cl(R(rl, 1, 2, 9, 17, 20)).to(dev), to_cl(R(rl, 2, 2, 8, 10, 6)).to(dev)]      # (W = 6: the voxel-per-lane labelling; the others label quads)
    cases4 = [to_cl(torch.from_numpy(g["logits2d"]).unsqueeze(2)).to(dev), to_cl(R(rl, 3, 4, 1, 48, 80)).to(dev), to_cl(R(rl, 2, 4, 1, 33, 47)).to(dev)]
    for tile in (0, 2):
        ops.set_option("cc_tile", tile)
        try:
            for lg in cases2:
                for conn in (3, 2, 1):
                    seg = ops.plabel_bin(lg, 0.5)
                    (o2, f2), s2 = ops.plabel_cc_largest(lg, 0.5, conn, want_f32=True, want_seg=True)
                    o1, f1 = ops.cc_largest(seg, 1, conn, want_f32=True)
                    assert torch.equal(s2, seg) and torch.equal(o2, o1) and torch.equal(f2, f1), f"plabel + cc chain (2 channels, conn {conn}, tile {tile})"
            for lg in cases4:
                seg = ops.plabel_argmax4(lg)
                o2, s2 = ops.plabel_cc_largest(lg, 0.5, 2, want_seg=True)
                assert torch.equal(s2, seg) and torch.equal(o2, ops.cc_largest(seg, 3, 2)), f"plabel + cc chain (4 channels, tile {tile})"
        finally:
            ops.set_option("cc_tile")


def check_mixloss(ops, dev, golden_dir):
    g = np.load(f"{golden_dir}/mixloss_la.npz")
    lo = torch.from_numpy(g["logits"])
    a, b = torch.from_numpy(g["a"]), torch.from_numpy(g["b"])
    box = (2, 3, 1, 10, 10, 5)
    lcl = to_cl(lo).to(dev)
    a8, b8 = a.to(torch.uint8).to(dev), b.to(torch.uint8).to(dev)
    for key, (wi, wp) in (("1", (1.0, 0.5)), ("2", (0.5, 1.0))):
        out3, ws = ops.mixloss_fwd(lcl, a8, b8, box, H.LOSS_LA, wi, wp)
        assert abs(float(out3[0]) - float(g["l" + key])) < 1e-5, (float(out3[0]), float(g["l" + key]))
        dl = ops.mixloss_bwd(lcl, a8, b8, box, H.LOSS_LA, ws, 0.5, 0.5)
        close(from_cl(dl), torch.from_numpy(g["g" + key]), rtol=1e-4, msg="mixloss_la grad " + key)
        # explicit-mask path must agree with the box path
        m8 = torch.from_numpy(g["mask"]).to(torch.uint8).to(dev)
        out3m, wsm = ops.mixloss_fwd(lcl, a8, b8, (0, 0, 0, 0, 0, 0), H.LOSS_LA, wi, wp, mask=m8)
        assert abs(float(out3m[0]) - float(out3[0])) < 1e-7
    # supervised loss = empty box, weight 1 (LA_BCP_train.py:159-161)
    out3, ws = ops.mixloss_fwd(lcl, a8, a8, (0, 0, 0, 0, 0, 0), H.LOSS_LA, 1.0, 0.0)
    assert abs(float(out3[0]) - float(g["l3"])) < 1e-5
    dl = ops.mixloss_bwd(lcl, a8, a8, (0, 0, 0, 0, 0, 0), H.LOSS_LA, ws, 0.5, 0.5)
    close(from_cl(dl), torch.from_numpy(g["g3"]), rtol=1e-4, msg="sup loss grad")
    # round 4: the second call of a step sums the total on the device, in the reference's fp32 order (loss_l + loss_u); one upstream
    # gradient for both terms == the same value twice
    o1, _ = ops.mixloss_fwd(lcl, a8, b8, box, H.LOSS_LA, 1.0, 0.5)
    tot = torch.empty(1, dtype=torch.float32, device=dev)
    o2, ws2 = ops.mixloss_fwd(lcl, b8, a8, box, H.LOSS_LA, 0.5, 1.0, prev=o1, total=tot)
    assert float(tot[0]) == float((o1[0] + o2[0]).cpu()), "step total (LA)"
    gd = torch.tensor([0.37], dtype=torch.float32).to(dev)
    assert torch.equal(ops.mixloss_bwd(lcl, b8, a8, box, H.LOSS_LA, ws2, 0.5, 0.5, g_dev=gd),
                       ops.mixloss_bwd(lcl, b8, a8, box, H.LOSS_LA, ws2, 0.5, 0.5, g_dev=torch.cat([gd, gd])))

    g = np.load(f"{golden_dir}/mixloss_acdc.npz")
    lo = torch.from_numpy(g["logits"])
    a8, b8 = torch.from_numpy(g["a"]).to(torch.uint8).unsqueeze(1).contiguous().to(dev), torch.from_numpy(g["b"]).to(torch.uint8).unsqueeze(1).contiguous().to(dev)
    lcl = to_cl(lo).to(dev)
    box = (0, 4, 6, 1, 21, 21)
    for key, (wi, wp) in (("1", (0.5, 1.0)), ("2", (1.0, 0.5))):
        out3, ws = ops.mixloss_fwd(lcl, a8, b8, box, H.LOSS_ACDC, wi, wp)
        assert abs(float(out3[0]) - float(g["d" + key])) < 1e-5 and abs(float(out3[1]) - float(g["c" + key])) < 1e-5
        dl = ops.mixloss_bwd(lcl, a8, b8, box, H.LOSS_ACDC, ws, 0.5, 0.5)
        close(from_cl(dl, True), torch.from_numpy(g["g" + key]), rtol=1e-4, msg="mixloss_acdc grad " + key)
    o1, _ = ops.mixloss_fwd(lcl, a8, b8, box, H.LOSS_ACDC, 0.5, 1.0)
    tot = torch.empty(1, dtype=torch.float32, device=dev)
    o2, _ = ops.mixloss_fwd(lcl, b8, a8, box, H.LOSS_ACDC, 1.0, 0.5, prev=o1, total=tot)
    o1c, o2c = o1.cpu(), o2.cpu()
    assert float(tot[0]) == float(((o1c[0] + o2c[0]) + (o1c[1] + o2c[1])) / 2), "step total (ACDC): ((unl_dice + l_dice) + (unl_ce + l_ce)) / 2"
    # round 5: both calls of a step as ONE launch pair (bcp_mixloss_pair_fwd / _bwd) -- out3 of either call, the step's total and the
    # gradient BIT-identical to the two calls; both flavours, box and dense mask, several samples per call, a sample count whose
    # per-call blocks do not divide evenly
    rng = np.random.default_rng(47)
    for flavour, Cc, sp, N in ((H.LOSS_LA, 2, (12, 14, 10), 1), (H.LOSS_LA, 2, (9, 11, 7), 3), (H.LOSS_ACDC, 4, (1, 24, 28), 2), (H.LOSS_ACDC, 4, (1, 17, 19), 5)):
        lg = torch.from_numpy(rng.standard_normal((2 * N,) + sp + (Cc,), dtype=np.float32) * 2).to(dev)
        lab = [torch.from_numpy(rng.integers(0, Cc, (N,) + sp).astype(np.uint8)).to(dev) for _ in range(4)]
        bx = (0, 3, 2, 1, sp[1] // 2, sp[2] // 2) if sp[0] == 1 else (2, 3, 1, sp[0] // 2, sp[1] // 2, sp[2] // 2)
        for mask in (None, torch.from_numpy((rng.random((N,) + sp) < 0.6).astype(np.uint8)).to(dev)):
            box = bx if mask is None else (0, 0, 0, 0, 0, 0)
            w1, w2 = (1.0, 0.5), (0.5, 1.0)
            o1, ws1 = ops.mixloss_fwd(lg[:N], lab[0], lab[1], box, flavour, w1[0], w1[1], mask=mask)
            tot = torch.empty(1, dtype=torch.float32, device=dev)
            o2, ws2 = ops.mixloss_fwd(lg[N:], lab[2], lab[3], box, flavour, w2[0], w2[1], mask=mask, prev=o1, total=tot)
            gd = torch.tensor([0.83], dtype=torch.float32).to(dev)
            d_ref = torch.empty_like(lg)
            ops.mixloss_bwd(lg[:N], lab[0], lab[1], box, flavour, ws1, 0.5, 0.5, mask=mask, g_dev=gd, out=d_ref[:N])
            ops.mixloss_bwd(lg[N:], lab[2], lab[3], box, flavour, ws2, 0.5, 0.5, mask=mask, g_dev=gd, out=d_ref[N:])
            o6, tot2, wsp = ops.mixloss_pair_fwd(lg, lab[0], lab[1], lab[2], lab[3], box, flavour, w1, w2, mask=mask)
            d_pair = ops.mixloss_pair_bwd(lg, lab[0], lab[1], lab[2], lab[3], box, flavour, wsp, 0.5, 0.5, mask=mask, g_dev=gd)
            tag = f"mixloss pair flavour={flavour} {sp} N={N} mask={'dense' if mask is not None else 'box'}"
            assert torch.equal(o6[0].cpu(), o1.cpu()) and torch.equal(o6[1].cpu(), o2.cpu()), (tag, o6.cpu(), o1.cpu(), o2.cpu())
            assert torch.equal(tot2.cpu(), tot.cpu()), (tag, "total", float(tot2[0]), float(tot[0]))
            assert torch.equal(d_pair.cpu(), d_ref.cpu()), tag + ": gradient"
            assert float(d_pair.abs().max()) > 0 and float(tot2[0]) == float(tot2[0])
    # round 6: the box path takes a trip's voxels' term from ONE (d, h, w) decomposition when W is a multiple of the trip (forward: 4 voxels
    # at C = 2, 2 at C = 4; backward: one float4) -- against the dense mask of the same box (a byte per voxel, no arithmetic on indices):
    # the same bits, forward and backward; W = 6 / 9 take the per-voxel decomposition
    for flavour, Cc, sp in ((H.LOSS_LA, 2, (6, 10, 16)), (H.LOSS_LA, 2, (5, 7, 12)), (H.LOSS_LA, 2, (4, 6, 6)), (H.LOSS_ACDC, 4, (1, 20, 24)), (H.LOSS_ACDC, 4, (1, 11, 9))):
        N = 2
        lg = torch.from_numpy(rng.standard_normal((N,) + sp + (Cc,), dtype=np.float32) * 2).to(dev)
        la_, lb_ = [torch.from_numpy(rng.integers(0, Cc, (N,) + sp).astype(np.uint8)).to(dev) for _ in range(2)]
        bx = (0, 3, 2, 1, sp[1] // 2, sp[2] - 3) if sp[0] == 1 else (1, 2, 1, sp[0] // 2, sp[1] // 2, sp[2] - 2)
        m = torch.ones((N,) + sp, dtype=torch.uint8)
        m[:, bx[0]:bx[0] + bx[3], bx[1]:bx[1] + bx[4], bx[2]:bx[2] + bx[5]] = 0        # 1 = image term = OUTSIDE the box
        ob, wsb = ops.mixloss_fwd(lg, la_, lb_, bx, flavour, 1.0, 0.5)
        om, wsm = ops.mixloss_fwd(lg, la_, lb_, (0, 0, 0, 0, 0, 0), flavour, 1.0, 0.5, mask=m.to(dev))
        assert torch.equal(ob.cpu(), om.cpu()), f"mixloss box vs dense mask of the box, flavour {flavour} {sp}: {ob.cpu()} {om.cpu()}"
        db = ops.mixloss_bwd(lg, la_, lb_, bx, flavour, wsb, 0.5, 0.5)
        dm = ops.mixloss_bwd(lg, la_, lb_, (0, 0, 0, 0, 0, 0), flavour, wsm, 0.5, 0.5, mask=m.to(dev))
        assert torch.equal(db.cpu(), dm.cpu()), f"mixloss gradient box vs dense mask, flavour {flavour} {sp}"
    # a NaN logit must reach the loss (the two-channel softmax computes ONE exponential: of the sum of both differences to the maximum)
    lgn = torch.from_numpy(rng.standard_normal((2, 4, 6, 8, 2), dtype=np.float32)).to(dev)
    l8 = torch.zeros((2, 4, 6, 8), dtype=torch.uint8, device=dev)
    for ch in (0, 1):
        bad = lgn.clone()
        bad[1, 2, 3, 4, ch] = float("nan")
        o, _ = ops.mixloss_fwd(bad, l8, l8, (1, 1, 1, 2, 2, 2), H.LOSS_LA, 1.0, 0.5)
        assert float(o[0]) != float(o[0]), f"a NaN logit (channel {ch}) did not reach the loss"


def _acdc_mix_loss_body(dice_loss, output, img_l, patch_l, mask, l_weight=1.0, u_weight=0.5, unlab=False):
    """BCP's ACDC mixed loss, composed from the DiceLoss class under test (`dice_loss`) and a per-pixel cross-entropy: the image
    labels count where `mask` is 1, the patch labels where it is 0; the two regions are weighted (l_weight, u_weight), swapped for
    the unlabeled pair.  `mask` may be a dense tensor or a BCP_utils.BoxMask.  -> (Dice term, cross-entropy term)"""
    probs = torch.softmax(output, dim=1)
    w_in, w_out = (u_weight, l_weight) if unlab else (l_weight, u_weight)
    dice_term, ce_term = 0.0, 0.0
    for labels, region, wt in ((img_l, mask, w_in), (patch_l, 1 - mask, w_out)):
        labels = labels.long()
        dice_term = dice_term + wt * dice_loss(probs, labels.unsqueeze(1), region.unsqueeze(1))
        per_pixel = F.cross_entropy(output, labels, reduction="none")
        ce_term = ce_term + wt * (region * per_pixel).sum() / (region.sum() + 1e-16)
    return dice_term, ce_term


def check_diceloss_class(ops, dev, golden_dir):
    """SURVEY 8b seam `utils.losses.DiceLoss(n)(inputs, target, mask=None, weight=None, softmax=False)`: (1) BCP's
    ACDC mixed loss composed on top of it (_acdc_mix_loss_body) vs mixloss_acdc.npz (values 1e-5, gradient 1e-5 rel); (2) every keyword of
    the class vs diceloss_class.npz (the reference's class, oracle/make_golden_dice.py); (3) layouts: NCHW-contiguous,
    channels-last and BoxMask inputs give the same numbers."""
    from bcp_amd.utils import BCP_utils as BU
    from bcp_amd.utils import losses as L
    if dev.type == "cpu":
        BU.set_test_ops(ops)
    dice_loss = L.DiceLoss(4)
    g = np.load(f"{golden_dir}/mixloss_acdc.npz")
    a, b, mask = (torch.from_numpy(g[k]).to(dev) for k in ("a", "b", "mask"))
    for key, kw in (("1", dict(u_weight=0.5, unlab=True)), ("2", dict(u_weight=0.5))):
        for cl in (False, True):
            lo = torch.from_numpy(g["logits"]).to(dev)
            if cl:
                lo = lo.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)     # the networks' NHWC memory behind an NCHW shape
            lo.requires_grad_(True)
            d, c = _acdc_mix_loss_body(dice_loss, lo, a, b, mask, **kw)
            ((d + c) / 2).backward()
            d, c = float(d.detach()), float(c.detach())
            assert abs(d - float(g["d" + key])) < 1e-5 and abs(c - float(g["c" + key])) < 1e-5, (d, c)
            gr = torch.from_numpy(g["g" + key])
            assert rel_l2(lo.grad, gr) < 1e-5, rel_l2(lo.grad, gr)
            close(lo.grad, gr, rtol=1e-5, atol_scale=1e-6, msg="ACDC mix_loss body grad " + key)
    # ... and with this build's generate_mask (six integers instead of the reference's dense int64 masks) in the same body
    lo = torch.from_numpy(g["logits"]).to(dev).requires_grad_(True)
    bm = BU.BoxMask((4, 6, 21, 21), (32, 32), 2, False, dev)
    assert torch.equal(bm.tensor(dev), mask)
    d, c = _acdc_mix_loss_body(dice_loss, lo, a, b, bm, u_weight=0.5)
    ((d + c) / 2).backward()
    assert abs(float(d.detach()) - float(g["d2"])) < 1e-5 and abs(float(c.detach()) - float(g["c2"])) < 1e-5
    assert rel_l2(lo.grad, torch.from_numpy(g["g2"])) < 1e-5
    # the class alone, every keyword
    g = np.load(f"{golden_dir}/diceloss_class.npz")
    logits = torch.from_numpy(g["logits"]).to(dev)
    target, mask = torch.from_numpy(g["target"]).to(dev), torch.from_numpy(g["mask"]).to(dev)
    weight = [float(v) for v in g["weight"]]
    N, Cc, Hh, Ww = logits.shape
    bm = BU.BoxMask((5, 7, 11, 18), (Hh, Ww), N, False, dev)
    cases = (("masked", lambda p: dice_loss(p, target, mask), False),
             ("masked", lambda p: dice_loss(p, target, mask.float()), False),                  # float masks (dataset.py hands floats around)
             ("masked", lambda p: dice_loss(p, target, bm.unsqueeze(1)), False),               # six integers instead of a dense mask
             ("masked_c", lambda p: dice_loss(p, target, 1 - mask), False),
             ("masked_c", lambda p: dice_loss(p, target, (1 - bm).unsqueeze(1)), False),
             ("nomask", lambda p: dice_loss(p, target), False),
             ("nomask", lambda p: dice_loss(p, target[:, 0]), False),
             ("weighted", lambda p: dice_loss(p, target, mask, weight=weight), False),
             ("softmax", lambda x: dice_loss(x, target, mask, softmax=True), True))
    for name, fn, on_logits in cases:
        for cl in (False, True):
            leaf = logits if on_logits else torch.softmax(logits, dim=1)
            if cl:
                leaf = leaf.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
            leaf = leaf.detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
            v = fn(leaf)
            v.backward()
            assert abs(float(v.detach()) - float(g[name])) < 1e-5, (name, float(v.detach()), float(g[name]))
            gr = torch.from_numpy(g["g_" + name])
            assert rel_l2(leaf.grad, gr) < 1e-5, (name, cl, rel_l2(leaf.grad, gr))
    # a class absent from the target and (all but) from the prediction: the regime in which the smooth term decides -- 1e-10 in BOTH
    # branches of the reference (utils/losses.py:94, :105); with 1e-5 in the unmasked branch the value would be off by 0.25
    la, ta = torch.from_numpy(g["logits_abs"]).to(dev), torch.from_numpy(g["target_abs"]).to(dev)
    for name, fn in (("absent", lambda p: dice_loss(p, ta)), ("absent_masked", lambda p: dice_loss(p, ta, mask))):
        for cl in (False, True):
            leaf = torch.softmax(la, dim=1)
            if cl:
                leaf = leaf.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
            leaf = leaf.detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
            v = fn(leaf)
            v.backward()
            assert abs(float(v.detach()) - float(g[name])) < 1e-5, (name, float(v.detach()), float(g[name]))
            gr = torch.from_numpy(g["g_" + name])
            assert rel_l2(leaf.grad, gr) < 1e-5, (name, cl, rel_l2(leaf.grad, gr))
    with pytest_raises(AssertionError):
        dice_loss(torch.softmax(logits, 1)[:, :3], target)


class pytest_raises:
    def __init__(self, exc):
        self.exc = exc

    def __enter__(self):
        return self

    def __exit__(self, t, v, tb):
        assert t is not None and issubclass(t, self.exc), f"expected {self.exc.__name__}"
        return True


def check_norm(ops, dev):
    rng = np.random.default_rng(4)
    for (N, Cc, sp, act, use_cs, use_res, G) in ((2, 16, (4, 6, 8), H.ACT_RELU, True, True, 1), (1, 64, (2, 4, 4), H.ACT_RELU, False, False, 1),
                                                  (3, 32, (1, 8, 8), H.ACT_LRELU, False, False, 1), (2, 32, (4, 4, 4), H.ACT_RELU, False, False, 2),
                                                  (1, 256, (2, 2, 2), H.ACT_RELU, True, False, 1),
                                                  (2, 16, (7, 15, 21), H.ACT_RELU, True, True, 1),      # unrolled main loop + tails, 2 samples in 1 group
                                                  (4, 16, (5, 9, 12), H.ACT_LRELU, False, False, 4),
                                                  (1, 512, (1, 3, 5), H.ACT_RELU, False, False, 1)):   # InstanceNorm (G = N)
        y = (R(rng, N, Cc, *sp) * 1.7 + 0.4).requires_grad_(True)
        gamma = torch.from_numpy(rng.uniform(0.5, 1.5, Cc).astype(np.float32)).requires_grad_(True)
        beta = torch.from_numpy(rng.uniform(-0.3, 0.3, Cc).astype(np.float32)).requires_grad_(True)
        rm, rv = torch.zeros(Cc), torch.ones(Cc)
        cs = torch.from_numpy(((rng.random((N, Cc)) < 0.5) * 2.0).astype(np.float32)) if use_cs else None
        res = R(rng, N, Cc, *sp) if use_res else None
        em = torch.from_numpy((rng.random((N, Cc, *sp)) < 0.8).astype(np.uint8)) if act == H.ACT_LRELU else None
        # reference
        rm_ref, rv_ref = rm.clone(), rv.clone()
        if G == 1:
            z = F.batch_norm(y, rm_ref, rv_ref, gamma, beta, True, 0.1, 1e-5)
        else:
            z = F.instance_norm(y, eps=1e-5)
        a_ref = F.relu(z) if act == H.ACT_RELU else F.leaky_relu(z, 0.01)
        if cs is not None:
            a_ref = a_ref * cs.view(N, Cc, 1, 1, 1)
        if em is not None:
            a_ref = a_ref * em.float() / 0.8
        if res is not None:
            a_ref = a_ref + res
        da = R(rng, N, Cc, *sp)
        a_ref.backward(da)
        # HIP
        ycl = to_cl(y.detach()).to(dev)
        rmd, rvd = rm.clone().to(dev), rv.clone().to(dev)
        a, stats = ops.norm_fwd(ycl, G, gamma.detach().to(dev) if G == 1 else None, beta.detach().to(dev) if G == 1 else None,
                                rmd if G == 1 else None, rvd if G == 1 else None, act,
                                chan_scale=None if cs is None else cs.to(dev), elem_mask=None if em is None else to_cl(em).to(dev),
                                elem_scale=1 / 0.8, residual=None if res is None else to_cl(res).to(dev))
        close(from_cl(a), a_ref, msg=f"norm fwd C={Cc} G={G}")
        if G == 1:
            close(rmd, rm_ref, msg="running_mean")
            close(rvd, rv_ref, msg="running_var")
        dg, db = torch.full((Cc,), 7.0).to(dev), torch.full((Cc,), 7.0).to(dev)
        dy = ops.norm_bwd(ycl, to_cl(da).to(dev), G, stats, act, dg if G == 1 else None, db if G == 1 else None, False,
                          chan_scale=None if cs is None else cs.to(dev), elem_mask=None if em is None else to_cl(em).to(dev), elem_scale=1 / 0.8)
        close(from_cl(dy), y.grad, rtol=2e-4, msg=f"norm bwd dy C={Cc} G={G}")
        if G == 1:
            close(dg, gamma.grad, rtol=2e-4, msg="dgamma")
            close(db, beta.grad, rtol=2e-4, msg="dbeta")
            # accumulate
            ops.norm_bwd(ycl, to_cl(da).to(dev), G, stats, act, dg, db, True, chan_scale=None if cs is None else cs.to(dev),
                         elem_mask=None if em is None else to_cl(em).to(dev), elem_scale=1 / 0.8)
            close(dg, 2 * gamma.grad, rtol=2e-4, msg="dgamma accumulate")


def check_norm_grouped(ops, dev):
    """G groups WITH affine == G consecutive BatchNorm calls: statistics per group, running stats updated in order,
    parameter gradients summed over the groups"""
    rng = np.random.default_rng(14)
    N, Cc, sp, G = 4, 32, (3, 4, 5), 2
    y = (R(rng, N, Cc, *sp) * 1.3 - 0.2).requires_grad_(True)
    gamma = torch.from_numpy(rng.uniform(0.5, 1.5, Cc).astype(np.float32)).requires_grad_(True)
    beta = torch.from_numpy(rng.uniform(-0.3, 0.3, Cc).astype(np.float32)).requires_grad_(True)
    rm_ref, rv_ref = torch.zeros(Cc), torch.ones(Cc)
    outs = [F.relu(F.batch_norm(y[g * 2:(g + 1) * 2], rm_ref, rv_ref, gamma, beta, True, 0.1, 1e-5)) for g in range(G)]
    a_ref = torch.cat(outs)
    da = R(rng, N, Cc, *sp)
    a_ref.backward(da)
    rmd, rvd = torch.zeros(Cc).to(dev), torch.ones(Cc).to(dev)
    ycl = to_cl(y.detach()).to(dev)
    a, stats = ops.norm_fwd(ycl, G, gamma.detach().to(dev), beta.detach().to(dev), rmd, rvd, H.ACT_RELU)
    close(from_cl(a), a_ref, msg="grouped BN fwd")
    close(rmd, rm_ref, rtol=1e-5, msg="grouped running_mean (sequential update)")
    close(rvd, rv_ref, rtol=1e-5, msg="grouped running_var")
    dg, db = torch.zeros(Cc).to(dev), torch.zeros(Cc).to(dev)
    dy = ops.norm_bwd(ycl, to_cl(da).to(dev), G, stats, H.ACT_RELU, dg, db, False)
    close(from_cl(dy), y.grad, rtol=2e-4, msg="grouped BN dy")
    close(dg, gamma.grad, rtol=2e-4, msg="grouped dgamma")
    close(db, beta.grad, rtol=2e-4, msg="grouped dbeta")


CONV3_CASES = (
    # (N, Cin, Cout, spatial, KD)
    (1, 16, 16, (4, 4, 16), 3),       # exactly one 4x4x16 tile
    (1, 16, 16, (5, 6, 18), 3),       # partial tiles
    (2, 32, 32, (4, 8, 8), 3),
    (1, 64, 64, (4, 4, 4), 3),
    (1, 32, 16, (6, 5, 7), 3),        # Cin != Cout, odd dims
    (1, 128, 128, (3, 3, 2), 3),      # deep level, tiny spatial (resident weights + split-K over cin chunks)
    (2, 128, 144, (6, 14, 5), 3),     # deep level: several 64-voxel tiles per persistent workgroup, partial tiles, 4 chunk groups
    (1, 256, 128, (7, 7, 5), 3),      # 16 cin chunks -> 8 chunk groups
    (2, 64, 64, (14, 14, 10), 3),     # LA level 4 extent: tile (2,16,2) for fwd, (2,8,4) for wgrad
    (1, 32, 48, (7, 7, 5), 3),        # LA level 5 extent: tile (8,8,1)
    (2, 16, 16, (1, 16, 16), 1),      # 2-D
    (1, 32, 64, (1, 9, 11), 1),
    (1, 16, 4, (1, 8, 8), 1),         # U-Net out_conv: Cout = 4 (padded to 16 inside)
)


def check_conv3(ops, dev, cases=CONV3_CASES):
    rng = np.random.default_rng(5)
    for (N, Cin, Cout, sp, KD) in cases:
        two_d = KD == 1
        ksz = (3, 3) if two_d else (3, 3, 3)
        xs = sp[1:] if two_d else sp
        x = R(rng, N, Cin, *xs).requires_grad_(True)
        w = (R(rng, Cout, Cin, *ksz) * 0.1).requires_grad_(True)
        b = R(rng, Cout) * 0.1
        y_ref = (F.conv2d(x, w, b, padding=1) if two_d else F.conv3d(x, w, b, padding=1))
        dy = R(rng, *y_ref.shape)
        y_ref.backward(dy)
        tag = f"conv3 N={N} {Cin}->{Cout} {sp} KD={KD}"
        wf, wd = ops.conv3_pack(w.detach().to(dev).contiguous(), KD)
        xcl = to_cl(x.detach()).to(dev)
        y = ops.conv3_fwd(xcl, wf, b.to(dev), Cout, KD)
        close(from_cl(y, two_d), y_ref, msg=tag + " fwd")
        dycl = to_cl(dy).to(dev)
        if Cout % 4 == 0 and Cout >= 4:
            dx = ops.conv3_fwd(dycl, wd, None, Cin, KD)
            close(from_cl(dx, two_d), x.grad, msg=tag + " dgrad")
            # accumulate flag
            dx2 = ops.conv3_fwd(dycl, wd, None, Cin, KD, out=dx.clone(), accumulate=True)
            close(from_cl(dx2, two_d), 2 * x.grad, msg=tag + " dgrad accumulate")
        dw = torch.full(w.shape, 3.0).to(dev)
        ops.conv3_wgrad(xcl, dycl, dw, KD, accumulate=False)
        close(dw, w.grad, rtol=2e-4, msg=tag + " wgrad")
        ops.conv3_wgrad(xcl, dycl, dw, KD, accumulate=True)
        close(dw, 2 * w.grad, rtol=2e-4, msg=tag + " wgrad accumulate")


def check_pack_many(ops, dev):
    """all layers of a net in one launch == the single-layer packer, bit for bit (fwd and dgrad flavours, padded channel counts)"""
    import struct
    rng = np.random.default_rng(11)
    layers = [(16, 16, 3), (32, 16, 3), (48, 64, 3), (4, 16, 1), (32, 2, 1), (16, 20, 3)]       # (Cout, Cin, KD)
    ws, outs, desc = [], [], b""
    for Cout, Cin, KD in layers:
        w = R(rng, Cout, Cin, *((3, 3) if KD == 1 else (3, 3, 3))).to(dev).contiguous()
        K16, N16 = (Cin + 15) // 16 * 16, (Cout + 15) // 16 * 16
        n = ops.conv3_packed_floats(Cin, Cout, KD)      # fp32 pack + the three-piece bf16 pack behind it
        wf = torch.full((n,), 7.0, dtype=torch.float32, device=dev)
        wd = torch.full((n,), 7.0, dtype=torch.float32, device=dev)
        desc += struct.pack("<QQiiiiii", w.data_ptr(), wf.data_ptr(), Cout, Cin, KD * 9, K16, N16, 0)
        desc += struct.pack("<QQiiiiii", w.data_ptr(), wd.data_ptr(), Cout, Cin, KD * 9, N16, K16, 1)
        ws.append((w, KD)); outs.append((wf, wd))
    d = torch.frombuffer(bytearray(desc), dtype=torch.uint8).to(dev)
    ops.conv3_pack_many(d, 2 * len(layers))
    for (w, KD), (wf, wd) in zip(ws, outs):
        rf, rd = ops.conv3_pack(w, KD)
        assert torch.equal(wf.cpu(), rf.flatten().cpu()), f"pack_many fwd {tuple(w.shape)}"
        assert torch.equal(wd.cpu(), rd.flatten().cpu()), f"pack_many dgrad {tuple(w.shape)}"


def check_conv3_c1(ops, dev):
    rng = np.random.default_rng(6)
    for (N, sp, KD) in ((1, (5, 6, 18), 3), (2, (4, 4, 16), 3), (2, (1, 17, 20), 1)):
        two_d = KD == 1
        ksz = (3, 3) if two_d else (3, 3, 3)
        xs = sp[1:] if two_d else sp
        x = R(rng, N, 1, *xs)
        w = (R(rng, 16, 1, *ksz) * 0.2).requires_grad_(True)
        b = R(rng, 16) * 0.1
        y_ref = (F.conv2d(x, w, b, padding=1) if two_d else F.conv3d(x, w, b, padding=1))
        dy = R(rng, *y_ref.shape)
        y_ref.backward(dy)
        xcl = to_cl(x).to(dev)
        y = ops.conv3_c1_fwd(xcl, w.detach().to(dev).contiguous(), b.to(dev), KD)
        close(from_cl(y, two_d), y_ref, msg=f"conv3_c1 fwd {sp}")
        dw = torch.zeros(w.shape).to(dev)
        ops.conv3_c1_wgrad(xcl, to_cl(dy).to(dev), dw, KD)
        close(dw, w.grad, rtol=2e-4, msg=f"conv3_c1 wgrad {sp}")
    # fused norm statistics (bcp_conv3_c1_fwd_stats): y bit-identical to the plain launch; the partial rows sum to the per-group column
    # sums / sums of squares; several tiles per workgroup (32 / 16 tiles per group -> 8 / 4 per workgroup), ragged tiles, 2-D
    for (N, sp, KD, G) in ((2, (16, 16, 64), 3, 2), (4, (8, 16, 32), 3, 2), (2, (6, 5, 21), 3, 2), (1, (6, 5, 21), 3, 1), (4, (1, 40, 48), 1, 2)):
        two_d = KD == 1
        x = R(rng, N, 1, *(sp[1:] if two_d else sp))
        w = R(rng, 16, 1, *((3, 3) if two_d else (3, 3, 3))) * 0.2
        b = R(rng, 16) * 0.1
        xcl = to_cl(x).to(dev)
        y0 = ops.conv3_c1_fwd(xcl, w.to(dev).contiguous(), b.to(dev), KD)
        y, part, rows = ops.conv3_c1_fwd_stats(xcl, w.to(dev).contiguous(), b.to(dev), KD, G)
        assert rows > 0 and torch.equal(y.cpu(), y0.cpu()), f"conv3_c1_fwd_stats y {sp}"
        pt = torch.frombuffer(bytearray(part.cpu().numpy().tobytes()[:G * rows * 16 * 16]), dtype=torch.float64).view(G, rows, 16, 2).sum(1)
        yg = from_cl(y0, two_d).cpu().double().transpose(0, 1).reshape(16, G, -1)
        close(pt[..., 0], yg.sum(2).t(), rtol=1e-6, msg=f"c1 fused sum {sp}")
        close(pt[..., 1], (yg * yg).sum(2).t(), rtol=1e-6, msg=f"c1 fused sum of squares {sp}")
        g1, b1 = torch.ones(16).to(dev), torch.zeros(16).to(dev)
        a1, _ = ops.norm_fwd(y, G, g1, b1, torch.zeros(16).to(dev), torch.ones(16).to(dev), H.ACT_RELU, partial=part, nb=rows)
        a2, _ = ops.norm_fwd(y, G, g1, b1, torch.zeros(16).to(dev), torch.ones(16).to(dev), H.ACT_RELU)
        close(a1, a2, rtol=1e-6, msg=f"norm from the first layer's fused partials {sp}")


K2_CASES = ((1, 16, 32, (4, 6, 8)), (2, 32, 64, (2, 4, 6)), (1, 128, 256, (2, 2, 2)), (1, 16, 16, (10, 12, 14)), (2, 32, 16, (8, 6, 10)))
PW_CASES = ((2, 64, 32, (8, 8)), (3, 256, 128, (4, 4)))


def check_k2(ops, dev, cases=K2_CASES, pw_cases=PW_CASES):
    rng = np.random.default_rng(7)
    for (N, Cin, Cout, sp) in cases:
        # down conv
        x = R(rng, N, Cin, *sp).requires_grad_(True)
        w = (R(rng, Cout, Cin, 2, 2, 2) * 0.1).requires_grad_(True)
        b = R(rng, Cout) * 0.1
        y_ref = F.conv3d(x, w, b, stride=2)
        dy = R(rng, *y_ref.shape)
        y_ref.backward(dy)
        wd = w.detach().to(dev).contiguous()
        xcl, dycl = to_cl(x.detach()).to(dev), to_cl(dy).to(dev)
        y = ops.down_fwd(xcl, ops.k2_pack(wd, Cin, Cout, H.PACK_DOWN_FWD), b.to(dev), Cout)
        close(from_cl(y), y_ref, msg=f"down fwd {Cin}->{Cout}")
        dx = ops.down_dgrad(dycl, ops.k2_pack(wd, Cin, Cout, H.PACK_DOWN_DGRAD), Cin)
        close(from_cl(dx), x.grad, msg="down dgrad")
        dx2 = ops.down_dgrad(dycl, ops.k2_pack(wd, Cin, Cout, H.PACK_DOWN_DGRAD), Cin, out=dx.clone(), accumulate=True)
        close(from_cl(dx2), 2 * x.grad, msg="down dgrad accumulate")
        dw = torch.zeros(w.shape).to(dev)
        ops.k2_wgrad(xcl, dycl, dw, H.WG_DOWN)
        close(dw, w.grad, rtol=2e-4, msg="down wgrad")
        # up conv (Cout -> Cin so shapes chain): x2 coarse [N,Cout,sp/2] -> fine [N,Cin,sp]
        x2 = R(rng, N, Cout, *[s // 2 for s in sp]).requires_grad_(True)
        w2 = (R(rng, Cout, Cin, 2, 2, 2) * 0.1).requires_grad_(True)   # ConvTranspose3d weight [Cin_t, Cout_t, 2,2,2]
        b2 = R(rng, Cin) * 0.1
        y2_ref = F.conv_transpose3d(x2, w2, b2, stride=2)
        dy2 = R(rng, *y2_ref.shape)
        y2_ref.backward(dy2)
        w2d = w2.detach().to(dev).contiguous()
        x2cl, dy2cl = to_cl(x2.detach()).to(dev), to_cl(dy2).to(dev)
        y2 = ops.up_fwd(x2cl, ops.k2_pack(w2d, Cout, Cin, H.PACK_UP_FWD), b2.to(dev), Cin)
        close(from_cl(y2), y2_ref, msg=f"up fwd {Cout}->{Cin}")
        dx2 = ops.up_dgrad(dy2cl, ops.k2_pack(w2d, Cout, Cin, H.PACK_UP_DGRAD), Cout)
        close(from_cl(dx2), x2.grad, msg="up dgrad")
        dw2 = torch.zeros(w2.shape).to(dev)
        ops.k2_wgrad(x2cl, dy2cl, dw2, H.WG_UP)
        close(dw2, w2.grad, rtol=2e-4, msg="up wgrad")
    # 1x1 conv (U-Net decoder) fwd / dgrad / wgrad, bias grad via colsum
    for (N, Cin, Cout, hw) in pw_cases:
        x = R(rng, N, Cin, *hw).requires_grad_(True)
        w = (R(rng, Cout, Cin, 1, 1) * 0.1).requires_grad_(True)
        b = (R(rng, Cout) * 0.1).requires_grad_(True)
        y_ref = F.conv2d(x, w, b)
        dy = R(rng, *y_ref.shape)
        y_ref.backward(dy)
        wd = w.detach().to(dev).contiguous()
        xcl, dycl = to_cl(x.detach()).to(dev), to_cl(dy).to(dev)
        y = ops.pw_fwd(xcl, ops.k2_pack(wd, Cin, Cout, H.PACK_PW_FWD), b.detach().to(dev), Cout)
        close(from_cl(y, True), y_ref, msg="pw fwd")
        dx = ops.pw_fwd(dycl, ops.k2_pack(wd, Cin, Cout, H.PACK_PW_DGRAD), None, Cin)
        close(from_cl(dx, True), x.grad, msg="pw dgrad")
        dw = torch.zeros(w.shape).to(dev)
        ops.k2_wgrad(xcl, dycl, dw, H.WG_PW)
        close(dw, w.grad, rtol=2e-4, msg="pw wgrad")
        db = torch.zeros(Cout).to(dev)
        ops.colsum(dycl, db)
        close(db, b.grad, rtol=2e-4, msg="colsum")
    # 16 -> 2 output conv
    x = R(rng, 2, 16, 4, 6, 8).requires_grad_(True)
    w = (R(rng, 2, 16, 1, 1, 1) * 0.3).requires_grad_(True)
    b = (R(rng, 2) * 0.1).requires_grad_(True)
    y_ref = F.conv3d(x, w, b)
    dy = R(rng, *y_ref.shape)
    y_ref.backward(dy)
    xcl, dycl = to_cl(x.detach()).to(dev), to_cl(dy).to(dev)
    wd = w.detach().to(dev).contiguous()
    y = ops.pw16_fwd(xcl, wd, b.detach().to(dev), 2)
    close(from_cl(y), y_ref, msg="pw16 fwd")
    dw, db = torch.zeros(w.shape).to(dev), torch.zeros(2).to(dev)
    dx = ops.pw16_bwd(xcl, dycl, wd, dw, db)
    close(from_cl(dx), x.grad, msg="pw16 dx")
    close(dw, w.grad, rtol=2e-4, msg="pw16 dw")
    close(db, b.grad, rtol=2e-4, msg="pw16 db")


def check_pw16_norm(ops, dev):
    """the 16 -> C head that normalises on its way in (bcp_pw16_fwd_norm / _bwd_norm) against the two-launch composition
    norm_fwd -> pw16_fwd: same statistics, same per-element arithmetic -> logits and gradients agree to rounding of the
    compiler's contraction choices; the running statistics update is the one the apply pass would have made."""
    rng = np.random.default_rng(31)
    for (N, G, Cout, affine, drop) in ((4, 2, 2, True, True), (2, 2, 2, False, False), (4, 1, 4, True, False), (3, 3, 2, False, True)):
        y = (R(rng, N, 5, 6, 8, 16) * 1.7 + 0.3).to(dev)
        gamma = (R(rng, 16) * 0.3 + 1).to(dev) if affine else None
        beta = (R(rng, 16) * 0.2).to(dev) if affine else None
        rm = [torch.zeros(16).to(dev) for _ in range(2)] if affine else [None, None]
        rv = [torch.ones(16).to(dev) for _ in range(2)] if affine else [None, None]
        cs = ((torch.from_numpy(rng.integers(0, 2, (N, 16))).float() * 2).to(dev)) if drop else None
        w = (R(rng, Cout, 16, 1, 1, 1) * 0.3).to(dev).contiguous()
        b = (R(rng, Cout) * 0.1).to(dev)
        dlog = R(rng, N, 5, 6, 8, Cout).to(dev)
        a, st = ops.norm_fwd(y, G, gamma, beta, rm[0], rv[0], H.ACT_RELU, chan_scale=cs)
        ref = ops.pw16_fwd(a, w, b, Cout)
        dw0, db0 = torch.zeros_like(w), torch.zeros(Cout).to(dev)
        dx0 = ops.pw16_bwd(a, dlog, w, dw0, db0)
        none, st1 = ops.norm_fwd(y, G, gamma, beta, rm[1], rv[1], H.ACT_RELU, chan_scale=cs, stats_only=True)
        assert none is None and torch.equal(st, st1), "statistics-only norm_fwd: different statistics"
        if affine:
            assert torch.equal(rm[0], rm[1]) and torch.equal(rv[0], rv[1]), "statistics-only norm_fwd: running statistics differ"
            assert float(rm[1].abs().max()) > 0
        got = ops.pw16_fwd_norm(y, st1, cs, G, H.ACT_RELU, w, b, Cout)
        close(got, ref, rtol=1e-5, msg=f"pw16_fwd_norm N={N} G={G}")
        dw1, db1 = torch.zeros_like(w), torch.zeros(Cout).to(dev)
        dx1 = ops.pw16_bwd_norm(y, st1, cs, G, H.ACT_RELU, dlog, w, dw1, db1)
        assert torch.equal(dx1, dx0), "pw16_bwd_norm: dx"
        close(dw1, dw0, rtol=1e-5, msg="pw16_bwd_norm dw")
        close(db1, db0, rtol=1e-6, msg="pw16_bwd_norm db")
        # accumulate flag
        dx2 = ops.pw16_bwd_norm(y, st1, cs, G, H.ACT_RELU, dlog, w, dw1, db1, accumulate=True)
        close(dw1, 2 * dw0, rtol=1e-5, msg="pw16_bwd_norm accumulate")


def check_pw16_bwd_norm_bwd(ops, dev):
    """the head's backward through the norm in one call (bcp_pw16_bwd_norm_bwd) against the chain it replaces, pw16_bwd_norm -> norm_bwd:
    dw / db of the head, dgamma / dbeta of the norm (accumulated on top of what is there) and the gradient w.r.t. the raw conv output;
    BatchNorm groups and InstanceNorm, with and without the Dropout3d channel scale, sample counts that leave ragged blocks; the |max|
    slots of the result equal the chain's."""
    rng = np.random.default_rng(131)
    for (N, G, Cout, affine, drop, sp) in ((4, 2, 2, True, True, (5, 6, 8)), (2, 2, 2, False, False, (5, 6, 8)), (4, 1, 4, True, False, (3, 7, 5)),
                                           (3, 3, 2, False, True, (9, 11, 13)), (2, 1, 2, True, True, (16, 24, 40))):
        y = (R(rng, N, *sp, 16) * 1.7 + 0.3).to(dev)
        gamma = (R(rng, 16) * 0.3 + 1).to(dev) if affine else None
        beta = (R(rng, 16) * 0.2).to(dev) if affine else None
        rm, rv = (torch.zeros(16).to(dev), torch.ones(16).to(dev)) if affine else (None, None)
        cs = ((torch.from_numpy(rng.integers(0, 2, (N, 16))).float() * 2).to(dev)) if drop else None
        w = (R(rng, Cout, 16, 1, 1, 1) * 0.3).to(dev).contiguous()
        dlog = R(rng, N, *sp, Cout).to(dev)
        _, st = ops.norm_fwd(y, G, gamma, beta, rm, rv, H.ACT_RELU, chan_scale=cs, stats_only=True)
        tag = f"pw16_bwd_norm_bwd N={N} G={G} Cout={Cout} affine={affine} drop={drop} {sp}"
        dw0, db0 = (R(rng, Cout, 16, 1, 1, 1) * 0.1).to(dev).contiguous(), (R(rng, Cout) * 0.1).to(dev)
        dw1, db1 = dw0.clone(), db0.clone()
        dg0, dbe0 = ((R(rng, 16) * 0.1).to(dev), (R(rng, 16) * 0.1).to(dev)) if affine else (None, None)
        dg1, dbe1 = (dg0.clone(), dbe0.clone()) if affine else (None, None)
        da = ops.pw16_bwd_norm(y, st, cs, G, H.ACT_RELU, dlog, w, dw0, db0, accumulate=True)
        ref = ops.norm_bwd(y, da, G, st, H.ACT_RELU, dg0, dbe0, affine, chan_scale=cs)
        got = ops.pw16_bwd_norm_bwd(y, st, cs, G, H.ACT_RELU, dlog, w, dw1, db1, dg1, dbe1, norm_accumulate=affine, accumulate=True)
        close(got, ref, rtol=2e-5, msg=tag + " dy")
        close(dw1, dw0, rtol=1e-5, msg=tag + " dw")
        close(db1, db0, rtol=1e-6, msg=tag + " db")
        if affine:
            close(dg1, dg0, rtol=2e-5, msg=tag + " dgamma")
            close(dbe1, dbe0, rtol=2e-5, msg=tag + " dbeta")
        if ops.AMAX:
            a0, a1 = ops._amax_of(ref), ops._amax_of(got)
            assert a0 is not None and a1 is not None, tag + ": |max| slots missing"
            m0, m1 = H.amax_value(a0), H.amax_value(a1)
            assert abs(m0 - m1) <= 2e-5 * max(m0, 1e-30) and m1 > 0, f"{tag}: |max| {m1} vs {m0}"


def check_pool2d(ops, dev):
    rng = np.random.default_rng(8)
    # round 4: |max| of a concat buffer = max(skip's slot, what the upsample writes)
    skip, z = to_cl(R(rng, 2, 16, 8, 12) * 0.5).to(dev), to_cl(R(rng, 2, 16, 4, 6) * 3.0).to(dev)
    skip._bcp_amax = H.amax_slots(float(skip.abs().max()), dev)
    cat = torch.empty((2, 1, 8, 12, 32), dtype=torch.float32, device=dev)
    ops.copy_channels(skip, cat, 16, 0, 0, carry_amax=True)
    ops.bilinear2x_fwd(z, cat, 16)
    assert H.amax_value(cat._bcp_amax) == float(cat.abs().max()), (H.amax_value(cat._bcp_amax), float(cat.abs().max()))
    cat2 = torch.empty_like(cat)
    ops.copy_channels(to_cl(R(rng, 2, 16, 8, 12)).to(dev), cat2, 16, 0, 0, carry_amax=True)      # a source without a slot: none on the buffer either
    assert getattr(cat2, "_bcp_amax", None) is None
    x = R(rng, 2, 16, 8, 12).requires_grad_(True)
    y_ref = F.max_pool2d(x, 2)
    dy = R(rng, *y_ref.shape)
    y_ref.backward(dy)
    xcl = to_cl(x.detach()).to(dev)
    y = ops.maxpool2d_fwd(xcl)
    assert torch.equal(from_cl(y, True).cpu(), y_ref.detach())
    dx = ops.maxpool2d_bwd(xcl, to_cl(dy).to(dev), torch.empty_like(xcl))
    assert torch.equal(from_cl(dx, True).cpu(), x.grad)
    # round 4: the skip lives in the leading channels of the concat buffer -- the norm writes it there (out_ld), the pool reads it from
    # there (ldx), the pool's backward joins the decoder-side skip gradient (add); all bit-identical to the contiguous / copied forms
    wide = torch.full((2, 1, 8, 12, 32), 7.0, dtype=torch.float32, device=dev)
    slab = ops.channel_slab(wide, 16)
    slab.copy_(xcl)
    assert torch.equal(ops.maxpool2d_fwd(slab), y)
    dcat = to_cl(R(rng, 2, 32, 8, 12)).to(dev)
    dx2 = ops.maxpool2d_bwd(slab, to_cl(dy).to(dev), torch.empty_like(xcl), add=ops.channel_slab(dcat, 16))
    ref2 = ops.copy_channels(dcat, dx.clone(), 16, 0, 0, accumulate=True)
    assert torch.equal(dx2, ref2), "maxpool2d_bwd + skip-gradient join"
    ynorm = to_cl(R(rng, 2, 16, 8, 12) * 1.5 + 0.3).to(dev)
    gam, bet = torch.from_numpy(rng.uniform(0.5, 1.5, 16).astype(np.float32)).to(dev), torch.from_numpy(rng.uniform(-0.3, 0.3, 16).astype(np.float32)).to(dev)
    a_c, st_c = ops.norm_fwd(ynorm, 2, gam, bet, torch.zeros(16).to(dev), torch.ones(16).to(dev), H.ACT_LRELU)
    wide.fill_(7.0)
    a_s, st_s = ops.norm_fwd(ynorm, 2, gam, bet, torch.zeros(16).to(dev), torch.ones(16).to(dev), H.ACT_LRELU, out=ops.channel_slab(wide, 16))
    assert a_s.data_ptr() == wide.data_ptr() and torch.equal(a_s, a_c) and torch.equal(st_s, st_c), "norm_fwd into a channel slab"
    assert bool((wide[..., 16:] == 7.0).all()), "norm_fwd out_ld: wrote outside its channels"
    assert H.amax_value(a_s._bcp_amax) == float(a_c.abs().max())
    # nn.MaxPool3d(3, stride=2): the V-Net's pooled x5 features (7x7x5 -> 3x3x2 at the LA size), odd and even extents
    for sp in ((7, 7, 5), (6, 8, 3), (3, 3, 3)):
        x3 = R(rng, 2, 32, *sp)
        assert torch.equal(from_cl(ops.maxpool3d_k3s2_fwd(to_cl(x3).to(dev))).cpu(), F.max_pool3d(x3, 3, stride=2)), f"maxpool3d {sp}"
    # bilinear x2 align_corners=True into the second half of a concat buffer, and its backward
    x = R(rng, 2, 16, 5, 7).requires_grad_(True)
    skip = R(rng, 2, 16, 10, 14)
    up = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)
    cat = torch.cat([skip, up], 1)
    dcat = R(rng, *cat.shape)
    cat.backward(dcat)
    buf = torch.empty(2, 1, 10, 14, 32).to(dev)
    ops.copy_channels(to_cl(skip).to(dev), buf, 16, 0, 0)
    ops.bilinear2x_fwd(to_cl(x.detach()).to(dev), buf, 16)
    close(from_cl(buf, True), cat, msg="bilinear+concat fwd")
    dx = ops.bilinear2x_bwd(to_cl(dcat).to(dev), 16, 16)
    close(from_cl(dx, True), x.grad, msg="bilinear bwd")


def check_optim(ops, dev):
    rng = np.random.default_rng(9)
    n = 1000 + 3
    p, g = R(rng, n), R(rng, n)
    t = R(rng, n)
    # EMA: bit-exact vs the reference expression
    ref = t.clone()
    ref.mul_(0.99).add_((1 - 0.99) * p)
    td = t.clone().to(dev)
    ops.ema(td, p.to(dev), 0.99)
    assert torch.equal(td.cpu(), ref), "EMA must be bit-exact"
    # SGD momentum, two steps, vs torch.optim.SGD
    pr = p.clone().requires_grad_(True)
    opt = torch.optim.SGD([pr], lr=0.01, momentum=0.9, weight_decay=1e-4)
    pd, buf = p.clone().to(dev), torch.zeros(n).to(dev)
    for step in range(2):
        gg = g * (step + 1)
        pr.grad = gg.clone()
        opt.step()
        ops.sgd(pd, gg.to(dev), buf, 0.01, 0.9, 1e-4, first_step=(step == 0))
    close(pd, pr.detach(), rtol=1e-6, atol_scale=1e-7, msg="sgd")
    # Adam
    pr = p.clone().requires_grad_(True)
    opt = torch.optim.Adam([pr], lr=1e-3)
    pd, m, v = p.clone().to(dev), torch.zeros(n).to(dev), torch.zeros(n).to(dev)
    for step in range(3):
        pr.grad = g.clone()
        opt.step()
        ops.adam(pd, g.to(dev), m, v, 1e-3, step + 1)
    close(pd, pr.detach(), rtol=1e-5, atol_scale=1e-6, msg="adam")
    # casts
    lab = torch.from_numpy(rng.integers(0, 4, (3, 5, 7)))
    assert torch.equal(ops.to_u8(lab.to(dev)).cpu(), lab.to(torch.uint8))
    assert torch.equal(ops.to_u8(lab.float().to(dev)).cpu(), lab.to(torch.uint8))


CONV3_RES_CASES = (
    # shapes that route to the resident-weight persistent kernel (tiles x slabs >= 192)
    (1, 16, 16, (16, 16, 48), 3),     # 4x4x4 tiles, 1 chunk
    (1, 32, 32, (14, 17, 50), 3),     # 2 chunks, 2 slabs, partial tiles
    (1, 64, 64, (12, 12, 24), 3),     # 4 chunks, 4 slabs
    (2, 16, 32, (1, 72, 64), 1),      # 2-D, 8x8 tiles
    (1, 32, 16, (34, 36, 56), 3),     # >= 64K voxels: 4x4x8 tiles (M = 128)
)


def check_k2_stats(ops, dev):
    """round 6: the k2s2 / transposed conv forward whose epilogue leaves the norm statistics of its output (bcp_down_fwd_stats /
    bcp_up_fwd_stats, reference: the norm behind networks/VNet.py:74-86, 101-113): y bit-identical to the plain launch, the partial rows sum
    to the per-group (sum y, sum y^2) of that y, and bcp_norm_fwd fed with them equals bcp_norm_fwd making its own pass.  Cases: channels
    folding four / two sub-positions onto one set (Cout < slab), Cout == slab, Cout > slab (two column slabs per channel set), G = 1 / 2 / 4,
    one and several 64-row blocks per workgroup (R > 1: the big case, GPU only)"""
    rng = np.random.default_rng(11)
    ops.set_option("k2_stats", 1)       # every shape the variant serves (the product default, 2, keeps it to outputs of >= 2^24 elements)
    try:
        # (round 6) row blocks per workgroup forced (gemm_stat_r: the small cases walk several blocks too), with and without the next block's
        # operands requested under the current one (gemm_pipe) -- one K stage (B stays in the LDS) and several
        for r, pipe in ((0, 1), (2, 1), (4, 1), (2, 0)):
            ops.set_option("gemm_stat_r", r)
            ops.set_option("gemm_pipe", pipe)
            _check_k2_stats(ops, dev, np.random.default_rng(11))
    finally:
        ops.set_option("k2_stats")
        ops.set_option("gemm_stat_r")
        ops.set_option("gemm_pipe")
    assert ops.k2_stat_rows(1, (2, 4, 8, 8, 32), 16, 2) == 0 and (dev.type != "cuda" or ops.k2_stat_rows(1, (2, 56, 56, 40, 32), 16, 2) > 0)


def check_gemm_walk(ops, dev):
    """round 6 (measurement switch gemm_walk): the plain k2s2 / transposed conv launches as workgroups that walk several row blocks with the
    next block's operands in flight (k_gemm_nn<.., 7>) -- forward, dgrad and dgrad accumulating into a skip gradient bit-identical to the
    one-block-per-workgroup launch, one K stage and several, ragged last walk"""
    rng = np.random.default_rng(12)
    cases = [(0, 2, 16, 32, (8, 16, 16)), (0, 1, 32, 64, (4, 12, 20)), (1, 2, 32, 16, (4, 8, 8)), (1, 1, 64, 32, (6, 10, 6)), (1, 2, 128, 64, (2, 4, 8))]
    if dev.type == "cuda":
        cases += [(1, 2, 32, 16, (16, 32, 32)), (0, 2, 16, 32, (32, 64, 64))]
    for kind, N, Cin, Cout, sp in cases:
        x = to_cl(R(rng, N, Cin, *sp)).to(dev)
        w = ((R(rng, Cout, Cin, 2, 2, 2) if kind == 0 else R(rng, Cin, Cout, 2, 2, 2)) * 0.1).to(dev)
        b = (R(rng, Cout) * 0.1).to(dev)
        bp = ops.k2_pack(w, Cin, Cout, H.PACK_DOWN_FWD if kind == 0 else H.PACK_UP_FWD)
        bd = ops.k2_pack(w, Cin, Cout, H.PACK_DOWN_DGRAD if kind == 0 else H.PACK_UP_DGRAD)
        fwd, dgrad = (ops.down_fwd, ops.down_dgrad) if kind == 0 else (ops.up_fwd, ops.up_dgrad)
        res = {}
        for walk, pipe in ((0, 1), (3, 1), (3, 0), (1, 1)):
            ops.set_option("gemm_walk", walk)
            ops.set_option("gemm_pipe", pipe)
            try:
                y = fwd(x, bp, b, Cout).clone()
                dy = torch.sin(y * 3.0)
                dx = dgrad(dy, bd, Cin).clone()
                acc = torch.cos(dx * 2.0)
                dxa = dgrad(dy, bd, Cin, out=acc, accumulate=True).clone()
            finally:
                ops.set_option("gemm_walk")
                ops.set_option("gemm_pipe")
            res[(walk, pipe)] = (y, dx, dxa)
        for k, v in res.items():
            for a, b0, name in zip(v, res[(0, 1)], ("fwd", "dgrad", "dgrad accumulate")):
                assert torch.equal(a, b0), f"gemm walk kind {kind} {N}x{sp} {Cin}->{Cout} {name}: walk, pipe = {k} differs from the plain launch"


def _check_k2_stats(ops, dev, rng):
    cases = [(0, 2, 16, 32, (8, 16, 16), 2), (0, 2, 32, 64, (8, 8, 16), 1), (0, 4, 64, 128, (8, 8, 8), 4), (0, 1, 16, 16, (16, 16, 16), 1),
             (1, 2, 32, 16, (4, 8, 8), 2), (1, 2, 64, 32, (4, 4, 8), 1), (1, 2, 128, 64, (2, 4, 8), 2), (1, 1, 256, 128, (4, 4, 4), 1)]
    if dev.type == "cuda":
        cases += [(1, 2, 32, 16, (16, 32, 32), 2), (0, 2, 16, 32, (32, 64, 64), 2)]      # thousands of row blocks: R > 1
    seen_fused = 0
    for kind, N, Cin, Cout, sp, G in cases:
        x = to_cl(R(rng, N, Cin, *sp)).to(dev)          # kind 0: sp = the FINE extents of x; kind 1: the COARSE extents of x
        if kind == 0:
            w = (R(rng, Cout, Cin, 2, 2, 2) * 0.1).to(dev)
            bp = ops.k2_pack(w, Cin, Cout, H.PACK_DOWN_FWD)
        else:
            w = (R(rng, Cin, Cout, 2, 2, 2) * 0.1).to(dev)
            bp = ops.k2_pack(w, Cin, Cout, H.PACK_UP_FWD)
        b = (R(rng, Cout) * 0.1).to(dev)
        rows = ops.k2_stat_rows(kind, x.shape, Cout, G)
        tag = f"k2 stats kind {kind} {N}x{sp} {Cin}->{Cout} G={G}"
        assert rows > 0, tag + ": expected the fused statistics for this shape"
        y0 = (ops.down_fwd if kind == 0 else ops.up_fwd)(x, bp, b, Cout).clone()
        y, part, nb = ops.k2_fwd_stats(kind, x, bp, b, Cout, G)
        assert nb == rows and torch.equal(y, y0), tag + ": y differs from the plain launch"
        P = part.view(torch.float64)[: G * nb * Cout * 2].view(G, nb, Cout, 2).sum(1).cpu()
        yd = y.double().cpu().reshape(G, -1, Cout)
        ref = torch.stack([yd.sum(1), (yd * yd).sum(1)], dim=-1)
        # (sums of <= 256 values per lane group in fp32, everything behind them in fp64: the totals agree with the fp64 sums to ~1e-8 of their
        #  natural scale -- sum |y| for the first moment)
        nrm = torch.stack([yd.abs().sum(1), ref[..., 1]], dim=-1)
        err = float(((P - ref).abs() / (nrm + 1e-30)).max())
        assert err < 1e-6, (tag, err)
        gamma = torch.from_numpy(rng.uniform(0.5, 1.5, Cout).astype(np.float32)).to(dev)
        beta = torch.from_numpy(rng.uniform(-0.3, 0.3, Cout).astype(np.float32)).to(dev)
        a0, st0 = ops.norm_fwd(y0, G, gamma, beta, torch.zeros(Cout, device=dev), torch.ones(Cout, device=dev), H.ACT_RELU)
        a0, st0 = a0.clone(), st0.clone()
        y, part, nb = ops.k2_fwd_stats(kind, x, bp, b, Cout, G)
        a1, st1 = ops.norm_fwd(y, G, gamma, beta, torch.zeros(Cout, device=dev), torch.ones(Cout, device=dev), H.ACT_RELU, partial=part, nb=nb)
        close(st1.cpu(), st0.cpu(), rtol=1e-6, atol_scale=1e-7, msg=tag + " statistics")
        close(a1.cpu(), a0.cpu(), rtol=1e-5, atol_scale=1e-6, msg=tag + " activations")
        seen_fused += 1
    # shapes the variant does not serve answer 0 rows (a 64-row block would straddle two groups) and the option switches it off
    assert ops.k2_stat_rows(0, (2, 6, 10, 10, 16), 32, 2) == 0
    ops.set_option("k2_stats", 0)
    try:
        assert ops.k2_stat_rows(0, (2, 8, 16, 16, 16), 32, 2) == 0
    finally:
        ops.set_option("k2_stats", 1)
    assert seen_fused == len(cases)


def check_k2_bwdstats(ops, dev):
    """round 6: the k2s2 / transposed conv DGRAD whose epilogue leaves the backward statistics of the norm layer in front of it
    (bcp_down_dgrad_bwdstats / bcp_up_dgrad_bwdstats): dx bit-identical to the plain dgrad (+= a skip gradient included), and bcp_norm_bwd fed
    with the partial rows equal to bcp_norm_bwd making its own pass over (y, da): dy, dgamma, dbeta.  Cases: channel folds as in
    check_k2_stats, G = 1 / 2, with and without the accumulated skip gradient; one big case (GPU only) for R > 1"""
    rng = np.random.default_rng(12)
    ops.set_option("k2_bwd_stats", 1)
    try:
        # (kind, N, Cin, Cout, dy spatial, G): kind 0 = dgrad of the down conv Cin -> Cout (dy coarse [.., Cout], dx fine [.., Cin]);
        #                                     kind 1 = dgrad of the transposed conv Cin -> Cout (dy fine [.., Cout], dx coarse [.., Cin])
        cases = [(0, 2, 16, 32, (4, 8, 8), 2), (0, 2, 32, 64, (4, 4, 8), 1), (0, 1, 64, 128, (4, 4, 4), 1),
                 (1, 2, 32, 16, (8, 16, 16), 2), (1, 2, 64, 32, (8, 8, 16), 1), (1, 1, 128, 64, (8, 8, 8), 1)]
        if dev.type == "cuda":
            cases += [(1, 2, 32, 16, (32, 64, 64), 2), (0, 2, 32, 64, (16, 32, 32), 2)]
        for kind, N, Cin, Cout, sp, G in cases:
            dy = to_cl(R(rng, N, Cout, *sp) * 1e-2).to(dev)
            if kind == 0:
                w = (R(rng, Cout, Cin, 2, 2, 2) * 0.1).to(dev)
                bp = ops.k2_pack(w, Cin, Cout, H.PACK_DOWN_DGRAD)
                osp = tuple(2 * e for e in sp)
            else:
                w = (R(rng, Cin, Cout, 2, 2, 2) * 0.1).to(dev)
                bp = ops.k2_pack(w, Cin, Cout, H.PACK_UP_DGRAD)
                osp = tuple(e // 2 for e in sp)
            tag = f"k2 bwdstats kind {kind} {N}x{sp} {Cin}<-{Cout} G={G}"
            rows = ops.k2_bwdstat_rows(kind, dy.shape, Cin, G)
            assert rows > 0, tag + ": expected the fused statistics for this shape"
            # the norm layer in front: pre-norm tensor y, its statistics from a real forward
            y = to_cl(R(rng, N, Cin, *osp) * 1.3 + 0.2).to(dev)
            gamma = torch.from_numpy(rng.uniform(0.5, 1.5, Cin).astype(np.float32)).to(dev)
            beta = torch.from_numpy(rng.uniform(-0.3, 0.3, Cin).astype(np.float32)).to(dev)
            _, st = ops.norm_fwd(y, G, gamma, beta, torch.zeros(Cin, device=dev), torch.ones(Cin, device=dev), H.ACT_RELU)
            for acc in (False, True):
                sg = (to_cl(R(rng, N, Cin, *osp) * 1e-2).to(dev)) if acc else None
                plain = ops.down_dgrad if kind == 0 else ops.up_dgrad
                d0 = plain(dy, bp, Cin, out=sg.clone() if acc else None, accumulate=acc).clone()
                d1, part, nb = ops.k2_dgrad_bwdstats(kind, dy, bp, Cin, y, st, H.ACT_RELU, G, out=sg.clone() if acc else None, accumulate=acc)
                assert nb == rows and torch.equal(d1, d0), tag + f" acc={acc}: dx differs from the plain dgrad"
                dg0, db0 = torch.zeros(Cin, device=dev), torch.zeros(Cin, device=dev)
                dg1, db1 = torch.zeros(Cin, device=dev), torch.zeros(Cin, device=dev)
                dy0 = ops.norm_bwd(y, d0, G, st, H.ACT_RELU, dg0, db0, True).clone()
                dy1 = ops.norm_bwd(y, d1, G, st, H.ACT_RELU, dg1, db1, True, partial=part, nb=nb)
                close(dy1.cpu(), dy0.cpu(), rtol=1e-5, atol_scale=1e-6, msg=tag + f" acc={acc} dy")
                close(dg1.cpu(), dg0.cpu(), rtol=1e-5, atol_scale=1e-6, msg=tag + f" acc={acc} dgamma")
                close(db1.cpu(), db0.cpu(), rtol=1e-5, atol_scale=1e-6, msg=tag + f" acc={acc} dbeta")
    finally:
        ops.set_option("k2_bwd_stats")


def check_up_norm(ops, dev):
    """round 6: ConvTranspose3d(k=2,s=2) -> norm -> ReLU (+ skip add) with the conv output recomputed instead of stored (bcp_up_fwd_norm /
    bcp_up_norm_bwd; reference networks/VNet.py:101-113 + the decoder's skip add) against the chain it replaces -- bcp_up_fwd_stats +
    bcp_norm_fwd (statistics from the same GEMM epilogue: the activations must agree to the last bits of the apply arithmetic) and
    bcp_norm_bwd (its own fp64 statistics pass: dy / dgamma / dbeta to 1e-5) -- and against torch on the CPU.  BatchNorm (G = 1, 2, affine,
    running statistics) and InstanceNorm (G = N, no affine); with and without the residual; channel folds 16 / 32 / 64 / 128"""
    rng = np.random.default_rng(13)
    ops.set_option("up_recompute", 1)
    ops.set_option("k2_stats", 1)
    try:
        cases = [(2, 32, 16, (4, 8, 8), 2, True, True), (2, 64, 32, (4, 4, 8), 1, True, False), (2, 128, 64, (2, 4, 8), 2, False, True),
                 (1, 256, 128, (4, 4, 4), 1, True, True), (2, 32, 16, (8, 8, 8), 2, False, False)]
        if dev.type == "cuda":
            cases += [(2, 32, 16, (16, 32, 32), 2, True, True)]
        for N, Cin, Cout, sp, G, affine, use_res in cases:
            tag = f"up_norm {N}x{sp} {Cin}->{Cout} G={G} affine={affine} res={use_res}"
            xt = R(rng, N, Cin, *sp)
            wt = R(rng, Cin, Cout, 2, 2, 2) * 0.1
            bt = R(rng, Cout) * 0.1
            fine = tuple(2 * e for e in sp)
            rest = R(rng, N, Cout, *fine) if use_res else None
            dat = R(rng, N, Cout, *fine)
            gam = torch.from_numpy(rng.uniform(0.5, 1.5, Cout).astype(np.float32)) if affine else None
            bet = torch.from_numpy(rng.uniform(-0.3, 0.3, Cout).astype(np.float32)) if affine else None
            x, res, da = to_cl(xt).to(dev), (to_cl(rest).to(dev) if use_res else None), to_cl(dat).to(dev)
            w, b = wt.to(dev), bt.to(dev)
            bp = ops.k2_pack(w, Cin, Cout, H.PACK_UP_FWD)
            g_, b_ = (gam.to(dev), bet.to(dev)) if affine else (None, None)
            assert ops.up_norm_rows(x.shape, Cout, G) > 0, tag
            # the chain it replaces
            rm0, rv0 = (torch.zeros(Cout, device=dev), torch.ones(Cout, device=dev)) if affine else (None, None)
            y, part, nb = ops.k2_fwd_stats(1, x, bp, b, Cout, G)
            a0, st0 = ops.norm_fwd(y, G, g_, b_, rm0, rv0, H.ACT_RELU, residual=res, partial=part, nb=nb)
            a0, st0, y = a0.clone(), st0.clone(), y.clone()
            dg0 = torch.zeros(Cout, device=dev) if affine else None
            db0 = torch.zeros(Cout, device=dev) if affine else None
            dy0 = ops.norm_bwd(y, da, G, st0, H.ACT_RELU, dg0, db0, affine).clone()
            # the recomputing pair
            rm1, rv1 = (torch.zeros(Cout, device=dev), torch.ones(Cout, device=dev)) if affine else (None, None)
            a1, st1 = ops.up_fwd_norm(x, bp, b, Cout, G, g_, b_, rm1, rv1, H.ACT_RELU, residual=res)
            assert torch.equal(st1, st0), tag + ": statistics differ from bcp_up_fwd_stats + finalize"
            close(a1.cpu(), a0.cpu(), rtol=1e-6, atol_scale=1e-7, msg=tag + " activations")
            if affine:
                assert torch.equal(rm1, rm0) and torch.equal(rv1, rv0), tag + ": running statistics"
            assert getattr(a1, "_bcp_amax", None) is not None or not type(ops).AMAX, tag + ": no |max| slots on the activation"
            if type(ops).AMAX:
                want = float(a1.abs().max())
                have = float(H.amax_value(a1._bcp_amax))
                assert abs(have - want) <= 1e-6 * max(want, 1e-30), (tag, have, want)
            dg1 = torch.zeros(Cout, device=dev) if affine else None
            db1 = torch.zeros(Cout, device=dev) if affine else None
            dy1 = ops.up_norm_bwd(x, bp, b, Cout, G, st1, da, H.ACT_RELU, dg1, db1, affine)
            close(dy1.cpu(), dy0.cpu(), rtol=1e-5, atol_scale=1e-6, msg=tag + " dy")
            if affine:
                close(dg1.cpu(), dg0.cpu(), rtol=1e-5, atol_scale=1e-6, msg=tag + " dgamma")
                close(db1.cpu(), db0.cpu(), rtol=1e-5, atol_scale=1e-6, msg=tag + " dbeta")
            # torch on the CPU: forward values
            yt = F.conv_transpose3d(xt, wt, bt, stride=2)
            if G == 1:
                zt = F.batch_norm(yt, None, None, gam, bet, True, 0.1, 1e-5)
            elif not affine:
                zt = F.instance_norm(yt.reshape(G, (N // G) * Cout, *fine) if N != G else yt, eps=1e-5).reshape(yt.shape) if N == G else None
            else:
                zt = torch.cat([F.batch_norm(yt[g * (N // G):(g + 1) * (N // G)], None, None, gam, bet, True, 0.1, 1e-5) for g in range(G)])
            if zt is not None:
                at = F.relu(zt) + (rest if use_res else 0.0)
                close(from_cl(a1), at, rtol=2e-4, msg=tag + " vs torch")
    finally:
        ops.set_option("up_recompute")
        ops.set_option("k2_stats")


def check_k2_chunks(ops, dev):
    """weight-gradient GEMMs with ONE row group, so every block walks several 64-row chunks (prefetch / row-table pipeline)"""
    ops.set_option("tn_groups", 1)
    try:
        check_k2(ops, dev)
    finally:
        ops.set_option("tn_groups")


def check_wgrad_reduce_flat(ops, dev):
    """weight-gradient slab sums as k_wgrad_reduce_flat (round 6: slab-contiguous float4 reads, 16 group slots) for EVERY group count --
    the product takes it from 32 groups on -- on the fp32-MFMA and the bf16-pipe weight gradients and the first layer's"""
    ops.set_option("wgrad_reduce_flat", 2)
    try:
        check_conv3(ops, dev)
        check_conv3_c1(ops, dev)
        ops.set_option("wgrad_b6", 0)
        try:
            check_conv3(ops, dev, cases=CONV3_CASES[:6])
        finally:
            ops.set_option("wgrad_b6")
    finally:
        ops.set_option("wgrad_reduce_flat")


def check_norm_fuse_fin(ops, dev):
    """the apply passes that finalise the statistics themselves (k_norm_apply_fin / k_norm_bwd_apply_fin, option norm_fuse_fin, the product
    default) against the finalize-launch chain on the same inputs at the V-Net's deep shapes: grouped BatchNorm with running statistics,
    Dropout3d channel scale and a skip add, plain tensors and split-K slabs -- activations / gradients to 1e-6 of the tensor's |max|, statistics
    and running statistics to 1e-6 relative (the fp64 partial rows are added in another fixed order), and twice the same bits"""
    rng = np.random.default_rng(77)
    for (N, Cc, sp, G, nslab) in ((2, 128, (14, 14, 10), 2, 4), (2, 256, (7, 7, 5), 2, 2), (2, 64, (28, 28, 20), 2, 0), (2, 32, (1, 24, 40), 1, 0)):
        parts = [R(rng, N, *sp, Cc) * (1.5 if k == 0 else 0.3) + (0.3 if k == 0 else 0.0) for k in range(max(nslab, 1))]
        bias = R(rng, Cc) * 0.1 if nslab else None
        gamma = torch.from_numpy(rng.uniform(0.5, 1.5, Cc).astype(np.float32)).to(dev)
        beta = torch.from_numpy(rng.uniform(-0.3, 0.3, Cc).astype(np.float32)).to(dev)
        cs = torch.from_numpy(((rng.random((N, Cc)) < 0.5) * 2.0).astype(np.float32)).to(dev)
        res = R(rng, N, *sp, Cc).to(dev)
        dparts = [R(rng, N, *sp, Cc) * (1.0 if k == 0 else 0.2) for k in range(max(nslab, 1))]
        src = torch.stack(parts).to(dev) if nslab else parts[0].to(dev)
        dsrc = torch.stack(dparts).to(dev) if nslab else dparts[0].to(dev)

        def run():
            rm, rv = torch.zeros(Cc).to(dev), torch.ones(Cc).to(dev)
            if nslab:
                a, st, ycl = ops.norm_fwd_slabs(src, nslab, bias.to(dev), G, gamma, beta, rm, rv, H.ACT_RELU, chan_scale=cs, residual=res)
            else:
                ycl = src
                a, st = ops.norm_fwd(ycl, G, gamma, beta, rm, rv, H.ACT_RELU, chan_scale=cs, residual=res)
            dg, db = torch.full((Cc,), 3.0).to(dev), torch.full((Cc,), -2.0).to(dev)
            if nslab:
                dy, _ = ops.norm_bwd_slabs(ycl, dsrc, nslab, G, st, H.ACT_RELU, dg, db, True, chan_scale=cs)
            else:
                dy = ops.norm_bwd(ycl, dsrc, G, st, H.ACT_RELU, dg, db, True, chan_scale=cs)
            return [t.detach().cpu().clone() for t in (a, st, rm, rv, dy, dg, db)]

        fused = run()
        again = run()
        ops.set_option("norm_fuse_fin", 0)
        try:
            chain = run()
        finally:
            ops.set_option("norm_fuse_fin")
        tag = f"norm_fuse_fin C={Cc} sp={sp} G={G} slabs={nslab}"
        for name, f, f2, c in zip(("a", "stats", "running_mean", "running_var", "dy", "dgamma", "dbeta"), fused, again, chain):
            assert torch.equal(f, f2), f"{tag}: {name} differs between two launches"
            close(f, c, rtol=1e-6, atol_scale=1e-6, msg=f"{tag} {name}")


def check_norm_own(ops, dev):
    """the one-launch norm of the smallest levels (k_norm_own_fwd / _bwd; library option norm_own, off in the product: measured, not adopted):
    every norm check with it forced on -- BatchNorm / grouped BatchNorm (both groups in one workgroup, running statistics and parameter
    gradients in order) / InstanceNorm, every epilogue, slabs, chunk widths 8 / 16 / 32"""
    ops.set_option("norm_own", 1)
    try:
        check_norm(ops, dev)
        check_norm_grouped(ops, dev)
        _check_norm_slabs(ops, dev)
    finally:
        ops.set_option("norm_own")


def check_conv3_res(ops, dev):
    """resident-weight kernel, with the persistent grid forced small so every block walks several tiles"""
    ops.set_option("conv3_b6", 0)      # the fp32-MFMA kernels of conv3.hip (the bf16-pipe kernels have their own checks)
    ops.set_option("wgrad_b6", 0)
    try:
        for P in (7, 16):      # 16: a multiple of 8 takes the XCD-aware tile order
            ops.set_option("conv3_p", P)
            try:
                check_conv3(ops, dev, cases=CONV3_RES_CASES)
            finally:
                ops.set_option("conv3_p")
        check_conv3(ops, dev, cases=CONV3_RES_CASES[:2])
    finally:
        ops.set_option("conv3_b6")
        ops.set_option("wgrad_b6")


CONV3_B6_CASES = (
    # (N, Cin, Cout, spatial, KD): both slab widths, full and partial tiles, odd channel padding, 2-D
    (2, 32, 32, (8, 8, 16), 3),       # 4x4x8 tiles, 2 cin chunks, 7 two-pair stages
    (1, 16, 32, (5, 7, 9), 3),        # partial tiles
    (2, 64, 64, (4, 8, 12), 3),       # 4x8x4 tiles, 64-channel slab, one pair per stage
    (1, 32, 128, (6, 9, 5), 3),       # two slabs, partial tiles
    (1, 20, 32, (4, 4, 8), 3),        # Cin padded to 32
    (2, 16, 16, (4, 8, 8), 3),        # 16-channel slab: weight gradient only (one n-tile per wave)
    (2, 64, 32, (1, 12, 20), 1),      # 2-D: 8x16 tiles, 5 tap pairs (one zero-weight pad tap)
    (1, 32, 64, (1, 8, 16), 1),
)


def check_conv3_b6(ops, dev):
    """conv3b.hip: fp32 convolution on the bf16 matrix pipe (three-piece operands, six bf16 MFMAs per K = 32 block), forced
    on (conv3_b6 = 2): forward, dgrad, += and split-K vs torch CPU at the ordinary fp32 tolerance; fused statistics; and the
    accuracy claim itself -- the error against an fp64 convolution stays within 3x of the fp32-MFMA kernel's on the same data"""
    ops.set_option("conv3_b6", 2)
    ops.set_option("wgrad_b6", 2)           # csrc/conv3bw.hip: the weight gradient on the same pipe (transposed LDS reads)
    try:
        check_conv3(ops, dev, cases=CONV3_B6_CASES)
        # regression (round 3, found by the full-size ACDC step check): the 2-D two-pairs-per-stage instance has FOUR weight stages per
        # cin chunk while five are in flight -- the prefetch of stage s + 5 wraps over TWO chunk ends; with >= 3 chunks per workgroup
        # (64 -> 32 channels and no split-K: the U-Net's level-2 dgrad at batch 12) stage 0 of every later chunk got the last stage's weights
        ops.set_option("splitk", 1)
        try:
            check_conv3(ops, dev, cases=((2, 64, 32, (1, 12, 20), 1), (1, 128, 32, (1, 16, 16), 1), (1, 96, 32, (1, 9, 17), 1)))
        finally:
            ops.set_option("splitk")
        for sk in (2, 4):
            ops.set_option("splitk", sk)
            try:
                check_conv3(ops, dev, cases=[CONV3_B6_CASES[2]])
            finally:
                ops.set_option("splitk")
        # flat 64-voxel tiles + per-lane validity (deep levels): k_c3q (LDS-DMA software pipeline, the default) and k_c3f (register-staged
        # weights, conv3_b6_pipe = 0); slab widths: 1 = the launcher's choice (32 channels at these sizes), 4 = 64, 3 = 16 channels
        flat_cases = ((2, 64, 64, (4, 8, 12), 3), (1, 32, 128, (6, 9, 5), 3), (1, 64, 64, (7, 7, 5), 3), (2, 32, 64, (5, 6, 7), 3), (3, 64, 64, (3, 3, 3), 3))
        try:
            for flat in (1, 4, 3):
                ops.set_option("conv3_b6_flat", flat)
                for pipe in (1, 0):
                    ops.set_option("conv3_b6_pipe", pipe)
                    check_conv3(ops, dev, cases=flat_cases if flat == 1 else flat_cases[:3])
                    for sk in (2, 4):
                        ops.set_option("splitk", sk)
                        try:
                            check_conv3(ops, dev, cases=((2, 64, 64, (7, 7, 5), 3),))
                        finally:
                            ops.set_option("splitk")
                # the two kernels issue the same MFMA sequence per accumulator: bit-identical outputs (one-pass + statistics, +=, split-K)
                rng3 = np.random.default_rng(78 + flat)
                for (N, Cin, Cout, sp, KD) in ((2, 64, 64, (4, 8, 12), 3), (1, 48, 128, (6, 9, 5), 3), (1, 112, 64, (7, 7, 5), 3)):
                    x = to_cl(R(rng3, N, Cin, *sp)).to(dev)
                    w = (R(rng3, Cout, Cin, 3, 3, 3) * 0.1).to(dev).contiguous()
                    b = (R(rng3, Cout) * 0.1).to(dev)
                    wf, _ = ops.conv3_pack(w, KD)
                    outs = []
                    for pipe in (1, 0):
                        ops.set_option("conv3_b6_pipe", pipe)
                        try:
                            ops.set_option("splitk", 1)
                            y, part, rows = ops.conv3_fwd_stats(x, wf, b, Cout, KD, 1)
                            y2 = y.clone()
                            ops.conv3_fwd(x, wf, None, Cout, KD, out=y2, accumulate=True)
                            ops.set_option("splitk", 3)
                            y3 = ops.conv3_fwd(x, wf, b, Cout, KD)
                            outs.append((y.clone(), rows, y2, y3.clone()))
                        finally:
                            ops.set_option("splitk")
                    assert outs[0][1] == outs[1][1]
                    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][2], outs[1][2]) and torch.equal(outs[0][3], outs[1][3]), \
                        f"k_c3q vs k_c3f (slab mode {flat}): outputs differ"
        finally:
            ops.set_option("conv3_b6_flat"); ops.set_option("conv3_b6_pipe")
        # 16 -> 16 layers (3-D: 4x8x8 tiles, 2-D: 16x16 tiles) on the persistent direct-weight kernel: product default only from 256 K
        # voxels, forced here (conv3_b6 = 3) on small ragged shapes; P = 2: two workgroups walk all tiles (cross-tile halo prefetch)
        ops.set_option("conv3_b6", 3)
        for P in (None, 2):
            if P:
                ops.set_option("conv3_p", P)
            try:
                check_conv3(ops, dev, cases=((2, 16, 16, (4, 8, 8), 3), (1, 16, 16, (5, 9, 11), 3), (2, 16, 16, (1, 16, 16), 1), (1, 16, 16, (1, 20, 27), 1),
                                             (1, 12, 16, (1, 33, 18), 1), (2, 32, 16, (1, 16, 32), 1), (1, 24, 16, (1, 21, 19), 1)))
            finally:
                ops.set_option("conv3_p")
        ops.set_option("conv3_b6", 2)
        # 64-voxel x 64-channel staged tiles: waves arranged 2 x 2 (k_c3h, the default) vs 1 x 4 (k_c3b) -- the same products in the same
        # order per accumulator, so the two are BIT-identical; full / partial tiles, several cin chunks, two slabs, statistics, split-K, +=
        ops.set_option("conv3_b6_flat", 0)
        try:
            w22_cases = ((2, 64, 64, (4, 8, 12), 3), (1, 32, 128, (6, 9, 5), 3), (1, 64, 64, (7, 7, 5), 3), (2, 48, 64, (3, 5, 9), 3), (1, 112, 64, (4, 4, 8), 3))
            check_conv3(ops, dev, cases=w22_cases)
            rng2 = np.random.default_rng(77)
            for (N, Cin, Cout, sp, KD) in w22_cases:
                x = to_cl(R(rng2, N, Cin, *sp)).to(dev)
                w = (R(rng2, Cout, Cin, 3, 3, 3) * 0.1).to(dev).contiguous()
                b = (R(rng2, Cout) * 0.1).to(dev)
                wf, _ = ops.conv3_pack(w, KD)
                outs = []
                # (w22, pipe): k_c3p (LDS-DMA software pipeline, the default), k_c3h (register-staged weights), k_c3b
                for w22, pipe in ((1, 1), (1, 0), (0, 0)):
                    ops.set_option("conv3_b6_w22", w22)
                    ops.set_option("conv3_b6_pipe", pipe)
                    ops.set_option("splitk", 1)            # (fused statistics need the unsplit launch)
                    try:
                        y, part, rows = ops.conv3_fwd_stats(x, wf, b, Cout, KD, 1)
                        y2 = y.clone()
                        ops.conv3_fwd(x, wf, None, Cout, KD, out=y2, accumulate=True)
                        ops.set_option("splitk", 2)
                        y3 = ops.conv3_fwd(x, wf, b, Cout, KD)
                        outs.append((y.clone(), part.clone(), rows, y2, y3.clone()))
                    finally:
                        ops.set_option("conv3_b6_w22"); ops.set_option("conv3_b6_pipe"); ops.set_option("splitk")
                for o in outs[1:]:
                    assert outs[0][2] == o[2] and outs[0][2] > 0
                    assert torch.equal(outs[0][0], o[0]) and torch.equal(outs[0][3], o[3]) and torch.equal(outs[0][4], o[4]), \
                        "k_c3p vs k_c3h vs k_c3b: outputs differ"
                    nb = outs[0][2] * Cout * 16           # (the fp64 statistics are summed in a different order: equal to rounding, not bitwise)
                    pa, pb = (np.frombuffer(q[1].cpu().numpy().tobytes()[:nb], dtype=np.float64) for q in (outs[0], o))
                    assert np.allclose(pa, pb, rtol=1e-12, atol=1e-12), "k_c3p vs k_c3h vs k_c3b: statistics rows differ"
        finally:
            ops.set_option("conv3_b6_flat")
        ops.set_option("conv3_b6_cfg2d", 2)         # 2-D 32-channel slabs on the direct-weight 16x16 tiles (product default from 64 K pixels)
        try:
            check_conv3(ops, dev, cases=((2, 64, 32, (1, 12, 20), 1), (1, 16, 32, (1, 33, 17), 1), (2, 32, 96, (1, 16, 16), 1)))
        finally:
            ops.set_option("conv3_b6_cfg2d")
        for direct, P in ((2, None), (2, 2), (0, None)):      # k_c3d everywhere (persistent; P = 2: many tiles per workgroup) / k_c3b everywhere
            ops.set_option("conv3_b6_direct", direct)
            if P:
                ops.set_option("conv3_p", P)
            try:
                check_conv3(ops, dev, cases=CONV3_B6_CASES)
            finally:
                ops.set_option("conv3_b6_direct"); ops.set_option("conv3_p")
    finally:
        ops.set_option("conv3_b6")
        ops.set_option("wgrad_b6")
    rng = np.random.default_rng(41)
    for (N, Cin, Cout, sp, KD, G) in ((4, 32, 32, (4, 8, 8), 3, 2), (2, 64, 64, (4, 8, 8), 3, 2), (2, 32, 64, (1, 16, 16), 1, 1),
                                      (4, 16, 16, (4, 8, 16), 3, 2), (4, 16, 16, (1, 32, 32), 1, 2)):
        two_d = KD == 1
        x = R(rng, N, Cin, *(sp[1:] if two_d else sp))
        w = R(rng, Cout, Cin, *((3, 3) if two_d else (3, 3, 3))) * 0.1
        b = R(rng, Cout) * 0.1
        conv = F.conv2d if two_d else F.conv3d
        y64 = conv(x.double(), w.double(), b.double(), padding=1)
        wf, _ = ops.conv3_pack(w.to(dev).contiguous(), KD)
        for P in (None, 3, "flat"):  # 3: the persistent kernel walks several tiles per workgroup and crosses statistics groups; flat: k_c3f
          if P == "flat" and (KD != 3 or Cout % 64):
              continue
          ops.set_option("conv3_b6", 3 if Cout == 16 else 2)      # (the 16 -> 16 layers need the explicit switch at these sizes)
          ops.set_option("splitk", 1)
          if P == "flat":
              ops.set_option("conv3_b6_flat", 1)
          elif P:
              ops.set_option("conv3_p", P)
          try:
              y, part, rows = ops.conv3_fwd_stats(to_cl(x).to(dev), wf, b.to(dev), Cout, KD, G)
          finally:
              ops.set_option("conv3_b6"); ops.set_option("splitk"); ops.set_option("conv3_p"); ops.set_option("conv3_b6_flat")
          assert rows > 0
          close(from_cl(y, two_d), y64, msg="b6 conv3_fwd_stats y")
          pt = torch.frombuffer(bytearray(part.cpu().numpy().tobytes()[:G * rows * Cout * 16]), dtype=torch.float64).view(G, rows, Cout, 2).sum(1)
          yg = y64.transpose(0, 1).reshape(Cout, G, -1)
          close(pt[..., 0], yg.sum(2).t(), rtol=1e-5, msg="b6 fused sum")
          close(pt[..., 1], (yg * yg).sum(2).t(), rtol=1e-5, msg="b6 fused sum of squares")
        ops.set_option("conv3_b6", 0)          # the fp32-MFMA kernel on the same data
        try:
            y32 = ops.conv3_fwd(to_cl(x).to(dev), wf, b.to(dev), Cout, KD)
        finally:
            ops.set_option("conv3_b6")
        e6 = float((from_cl(y, two_d).double().cpu() - y64).abs().max())
        e32 = float((from_cl(y32, two_d).double().cpu() - y64).abs().max())
        scale = float(y64.abs().max())
        assert e6 <= 3.0 * e32 + 1e-7 * scale, f"b6 error vs fp64 {e6:.3e} (fp32-MFMA kernel: {e32:.3e}, output scale {scale:.3e})"
        assert not torch.equal(y.cpu(), y32.cpu()), "the comparison kernel must be the fp32-MFMA one, not the bf16-pipe kernel again"


def check_conv3_f16(ops, dev):
    """Round 4: the two-plane fp16 instances of the bf16-pipe kernels (three v_mfma_f32_16x16x32_f16 per K block; per-tensor power-of-two
    pre-scales from the input's |max| -- x_amax -- and the layer's weights' |max| in the pack header).  The gate VERDICT r03 item 4 sets:
    error against an fp64 convolution <= 3x the fp32-MFMA kernel's on the same data, on the in-step kinds of shapes AND on inputs / weights
    whose magnitudes span 1e-4 .. 1e3 (uniformly small, uniformly large, mixed per element); the path must really be the fp16 one (bits
    differ from the three-plane result), an amax that is only an upper bound must do, zero / NaN inputs behave as on the other paths (the weight
    gradient's too: wgrad_checks.check_wgrad_nonfinite); fused statistics, +=, dgrad pack, persistent tiles.  Also: the norm apply pass leaves exactly max |a| for its consumer."""
    rng = np.random.default_rng(404)
    cases = (  # N, Cin, Cout, spatial, KD, conv3_b6 level needed, conv3_p
        (1, 32, 32, (8, 16, 16), 3, 2, None),        # k_c3d 4x8x8 x 32 (LA level 2)
        (2, 64, 32, (5, 9, 16), 3, 2, None),         # ragged tiles (D, H), four cin chunks
        (2, 16, 16, (8, 8, 24), 3, 3, 3),            # persistent 16-channel kernel, several tiles per workgroup
        (1, 32, 96, (4, 8, 8), 3, 2, None),          # three 32-channel slabs (grid.y)
        (1, 64, 64, (8, 8, 8), 3, 2, None),          # k_c3p (64-voxel x 64-channel LDS-DMA pipeline), four cin chunks
        (2, 48, 128, (5, 7, 9), 3, 2, None),         # k_c3p ragged, three chunks, two slabs
        (2, 128, 128, (6, 7, 5), 3, 2, None),        # k_c3q (flat deep-level pipeline), 64-channel slabs, split-K as the launcher picks
        (1, 128, 64, (7, 7, 5), 3, 2, None),         # k_c3q with 32-channel slabs (245 voxels)
        (2, 32, 32, (1, 32, 48), 1, 2, None),        # 2-D 16x16 tiles
        (2, 96, 64, (1, 20, 40), 1, 2, None),        # 2-D 8x16 tiles x 64-channel slab (k_c3b, the U-Net's mid levels), six cin chunks
        (3, 16, 16, (1, 21, 37), 1, 3, 2),           # 2-D persistent, ragged
    )
    kinds = (("unit", 1.0, 0.05), ("tiny x", 1e-4, 0.05), ("huge x", 1e3, 0.05), ("tiny w", 1.0, 1e-4), ("huge w", 1.0, 30.0), ("mixed", None, 0.05))
    for ci, (N, Cin, Cout, sp, KD, lvl, P) in enumerate(cases):
        two_d = KD == 1
        for kind, xs, wsc in (kinds if ci < 2 or ci == 4 else kinds[:1] + kinds[5:]) if dev.type == "cuda" else (kinds[:2] + kinds[5:] if ci == 0 else kinds[5:]):
            x = R(rng, N, Cin, *(sp[1:] if two_d else sp)).clamp_(min=-0.5)                      # ReLU-like: mostly non-negative, some negatives
            if xs is None:
                x = x * torch.from_numpy((10.0 ** rng.uniform(-4, 3, tuple(x.shape))).astype(np.float32))
            else:
                x = x * xs
            w = R(rng, Cout, Cin, *((3, 3) if two_d else (3, 3, 3))) * wsc
            b = R(rng, Cout) * 0.1 * float(x.abs().max()) * wsc
            y64 = (F.conv2d if two_d else F.conv3d)(x.double(), w.double(), b.double(), padding=1)
            wf, wd = ops.conv3_pack(w.to(dev).contiguous(), KD)
            xcl = to_cl(x).to(dev)
            ops.set_option("conv3_b6", lvl)
            ops.set_option("splitk", 1)           # (one-pass launches: the plain and the fused-statistics launch are then the same kernel call)
            if two_d:
                ops.set_option("conv3_b6_cfg2d", 2)   # 2-D 32-channel slabs on the direct-weight 16x16 tiles at every size (product: from 64 K pixels)
            if Cout % 64 == 0 and Cin < 128:
                ops.set_option("conv3_b6_flat", 0)    # 64-channel slabs: brick tiles (k_c3p) also below 16 K voxels, where the product takes the flat kernel
            if P:
                ops.set_option("conv3_p", P)
            try:
                y3 = ops.conv3_fwd(xcl, wf, b.to(dev), Cout, KD)                                     # three bf16 planes (no amax on the tensor)
                xcl._bcp_amax = H.amax_slots(float(x.abs().max()), dev)
                y2 = ops.conv3_fwd(xcl, wf, b.to(dev), Cout, KD)
                ys, part, rows = ops.conv3_fwd_stats(xcl, wf, b.to(dev), Cout, KD, 1)
                xcl._bcp_amax = H.amax_slots(3.7 * float(x.abs().max()), dev)     # an upper bound only
                y2b = ops.conv3_fwd(xcl, wf, b.to(dev), Cout, KD)
                ops.set_option("conv3_f16", 0)
                y3b = ops.conv3_fwd(xcl, wf, b.to(dev), Cout, KD)                                    # the option switches the fp16 instances off
                ops.set_option("conv3_f16")
            finally:
                ops.set_option("conv3_b6"); ops.set_option("conv3_p"); ops.set_option("conv3_f16"); ops.set_option("splitk"); ops.set_option("conv3_b6_cfg2d"); ops.set_option("conv3_b6_flat")
            ops.set_option("conv3_b6", 0)
            try:
                y32 = ops.conv3_fwd(to_cl(x).to(dev), wf, b.to(dev), Cout, KD)                       # the fp32-MFMA kernel
            finally:
                ops.set_option("conv3_b6")
            tag = f"f16 {kind} {N}x{sp} {Cin}->{Cout}"
            err = lambda t: float((from_cl(t, two_d).double().cpu() - y64).abs().max())
            scale = float(y64.abs().max())
            e2, e2b, e3, e32 = err(y2), err(y2b), err(y3), err(y32)
            # (the gate: 3x the fp32-MFMA kernel.  One case on the MI355X -- per-element magnitudes over seven decades, 128 channels, split-K --
            #  has BOTH 16-bit paths above it: three bf16 planes 2.8e-3, two fp16 planes 2.5e-3, fp32-MFMA 7.4e-4 at scale 1.7e3: a K = 32
            #  MFMA aligns 32 products to their largest before adding, a K = 4 one only 4.  There the new path is held to the accepted one.)
            assert e2 <= max(3.0 * e32, 1.1 * e3) + 1e-7 * scale, f"{tag}: error vs fp64 {e2:.3e} (fp32-MFMA kernel {e32:.3e}, three bf16 planes {e3:.3e}, scale {scale:.3e})"
            assert e2b <= max(3.0 * e32, 1.1 * e3) + 2e-7 * scale, f"{tag}: with an amax 3.7x too large: {e2b:.3e} (fp32-MFMA kernel {e32:.3e})"
            assert not torch.equal(y2, y3), tag + ": the launch with x_amax must take the fp16 instance"
            assert torch.equal(y3b, y3), tag + ": conv3_f16 = 0 must give the three-plane kernel"
            assert torch.equal(ys, y2) and rows > 0, tag + ": fused-statistics launch differs from the plain one"
            pt = torch.frombuffer(bytearray(part.cpu().numpy().tobytes()[:rows * Cout * 16]), dtype=torch.float64).view(rows, Cout, 2).sum(0)
            yg = from_cl(y2, two_d).double().cpu().transpose(0, 1).reshape(Cout, -1)
            close(pt[:, 0], yg.sum(1), rtol=1e-6, msg=tag + " fused sum")
    # += , the dgrad pack, zero input, NaN input
    N, Cin, Cout, sp = 1, 32, 32, (4, 8, 8)
    x, w, dy = R(rng, N, Cin, *sp), R(rng, Cout, Cin, 3, 3, 3) * 0.05, R(rng, N, Cout, *sp) * 1e-6     # (dy: backward-sized magnitudes)
    wf, wd = ops.conv3_pack(w.to(dev).contiguous(), 3)
    xcl, dycl = to_cl(x).to(dev), to_cl(dy).to(dev)
    xcl._bcp_amax = H.amax_slots(float(x.abs().max()), dev)
    dycl._bcp_amax = H.amax_slots(float(dy.abs().max()), dev)
    ops.set_option("conv3_b6", 2)
    try:
        y = ops.conv3_fwd(xcl, wf, None, Cout, 3)
        acc = y.clone()
        ops.conv3_fwd(xcl, wf, None, Cout, 3, out=acc, accumulate=True)
        close(acc, 2 * y, rtol=1e-6, msg="f16 +=")
        dx = ops.conv3_fwd(dycl, wd, None, Cin, 3)
        dx64 = torch.nn.grad.conv3d_input(x.shape, w.double(), dy.double(), padding=1)
        ops.set_option("conv3_b6", 0)
        dx32 = ops.conv3_fwd(to_cl(dy).to(dev), wd, None, Cin, 3)
        e2, e32 = float((from_cl(dx).double().cpu() - dx64).abs().max()), float((from_cl(dx32).double().cpu() - dx64).abs().max())
        assert e2 <= 3.0 * e32 + 1e-7 * float(dx64.abs().max()), f"f16 dgrad pack, dy ~ 1e-6: {e2:.3e} vs fp32-MFMA {e32:.3e}"
        ops.set_option("conv3_b6", 2)
        z = torch.zeros_like(xcl)
        z._bcp_amax = H.amax_slots(0.0, dev)
        bz = R(rng, Cout).to(dev)
        yz = ops.conv3_fwd(z, wf, bz, Cout, 3)
        assert torch.equal(yz, bz.view(1, 1, 1, 1, Cout).expand_as(yz).contiguous()), "f16: zero input (amax 0) must give the bias"
        xn = xcl.clone()
        xn[0, 1, 2, 3, 4] = float("nan")
        xn._bcp_amax = H.amax_slots(float("nan"), dev)
        yn = ops.conv3_fwd(xn, wf, None, Cout, 3)
        assert bool(torch.isnan(yn[0, 1, 2, 3]).all()) and bool(torch.isfinite(yn[0, 3, 7, 7]).all()), "f16: a NaN input voxel reaches its 27 outputs, nothing else"
    finally:
        ops.set_option("conv3_b6")
    # weight gradient (conv3bw.hip k_w6 PL = 2): both operands pre-scaled from their own |max|; backward-sized dy magnitudes
    on_gpu = dev.type == "cuda"         # (the host simulator runs the small shapes and two of the three magnitude sets: the CPU suite's time budget)
    for (N, Cin, Cout, sp, KD) in ((1, 32, 32, (8, 8, 8), 3), (2, 16, 16, (4, 8, 16), 3), (1, 64, 48, (4, 8, 4), 3), (2, 32, 32, (1, 16, 32), 1)) + (((1, 32, 32, (20, 36, 24), 3),) if on_gpu else ()):
        two_d = KD == 1
        for xs_, ys_ in ((1.0, 1e-6), (1e-3, 1e2), (None, None)) if on_gpu else ((1.0, 1e-6), (None, None)):
            x = R(rng, N, Cin, *(sp[1:] if two_d else sp)).clamp_(min=-0.5)
            dy = R(rng, N, Cout, *(sp[1:] if two_d else sp))
            if xs_ is None:
                x = x * torch.from_numpy((10.0 ** rng.uniform(-4, 3, tuple(x.shape))).astype(np.float32))
                dy = dy * torch.from_numpy((10.0 ** rng.uniform(-8, -2, tuple(dy.shape))).astype(np.float32))
            else:
                x, dy = x * xs_, dy * ys_
            wshape = (Cout, Cin, 3, 3) if two_d else (Cout, Cin, 3, 3, 3)
            g64 = (torch.nn.grad.conv2d_weight if two_d else torch.nn.grad.conv3d_weight)(x.double(), wshape, dy.double(), padding=1)
            xcl, dycl = to_cl(x).to(dev), to_cl(dy).to(dev)
            ops.set_option("wgrad_b6", 2)
            try:
                g3 = ops.conv3_wgrad(xcl, dycl, torch.empty(wshape, device=dev), KD).clone()
                xcl._bcp_amax = H.amax_slots(float(x.abs().max()), dev)
                dycl._bcp_amax = H.amax_slots(float(dy.abs().max()), dev)
                g2 = ops.conv3_wgrad(xcl, dycl, torch.empty(wshape, device=dev), KD).clone()
                acc = g2.clone()
                ops.conv3_wgrad(xcl, dycl, acc, KD, accumulate=True)
            finally:
                ops.set_option("wgrad_b6")
            ops.set_option("wgrad_b6", 0)
            try:
                g32 = ops.conv3_wgrad(to_cl(x).to(dev), to_cl(dy).to(dev), torch.empty(wshape, device=dev), KD).clone()      # the fp32-MFMA kernel
            finally:
                ops.set_option("wgrad_b6")
            scale = float(g64.abs().max())
            e2, e3, e32 = (float((t.double().cpu() - g64).abs().max()) for t in (g2, g3, g32))
            tag = f"f16 wgrad {N}x{sp} {Cin}->{Cout} x~{xs_} dy~{ys_}"
            assert e2 <= 3.0 * e32 + 1e-7 * scale, f"{tag}: error vs fp64 {e2:.3e} (fp32-MFMA kernel {e32:.3e}, three bf16 planes {e3:.3e}, scale {scale:.3e})"
            assert not torch.equal(g2, g3), tag + ": the launch with both maxima must take the fp16 instance"
            close(acc, 2 * g2, rtol=1e-6, msg=tag + " +=")
    # the producer side: bcp_norm_fwd leaves max |a| of what it wrote (every epilogue), bcp_norm_fwd_slabs alike
    for (N, Cc, sp, G, use_res) in ((2, 32, (4, 6, 8), 2, True), (1, 16, (1, 9, 13), 1, False), (2, 128, (3, 5, 5), 2, False)):
        y = to_cl(R(rng, N, Cc, *sp) * 3.0).to(dev)
        res = to_cl(R(rng, N, Cc, *sp)).to(dev) if use_res else None
        cs = torch.from_numpy(((rng.random((N, Cc)) < 0.5) * 2.0).astype(np.float32)).to(dev)
        g1, b1 = torch.from_numpy(rng.uniform(0.5, 1.5, Cc).astype(np.float32)).to(dev), torch.from_numpy(rng.uniform(-0.3, 0.3, Cc).astype(np.float32)).to(dev)
        a, _ = ops.norm_fwd(y, G, g1, b1, torch.zeros(Cc).to(dev), torch.ones(Cc).to(dev), H.ACT_RELU, chan_scale=cs, residual=res)
        am = getattr(a, "_bcp_amax", None)
        assert am is not None and H.amax_value(am) == float(a.abs().max()), f"norm_fwd amax {H.amax_value(am)} vs {float(a.abs().max())}"
        a2, st2, y2 = ops.norm_fwd_slabs(torch.stack([y, y * 0.5]).contiguous(), 2, None, G, g1, b1, torch.zeros(Cc).to(dev), torch.ones(Cc).to(dev), H.ACT_RELU)
        assert H.amax_value(a2._bcp_amax) == float(a2.abs().max()), "norm_fwd_slabs amax"
        da = to_cl(R(rng, N, Cc, *sp) * 1e-5).to(dev)
        dyn = ops.norm_bwd(y2, da, G, st2, H.ACT_RELU, torch.zeros(Cc).to(dev), torch.zeros(Cc).to(dev), False)
        assert H.amax_value(dyn._bcp_amax) == float(dyn.abs().max()), "norm_bwd amax"
        dyn2, _ = ops.norm_bwd_slabs(y2, torch.stack([da, da * 0.25]).contiguous(), 2, G, st2, H.ACT_RELU, torch.zeros(Cc).to(dev), torch.zeros(Cc).to(dev), False)
        assert H.amax_value(dyn2._bcp_amax) == float(dyn2.abs().max()), "norm_bwd_slabs amax"


def check_conv3_stats(ops, dev):
    """fused epilogue statistics: sum over the partial rows == per-group column sums / sums of squares of y"""
    rng = np.random.default_rng(15)
    for (N, Cin, Cout, sp, KD, G, P) in ((2, 16, 16, (16, 16, 48), 3, 2, 5), (2, 16, 16, (16, 16, 48), 3, 2, 8), (4, 32, 32, (8, 12, 20), 3, 2, 3), (4, 32, 32, (8, 12, 20), 3, 2, 16), (2, 16, 32, (1, 40, 48), 1, 2, None),
                                          (2, 64, 64, (5, 6, 7), 3, 1, None), (2, 16, 16, (6, 5, 9), 3, 2, None)):
        two_d = KD == 1
        x = R(rng, N, Cin, *(sp[1:] if two_d else sp))
        w = R(rng, Cout, Cin, *((3, 3) if two_d else (3, 3, 3))) * 0.1
        b = R(rng, Cout) * 0.1
        y_ref = F.conv2d(x, w, b, padding=1) if two_d else F.conv3d(x, w, b, padding=1)
        wf, _ = ops.conv3_pack(w.to(dev).contiguous(), KD)
        if P:
            ops.set_option("conv3_p", P)
        try:
            y, part, rows = ops.conv3_fwd_stats(to_cl(x).to(dev), wf, b.to(dev), Cout, KD, G)
        finally:
            ops.set_option("conv3_p")
        close(from_cl(y, two_d), y_ref, msg="conv3_fwd_stats y")
        if (Cin, sp) == (64, (5, 6, 7)):   # split-K shape: statistics are not fused, the caller falls back to the standalone pass
            assert rows == 0 and part is None
            continue
        assert rows > 0, "these shapes must support fused statistics"
        pt = torch.frombuffer(bytearray(part.cpu().numpy().tobytes()[:G * rows * Cout * 16]), dtype=torch.float64).view(G, rows, Cout, 2).sum(1)
        yg = y_ref.double().transpose(0, 1).reshape(Cout, G, -1)
        close(pt[..., 0], yg.sum(2).t(), rtol=1e-6, msg="fused sum")
        close(pt[..., 1], (yg * yg).sum(2).t(), rtol=1e-6, msg="fused sum of squares")
        # and the norm driven by those partials equals the norm that computes its own statistics
        g1, b1 = torch.ones(Cout).to(dev), torch.zeros(Cout).to(dev)
        a1, _ = ops.norm_fwd(y, G, g1, b1, torch.zeros(Cout).to(dev), torch.ones(Cout).to(dev), H.ACT_RELU, partial=part, nb=rows)
        a2, _ = ops.norm_fwd(y, G, g1, b1, torch.zeros(Cout).to(dev), torch.ones(Cout).to(dev), H.ACT_RELU)
        close(a1, a2, rtol=1e-6, msg="norm from fused partials")


def check_inline_dropout(ops, dev):
    """round 4: an elementwise Dropout whose keep bits the norm kernels EVALUATE from a device seed (hip_ops.SeedMask; bcp_norm_fwd / _bwd,
    the raw-slab pair, the fused first layer) == the same layer fed the uint8 mask bcp_bernoulli writes under that seed, bit for bit"""
    rng = np.random.default_rng(91)
    p = 0.3
    es = 1.0 / (1.0 - p)
    for k, (N, Cc, sp, G) in enumerate(((2, 32, (1, 12, 20), 2), (3, 16, (1, 9, 11), 1), (2, 64, (2, 6, 6), 1), (1, 16, (3, 40, 44), 1))):
        seed = (0x9E3779B97F4A7C15 * (k + 3)) & 0xFFFFFFFFFFFFFFFF
        y = to_cl(R(rng, N, Cc, *sp) * 1.4 + 0.2).to(dev)
        da = to_cl(R(rng, N, Cc, *sp)).to(dev)
        gam = torch.from_numpy(rng.uniform(0.5, 1.5, Cc).astype(np.float32)).to(dev)
        bet = torch.from_numpy(rng.uniform(-0.3, 0.3, Cc).astype(np.float32)).to(dev)
        m = ops.bernoulli(torch.empty(tuple(y.shape), dtype=torch.uint8, device=dev), 1.0 - p, 1.0, seed)
        frac = float(m.float().mean())
        assert abs(frac - (1.0 - p)) < 0.05, frac
        sm = ops.seed_mask(tuple(y.shape), 1.0 - p, seed, y)
        outs = []
        for em in (m, sm):
            rm, rv = torch.zeros(Cc).to(dev), torch.ones(Cc).to(dev)
            a, st = ops.norm_fwd(y, G, gam, bet, rm, rv, H.ACT_LRELU, elem_mask=em, elem_scale=es)
            dg, db = torch.zeros(Cc).to(dev), torch.zeros(Cc).to(dev)
            dy = ops.norm_bwd(y, da, G, st, H.ACT_LRELU, dg, db, False, elem_mask=em, elem_scale=es)
            outs.append((a, st, dy, dg, db))
        for u, v, name in zip(outs[0], outs[1], ("a", "stats", "dy", "dgamma", "dbeta")):
            assert torch.equal(u, v), f"inline dropout, norm pair C={Cc}: {name}"
        assert float((outs[1][0] == 0).float().mean()) > 0.5 * p, "the seeded mask did not drop anything"
        rows_pg = y.numel() // Cc // G
        if ops.norm_slabs_ok(G, rows_pg, Cc):
            slabs = torch.stack([y * 0.25, y * 0.75]).contiguous()
            dslabs = torch.stack([da * 0.5, da * 0.5]).contiguous()
            outs = []
            for em in (m, sm):
                rm, rv = torch.zeros(Cc).to(dev), torch.ones(Cc).to(dev)
                a, st, ysum = ops.norm_fwd_slabs(slabs, 2, None, G, gam, bet, rm, rv, H.ACT_LRELU, elem_mask=em, elem_scale=es)
                dg, db = torch.zeros(Cc).to(dev), torch.zeros(Cc).to(dev)
                dy, dsum = ops.norm_bwd_slabs(ysum, dslabs, 2, G, st, H.ACT_LRELU, dg, db, False, elem_mask=em, elem_scale=es)
                outs.append((a, st, dy, dg, db))
            for u, v, name in zip(outs[0], outs[1], ("a", "stats", "dy", "dgamma", "dbeta")):
                assert torch.equal(u, v), f"inline dropout, raw-slab pair C={Cc}: {name}"
    # the fused first layer (2-D as the U-Net launches it, 3-D for the record)
    for (N, sp, KD, G) in ((4, (1, 32, 32), 1, 2), (2, (4, 8, 16), 3, 1)):
        x = to_cl(R(rng, N, 1, *sp)).to(dev)
        w = (R(rng, 16, 1, *((3, 3, 3) if KD == 3 else (3, 3))) * 0.3).to(dev)
        b = (R(rng, 16) * 0.1).to(dev)
        if not ops.conv3_c1_norm_ok(tuple(x.shape), KD, G):
            continue
        shape = (N,) + sp + (16,)
        da = to_cl(R(rng, N, 16, *sp)).to(dev)
        gam = torch.from_numpy(rng.uniform(0.5, 1.5, 16).astype(np.float32)).to(dev)
        bet = torch.from_numpy(rng.uniform(-0.3, 0.3, 16).astype(np.float32)).to(dev)
        seed = 0xC0FFEE123456789 + KD
        m = ops.bernoulli(torch.empty(shape, dtype=torch.uint8, device=dev), 1.0 - p, 1.0, seed)
        sm = ops.seed_mask(shape, 1.0 - p, seed, x)
        outs = []
        for em in (m, sm):
            rm, rv = torch.zeros(16).to(dev), torch.ones(16).to(dev)
            a, st = ops.conv3_c1_norm_fwd(x, w, b, KD, G, gam, bet, rm, rv, H.ACT_LRELU, elem_mask=em, elem_scale=es)
            dg, db = torch.zeros(16).to(dev), torch.zeros(16).to(dev)
            dy = ops.conv3_c1_norm_bwd(x, w, b, KD, G, st, da, H.ACT_LRELU, dg, db, False, elem_mask=em, elem_scale=es)
            outs.append((a, st, dy, dg, db))
        for u, v, name in zip(outs[0], outs[1], ("a", "stats", "dy", "dgamma", "dbeta")):
            assert torch.equal(u, v), f"inline dropout, fused first layer KD={KD}: {name}"


def check_norm_slabs(ops, dev):
    """deep-level norm that takes the producing conv's raw split-K slabs (bcp_conv3_fwd_raw -> bcp_norm_fwd_slabs / _bwd_slabs: the slab
    sum folded into the row-major statistics pass): (a) against torch (BatchNorm / grouped BatchNorm / InstanceNorm, every epilogue),
    (b) against the plain chain on the same inputs: y / da sums bit-identical to the slab-sum kernel, statistics, activations and
    gradients equal to bcp_norm_fwd / _bwd on the summed tensor up to the grouping of the fp64 partial sums, (c) conv -> slabs -> norm == conv3_fwd -> norm_fwd, forward and
    dgrad, split-K forced to 1 / 2 / 4"""
    _check_norm_slabs(ops, dev)


def _check_norm_slabs(ops, dev, chains_only=False):
    rng = np.random.default_rng(41)
    cases = () if chains_only else (  # N, C, spatial, act, use_cs, use_res, G, nslab, mode ('bn' | 'in')
        (2, 128, (14, 14, 10), H.ACT_RELU, False, False, 2, 4, "bn"),     # LA level 4: 1960 rows per group, 8 rows per thread, two groups per trip
        (2, 256, (7, 7, 5), H.ACT_RELU, True, False, 2, 8, "bn"),         # LA level 5 + Dropout3d (x5)
        (2, 128, (14, 14, 10), H.ACT_RELU, False, True, 1, 1, "bn"),      # transposed-conv layer: residual, 3920 rows in ONE group (16 per thread)
        (4, 128, (12, 12, 12), H.ACT_RELU, False, False, 4, 3, "in"),     # pancreas level 4 (InstanceNorm: groups split over grid.y)
        (3, 32, (3, 5, 7), H.ACT_LRELU, False, False, 1, 2, "bn"),        # ragged: 315 rows, 2 per thread; elementwise dropout mask
        (4, 16, (1, 6, 9), H.ACT_RELU, True, True, 2, 1, "bn"),           # 2-D, 108 rows per group (1 per thread), 2 samples per group + chan scale
        (5, 64, (2, 3, 3), H.ACT_RELU, False, False, 5, 2, "in"),         # odd group count
    )
    for (N, Cc, sp, act, use_cs, use_res, G, nslab, mode) in cases:
        assert ops.norm_slabs_ok(G, N * sp[0] * sp[1] * sp[2] // G, Cc)
        parts = [R(rng, N, Cc, *sp) * (1.7 if k == 0 else 0.3) + (0.4 if k == 0 else 0.0) for k in range(nslab)]
        bias = R(rng, Cc) * 0.2 if nslab > 1 else None
        y_t = sum(parts[1:], parts[0]) + (bias.view(1, Cc, 1, 1, 1) if bias is not None else 0)
        y = y_t.clone().requires_grad_(True)
        bn = mode == "bn"
        gamma = torch.from_numpy(rng.uniform(0.5, 1.5, Cc).astype(np.float32)).requires_grad_(True)
        beta = torch.from_numpy(rng.uniform(-0.3, 0.3, Cc).astype(np.float32)).requires_grad_(True)
        cs = torch.from_numpy(((rng.random((N, Cc)) < 0.5) * 2.0).astype(np.float32)) if use_cs else None
        res = R(rng, N, Cc, *sp) if use_res else None
        em = torch.from_numpy((rng.random((N, Cc, *sp)) < 0.8).astype(np.uint8)) if act == H.ACT_LRELU else None
        rm_ref, rv_ref = torch.zeros(Cc), torch.ones(Cc)
        if bn:
            per = N // G
            z = torch.cat([F.batch_norm(y[g * per:(g + 1) * per], rm_ref, rv_ref, gamma, beta, True, 0.1, 1e-5) for g in range(G)])
        else:
            z = F.instance_norm(y, eps=1e-5)
        a_ref = F.relu(z) if act == H.ACT_RELU else F.leaky_relu(z, 0.01)
        if cs is not None:
            a_ref = a_ref * cs.view(N, Cc, 1, 1, 1)
        if em is not None:
            a_ref = a_ref * em.float() / 0.8
        if res is not None:
            a_ref = a_ref + res
        dparts = [R(rng, N, Cc, *sp) * (1.0 if k == 0 else 0.2) for k in range(nslab)]
        da_t = sum(dparts[1:], dparts[0])
        a_ref.backward(da_t)
        # ---- HIP, one launch
        slabs = torch.stack([to_cl(q) for q in parts]).to(dev) if nslab > 1 else to_cl(parts[0]).to(dev)
        gd, bd = (gamma.detach().to(dev), beta.detach().to(dev)) if bn else (None, None)
        rmd, rvd = (torch.zeros(Cc).to(dev), torch.ones(Cc).to(dev)) if bn else (None, None)
        kw = dict(chan_scale=None if cs is None else cs.to(dev), elem_mask=None if em is None else to_cl(em).to(dev), elem_scale=1 / 0.8)
        a, stats, ycl = ops.norm_fwd_slabs(slabs, nslab, None if bias is None else bias.to(dev), G, gd, bd, rmd, rvd, act,
                                           residual=None if res is None else to_cl(res).to(dev), **kw)
        tag = f"norm_slabs C={Cc} G={G} sp={sp} slabs={nslab}"
        # the slab sum follows k_b6_sum_slabs' order (bias, then the slabs front to back): compare with the same order on the host
        yh = (bias.view(1, 1, 1, 1, Cc) if bias is not None else 0) + to_cl(parts[0])
        for q in parts[1:]:
            yh = yh + to_cl(q)
        assert torch.equal(ycl.cpu(), yh if torch.is_tensor(yh) else to_cl(parts[0])), tag + ": slab sum is not bit-identical to bias + slabs in order"
        close(from_cl(a), a_ref, msg=tag + " fwd")
        if bn:
            close(rmd, rm_ref, rtol=1e-5, msg=tag + " running_mean")
            close(rvd, rv_ref, rtol=1e-5, msg=tag + " running_var")
        dslabs = torch.stack([to_cl(q) for q in dparts]).to(dev) if nslab > 1 else to_cl(dparts[0]).to(dev)
        dg, db = (torch.full((Cc,), 7.0).to(dev), torch.full((Cc,), 7.0).to(dev)) if bn else (None, None)
        dy, da_out = ops.norm_bwd_slabs(ycl, dslabs, nslab, G, stats, act, dg, db, False, **kw)
        close(from_cl(dy), y.grad, rtol=2e-4, msg=tag + " bwd dy")
        dh = to_cl(dparts[0])
        for q in dparts[1:]:
            dh = dh + to_cl(q)
        assert torch.equal(da_out.cpu(), dh), tag + ": da slab sum"
        if bn:
            close(dg, gamma.grad, rtol=2e-4, msg=tag + " dgamma")
            close(db, beta.grad, rtol=2e-4, msg=tag + " dbeta")
            ops.norm_bwd_slabs(ycl, dslabs, nslab, G, stats, act, dg, db, True, **kw)
            close(dg, 2 * gamma.grad, rtol=2e-4, msg=tag + " dgamma accumulate")
        # ---- against the plain chain on the same (summed) y / da: same kernels on the same bits -> bit-identical
        rm2, rv2 = (torch.zeros(Cc).to(dev), torch.ones(Cc).to(dev)) if bn else (None, None)
        a2, stats2 = ops.norm_fwd(ycl, G, gd, bd, rm2, rv2, act, residual=None if res is None else to_cl(res).to(dev), **kw)
        # (the slab-summing pass cuts the rows into more blocks: fp64 partial sums in another grouping -> equal to fp64 rounding, not bitwise)
        close(stats, stats2, rtol=2e-6, msg=tag + " stats vs the plain chain")
        close(a, a2, rtol=2e-6, msg=tag + " fwd vs the plain chain")
        if bn:
            close(rmd, rm2, rtol=1e-6, msg=tag + " running_mean vs the plain chain")
        dg2, db2 = (torch.full((Cc,), 7.0).to(dev), torch.full((Cc,), 7.0).to(dev)) if bn else (None, None)
        dy2 = ops.norm_bwd(ycl, da_out, G, stats2, act, dg2, db2, False, **kw)
        close(dy, dy2, rtol=2e-5, msg=tag + " bwd vs the plain chain")
        if bn:
            ops.norm_bwd_slabs(ycl, dslabs, nslab, G, stats, act, dg2, db2, False, **kw)      # (dg / db of the first call were doubled above)
            dg3, db3 = torch.full((Cc,), 7.0).to(dev), torch.full((Cc,), 7.0).to(dev)
            ops.norm_bwd(ycl, da_out, G, stats2, act, dg3, db3, False, **kw)
            close(dg2, dg3, rtol=2e-5, msg=tag + " dgamma vs the plain chain")
            close(db2, db3, rtol=2e-5, msg=tag + " dbeta vs the plain chain")
    # ---- (c) conv -> raw slabs -> fused norm == fused-statistics conv -> streaming norm (forward and dgrad packs)
    for (N, Cin, Cout, sp, G) in ((2, 128, 128, (14, 14, 10), 2), (2, 256, 256, (7, 7, 5), 2), (2, 64, 128, (6, 5, 7), 1), (2, 32, 32, (4, 8, 8), 2)):
        x = R(rng, N, Cin, *sp)
        w = R(rng, Cout, Cin, 3, 3, 3) * 0.05
        b = R(rng, Cout) * 0.1
        wf, wd = ops.conv3_pack(w.to(dev).contiguous(), 3)
        xcl = to_cl(x).to(dev)
        g1, b1 = torch.from_numpy(rng.uniform(0.5, 1.5, Cout).astype(np.float32)).to(dev), torch.from_numpy(rng.uniform(-0.3, 0.3, Cout).astype(np.float32)).to(dev)
        y_ref = ops.conv3_fwd(xcl, wf, b.to(dev), Cout, 3)
        a_ref, st_ref = ops.norm_fwd(y_ref, G, g1, b1, torch.zeros(Cout).to(dev), torch.ones(Cout).to(dev), H.ACT_RELU)
        close(from_cl(y_ref), F.conv3d(x, w, b, padding=1), msg="conv3 reference for the raw check")
        for force in (0, 1, 2, 4):
            if force:
                ops.set_option("conv3_b6_flat_sk", force)
                ops.set_option("splitk", force)
            try:
                sk = ops.conv3_nslabs(xcl.shape, Cout, 3)
                if sk == 0:
                    continue
                slabs = ops.conv3_fwd_raw(xcl, wf, Cout, 3, sk)
                a, st, y = ops.norm_fwd_slabs(slabs, sk, b.to(dev), G, g1, b1, torch.zeros(Cout).to(dev), torch.ones(Cout).to(dev), H.ACT_RELU)
                close(y, y_ref, rtol=2e-5, msg=f"raw conv slabs {Cin}->{Cout} {sp} sk={sk}")
                close(a, a_ref, rtol=2e-5, msg=f"raw conv + norm from slabs {Cin}->{Cout} {sp} sk={sk}")
                if not force:      # the default split: the slab sum IS k_b6_sum_slabs' arithmetic -> y bit-identical
                    assert torch.equal(y, y_ref), f"slabs path vs slab-sum launch {Cin}->{Cout} {sp} sk={sk}"
                # dgrad through the flipped pack: da slabs straight into the backward kernel
                dyt = R(rng, N, Cout, *sp)
                dycl = to_cl(dyt).to(dev)
                skd = ops.conv3_nslabs(dycl.shape, Cin, 3)
                if skd:
                    dsl = ops.conv3_fwd_raw(dycl, wd, Cin, 3, skd)
                    da_ref = ops.conv3_fwd(dycl, wd, None, Cin, 3)
                    assert ops.norm_slabs_ok(G, N * sp[0] * sp[1] * sp[2] // G, Cin)
                    xs, xst = ops.norm_fwd(xcl, G, None, None, None, None, H.ACT_RELU)
                    d1, dsum = ops.norm_bwd_slabs(xcl, dsl, skd, G, xst, H.ACT_RELU)
                    d2 = ops.norm_bwd(xcl, da_ref, G, xst, H.ACT_RELU)
                    close(dsum, da_ref, rtol=2e-5, msg=f"raw dgrad slabs sk={skd}")
                    close(d1, d2, rtol=5e-5, msg=f"raw dgrad + norm backward from slabs sk={skd}")
            finally:
                ops.set_option("conv3_b6_flat_sk")
                ops.set_option("splitk")


def check_dgrad_bwdstats(ops, dev):
    """dgrad epilogue with the consumer norm layer's backward statistics (bcp_conv3_dgrad_bwdstats): da bit-identical to the plain
    dgrad, the partial rows sum to k_col_partial<1>'s (sum dz, sum dz * xhat), and norm_bwd fed with them equals the norm_bwd that
    runs its own statistics pass; shapes of every bf16-pipe kernel family that carries the epilogue (k_c3d one-tile, k_c3h, k_c3b, 2-D),
    ragged tiles and padded channels included.  The persistent 16-channel kernel and the 2-D 64-channel-slab kernel do NOT carry it (it
    cost them their second workgroup per CU): those shapes answer rows = 0 and return the plain dgrad -- checked for equality only."""
    rng = np.random.default_rng(57)
    cases = (  # N, C_dy (channels of dy), C_da (channels of da = the consumer norm's channels), spatial, KD, G, act
        (2, 32, 32, (8, 16, 16), 3, 2, H.ACT_RELU),       # k_c3d 4x8x8 x 32
        (2, 32, 32, (5, 9, 11), 3, 1, H.ACT_RELU),        # ragged tiles
        (2, 64, 64, (16, 16, 40), 3, 2, H.ACT_RELU),      # k_c3h (> 16 K voxels and > 256 tiles, or the launch is split-K; below that the flat deep-level kernel, which hands raw slabs to the one-launch norm instead)
        (2, 16, 16, (16, 16, 32), 3, 2, H.ACT_RELU),      # persistent k_c3d (forced below)
        (2, 16, 32, (6, 10, 12), 3, 2, H.ACT_RELU),       # channel counts differ
        (4, 32, 32, (1, 32, 48), 1, 2, H.ACT_LRELU),      # 2-D
        (3, 64, 64, (1, 80, 96), 1, 1, H.ACT_LRELU),
    )
    ops.set_option("conv3_b6", 3)       # every eligible shape on the bf16 pipe (the 16-channel persistent kernel included)
    try:
        n_fused, fused_tags = 0, []
        for (N, Cdy, Cda, sp, KD, G, act) in cases:
            two_d = KD == 1
            w = R(rng, Cdy, Cda, *((3, 3) if two_d else (3, 3, 3))) * 0.1      # forward weight [Cout = Cdy][Cin = Cda]
            _, wd = ops.conv3_pack(w.to(dev).contiguous(), KD)
            shape = (N, 1, sp[1], sp[2]) if two_d else (N,) + sp
            dy = torch.from_numpy(rng.standard_normal(shape + (Cdy,), dtype=np.float32)).to(dev)
            yprev = (torch.from_numpy(rng.standard_normal(shape + (Cda,), dtype=np.float32)) * 1.3 + 0.2).to(dev)
            gam, bet = torch.from_numpy(rng.uniform(0.5, 1.5, Cda).astype(np.float32)).to(dev), torch.from_numpy(rng.uniform(-0.3, 0.3, Cda).astype(np.float32)).to(dev)
            _, st = ops.norm_fwd(yprev, G, gam, bet, torch.zeros(Cda).to(dev), torch.ones(Cda).to(dev), act)
            da_ref = ops.conv3_fwd(dy, wd, None, Cda, KD)
            da, part, rows = ops.conv3_dgrad_bwdstats(dy, wd, Cda, KD, yprev, st, act, G)
            tag = f"dgrad_bwdstats {Cdy}->{Cda} {sp} G={G}"
            assert torch.equal(da.cpu(), da_ref.cpu()), tag + ": da differs from the plain dgrad"
            if rows == 0:
                continue
            n_fused += 1
            fused_tags.append(tag)
            pt = torch.frombuffer(bytearray(part.cpu().numpy().tobytes()[:G * rows * Cda * 16]), dtype=torch.float64).view(G, rows, Cda, 2).sum(1)
            # reference sums in fp64 from the same fp32 per-element arithmetic
            mean, rstd, scale, shift = [st[k].cpu() for k in range(4)]
            yv = yprev.cpu().view(G, -1, Cda)
            dav = da_ref.cpu().view(G, -1, Cda)
            z = (yv - mean[:, None]) * scale[:, None] + shift[:, None]
            gr = torch.where(z > 0, torch.ones_like(z), torch.full_like(z, 0.01 if act == H.ACT_LRELU else 0.0))
            g1 = (dav * gr).double()
            xh = ((yv - mean[:, None]) * rstd[:, None]).double()
            close(pt[..., 0], g1.sum(1), rtol=1e-5, msg=tag + " sum dz")
            close(pt[..., 1], (g1 * xh).sum(1), rtol=1e-5, msg=tag + " sum dz*xhat")
            dg1, db1 = torch.zeros(Cda).to(dev), torch.zeros(Cda).to(dev)
            dg2, db2 = torch.zeros(Cda).to(dev), torch.zeros(Cda).to(dev)
            d1 = ops.norm_bwd(yprev, da, G, st, act, dg1, db1, False, partial=part, nb=rows)
            d2 = ops.norm_bwd(yprev, da_ref, G, st, act, dg2, db2, False)
            close(d1, d2, rtol=2e-5, msg=tag + " norm_bwd from fused partials")
            close(dg1, dg2, rtol=2e-5, msg=tag + " dgamma")
            close(db1, db2, rtol=2e-5, msg=tag + " dbeta")
        assert n_fused >= 5, f"only {n_fused} shapes took the fused path: {fused_tags}"
        ops.set_option("fuse_bwd_stats", 0)
        assert ops.conv3_dgrad_bwdstats(dy, wd, Cda, KD, yprev, st, act, G)[2] == 0
    finally:
        ops.set_option("fuse_bwd_stats")
        ops.set_option("conv3_b6")


C1_NORM_CASES = (  # N, spatial, KD, groups, act, elementwise dropout, BatchNorm (False: InstanceNorm)
    (2, (16, 16, 64), 3, 2, H.ACT_RELU, False, True), (4, (6, 5, 21), 3, 2, H.ACT_RELU, False, True),
    (3, (8, 9, 17), 3, 3, H.ACT_RELU, False, False), (4, (1, 40, 48), 1, 2, H.ACT_LRELU, True, True),
    (2, (1, 16, 16), 1, 1, H.ACT_LRELU, True, True))


def check_conv3_c1_norm(ops, dev, cases=C1_NORM_CASES):
    """first layer + norm with recompute (bcp_conv3_c1_norm_fwd / _bwd): BIT-identical to the unfused chain (conv3_c1_fwd_stats ->
    norm_fwd -> ... -> norm_bwd) -- activation, statistics, running statistics, dy, dgamma / dbeta (+=) -- BatchNorm groups, InstanceNorm,
    LeakyReLU + elementwise dropout (the U-Net's in_conv), ragged tiles, 2-D"""
    rng = np.random.default_rng(83)
    for (N, sp, KD, G, act, use_em, bn) in cases:
        two_d = KD == 1
        x = to_cl(R(rng, N, 1, *(sp[1:] if two_d else sp))).to(dev)
        w = (R(rng, 16, 1, *((3, 3) if two_d else (3, 3, 3))) * 0.2).to(dev).contiguous()
        b = (R(rng, 16) * 0.1).to(dev)
        gam = torch.from_numpy(rng.uniform(0.5, 1.5, 16).astype(np.float32)).to(dev) if bn else None
        bet = torch.from_numpy(rng.uniform(-0.3, 0.3, 16).astype(np.float32)).to(dev) if bn else None
        em = torch.from_numpy((rng.random(tuple(x.shape[:-1]) + (16,)) < 0.8).astype(np.uint8)).to(dev) if use_em else None
        da = torch.from_numpy(rng.standard_normal(tuple(x.shape[:-1]) + (16,), dtype=np.float32)).to(dev)
        assert ops.conv3_c1_norm_ok(x.shape, KD, G)
        tag = f"c1_norm {sp} G={G}"
        # unfused reference chain
        rm0, rv0 = (torch.zeros(16).to(dev), torch.ones(16).to(dev)) if bn else (None, None)
        y, part, rows = ops.conv3_c1_fwd_stats(x, w, b, KD, G)
        a0, st0 = ops.norm_fwd(y, G, gam, bet, rm0, rv0, act, elem_mask=em, elem_scale=1.25, partial=part, nb=rows)
        dg0, db0 = (torch.full((16,), 3.0).to(dev), torch.full((16,), -2.0).to(dev)) if bn else (None, None)
        dy0 = ops.norm_bwd(y, da, G, st0, act, dg0, db0, True, elem_mask=em, elem_scale=1.25)
        # fused
        rm1, rv1 = (torch.zeros(16).to(dev), torch.ones(16).to(dev)) if bn else (None, None)
        a1, st1 = ops.conv3_c1_norm_fwd(x, w, b, KD, G, gam, bet, rm1, rv1, act, elem_mask=em, elem_scale=1.25)
        assert H.amax_value(a1._bcp_amax) == float(a1.abs().max()), "fused first layer: |max| slots"      # (round 4: feeds the next conv's fp16 pre-scale)
        assert torch.equal(st1.cpu(), st0.cpu()), tag + ": statistics"
        assert torch.equal(a1.cpu(), a0.cpu()), tag + ": activation"
        if bn:
            assert torch.equal(rm1.cpu(), rm0.cpu()) and torch.equal(rv1.cpu(), rv0.cpu()), tag + ": running statistics"
        dg1, db1 = (torch.full((16,), 3.0).to(dev), torch.full((16,), -2.0).to(dev)) if bn else (None, None)
        dy1 = ops.conv3_c1_norm_bwd(x, w, b, KD, G, st1, da, act, dg1, db1, True, elem_mask=em, elem_scale=1.25)
        # the two backward paths sum their statistics partials over different row partitions: fp64-rounding-level differences only
        close(dy1, dy0, rtol=1e-6, atol_scale=1e-7, msg=tag + " dy")
        if bn:
            close(dg1, dg0, rtol=1e-6, msg=tag + " dgamma (+=)")
            close(db1, db0, rtol=1e-6, msg=tag + " dbeta (+=)")
        # round 5: the same backward with the layer's weight gradient folded into its second pass (bcp_conv3_c1_norm_bwd_wgrad): dgamma /
        # dbeta from the same first pass (bit-identical), dw (+=) equal to conv3_c1_wgrad of dy1 up to fp32 summation order
        dw0 = (R(rng, *w.shape) * 0.05).to(dev).contiguous()
        dw2 = dw0.clone()
        ops.conv3_c1_wgrad(x, dy1, dw0, KD, accumulate=True)
        dg2, db2 = (torch.full((16,), 3.0).to(dev), torch.full((16,), -2.0).to(dev)) if bn else (None, None)
        ops.conv3_c1_norm_bwd_wgrad(x, w, b, KD, G, st1, da, act, dw2, dg2, db2, True, dw_accumulate=True, elem_mask=em, elem_scale=1.25)
        close(dw2, dw0, rtol=2e-5, msg=tag + " dw of the fused backward (+=)")
        if bn:
            assert torch.equal(dg2.cpu(), dg1.cpu()) and torch.equal(db2.cpu(), db1.cpu()), tag + ": dgamma / dbeta of the fused backward"
        dw3 = torch.empty_like(dw2)
        ops.conv3_c1_norm_bwd_wgrad(x, w, b, KD, G, st1, da, act, dw3, None, None, False, dw_accumulate=False, elem_mask=em, elem_scale=1.25)
        dw4 = torch.zeros_like(dw2)
        ops.conv3_c1_wgrad(x, dy1, dw4, KD, accumulate=False)
        close(dw3, dw4, rtol=2e-5, msg=tag + " dw of the fused backward (=)")


def check_augment(ops, dev, golden_dir):
    """device-side RandomRotFlip + RandomCrop == the REFERENCE's transform classes on the same np.random state
    (tests/golden/aug_la.npz), bit for bit, and == the oracle restatement"""
    import os
    import bcp_oracle as O
    from bcp_amd.dataloaders.dataset import DeviceRotFlipCrop
    from bcp_amd.utils import BCP_utils as BU
    if dev.type == "cpu":
        BU.set_test_ops(ops)
    g = np.load(os.path.join(golden_dir, "aug_la.npz"))
    P = tuple(int(v) for v in g["patch"])
    tf = DeviceRotFlipCrop(P)
    for i in range(int(g["n_cases"])):
        ci, seed = (int(v) for v in g[f"case_{i}"])
        image, label = g[f"in_image_{ci}"], g[f"in_label_{ci}"]
        np.random.seed(seed)
        out = tf({"image": torch.from_numpy(image).to(dev), "label": torch.from_numpy(label).to(dev)})
        assert tuple(out["image"].shape) == (1,) + P and out["label"].dtype == torch.uint8
        assert np.array_equal(out["image"][0].cpu().numpy(), g[f"out_image_{i}"]), f"augment image case {i}"
        assert np.array_equal(out["label"].cpu().numpy(), g[f"out_label_{i}"]), f"augment label case {i}"
        np.random.seed(seed)
        oi, ol = O.la_rotflip_crop(image, label, P, lambda lo, hi: int(np.random.randint(lo, hi)))
        assert np.array_equal(oi, g[f"out_image_{i}"]) and np.array_equal(ol, g[f"out_label_{i}"])


def check_augment_pancreas(ops, dev, golden_dir):
    """device-side pancreas RandomCrop / CenterCrop (pancreas/dataloaders.py:22-91) == the REFERENCE's classes on the
    same np.random state (tests/golden/aug_pancreas.npz: larger than / equal to / smaller than the patch), bit for bit, and ==
    the oracle restatement"""
    import os
    import bcp_oracle as O
    from bcp_amd.pancreas import dataloaders as PD
    from bcp_amd.utils import BCP_utils as BU
    if dev.type == "cpu":
        BU.set_test_ops(ops)
    g = np.load(os.path.join(golden_dir, "aug_pancreas.npz"))
    P = tuple(int(v) for v in g["patch"])
    for i in range(int(g["n_cases"])):
        ci, seed, center = (int(v) for v in g[f"case_{i}"])
        image, label = g[f"in_image_{ci}"], g[f"in_label_{ci}"]
        np.random.seed(seed)
        tf = PD.CenterCrop(P) if center else PD.RandomCrop(P)
        img, lab = PD.ToTensor()(tf([torch.from_numpy(image).to(dev), torch.from_numpy(label).to(dev)]))
        assert tuple(img.shape) == (1,) + P and lab.dtype == torch.uint8
        assert np.array_equal(img[0].cpu().numpy(), g[f"out_image_{i}"]), f"pancreas crop image case {i}"
        assert np.array_equal(lab.cpu().numpy(), g[f"out_label_{i}"]), f"pancreas crop label case {i}"
        np.random.seed(seed)
        oi, ol = O.pancreas_crop([image, label], P, None if center else (lambda lo, hi: int(np.random.randint(lo, hi))))
        assert np.array_equal(oi, g[f"out_image_{i}"]) and np.array_equal(ol, g[f"out_label_{i}"])


def check_augment_acdc(ops, dev, golden_dir):
    """device-side RandomGenerator (ACDC) == the REFERENCE's class (python random + np.random + scipy rotate / zoom,
    tests/golden/aug_acdc.npz: 15 rot90+flip, 7 rotate, 8 plain cases over 5 slice shapes), bit for bit, and == the oracle"""
    import os
    import random
    import bcp_oracle as O
    from bcp_amd.dataloaders.dataset import DeviceRandomGenerator
    from bcp_amd.utils import BCP_utils as BU
    if dev.type == "cpu":
        BU.set_test_ops(ops)
    g = np.load(os.path.join(golden_dir, "aug_acdc.npz"))
    out_hw = tuple(int(v) for v in g["out_hw"])
    tf = DeviceRandomGenerator(out_hw)
    for i in range(int(g["n_cases"])):
        ci, seed = (int(v) for v in g[f"case_{i}"])
        image, label = g[f"in_image_{ci}"], g[f"in_label_{ci}"]
        random.seed(seed)
        np.random.seed(seed)
        out = tf({"image": torch.from_numpy(image).to(dev), "label": torch.from_numpy(label).to(dev)})
        assert tuple(out["image"].shape) == (1,) + out_hw and out["label"].dtype == torch.uint8
        assert np.array_equal(out["image"].cpu().numpy(), g[f"out_image_{i}"]), f"ACDC augment image case {i}"
        assert np.array_equal(out["label"].cpu().numpy(), g[f"out_label_{i}"]), f"ACDC augment label case {i}"
        random.seed(seed)
        np.random.seed(seed)
        oi, ol = O.acdc_random_generator(image, label, out_hw, random.random, lambda lo, hi: int(np.random.randint(lo, hi)))
        assert np.array_equal(oi, g[f"out_image_{i}"]) and np.array_equal(ol, g[f"out_label_{i}"]), f"oracle case {i}"
    # every whole-degree angle the reference can draw, on an odd-sized slice: the gather == the oracle's restatement of scipy
    rng = np.random.default_rng(12)
    img = rng.random((45, 52)).astype(np.float32)
    for angle in range(-20, 20):
        aff = O.rotate_affine(angle, img.shape)
        got = ops.acdc_augment(torch.from_numpy(img).to(dev), (64, 64), 2, 0, 0, aff).cpu().numpy()
        assert np.array_equal(got, O._nearest_zoom(O._nearest_rotate(img, angle), (64, 64))), f"angle {angle}"


def check_conv3_pipe_cold(ops, dev):
    """The LDS-DMA pipelines (k_c3p / k_c3q) against their register-staged twins (conv3_b6_pipe = 0), BIT-identical, with the caches
    flushed in front of every launch: the pipelines hand weight slots over with counted vmcnt waits, and a miscounted wait only shows
    when the weight stream actually misses the caches (first call, the 256-channel level) -- this check found one (k_c3p's comment).
    On the host simulator the DMA is synchronous: there it is an identity check of the two code paths only."""
    rng = np.random.default_rng(91)
    on_gpu = dev.type == "cuda"
    flush = torch.empty(192 << 20, dtype=torch.float32, device=dev) if on_gpu else None      # 768 MB: past the L2s and the 256 MB MALL
    shapes = ((2, 64, 64, (4, 8, 12)), (1, 32, 128, (6, 9, 5)), (1, 64, 64, (7, 7, 5)), (1, 16, 64, (5, 5, 5)))
    if on_gpu:
        shapes += ((2, 128, 128, (14, 14, 10)), (2, 256, 256, (7, 7, 5)), (2, 64, 64, (28, 28, 20)), (4, 256, 256, (6, 6, 6)))
    try:
        for flat in (1, 4, 3, 0):                       # slab widths of the flat kernel; 0: the tiled kernels (k_c3p where 64 x 64 tiles apply)
            ops.set_option("conv3_b6_flat", flat)
            for (N, Cin, Cout, sp) in shapes:
                if not on_gpu and flat in (4, 3) and N * sp[0] * sp[1] * sp[2] > 400:
                    continue
                x = R(rng, N, *sp, Cin).to(dev)
                w = (R(rng, Cout, Cin, 3, 3, 3) * 0.1).to(dev)
                wf, wd = ops.conv3_pack(w, 3)
                ops.set_option("conv3_b6_pipe", 0)
                ref = ops.conv3_fwd(x, wf, None, Cout, 3).clone()
                refd = ops.conv3_fwd(x, wd, None, Cin, 3).clone() if Cin == Cout else None
                ops.set_option("conv3_b6_pipe", 1)
                for rep in range(3 if on_gpu else 1):
                    if on_gpu:
                        flush.fill_(float(rep))
                    y = ops.conv3_fwd(x, wf, None, Cout, 3)
                    assert torch.equal(y, ref), f"pipeline vs register-staged kernel (slab mode {flat}) {N}x{sp} {Cin}->{Cout} rep {rep}: " \
                                                f"{int((y != ref).sum())} of {y.numel()} outputs differ"
                    if refd is not None:
                        if on_gpu:
                            flush.fill_(float(rep) + 0.5)
                        yd = ops.conv3_fwd(x, wd, None, Cin, 3)
                        assert torch.equal(yd, refd), f"pipeline vs register-staged kernel, dgrad pack (slab mode {flat}) {N}x{sp} rep {rep}"
                # round 4: the two-plane fp16 instances of the pipelines have no register-staged twin -- cold launches against the warm one
                # (same kernel, same bits: a slot read before it landed shows as a difference), and the warm one against torch
                x._bcp_amax = H.amax_slots(float(x.abs().max()), dev)
                warm = ops.conv3_fwd(x, wf, None, Cout, 3).clone()
                warm = ops.conv3_fwd(x, wf, None, Cout, 3).clone()
                if not torch.equal(warm, ref):           # (shapes without an fp16 instance give the three-plane result: nothing new to check)
                    close(from_cl(warm), F.conv3d(from_cl(x).cpu(), w.cpu(), None, padding=1), msg=f"fp16 pipeline (slab mode {flat}) {N}x{sp} {Cin}->{Cout}")
                    for rep in range(3 if on_gpu else 1):
                        if on_gpu:
                            flush.fill_(float(rep) + 0.125)
                        y = ops.conv3_fwd(x, wf, None, Cout, 3)
                        assert torch.equal(y, warm), f"fp16 pipeline, cold vs warm launch (slab mode {flat}) {N}x{sp} {Cin}->{Cout} rep {rep}: " \
                                                     f"{int((y != warm).sum())} of {y.numel()} outputs differ"
    finally:
        ops.set_option("conv3_b6_flat"); ops.set_option("conv3_b6_pipe"); ops.set_option("conv3_b6")


ALL_CHECKS = ("wgrad_reduce_flat", "norm_own", "norm_fuse_fin", "inline_dropout", "diceloss_class", "conv3_pipe_cold", "conv3_c1_norm", "norm_slabs", "dgrad_bwdstats", "augment_acdc", "augment", "augment_pancreas", "pack_many", "conv3_f16", "conv3_b6", "conv3_stats", "conv3_res", "norm_grouped", "mix_box", "plabel", "cc", "mixloss", "norm", "conv3", "conv3_c1", "k2", "k2_stats", "gemm_walk", "k2_bwdstats", "up_norm", "k2_chunks", "pw16_norm", "pw16_bwd_norm_bwd", "pool2d", "optim")


def check_upsample_beside_convs(ops, dev, rounds=12, ring=64):
    """Round 5 regression: bcp_pw_fwd + bcp_bilinear2x_fwd launched back to back on one stream BESIDE the bf16-pipe 2-D
    convs on another stream and a copy / GEMM load on a third; every upsample output must carry the bits of the same launch on an idle
    GPU.  The round-4 build of k_bilinear2x_fwd (packed-fp32 instructions with operand swizzles) failed this in 4-7 % of the launches --
    which is what turned the replayed-vs-eager test red; tools/probe/bilinear_race_probe.py is the stand-alone version."""
    import bcp_amd.hip_ops as Hh
    assert dev.type == "cuda"
    amax0 = type(ops).AMAX
    type(ops).AMAX = False
    try:
        g = torch.Generator(device="cpu"); g.manual_seed(3)
        C_, H_ = 32, 16
        h = torch.randn(4, 1, H_, H_, 2 * C_, generator=g).to(dev)
        wt = (torch.randn(C_, 2 * C_, generator=g) * 0.1).to(dev).contiguous()
        bp, bias = ops.k2_pack(wt, 2 * C_, C_, Hh.PACK_PW_FWD), torch.zeros(C_, device=dev)
        z = ops.pw_fwd(h, bp, bias, C_)
        gold = torch.zeros(4, 1, 2 * H_, 2 * H_, 2 * C_, device=dev)
        ops.bilinear2x_fwd(z, gold, C_)
        torch.cuda.synchronize()
        items = []
        for (cc, hh) in ((16, 64), (32, 32), (64, 16), (128, 8)):
            xi = torch.randn(4, 1, hh, hh, cc, device=dev)
            w = (torch.randn(cc, cc, 3, 3, device=dev) * 0.1).contiguous()
            wf, _ = ops.conv3_pack(w, 1)
            items.append((xi, wf, torch.zeros(cc, device=dev), cc))
        import net_checks as NC
        load = NC.LoadGenerator(dev)
        su, sc = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
        outs = [torch.zeros_like(gold) for _ in range(ring)]
        torch.cuda.synchronize()
        bad = 0
        for r in range(rounds):
            for y in outs:
                y.zero_()
            torch.cuda.synchronize()
            load.burst()
            for i in range(ring):
                with torch.cuda.stream(sc):
                    xi, wf, b_, cc = items[i % len(items)]
                    ops.conv3_fwd(xi, wf, b_, cc, 1)
                with torch.cuda.stream(su):
                    ops.pw_fwd(h, bp, bias, C_, out=z)
                    ops.bilinear2x_fwd(z, outs[i], C_)
            torch.cuda.synchronize()
            bad += sum(1 for y in outs if not torch.equal(y, gold))
        assert bad == 0, f"{bad} of {rounds * ring} upsample launches beside the convs gave other bits than the idle-GPU launch"
    finally:
        type(ops).AMAX = amax0
