"""Whole-network / whole-step parity checks shared by the simulator tests (CPU) and the -m gpu tests.

Gradient tolerances (measured, see DESIGN.md "parity"): in the reference's own arithmetic a ReLU whose
pre-activation is within an ulp of zero flips between fp32 and fp64 runs; with ~1e7 units a handful of
flips moves every weight-gradient tensor by 1e-3..1e-2 relative -- the fp32 torch reference itself sits
at 4e-3 (median, per tensor) from its fp64 twin.  So:
  * STANDARD regime (golden vectors): logits rtol 2e-4, loss 1e-5, gradients within 3e-2 rel-L2.
  * SMOOTH regime (all BN betas = +5, every ReLU active): no kinks, gradients must match the fp64 oracle
    to 1e-4 rel-L2 per tensor (north_star), which pins the backward wiring and formulas exactly.
"""
import json
import os

import numpy as np
import torch

import bcp_oracle as O
import kernel_checks as K
from bcp_amd.utils import BCP_utils as BU


def load_params(net, P):
    net.load_state_dict({k: P[k].clone() for k in net.state_dict()})
    return net


def make_vnet(P, dev, ops, variant="la", has_dropout=True):
    from bcp_amd.networks.VNet import VNet
    norm = "batchnorm" if variant == "la" else "instancenorm"
    net = VNet(n_channels=1, n_classes=2, normalization=norm, has_dropout=has_dropout and variant == "la", variant=variant).to(dev)
    load_params(net, P).flatten_()
    if dev.type == "cpu":
        net.set_ops(ops)
        BU.set_test_ops(ops)
    net.train()
    return net


def oracle_grads(P, x, tgt, dm, variant="la", dtype=torch.float64):
    Pd = {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in P.items()}
    Q = O._with_grad(Pd, set(O.trainable_keys(Pd)))
    out = O.vnet_forward(Q, x.to(dtype), dm, True, variant)
    loss = O.sup_loss_la(out, tgt)
    loss.backward()
    return out.detach(), float(loss), {k: Q[k].grad for k in Q if getattr(Q[k], "grad", None) is not None}


def is_prenorm_bias(name, params):
    """conv bias feeding a norm layer: exact gradient 0 (we write 0; the reference holds rounding noise)"""
    if not name.endswith(".bias"):
        return False
    w = params.get(name[:-5] + ".weight")
    return w is not None and w.dim() >= 4 and "out_conv" not in name and not name.startswith("branchs.0.1") and "conv1x1" not in name


def check_vnet_golden_tiny(ops, dev, golden_dir):
    g = np.load(os.path.join(golden_dir, "vnet_la_tiny.npz"))
    meta = json.load(open(os.path.join(golden_dir, "meta.json")))
    P = O.init_params(O.vnet_param_shapes(), seed=meta["vnet_la_tiny"]["param_seed"], random_affine=True)
    net = make_vnet(P, dev, ops)
    net.drop_masks = {"x5": torch.from_numpy(g["drop_x5"]), "x9": torch.from_numpy(g["drop_x9"])}
    out, _ = net(torch.from_numpy(g["x"]).to(dev))
    K.close(out, torch.from_numpy(g["logits"]), rtol=2e-4, msg="vnet logits")
    loss = BU.sup_loss(out, torch.from_numpy(g["tgt"]).to(dev))
    assert abs(float(loss.detach()) - float(g["loss"])) < 1e-5, (float(loss.detach()), float(g["loss"]))
    loss.backward()
    params = dict(net.named_parameters())
    for n_, st in zip([str(n) for n in g["grad_names"]], g["grad_stats"]):
        gr = params[n_].grad
        assert gr is not None, n_
        l2 = float(gr.double().norm())
        if is_prenorm_bias(n_, params):
            assert l2 <= 1e-6 and st[2] < 1e-4, (n_, l2, st[2])
            continue
        assert abs(l2 - st[2]) / max(st[2], 1e-12) < 3e-2, (n_, l2, st[2])
    for key, name in (("grad_block_one_w", "encoder.block_one.conv.0.weight"), ("grad_block_nine_w", "decoder.block_nine.conv.0.weight"),
                      ("grad_five_up_w", "decoder.block_five_up.conv.0.weight"), ("grad_one_dw_w", "encoder.block_one_dw.conv.0.weight"),
                      ("grad_out_conv_w", "decoder.out_conv.weight"), ("grad_bn1_w", "encoder.block_one.conv.1.weight")):
        r = K.rel_l2(params[name].grad, torch.from_numpy(g[key]))
        assert r < 3e-2, (name, r)
    sd = net.state_dict()
    K.close(sd["encoder.block_one.conv.1.running_mean"], torch.from_numpy(g["rm_block_one"]), msg="running_mean")
    K.close(sd["decoder.block_nine.conv.1.running_var"], torch.from_numpy(g["rv_block_nine"]), msg="running_var")
    assert int(sd["encoder.block_one.conv.1.num_batches_tracked"]) == 1


def check_vnet_smooth(ops, dev, shape=(32, 32, 16), variant="la", seed=3, N=1):
    """every ReLU active (beta = +5): gradients vs the fp64 oracle to 1e-4 per tensor"""
    rng = np.random.default_rng(seed)
    P = O.init_params(O.vnet_param_shapes(variant=variant), seed=seed + 100, random_affine=True)
    for k in list(P):
        if k.endswith(".bias") and (k[:-5] + ".running_mean") in P:
            P[k] = torch.full_like(P[k], 5.0)
    x = torch.from_numpy(rng.standard_normal((N, 1) + shape, dtype=np.float32))
    tgt = torch.from_numpy(rng.integers(0, 2, (N,) + shape))
    dm = None
    if variant == "la":
        dm = {"x5": torch.from_numpy((rng.random((N, 256)) < 0.5).astype(np.float32)), "x9": torch.from_numpy((rng.random((N, 16)) < 0.5).astype(np.float32))}
    o64, l64, g64 = oracle_grads(P, x, tgt, dm, variant)
    net = make_vnet(P, dev, ops, variant)
    net.drop_masks = dm
    r = net(x.to(dev))
    out = r[0]
    loss = BU.sup_loss(out, tgt.to(dev))
    loss.backward()
    assert K.rel_l2(out, o64) < 1e-4
    assert abs(float(loss.detach()) - l64) < 1e-5
    params = dict(net.named_parameters())
    worst = ("", 0.0)
    for k, gref in g64.items():
        if is_prenorm_bias(k, params) or float(gref.norm()) < 1e-7:
            continue
        if variant != "la":  # InstanceNorm net has no betas: kinks stay, keep the loose bound
            bound = 3e-2
        else:
            bound = 1e-4
        r = K.rel_l2(params[k].grad, gref)
        if r > worst[1]:
            worst = (k, r)
        assert r < bound, (k, r)
    return worst


def check_grouped_equals_separate(ops, dev):
    """one grouped forward/backward over [x1; x2] == two separate calls (what the reference does): logits, BN
    running statistics and accumulated gradients"""
    rng = np.random.default_rng(21)
    P = O.init_params(O.vnet_param_shapes(), seed=77, random_affine=True)
    x = torch.from_numpy(rng.standard_normal((2, 1, 32, 32, 16), dtype=np.float32)).to(dev)
    tgt = torch.from_numpy(rng.integers(0, 2, (2, 32, 32, 16))).to(dev)
    dm = {"x5": torch.from_numpy((rng.random((2, 256)) < 0.5).astype(np.float32)), "x9": torch.from_numpy((rng.random((2, 16)) < 0.5).astype(np.float32))}
    a, b = make_vnet(P, dev, ops), make_vnet(P, dev, ops)
    a.drop_masks = dm
    oa = a(x, groups=2)[0]
    (BU.sup_loss(oa[:1], tgt[:1]) + BU.sup_loss(oa[1:], tgt[1:])).backward()
    outs = []
    for i in range(2):
        b.drop_masks = {k: v[i:i + 1] for k, v in dm.items()}
        o = b(x[i:i + 1])[0]
        outs.append(o.detach())
        BU.sup_loss(o, tgt[i:i + 1]).backward()
    K.close(oa.detach(), torch.cat(outs), rtol=1e-5, msg="grouped logits")
    sa, sb = a.state_dict(), b.state_dict()
    for k in sa:
        if "running" in k:
            K.close(sa[k], sb[k], rtol=1e-5, msg=k)
        if k.endswith("num_batches_tracked") and (k.startswith("encoder") or k.startswith("decoder")):
            assert int(sa[k]) == int(sb[k]) == 2, k
    ga, gb = a.flat_trainable()[1], b.flat_trainable()[1]
    assert K.rel_l2(ga, gb) < 1e-5, K.rel_l2(ga, gb)


def check_la_step(ops, dev, golden_dir):
    """3 self-training steps through the drop-in API (teacher fwd, pseudo-label, CC, box mix, student fwd/bwd,
    mix_loss, SGD, EMA) vs the trajectory recorded from the reference's own functions (la_traj.npz)."""
    from bcp_amd import train_step
    g = np.load(os.path.join(golden_dir, "la_traj.npz"))
    meta = json.load(open(os.path.join(golden_dir, "meta.json")))["la_traj"]
    P = O.init_params(O.vnet_param_shapes(), seed=meta["param_seed"], random_affine=True)
    model, ema = make_vnet(P, dev, ops), make_vnet(P, dev, ops)
    for p in ema.parameters():
        p.detach_()
    vol, lab = O.synth_la_batch(4, shape=tuple(meta["shape"]), seed=meta["data_seed"])
    vol, lab = vol.to(dev), lab.to(dev)
    opt = train_step.FlatSGD(model, lr=0.01, momentum=0.9, weight_decay=1e-4)
    for it in range(meta["steps"]):
        drops = {}
        for j, k in enumerate(("t_a", "t_b", "s_l", "s_u")):
            v = torch.from_numpy(g["drops"][it, j])
            drops[k] = {"x5": v[:256].view(1, 256), "x9": v[256:].view(1, 16)}
        r = train_step.la_self_train_step(model, ema, opt, vol, lab, 2, box=tuple(int(v) for v in g["boxes"][it]), drops=drops)
        ref = g["traj"][it]
        # chaos budget: the reference's OWN fp32-vs-fp64 trajectories differ by 3e-8 / 8e-5 / 2e-4 in loss and by
        # 17 of 3912 pseudo-label voxels at step 2 on this fixture (oracle run in both precisions; DESIGN.md "parity");
        # the HIP path measured 1e-7 / 2e-4 / 8e-4 (MI355X) -- same order, bounds set 5x above; step 2 at 1e-2 since round 4 (free-running
        # pseudo-labels on the 32x32x16 fixture: ~5e-3 measured with the two-plane fp16 conv instances, as in check_la_unfused_loop)
        tol = (1e-5, 2e-3, 1e-2)[it]            # (step 1: 1.25e-3 measured once the weight gradients run on two fp16 planes too; the full-size
                                                #  trajectory -- la_traj5f, asserted against the reference's ensemble -- did not move: 7.5e-6 / 2.4e-4 / 3.0e-4 / 6.3e-4)
        for key, j in (("loss", 0), ("loss_l", 1), ("loss_u", 2)):
            assert abs(float(r[key]) - ref[j]) < tol, (it, key, float(r[key]), ref[j])
        for key, j in (("plab_a", 3), ("plab_b", 4)):
            # pseudo-labels of a random-init net sit near the 0.5 threshold: the reference's own fp32/fp64 runs differ by
            # 17 of 3912 voxels at step 2; any change of fp32 summation order (tile shape) moves a few voxels
            assert abs(float(r[key].sum()) - ref[j]) <= max(4.0, 0.03 * ref[j]), (it, key, float(r[key].sum()), ref[j])
    names = json.load(open(os.path.join(golden_dir, "meta.json")))["vnet_la_param_names"][:60]
    sdm, sde = model.state_dict(), ema.state_dict()
    for k, st in zip(names, g["final_w_stats"]):
        a = sdm[k].double()
        # (one sample of the chaotic 3-step trajectory per kernel choice: fp32-MFMA kernels only 1.05e-3, bf16-pipe kernels from
        #  2 K voxels 1.27e-3, from 256 voxels 2.39e-3 on the worst tensor -- always the first block's BatchNorm bias; the
        #  ensemble-bounded 5-step check is the principled one, check_la_traj5)
        assert abs(float(a.abs().sum()) - st[1]) / max(st[1], 1e-9) < 5e-3, k
    for k, st in zip(names, g["final_ema_stats"]):
        a = sde[k].double()
        assert abs(float(a.abs().sum()) - st[1]) / max(st[1], 1e-9) < 1e-4, k
    K.close(sde["decoder.block_nine.conv.1.running_mean"], torch.from_numpy(g["final_ema_rm"]), rtol=1e-3, msg="teacher running_mean")


# ------------------------------------------------------------------------------------------ U-Net / ACDC
def check_la_step_batch8(ops, dev):
    """the reference's default LA batch layout (--batch_size 8 --labeled_bs 4: sub-batches of TWO volumes, so every grouped
    BatchNorm group holds two samples and Dropout3d masks differ per sample) vs the oracle: loss, pseudo-labels, gradients"""
    from bcp_amd import train_step
    rng = np.random.default_rng(5)
    shape, sub = (32, 32, 16), 2
    P = O.init_params(O.vnet_param_shapes(), seed=81, random_affine=True)
    vol, lab = O.synth_la_batch(4 * sub, shape=shape, seed=82)
    drops = {k: {"x5": torch.from_numpy((rng.random((sub, 256)) < 0.5).astype(np.float32)),
                 "x9": torch.from_numpy((rng.random((sub, 16)) < 0.5).astype(np.float32))} for k in ("t_a", "t_b", "s_l", "s_u")}
    box = (3, 5, 2, 21, 21, 10)
    ro = O.la_self_train_step({k: v.clone() for k, v in P.items()}, {k: v.clone() for k, v in P.items()}, vol, lab, box, drops, sub)
    model, ema = make_vnet(P, dev, ops), make_vnet(P, dev, ops)
    for p in ema.parameters():
        p.detach_()
    r = train_step.la_self_train_step(model, ema, None, vol.to(dev), lab.to(dev), 2 * sub, box=box, drops=drops)
    assert abs(float(r["loss"]) - float(ro["loss"])) < 1e-5
    assert int((r["plab_a"].cpu().float() != ro["plab_a"]).sum() + (r["plab_b"].cpu().float() != ro["plab_b"]).sum()) <= 4
    params = dict(model.named_parameters())
    for k in ("decoder.out_conv.weight", "decoder.block_nine.conv.0.weight", "encoder.block_one.conv.0.weight"):
        assert K.rel_l2(params[k].grad, ro["grads"][k]) < 3e-2, k


def check_la_unfused_loop(ops, dev, golden_dir, steps=2):
    """INTEGRATION.md section A, literally: the reference's loop body (LA_BCP_train.py:235-270) typed out against the drop-in
    modules -- two teacher calls, get_cut_mask, a DENSE torch mask built the way context_mask builds it, torch-expression
    mixing, two student calls, mix_loss twice, torch.optim.SGD, update_ema_variables -- no fused step function, no grouped
    forward, no flat optimiser; two steps vs the trajectory recorded from the reference (la_traj.npz)."""
    from bcp_amd.utils import BCP_utils as BU
    from bcp_amd.utils.BCP_utils import update_ema_variables
    from bcp_amd.train_step import get_cut_mask
    g = np.load(os.path.join(golden_dir, "la_traj.npz"))
    meta = json.load(open(os.path.join(golden_dir, "meta.json")))["la_traj"]
    P = O.init_params(O.vnet_param_shapes(), seed=meta["param_seed"], random_affine=True)
    model, ema_model = make_vnet(P, dev, ops), make_vnet(P, dev, ops)
    for p in ema_model.parameters():
        p.detach_()
    volume_batch, label_batch = O.synth_la_batch(4, shape=tuple(meta["shape"]), seed=meta["data_seed"])
    volume_batch, label_batch = volume_batch.to(dev), label_batch.to(dev)
    optimizer = torch.optim.SGD(model.parameters(), lr=0.01, momentum=0.9, weight_decay=0.0001)
    labeled_bs, sub_bs, u_weight = 2, 1, 0.5
    for it in range(steps):
        dm = {}
        for j, k in enumerate(("t_a", "t_b", "s_l", "s_u")):
            v = torch.from_numpy(g["drops"][it, j])
            dm[k] = {"x5": v[:256].view(1, 256), "x9": v[256:].view(1, 16)}
        img_a, img_b = volume_batch[:sub_bs], volume_batch[sub_bs:labeled_bs]
        lab_a, lab_b = label_batch[:sub_bs], label_batch[sub_bs:labeled_bs]
        unimg_a, unimg_b = volume_batch[labeled_bs:labeled_bs + sub_bs], volume_batch[labeled_bs + sub_bs:]
        with torch.no_grad():
            ema_model.drop_masks = dm["t_a"]
            unoutput_a, _ = ema_model(unimg_a)
            ema_model.drop_masks = dm["t_b"]
            unoutput_b, _ = ema_model(unimg_b)
            plab_a = get_cut_mask(unoutput_a, nms=1)
            plab_b = get_cut_mask(unoutput_b, nms=1)
            w, h, z, pw, ph, pz = (int(v) for v in g["boxes"][it])          # context_mask's draw, from the fixture
            X, Y, Z = img_a.shape[2:]
            loss_mask = torch.ones(sub_bs, X, Y, Z, device=dev)
            img_mask = torch.ones(X, Y, Z, device=dev)
            img_mask[w:w + pw, h:h + ph, z:z + pz] = 0
            loss_mask[:, w:w + pw, h:h + ph, z:z + pz] = 0
        mixl_img = img_a * img_mask + unimg_a * (1 - img_mask)
        mixu_img = unimg_b * img_mask + img_b * (1 - img_mask)
        model.drop_masks = dm["s_l"]
        outputs_l, _ = model(mixl_img)
        model.drop_masks = dm["s_u"]
        outputs_u, _ = model(mixu_img)
        loss_l = BU.mix_loss(outputs_l, lab_a, plab_a, loss_mask, u_weight=u_weight)
        loss_u = BU.mix_loss(outputs_u, plab_b, lab_b, loss_mask, u_weight=u_weight, unlab=True)
        loss = loss_l + loss_u
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        update_ema_variables(model, ema_model, 0.99)
        ref = g["traj"][it]
        tol = (1e-5, 2e-3, 1e-2)[it]          # same chaos budget as check_la_step (the reference's own fp32/fp64 drift, x5; step 2: x10 since
                                              # round 4 -- free-running pseudo-labels on the 32x32x16 fixture: 5.05e-3 measured with the two-plane fp16 conv instances)
        for val, j in ((loss, 0), (loss_l, 1), (loss_u, 2)):
            assert abs(float(val.detach()) - ref[j]) < tol, (it, j, float(val.detach()), ref[j])
        for val, j in ((plab_a, 3), (plab_b, 4)):
            assert abs(float(val.sum()) - ref[j]) <= max(4.0, 0.03 * ref[j]), (it, j, float(val.sum()), ref[j])
    model.drop_masks = ema_model.drop_masks = None


def check_la_step_full(ops, dev, report=None):
    """configs[1] at FULL size -- batch 4 (labeled_bs 2), 112x112x80 -- one self-training step vs the fp32 oracle run beside it
    (LA_BCP_train.py:235-257): free run first (loss 1e-5, pseudo-label voxel budget), then with the oracle's pseudo-labels
    forced so no threshold/CC bifurcation separates the two paths (loss terms 1e-5, every gradient tensor by rel-L2 of the
    difference)."""
    from bcp_amd import train_step
    rng = np.random.default_rng(41)
    shape, sub = (112, 112, 80), 1
    P = O.init_params(O.vnet_param_shapes(), seed=43, random_affine=True)
    vol, lab = O.synth_la_batch(4 * sub, shape=shape, seed=44)
    drops = {k: {"x5": torch.from_numpy((rng.random((sub, 256)) < 0.5).astype(np.float32)),
                 "x9": torch.from_numpy((rng.random((sub, 16)) < 0.5).astype(np.float32))} for k in ("t_a", "t_b", "s_l", "s_u")}
    box = (13, 30, 7, 74, 74, 53)                                     # a 2/3-size box as context_mask draws it (BCP_utils.py:10-24)
    ro = O.la_self_train_step({k: v.clone() for k, v in P.items()}, {k: v.clone() for k, v in P.items()}, vol, lab, box, drops, sub)
    model, ema = make_vnet(P, dev, ops), make_vnet(P, dev, ops)
    for p in ema.parameters():
        p.detach_()
    r = train_step.la_self_train_step(model, ema, None, vol.to(dev), lab.to(dev), 2 * sub, box=box, drops=drops)
    nvox = 2 * sub * shape[0] * shape[1] * shape[2]
    flips = int((r["plab_a"].cpu().float() != ro["plab_a"]).sum() + (r["plab_b"].cpu().float() != ro["plab_b"]).sum())
    dl = abs(float(r["loss"]) - float(ro["loss"]))
    # budget: voxels whose teacher probability sits within fp32 rounding of 0.5 (plus what the largest-CC filter then moves)
    assert flips <= max(8, nvox // 50000), (flips, nvox)
    assert dl < 1e-5 + 2.0 * flips / nvox, (dl, flips)
    # forced pseudo-labels: the same targets on both sides
    model = make_vnet(P, dev, ops)
    r2 = train_step.la_self_train_step(model, ema, None, vol.to(dev), lab.to(dev), 2 * sub, box=box, drops=drops,
                                       plabs=(ro["plab_a"].to(dev), ro["plab_b"].to(dev)))
    for k in ("loss", "loss_l", "loss_u"):
        assert abs(float(r2[k]) - float(ro[k])) < 1e-5, (k, float(r2[k]), float(ro[k]))
    params = dict(model.named_parameters())
    errs = sorted(((K.rel_l2(params[k].grad, gref), k) for k, gref in ro["grads"].items() if not is_prenorm_bias(k, params)), reverse=True)
    worst, med = (errs[0][1], errs[0][0]), errs[len(errs) // 2][0]
    if report is not None:
        report.update(flips=flips, nvox=nvox, dloss=dl, worst_grad=worst, median_grad=med, top5=errs[:5])
    # fp32 oracle vs fp32 HIP in the standard (ReLU) regime compares two NOISY gradients: the oracle's own fp32 and fp64 runs of
    # this step differ by 2.9e-3 (median tensor, 64x64x32; activation-sign flips feed whole-channel BatchNorm backward sums);
    # HIP vs the fp32 oracle measured 4.9e-3 median / 7.7e-3 worst at full size.  This is a sanity bound; what PINS the full-size
    # backward is the fp64 oracle linearised on the HIP run's activation pattern (check_vnet_pattern_grads at 112x112x80: 1e-4).
    assert med < 1.5e-2 and worst[1] < 3e-2, (med, errs[:5])
    return flips, dl, worst


def check_pancreas_step(ops, dev, modes=(True, False)):
    """the pancreas flavour of the self-training step (train_pancreas.py:145-171: IN-V-Net, 18-connectivity CC, its own mix directions --
    unlabeled image a with a box of labeled image b, labeled image a with a box of unlabeled b -- and loss terms) vs the oracle,
    grouped and as four separate calls"""
    from bcp_amd import train_step
    shape, box = (32, 32, 32), (4, 6, 3, 20, 20, 20)
    P = O.init_params(O.vnet_param_shapes(variant="pancreas"), seed=91, random_affine=True)
    vol, lab = O.synth_la_batch(4, shape=shape, seed=92)
    ro = O.la_self_train_step({k: v.clone() for k, v in P.items()}, {k: v.clone() for k, v in P.items()}, vol, lab, box, {}, 1,
                              variant="pancreas", connectivity=2)
    for grouped in modes:
        model = make_vnet(P, dev, ops, variant="pancreas", has_dropout=False)
        ema = make_vnet(P, dev, ops, variant="pancreas", has_dropout=False)
        for p in ema.parameters():
            p.detach_()
        r = train_step.la_self_train_step(model, ema, None, vol.to(dev), lab.to(dev), 2, box=box, variant="pancreas", connect_mode=2, grouped=grouped)
        assert abs(float(r["loss"]) - float(ro["loss"])) < 1e-5 and abs(float(r["loss_l"]) - float(ro["loss_l"])) < 1e-5, (grouped, float(r["loss"]), float(ro["loss"]))
        assert int((r["plab_a"].cpu().float() != ro["plab_a"]).sum() + (r["plab_b"].cpu().float() != ro["plab_b"]).sum()) <= 4
        params = dict(model.named_parameters())
        for k in ("branchs.0.1.weight", "branchs.0.0.conv.0.weight", "block_one.conv.0.weight"):
            assert K.rel_l2(params[k].grad, ro["grads"][k]) < 3e-2, (grouped, k)


def _rand_unet_drops(rng, n, hw):
    return {f"d{i}": torch.from_numpy((rng.random((n, c, hw[0] >> i, hw[1] >> i)) < 1.0 - O.UNET_DROP[i]).astype(np.float32)) for i, c in enumerate(O.UNET_CH)}


def check_acdc_step_full(ops, dev, batch=24, labeled_bs=12, hw=(256, 256), report=None, seed=61):
    """BASELINE.json configs[3] at FULL size -- batch 24 (labeled_bs 12), 256x256 -- one whole ACDC self-training step
    (ACDC_BCP_train.py:353-390) vs the fp32 oracle run beside it; also configs[0]'s layout (batch 8 / labeled 4).
    Free run: dice and ce to 1e-5 plus the pseudo-label budget; then with the oracle's pseudo-labels forced: dice / ce / loss 1e-5
    and every gradient tensor by rel-L2 of the difference (two noisy fp32 gradients -- the pattern check pins the backward).
    PSEUDO-LABEL BUDGET (stated, per config): argmax over 4 softmax channels flips where the two largest logits agree to fp32
    rounding, and the per-class largest-CC filter can then move a whole small component: <= max(16, pixels / 20000) pixels."""
    from bcp_amd import train_step
    rng = np.random.default_rng(seed)
    lsub, usub = labeled_bs // 2, (batch - labeled_bs) // 2
    P = O.init_params(O.unet_param_shapes(), seed=seed + 1, random_affine=True)
    vol, lab = O.synth_acdc_batch(batch, shape=hw, seed=seed + 2)
    drops = {k: _rand_unet_drops(rng, lsub if k.startswith("s") else usub, hw) for k in ("t_a", "t_b", "s_unl", "s_l")}
    box = (37, 61, int(hw[0] * 2 / 3), int(hw[1] * 2 / 3))            # a 2/3-size box as generate_mask draws it (ACDC_BCP_train.py:141-150)
    ro = O.acdc_self_train_step({k: v.clone() for k, v in P.items()}, {k: v.clone() for k, v in P.items()}, vol, lab, box, drops, lsub, usub)
    model, ema = make_unet(P, dev, ops), make_unet(P, dev, ops)
    for p in ema.parameters():
        p.detach_()
    r = train_step.acdc_self_train_step(model, ema, None, vol.to(dev), lab.to(dev), labeled_bs, box=box, drops=drops)
    npix = 2 * usub * hw[0] * hw[1]
    flips = int((r["plab_a"].cpu().float() != ro["plab_a"].float()).sum() + (r["plab_b"].cpu().float() != ro["plab_b"].float()).sum())
    dd, dc = abs(float(r["loss_dice"]) - float(ro["loss_dice"])), abs(float(r["loss_ce"]) - float(ro["loss_ce"]))
    assert flips <= max(16, npix // 20000), (flips, npix)
    assert dd < 1e-5 + 4.0 * flips / npix and dc < 1e-5 + 8.0 * flips / npix, (dd, dc, flips)
    model = make_unet(P, dev, ops)
    r2 = train_step.acdc_self_train_step(model, ema, None, vol.to(dev), lab.to(dev), labeled_bs, box=box, drops=drops,
                                         plabs=(ro["plab_a"].to(torch.uint8).to(dev), ro["plab_b"].to(torch.uint8).to(dev)))
    for k in ("loss", "loss_dice", "loss_ce"):
        assert abs(float(r2[k]) - float(ro[k])) < 1e-5, (k, float(r2[k]), float(ro[k]))
    params = dict(model.named_parameters())
    errs = sorted(((K.rel_l2(params[k].grad, gref), k) for k, gref in ro["grads"].items() if not is_prenorm_bias(k, params) and float(gref.norm()) > 1e-9),
                  reverse=True)
    worst, med = (errs[0][1], errs[0][0]), errs[len(errs) // 2][0]
    if report is not None:
        report.update(flips=flips, npix=npix, ddice=dd, dce=dc, worst_grad=worst, median_grad=med, top5=errs[:5])
    assert med < 1.5e-2 and worst[1] < 5e-2, (med, errs[:5])          # sanity bound on two noisy fp32 gradients (see check_la_step_full)
    return flips, dd, dc, worst


def check_pancreas_step_full(ops, dev, shape=(96, 96, 96), report=None, seed=71):
    """BASELINE.json configs[4] per rank at FULL size -- four streams x 1, 96^3, InstanceNorm V-Net -- one whole self-training step
    (pancreas/train_pancreas.py:144-171) vs the fp32 oracle beside it, then the FIRST Adam update (lr 1e-3) and the EMA.
    Pseudo-label budget: <= max(8, voxels / 50000) (threshold at 0.5 + 18-connectivity largest component), as for LA."""
    from bcp_amd import train_step
    P = O.init_params(O.vnet_param_shapes(variant="pancreas"), seed=seed, random_affine=True)
    vol, lab = O.synth_la_batch(4, shape=shape, seed=seed + 1)
    box = (11, 17, 9, 64, 64, 64)                                     # generate_mask(img, 64): a 64^3 box inside the 96^3 patch
    Ps, Pt = {k: v.clone() for k, v in P.items()}, {k: v.clone() for k, v in P.items()}
    ro = O.la_self_train_step(Ps, Pt, vol, lab, box, {}, 1, variant="pancreas", connectivity=2)
    model = make_vnet(P, dev, ops, variant="pancreas", has_dropout=False)
    ema = make_vnet(P, dev, ops, variant="pancreas", has_dropout=False)
    for p in ema.parameters():
        p.detach_()
    r = train_step.la_self_train_step(model, ema, None, vol.to(dev), lab.to(dev), 2, box=box, variant="pancreas", connect_mode=2)
    nvox = 2 * shape[0] * shape[1] * shape[2]
    flips = int((r["plab_a"].cpu().float() != ro["plab_a"]).sum() + (r["plab_b"].cpu().float() != ro["plab_b"]).sum())
    dl = abs(float(r["loss"]) - float(ro["loss"]))
    assert flips <= max(8, nvox // 50000), (flips, nvox)
    assert dl < 1e-5 + 2.0 * flips / nvox, (dl, flips)
    # forced pseudo-labels + the optimiser: loss terms 1e-5, then Adam's first update and the EMA against the oracle's
    model = make_vnet(P, dev, ops, variant="pancreas", has_dropout=False)
    ema = make_vnet(P, dev, ops, variant="pancreas", has_dropout=False)
    for p in ema.parameters():
        p.detach_()
    opt = train_step.FlatAdam(model, lr=1e-3)
    r2 = train_step.la_self_train_step(model, ema, opt, vol.to(dev), lab.to(dev), 2, box=box, variant="pancreas", connect_mode=2,
                                       plabs=(ro["plab_a"].to(torch.uint8).to(dev), ro["plab_b"].to(torch.uint8).to(dev)))
    for k in ("loss", "loss_l", "loss_u"):
        assert abs(float(r2[k]) - float(ro[k])) < 1e-5, (k, float(r2[k]), float(ro[k]))
    tkeys = O.trainable_keys(O.vnet_param_shapes(variant="pancreas"))
    P0 = {k: v.clone() for k, v in Ps.items()}
    O.adam_step(Ps, ro["grads"], {}, tkeys)
    O.ema_params(Ps, Pt, tkeys, 0.99)
    params, eparams = dict(model.named_parameters()), dict(ema.named_parameters())
    # Adam's first update is lr * g / (|g| + eps) ~ lr * sign(g): elements with |g| ~ eps (1e-8) amplify fp32 gradient noise, so the
    # update is compared where it is well-conditioned (|g| > 1e-6: > 99 % of the elements) and in the mean over everything
    agree, total, mean_d = 0, 0, 0.0
    for k in tkeys:
        if is_prenorm_bias(k, params):
            continue
        du, dr = (params[k].detach().cpu() - P0[k]), (Ps[k] - P0[k])
        g = ro["grads"][k].abs()
        sel = g > 1e-6
        agree += int(((du - dr).abs()[sel] < 2e-4).sum())
        total += int(sel.sum())
        mean_d += float((du - dr).abs().sum())
        # EMA (update_ema_variables, alpha 0.99) of the teacher towards the UPDATED student: exact against the HIP student's own new weights
        # (the EMA kernel is bit-exact, kernel_checks.check_optim), and against the oracle's wherever Adam's update agreed
        K.close(eparams[k].detach().cpu(), 0.99 * P0[k] + 0.01 * params[k].detach().cpu(), rtol=1e-6, atol_scale=1e-7, msg="EMA " + k)
        assert float((eparams[k].detach().cpu() - Pt[k]).abs().max()) <= 0.01 * float((du - dr).abs().max()) + 1e-7, "EMA vs oracle " + k
    n_all = sum(Ps[k].numel() for k in tkeys)
    if report is not None:
        report.update(flips=flips, nvox=nvox, dloss=dl, adam_agree=agree / max(total, 1), adam_mean_abs_diff=mean_d / n_all)
    assert agree / max(total, 1) > 0.98 and mean_d / n_all < 2e-5, (agree / max(total, 1), mean_d / n_all)
    return flips, dl


def check_pre_train_steps(ops, dev):
    """the pre-training step functions the train scripts call (LA_BCP_train.py:150-167, ACDC_BCP_train.py:236-256): loss and the
    updated weights after one SGD step vs the oracle (labeled halves copy-pasted into each other, supervised / mix loss)"""
    from bcp_amd import train_step
    rng = np.random.default_rng(17)
    # ---- LA: V-Net, images AND labels mixed, (CE + Dice) / 2
    shape, box = (32, 32, 16), (3, 5, 2, 21, 21, 10)
    P = O.init_params(O.vnet_param_shapes(), seed=61, random_affine=True)
    vol, lab = O.synth_la_batch(2, shape=shape, seed=62)
    dm = {"x5": torch.from_numpy((rng.random((1, 256)) < 0.5).astype(np.float32)), "x9": torch.from_numpy((rng.random((1, 16)) < 0.5).astype(np.float32))}
    img_mask, _ = O.box_to_mask(box, shape, 1)
    keys = set(O.trainable_keys(P))
    Q = O._with_grad({k: v.clone() for k, v in P.items()}, keys)
    out = O.vnet_forward(Q, O.mix(vol[:1], vol[1:], img_mask), dm, True, "la")
    ref = O.sup_loss_la(out, O.mix(lab[:1], lab[1:], img_mask))
    ref.backward()
    net = make_vnet(P, dev, ops)
    net.drop_masks = dm
    opt = train_step.FlatSGD(net, lr=0.01, momentum=0.9, weight_decay=1e-4)
    r = train_step.la_pre_train_step(net, opt, vol.to(dev), lab.to(dev), box=box)
    assert abs(float(r["loss"]) - float(ref.detach())) < 1e-5, (float(r["loss"]), float(ref.detach()))
    sd = net.state_dict()
    for k in ("decoder.block_nine.conv.0.weight", "decoder.out_conv.weight", "encoder.block_five.conv.0.weight"):
        upd = P[k] - 0.01 * (Q[k].grad + 1e-4 * P[k])            # first SGD step: buf = g + wd * p
        K.close(sd[k].cpu() - P[k], upd - P[k], rtol=3e-2, atol_scale=3e-2, msg=f"LA pre-train update {k}")
    # ---- pancreas: IN-V-Net (no dropout), the same copy-paste of images AND labels with a cubic box, (CE + Dice) / 2, Adam
    #      (train_pancreas.py:83-97; optimiser :57 Adam lr 1e-3)
    shape_p, box_p = (32, 32, 32), (5, 7, 4, 21, 21, 21)
    Pp = O.init_params(O.vnet_param_shapes(variant="pancreas"), seed=63, random_affine=True)
    volp, labp = O.synth_la_batch(2, shape=shape_p, seed=64)
    mp, _ = O.box_to_mask(box_p, shape_p, 1)
    Qp = O._with_grad({k: v.clone() for k, v in Pp.items()}, set(O.trainable_keys(Pp)))
    outp = O.vnet_forward(Qp, O.mix(volp[:1], volp[1:], mp), None, True, "pancreas")
    refp = O.sup_loss_la(outp, O.mix(labp[:1], labp[1:], mp))
    refp.backward()
    netp = make_vnet(Pp, dev, ops, variant="pancreas", has_dropout=False)
    optp = train_step.FlatAdam(netp, lr=1e-3)
    rp = train_step.la_pre_train_step(netp, optp, volp.to(dev), labp.to(dev), box=box_p, variant="pancreas")
    assert abs(float(rp["loss"]) - float(refp.detach())) < 1e-5, (float(rp["loss"]), float(refp.detach()))
    paramsp = dict(netp.named_parameters())
    sdp = netp.state_dict()
    for k in ("branchs.0.1.weight", "branchs.0.0.conv.0.weight", "block_five.conv.0.weight", "block_one.conv.0.weight"):
        gk = Qp[k].grad
        assert K.rel_l2(paramsp[k].grad, gk) < 3e-2, (k, K.rel_l2(paramsp[k].grad, gk))
        upd = -1e-3 * gk / (gk.abs() + 1e-8)                      # first Adam step: m_hat = g, v_hat = g^2
        big = gk.abs() > 1e-3 * gk.abs().max()                    # away from the sign flip of a near-zero gradient
        d = (sdp[k].cpu() - Pp[k])[big] - upd[big]
        assert float(d.abs().mean()) < 2e-5, (k, float(d.abs().mean()))
    # ---- ACDC: U-Net, image a with a box of image b, mix_loss(u_weight=1.0, unlab=True) against both label maps
    hw, box2 = (64, 64), (9, 13, 42, 42)
    Pu = O.init_params(O.unet_param_shapes(), seed=71, random_affine=True)
    vol2, lab2 = O.synth_acdc_batch(4, shape=hw, seed=72)
    bits = rng.integers(0, 256, size=4 * 2 * sum(c * (hw[0] >> i) * (hw[1] >> i) for i, c in enumerate(O.UNET_CH)) // 8 + 64, dtype=np.uint8)
    dmu = unet_drops(bits, 2, hw)
    m2, lm2 = O.box_to_mask(box2, hw, 2)
    Qu = O._with_grad({k: v.clone() for k, v in Pu.items()}, set(O.trainable_keys(Pu)))
    outu = O.unet_forward(Qu, O.mix(vol2[:2], vol2[2:], m2), dmu, True)
    rd, rc = O.mix_loss_acdc(outu, lab2[:2], lab2[2:], lm2, u_weight=1.0, unlab=True)
    unet = make_unet(Pu, dev, ops)
    unet.drop_masks = dmu
    optu = train_step.FlatSGD(unet, lr=0.01, momentum=0.9, weight_decay=1e-4)
    ru = train_step.acdc_pre_train_step(unet, optu, vol2.to(dev), lab2.to(dev), box=box2)
    assert abs(float(ru["loss_dice"]) - float(rd.detach())) < 1e-5 and abs(float(ru["loss_ce"]) - float(rc.detach())) < 1e-5
    assert abs(float(ru["loss"]) - float(((rd + rc) / 2).detach())) < 1e-5


def make_unet(P, dev, ops):
    from bcp_amd.networks.unet import UNet_2d
    net = UNet_2d(in_chns=1, class_num=4).to(dev)
    load_params(net, P).flatten_()
    if dev.type == "cpu":
        net.set_ops(ops)
        BU.set_test_ops(ops)
    net.train()
    return net


def _unpack(bits, shape):
    n = int(np.prod(shape))
    return torch.from_numpy(np.unpackbits(bits)[:n].reshape(shape).astype(np.float32))


def unet_drops(src, n, hw, prefix=None):
    dm, off = {}, 0
    for i, c in enumerate(O.UNET_CH):
        shp = (n, c, hw[0] >> i, hw[1] >> i)
        if prefix is not None:
            dm[f"d{i}"] = _unpack(src[f"{prefix}{i}"], shp)
        else:
            nb = (int(np.prod(shp)) + 7) // 8
            dm[f"d{i}"] = _unpack(src[off:off + nb], shp)
            off += nb
    return dm


def check_unet_golden_tiny(ops, dev, golden_dir):
    from bcp_amd import train_step
    g = np.load(os.path.join(golden_dir, "unet_tiny.npz"))
    meta = json.load(open(os.path.join(golden_dir, "meta.json")))["unet_tiny"]
    P = O.init_params(O.unet_param_shapes(), seed=meta["param_seed"], random_affine=True)
    net = make_unet(P, dev, ops)
    net.drop_masks = unet_drops(g, 2, (64, 64), prefix="drop_d")
    out = net(torch.from_numpy(g["x"]).to(dev))
    K.close(out, torch.from_numpy(g["logits"]), rtol=2e-4, msg="unet logits")
    tgt = torch.from_numpy(g["tgt"]).to(dev)
    w, h, pw, ph = meta["mask_box"]
    lm = BU.BoxMask((w, h, pw, ph), (64, 64), 2, False, dev)
    d, c = train_step.acdc_mix_loss(out, tgt, (tgt + 1) % 4, lm, u_weight=0.5)
    loss = (d + c) / 2
    assert abs(float(loss.detach()) - float(g["loss"])) < 1e-5, (float(loss.detach()), float(g["loss"]))
    loss.backward()
    params = dict(net.named_parameters())
    for n_, st in zip([str(n) for n in g["grad_names"]], g["grad_stats"]):
        gr = params[n_].grad
        assert gr is not None, n_
        l2 = float(gr.double().norm())
        if is_prenorm_bias(n_, params):
            assert l2 <= 1e-6, (n_, l2)
            continue
        assert abs(l2 - st[2]) / max(st[2], 1e-12) < 3e-2, (n_, l2, st[2])
    for key, name in (("grad_in_conv_w", "encoder.in_conv.conv_conv.0.weight"), ("grad_up4_1x1_w", "decoder.up4.conv1x1.weight"),
                      ("grad_out_conv_w", "decoder.out_conv.weight")):
        assert K.rel_l2(params[name].grad, torch.from_numpy(g[key])) < 3e-2, name
    sd = net.state_dict()
    K.close(sd["encoder.in_conv.conv_conv.1.running_var"], torch.from_numpy(g["rv_in"]), msg="running_var")


def check_unet_smooth(ops, dev, hw=(64, 64), N=2, seed=4):
    """all LeakyReLUs on their positive branch (beta = +5): gradients vs the fp64 oracle to 1e-4 per tensor"""
    from bcp_amd import train_step
    rng = np.random.default_rng(seed)
    P = O.init_params(O.unet_param_shapes(), seed=seed + 100, random_affine=True)
    for k in list(P):
        if k.endswith(".bias") and (k[:-5] + ".running_mean") in P and "head" not in k and "selector" not in k:
            P[k] = torch.full_like(P[k], 5.0)
    x = torch.from_numpy(rng.random((N, 1) + hw, dtype=np.float32))
    tgt = torch.from_numpy(rng.integers(0, 4, (N,) + hw))
    dm = {f"d{i}": torch.from_numpy((rng.random((N, c, hw[0] >> i, hw[1] >> i)) >= p).astype(np.float32)) for i, (c, p) in enumerate(zip(O.UNET_CH, O.UNET_DROP))}
    box = (5, 9, int(hw[0] * 2 / 3), int(hw[1] * 2 / 3))
    _, lm = O.box_to_mask(box, hw, N)
    Pd = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in P.items()}
    Q = O._with_grad(Pd, set(O.trainable_keys(Pd)))
    o64 = O.unet_forward(Q, x.double(), dm, True)
    d, c = O.mix_loss_acdc(o64, tgt, (tgt + 1) % 4, lm, u_weight=0.5, unlab=True)
    ((d + c) / 2).backward()
    net = make_unet(P, dev, ops)
    net.drop_masks = dm
    out = net(x.to(dev))
    dd, cc = train_step.acdc_mix_loss(out, tgt.to(dev), ((tgt + 1) % 4).to(dev), BU.BoxMask(box, hw, N, False, dev), u_weight=0.5, unlab=True)
    ((dd + cc) / 2).backward()
    assert K.rel_l2(out, o64.detach()) < 1e-4
    assert abs(float(dd.detach()) - float(d)) < 1e-5 and abs(float(cc.detach()) - float(c)) < 1e-5
    params = dict(net.named_parameters())
    for k in O.trainable_keys(P):
        gref = Q[k].grad
        if gref is None or is_prenorm_bias(k, params) or float(gref.norm()) < 1e-7:
            continue
        r = K.rel_l2(params[k].grad, gref)
        assert r < 1e-4, (k, r)


def check_acdc_step(ops, dev, golden_dir):
    from bcp_amd import train_step
    g = np.load(os.path.join(golden_dir, "acdc_traj.npz"))
    m = json.load(open(os.path.join(golden_dir, "meta.json")))["acdc_traj"]
    P = O.init_params(O.unet_param_shapes(), seed=m["param_seed"], random_affine=True)
    model, ema = make_unet(P, dev, ops), make_unet(P, dev, ops)
    for p in ema.parameters():
        p.detach_()
    vol, lab = O.synth_acdc_batch(8, shape=tuple(m["shape"]), seed=m["data_seed"])
    vol, lab = vol.to(dev), lab.to(dev)
    opt = train_step.FlatSGD(model, lr=0.01, momentum=0.9, weight_decay=1e-4)
    for it in range(m["steps"]):
        drops = {k: unet_drops(g["dropbits"][it, j], 2, tuple(m["shape"])) for j, k in enumerate(("t_a", "t_b", "s_unl", "s_l"))}
        r = train_step.acdc_self_train_step(model, ema, opt, vol, lab, 4, box=tuple(int(v) for v in g["boxes"][it]), drops=drops)
        ref = g["traj"][it]
        tol = (1e-5, 1e-3)[it]
        assert abs(float(r["loss"]) - ref[0]) < tol and abs(float(r["loss_dice"]) - ref[1]) < tol and abs(float(r["loss_ce"]) - ref[2]) < tol, (it, float(r["loss"]), ref)
        for key, j in (("plab_a", 3), ("plab_b", 4)):
            assert abs(float(r[key].float().sum()) - ref[j]) <= max(4.0, 0.03 * ref[j]), (it, key)
    sde = ema.state_dict()
    K.close(sde["encoder.in_conv.conv_conv.1.running_mean"], torch.from_numpy(g["final_ema_rm"]), rtol=1e-3, msg="teacher running_mean")


def check_sliding_window(ops, dev, golden_dir):
    """validation path: eval-mode V-Net + sliding-window accumulation on the device vs the REFERENCE's
    test_single_case output (tests/golden/sw_la.npz, made by oracle/make_golden_eval.py) and vs the oracle restatement"""
    from bcp_amd.utils import test_3d_patch as T3
    g = np.load(os.path.join(golden_dir, "sw_la.npz"))
    P = O.eval_params(int(g["seed"]))
    net = make_vnet(P, dev, ops)
    rm0 = net.state_dict()["encoder.block_one.conv.1.running_mean"].clone()
    patch, (sxy, sz) = tuple(int(v) for v in g["patch"]), (int(v) for v in g["stride"])
    label, score = T3.test_single_case(net, g["image"], sxy, sz, patch, num_classes=2, batch=4)
    assert net.training, "test_single_case must restore train() mode"
    assert torch.equal(net.state_dict()["encoder.block_one.conv.1.running_mean"], rm0), "eval-mode BatchNorm must not touch the running statistics"
    score, label = score[0].cpu().numpy(), label.cpu().numpy()
    assert score.shape == g["score_map"].shape and label.shape == g["label_map"].shape
    err = np.abs(score - g["score_map"]).max()
    assert err < 2e-5, f"score map vs reference: {err:.3e}"
    border = np.abs(g["score_map"] - 0.5) < 1e-4          # voxels within rounding of the 0.5 threshold may legitimately flip
    assert np.array_equal(label[~border], g["label_map"][~border])
    dc, jc = T3.dice_jaccard(torch.from_numpy(g["label_map"]).to(dev), torch.from_numpy(g["gt"]).to(dev))
    assert abs(dc - float(g["dice"])) < 1e-12 and 0.0 < jc < dc
    # batch size must not change anything (eval-mode BatchNorm is per element)
    label1, score1 = T3.test_single_case(net, g["image"], *(int(v) for v in g["stride"]), patch, num_classes=2, batch=1)
    assert float((score1[0].cpu() - torch.from_numpy(score)).abs().max()) < 1e-6
    mean_dice = T3.var_all_case_LA(net, 2, patch, *(int(v) for v in g["stride"]), cases=[(g["image"], g["gt"])])
    assert abs(mean_dice - O.dice_binary(label, g["gt"])) < 1e-3


def check_sliding_window_pancreas(ops, dev, golden_dir):
    """pancreas validation path: IN-V-Net + two-channel sliding window + argmax on the device vs the REFERENCE's
    pancreas/test_util.py:test_single_case (tests/golden/sw_pancreas.npz) and vs the oracle restatement"""
    from bcp_amd.pancreas import test_util as PT
    g = np.load(os.path.join(golden_dir, "sw_pancreas.npz"))
    P = O.init_params(O.vnet_param_shapes(variant="pancreas"), seed=int(g["seed"]), random_affine=True)
    net = make_vnet(P, dev, ops, variant="pancreas", has_dropout=False)
    patch, (sxy, sz) = tuple(int(v) for v in g["patch"]), (int(v) for v in g["stride"])
    label, score = PT.test_single_case(net, g["image"], sxy, sz, patch, num_classes=2, batch=3)
    assert net.training, "test_single_case must restore train() mode"
    score, label = score.cpu().numpy(), label.cpu().numpy()
    assert score.shape == g["score_map"].shape and label.shape == g["label_map"].shape
    err = np.abs(score - g["score_map"]).max()
    assert err < 2e-5, f"score map vs reference: {err:.3e}"
    border = np.abs(g["score_map"][1] - g["score_map"][0]) < 2e-4     # voxels within rounding of a tie may legitimately flip
    assert np.array_equal(label[~border], g["label_map"][~border]) and border.mean() < 0.01
    (avg, lst) = PT.test_calculate_metric(net, [(g["image"], g["label_map"])], num_classes=2, dim=patch, s_xy=int(g["stride"][0]), s_z=int(g["stride"][1]))
    assert avg[0] > 0.99 and len(lst) == 1 and net.training      # the prediction against the reference's own label map


def check_unet_skip_in_concat(ops, dev, hw=(64, 64), N=4, seed=23, min_direct=3):
    """encoder outputs written straight into the decoder's concat buffers + pool backward joining the skip gradient (UNet_2d.skip_in_concat,
    round 4) against the torch.cat-style copies they replace: same network, same input, live dropout off.  Not bit for bit -- the concat
    buffer shares the skip's |max| slots, so the skip's own readers scale their fp16 planes by an upper bound instead of the exact maximum --
    but far inside the parity tolerance"""
    rng = np.random.default_rng(seed)
    P = O.init_params(O.unet_param_shapes(), seed=seed + 100, random_affine=True)
    x = torch.from_numpy(rng.random((N, 1) + hw, dtype=np.float32)).to(dev)
    dm = {f"d{i}": torch.from_numpy((rng.random((N, c, hw[0] >> i, hw[1] >> i)) >= p).astype(np.float32)) for i, (c, p) in enumerate(zip(O.UNET_CH, O.UNET_DROP))}
    w = torch.from_numpy(rng.standard_normal((N, 4) + hw).astype(np.float32)).to(dev)
    res, copies = {}, {}
    real_copy = ops.copy_channels
    for flag in (True, False):
        n = [0]

        def counting(*a, **k):
            n[0] += 1
            return real_copy(*a, **k)
        ops.copy_channels = counting
        try:
            net = make_unet(P, dev, ops)
            net.skip_in_concat = flag
            net.drop_masks = dm
            out = net(x, groups=2)
            (out * w).sum().backward()
        finally:
            del ops.copy_channels
        copies[flag] = n[0]
        assert n[0] == sum(not d for d in net.plan_call(N, *hw).direct), (flag, n[0])      # ... as the planner said
        res[flag] = (out.detach().cpu(), {k: p.grad.detach().cpu().clone() for k, p in net.named_parameters() if p.grad is not None})
    assert copies[False] == 4 and copies[True] <= min_direct, copies      # the four concat copies; a level served by the raw-slab norm still copies (tiny extents only)
    assert K.rel_l2(res[True][0], res[False][0]) < 1e-5, K.rel_l2(res[True][0], res[False][0])
    for k, g in res[False][1].items():
        if float(g.norm()) < 1e-7:
            continue
        r = K.rel_l2(res[True][1][k], g)
        assert r < 1e-4, (k, r)


def check_unet_inline_dropout(ops, dev, hw=(64, 64), N=4, seed=31):
    """live nn.Dropout with the keep bits evaluated inside the norm kernels (UNet_2d.inline_dropout, hip_ops.SeedMask) == the same network
    drawing uint8 masks with bcp_bernoulli from the same dropout stream: logits and every gradient bit for bit, two passes in a row (the
    second one is a plan replay with refreshed seeds when plans are on)"""
    rng = np.random.default_rng(seed)
    P = O.init_params(O.unet_param_shapes(), seed=seed + 100, random_affine=True)
    x = torch.from_numpy(rng.random((N, 1) + hw, dtype=np.float32)).to(dev)
    w = torch.from_numpy(rng.standard_normal((N, 4) + hw).astype(np.float32)).to(dev)
    res = {}
    for flag in (True, False):
        net = make_unet(P, dev, ops)
        net.inline_dropout = flag
        net.seed_dropout(777)
        got = []
        for _ in range(2):
            for p_ in net.parameters():
                p_.grad = None
            out = net(x, groups=2)
            (out * w).sum().backward()
            got.append((out.detach().cpu(), {k: p_.grad.detach().cpu().clone() for k, p_ in net.named_parameters() if p_.grad is not None}))
        res[flag] = got
    assert not torch.equal(res[True][0][0], res[True][1][0]), "two passes drew the same dropout masks"
    for it in range(2):
        assert torch.equal(res[True][it][0], res[False][it][0]), f"inline dropout: logits differ (pass {it})"
        for k, g in res[False][it][1].items():
            assert torch.equal(res[True][it][1][k], g), (f"inline dropout: gradient differs (pass {it})", k)


def check_unet_eval(ops, dev, seed=5):
    """model.eval() U-Net forward (running statistics, no dropout) vs the oracle; the running statistics stay untouched"""
    rng = np.random.default_rng(seed)
    P = O.init_params(O.unet_param_shapes(), seed=seed + 50, random_affine=True)
    for k in P:
        if k.endswith("running_mean"):
            P[k] = torch.from_numpy(rng.normal(0.0, 0.2, tuple(P[k].shape)).astype(np.float32))
        elif k.endswith("running_var"):
            P[k] = torch.from_numpy(rng.uniform(0.5, 1.5, tuple(P[k].shape)).astype(np.float32))
    x = torch.from_numpy(rng.standard_normal((3, 1, 32, 48), dtype=np.float32))
    ref = O.unet_forward({k: v.clone() for k, v in P.items()}, x, None, train=False)
    net = make_unet(P, dev, ops)
    sd0 = {k: v.clone() for k, v in net.state_dict().items() if "running" in k}
    net.eval()
    out = net(x.to(dev))
    K.close(out, ref, rtol=2e-5, msg="unet eval logits")
    for k, v in net.state_dict().items():
        if "running" in k:
            assert torch.equal(v, sd0[k]), k


def check_val_2d(ops, dev, seed=9):
    """utils/val_2d.py:test_single_volume counterpart: eval-mode U-Net over a volume's slices, per-class Dice vs the oracle
    (torch eval forward + argmax + numpy Dice), device path (slice size == patch size) and host-zoom path"""
    from bcp_amd.utils import val_2d as V
    rng = np.random.default_rng(seed)
    P = O.init_params(O.unet_param_shapes(), seed=seed + 50, random_affine=True)
    for k in P:
        if k.endswith("running_mean"):
            P[k] = torch.from_numpy(rng.normal(0.0, 0.2, tuple(P[k].shape)).astype(np.float32))
        elif k.endswith("running_var"):
            P[k] = torch.from_numpy(rng.uniform(0.5, 1.5, tuple(P[k].shape)).astype(np.float32))
    net = make_unet(P, dev, ops)
    for shape, patch in (((5, 32, 48), (32, 48)), ((3, 24, 40), (32, 48))):
        image = torch.from_numpy(rng.standard_normal((1,) + shape, dtype=np.float32))
        label = torch.from_numpy(rng.integers(0, 4, (1,) + shape).astype(np.uint8))
        got = V.test_single_volume(image, label, net, 4, patch_size=patch, batch=2)
        # oracle: the reference's loop (val_2d.py:20-40) with the oracle's eval-mode forward
        from scipy.ndimage import zoom
        pred = np.zeros(shape, dtype=np.uint8)
        for i in range(shape[0]):
            sl = zoom(image[0, i].numpy(), (patch[0] / shape[1], patch[1] / shape[2]), order=0)
            out = O.unet_forward({k: v.clone() for k, v in P.items()}, torch.from_numpy(sl)[None, None], None, train=False)
            o = torch.argmax(torch.softmax(out, dim=1), dim=1)[0].numpy()
            pred[i] = zoom(o, (shape[1] / patch[0], shape[2] / patch[1]), order=0)
        for c in range(1, 4):
            ref = O.dice_binary(pred == c, label[0].numpy() == c) if (pred == c).sum() > 0 else 0
            assert abs(got[c - 1][0] - ref) < 5e-3, (shape, c, got[c - 1][0], ref)   # a logit tie may flip a pixel
    assert net.training


def check_opt_state_compat(ops, dev, golden_dir, variant="la"):
    """the 'opt' entry of a {'net','opt'} checkpoint is interchangeable with the reference's in BOTH directions.
    torch.optim.SGD / Adam over `model.parameters()` is exactly what the reference's save_net_opt serialises
    (LA_BCP_train.py:79-84, ACDC_BCP_train.py:60-64, pancreas_utils.py:160-166); tests/golden/opt_layout.json pins the layout
    the REFERENCE networks produce (which indices carry state, the field names).  Checked: (1) a torch-written state loads into
    the flat optimiser and the next step equals torch's; (2) the flat optimiser's state_dict has the reference's layout and
    loads into a fresh torch optimiser whose next step equals ours."""
    import io
    from bcp_amd import train_step
    layout = json.load(open(os.path.join(golden_dir, "opt_layout.json")))
    adam = variant == "pancreas"
    lay = layout["pancreas_adam" if adam else "la_sgd"]
    P = O.init_params(O.vnet_param_shapes(variant=variant), seed=41)
    net = make_vnet(P, dev, ops, variant=variant)
    names = [n for n, _ in net.named_parameters()]
    assert len(names) == lay["n_params"], "parameters() must enumerate what the reference's does"
    rng = np.random.default_rng(77)
    ref_params = [torch.nn.Parameter(p.detach().cpu().clone()) for p in net.parameters()]
    mk = (lambda ps: torch.optim.Adam(ps, lr=1e-3)) if adam else (lambda ps: torch.optim.SGD(ps, lr=0.01, momentum=0.9, weight_decay=1e-4))
    opt_ref = mk(ref_params)
    idx = lay["state_indices"]

    def grads(scale):
        return {i: torch.from_numpy(rng.standard_normal(tuple(ref_params[i].shape)).astype(np.float32)) * scale for i in idx}

    def ref_step(g):
        for i, p in enumerate(ref_params):
            p.grad = g[i].clone() if i in g else None
        opt_ref.step()

    def set_flat_grads(g):
        _, gr = net.flat_trainable()
        for i, off, q in train_step._opt_param_slices(net):
            gr[off:off + q.numel()].copy_(g[i].reshape(-1).to(dev))

    ref_step(grads(1.0))
    buf = io.BytesIO()
    torch.save({"opt": opt_ref.state_dict()}, buf)                      # what save_net_opt writes for 'opt'
    sd_ref = torch.load(io.BytesIO(buf.getvalue()), weights_only=False)["opt"]
    assert sorted(int(k) for k in sd_ref["state"]) == idx, "torch here and the reference fixture agree on which parameters carry state"
    # (1) reference -> ours
    with torch.no_grad():
        for p, r in zip(net.parameters(), ref_params):
            p.copy_(r.detach().to(dev))
    net.bump()
    fo = (train_step.FlatAdam(net, lr=1e-3) if adam else train_step.FlatSGD(net, lr=0.5, momentum=0.1, weight_decay=0.0))
    fo.load_state_dict(sd_ref)                                          # lr / momentum / wd come from the checkpoint, as in torch
    g2 = grads(0.5)
    set_flat_grads(g2)
    fo.step()
    ref_step(g2)
    for n, p, r in zip(names, net.parameters(), ref_params):
        K.close(p.detach(), r.detach(), rtol=2e-6, atol_scale=1e-6, msg=f"step after loading a torch 'opt' state: {n}")
    # (2) ours -> reference
    sd = fo.state_dict()
    assert sorted(sd["state"].keys()) == idx and sorted(next(iter(sd["state"].values())).keys()) == lay["state_entry_keys"]
    assert set(sd["param_groups"][0].keys()) >= set(lay["param_group"].keys()) | {"params"}
    assert sd["param_groups"][0]["params"] == list(range(lay["n_params"]))
    buf = io.BytesIO()
    torch.save({"opt": sd}, buf)
    fresh = [torch.nn.Parameter(r.detach().clone()) for r in ref_params]
    opt2 = mk(fresh)
    opt2.load_state_dict(torch.load(io.BytesIO(buf.getvalue()), weights_only=False)["opt"])
    g3 = grads(0.25)
    for i, p in enumerate(fresh):
        p.grad = g3[i].clone() if i in g3 else None
    opt2.step()
    set_flat_grads(g3)
    fo.step()
    for n, p, r in zip(names, net.parameters(), fresh):
        K.close(p.detach(), r.detach(), rtol=2e-6, atol_scale=1e-6, msg=f"torch step after loading OUR 'opt' state: {n}")


def check_dropout_streams(dev):
    """every network owns a dropout stream seeded from torch's generator -- student and teacher draw independent
    masks, torch.manual_seed reproduces them, data-parallel ranks differ"""
    from bcp_amd.networks.VNet import VNet
    from bcp_amd.networks._hipnet import HipNet

    def two(seed):
        torch.manual_seed(seed)
        HipNet._instances = 0
        a = VNet(n_channels=1, n_classes=2, normalization="batchnorm", has_dropout=True)
        b = VNet(n_channels=1, n_classes=2, normalization="batchnorm", has_dropout=True)
        return [a.next_seed() for _ in range(3)], [b.next_seed() for _ in range(3)]

    a1, b1 = two(1337)
    a2, b2 = two(1337)
    a3, _ = two(1338)
    assert a1 == a2 and b1 == b2, "torch.manual_seed must reproduce the dropout streams"
    assert a1 != b1 and not set(a1) & set(b1), "student and teacher must not share a dropout stream"
    assert a1 != a3, "--seed must change the dropout stream"
    os.environ["RANK"] = "1"
    try:
        r1, _ = two(1337)
    finally:
        del os.environ["RANK"]
    assert r1 != a1, "data-parallel ranks must draw different masks"


def _traj_bounds(g, floor=1e-5, factor=2.0):
    """per-step loss tolerance from the fixture itself: twice the reference's OWN fp32-vs-fp64 drift (two fp32 implementations
    are each that far from the exact trajectory, so up to twice that far from each other), never below the 1e-5 loss tolerance"""
    d = np.abs(g["traj"][:, :3] - g["traj64"][:, :3]).max(axis=1)
    return np.maximum(floor, factor * d), d


def check_la_traj5(ops, dev, golden_dir, report=None, fixture="la_traj5.npz"):
    """K = 5 self-training steps through the drop-in API vs a fixture made by oracle/make_golden_traj.py: the
    REFERENCE's functions driven for 5 steps in fp32 (traj), in fp64 free-running (traj64: shows the bifurcations -- a random-
    init teacher sits on the 0.5 threshold, rounding flips pseudo-label voxels, the largest-CC filter then keeps different
    components: 358 / 363 / 615 voxels differ between the reference's own two precisions at steps 2-4 of the small fixture) and
    in fp64 FORCED onto the fp32 run's pseudo-labels (traj64f: arithmetic drift only).  The HIP run is forced onto the same
    pseudo-labels (`plabs` hook), so what is compared is arithmetic.

    The bound is the reference's OWN fp32 drift from that fp64 trajectory -- measured as an ensemble (drift_ens: the reference's
    fp32 run, plus 8 repeats with every parameter moved by <= 1 ulp, all forced alike), because ONE run is one sample of a
    chaotic process: the drift grows ~10x per step (the deepest BatchNorm layers of these small fixtures normalise over 4 / 32
    values per channel) and at step 2 the ensemble spans 3.6e-4 .. 5.2e-3 (32x32x16) and 5.5e-5 .. 9.4e-4 (64x64x32) with the
    UNJITTERED run the smallest member both times.  That is the "4x the reference's noise at step 3" round 1 recorded: the single
    reference sample it compared with is a low outlier of the reference's own spread; the HIP path (2e-3 / 4e-4 on the MI355X)
    sits at the ensemble median.
        |loss_hip - loss_ref64f| <= max(1e-5, 2 x max_ensemble |loss_ref32' - loss_ref64f|)    per step
    The HIP run's OWN pseudo-labels must agree with the reference's up to three times the reference's own fp32-vs-fp64
    disagreement + 2 %."""
    from bcp_amd import train_step
    g = np.load(os.path.join(golden_dir, fixture))
    drift = np.median(g["drift_ens"], axis=0)                    # reported next to the HIP distance
    tol = np.maximum(1e-5, 2.0 * g["drift_ens"].max(axis=0))
    P = O.init_params(O.vnet_param_shapes(), seed=int(g["param_seed"]), random_affine=True)
    model, ema = make_vnet(P, dev, ops), make_vnet(P, dev, ops)
    for p in ema.parameters():
        p.detach_()
    shape = tuple(int(v) for v in g["shape"])
    nvox = shape[0] * shape[1] * shape[2]
    vol, lab = O.synth_la_batch(4, shape=shape, seed=int(g["data_seed"]))
    vol, lab = vol.to(dev), lab.to(dev)
    opt = train_step.FlatSGD(model, lr=0.01, momentum=0.9, weight_decay=1e-4)
    rows = []
    for it in range(g["traj"].shape[0]):
        drops = {}
        for j, k in enumerate(("t_a", "t_b", "s_l", "s_u")):
            v = torch.from_numpy(g["drops"][it, j])
            drops[k] = {"x5": v[:256].view(1, 256), "x9": v[256:].view(1, 16)}
        forced = tuple(torch.from_numpy(np.unpackbits(g["plab_bits"][it, j])[:nvox].reshape((1,) + shape)).to(dev) for j in range(2))
        r = train_step.la_self_train_step(model, ema, opt, vol, lab, 2, box=tuple(int(v) for v in g["boxes"][it]), drops=drops, plabs=forced)
        got = np.array([float(r["loss"]), float(r["loss_l"]), float(r["loss_u"])])
        own_diff = float((r["plab_a"].cpu() != forced[0].cpu()).sum() + (r["plab_b"].cpu() != forced[1].cpu()).sum())
        rows.append((it, float(np.abs(got - g["traj"][it, :3]).max()), float(np.abs(got - g["traj64f"][it, :3]).max()), float(drift[it]), own_diff,
                     float(g["plab_xor"][it])))
    if report is not None:
        report.extend(rows)
    for it, d32, d64, dr, pl, plr in rows:
        assert d64 <= tol[it], f"step {it}: |loss - reference fp64| = {d64:.2e} > {tol[it]:.2e} (the reference's own fp32 ensemble: median {dr:.2e} from it; HIP vs ref fp32 {d32:.2e})"
        # (a single-sample statistic of the same chaotic process as the loss drift: by step 4 the reference's own two precisions
        #  disagree on 615 of ~2000 positive voxels of the small fixture; measured 907 on the MI355X, 1368 on the simulator, whose
        #  bf16-MFMA model rounds a 32-term dot product once where the hardware rounds along the way)
        #  Round 4: with the two-plane fp16 conv instances (operands carry 23 bits: every activation is perturbed by < 1 fp32 ulp, the
        #  kind of perturbation the fixture's ensemble applies to the parameters) the full-size run counted 81 / 471 / 4127 / 4567 at
        #  steps 1-4 against 22 / 386 / 1308 / 3809 with three bf16 planes and the reference's own 29 / 548 / 1021 / 4547: the same
        #  process one step further along at step 3, level with it at step 4 -> 5x instead of 3x; the loss bound above is unchanged
        assert pl <= 5 * plr + max(8.0, 0.02 * float(g["traj"][it, 3:].sum())), f"step {it}: {pl} pseudo-label voxels differ from the reference's (its own fp32 vs fp64: {plr})"


def check_acdc_traj5(ops, dev, golden_dir, report=None, fixture="acdc_traj5.npz", floor=1e-5, factor=2.0):
    """K = 5 ACDC self-training steps vs tests/golden/acdc_traj5.npz (same construction as check_la_traj5); acdc_traj5f.npz = the
    same at 256x256, whose dropout masks and boxes are re-drawn here from the fixture's generator seed in the generator's order
    (oracle/make_golden_traj.py:acdc -- per step four unet_drop_masks draws, then the box) instead of being stored"""
    from bcp_amd import train_step
    g = np.load(os.path.join(golden_dir, fixture))
    rngd = np.random.default_rng(int(g["drop_seed"])) if "drop_seed" in g else None
    tol, drift = _traj_bounds(g, floor, factor)
    P = O.init_params(O.unet_param_shapes(), seed=int(g["param_seed"]), random_affine=True)
    model, ema = make_unet(P, dev, ops), make_unet(P, dev, ops)
    for p in ema.parameters():
        p.detach_()
    shape = tuple(int(v) for v in g["shape"])
    vol, lab = O.synth_acdc_batch(8, shape=shape, seed=int(g["data_seed"]))
    vol, lab = vol.to(dev), lab.to(dev)
    opt = train_step.FlatSGD(model, lr=0.01, momentum=0.9, weight_decay=1e-4)
    rows = []
    for it in range(g["traj"].shape[0]):
        if rngd is None:
            drops = {k: unet_drops(g["dropbits"][it, j], 2, shape) for j, k in enumerate(("t_a", "t_b", "s_unl", "s_l"))}
        else:
            drops = {k: {f"d{i}": torch.from_numpy((rngd.random((2, c, shape[0] >> i, shape[1] >> i)) >= p).astype(np.float32))
                         for i, (c, p) in enumerate(zip(O.UNET_CH, O.UNET_DROP))} for k in ("t_a", "t_b", "s_unl", "s_l")}
            bsz = (int(shape[0] * 2 / 3), int(shape[1] * 2 / 3))
            box = (int(rngd.integers(0, shape[0] - bsz[0])), int(rngd.integers(0, shape[1] - bsz[1]))) + bsz
            assert box == tuple(int(v) for v in g["boxes"][it]), "the re-drawn stream left the fixture's draw order"
        r = train_step.acdc_self_train_step(model, ema, opt, vol, lab, 4, box=tuple(int(v) for v in g["boxes"][it]), drops=drops)
        got = np.array([float(r["loss"]), float(r["loss_dice"]), float(r["loss_ce"]), float(r["plab_a"].float().sum()), float(r["plab_b"].float().sum())])
        rows.append((it, float(np.abs(got[:3] - g["traj"][it, :3]).max()), float(np.abs(got[:3] - g["traj64"][it, :3]).max()), float(drift[it]),
                     float(np.abs(got[3:] - g["traj"][it, 3:]).sum()), float(np.abs(g["traj"][it, 3:] - g["traj64"][it, 3:]).sum())))
    if report is not None:
        report.extend(rows)
    for it, d32, d64, dr, pl, plr in rows:
        assert d64 <= tol[it], f"step {it}: |loss - reference fp64| = {d64:.2e} > {tol[it]:.2e} (the reference's own fp32 run is {dr:.2e} from it; HIP vs ref fp32 {d32:.2e})"
        assert pl <= plr + max(4.0, 0.01 * float(g["traj"][it, 3:].sum())), f"step {it}: pseudo-label sum differs by {pl} (reference fp32 vs fp64: {plr})"


def _pattern(y_cl, stats, G):
    """activation pattern of one norm layer from what the HIP forward saved: z = (y - mean) * scale + shift > 0, as [N,C,...] bool"""
    N, C = y_cl.shape[0], y_cl.shape[-1]
    st = stats.view(5, G, C)
    g = torch.arange(N, device=y_cl.device) // (N // G)
    shp = (N,) + (1,) * (y_cl.dim() - 2) + (C,)
    z = (y_cl - st[0][g].view(shp)) * st[2][g].view(shp) + st[3][g].view(shp)
    m = z > 0
    return m.permute(0, 4, 1, 2, 3).cpu() if y_cl.dim() == 5 else m


def check_vnet_pattern_grads(ops, dev, variant="la", shape=(32, 32, 16), seed=11, N=2, bound=1e-4):
    """STANDARD regime (random affine parameters, half of the ReLUs inactive), EVERY gradient tensor, rel-L2 of the DIFFERENCE:
    the fp64 oracle is linearised on the activation pattern the HIP forward actually took (act_masks hook), so the only thing
    left between the two is fp32 rounding of the same piecewise-linear function -- bound 1e-4 per tensor (north_star), also for
    the InstanceNorm V-Net, whose backward round 1 could only hold to 3e-2 (no betas to push the ReLUs open)."""
    rng = np.random.default_rng(seed)
    P = O.init_params(O.vnet_param_shapes(variant=variant), seed=seed + 200, random_affine=True)
    x = torch.from_numpy(rng.standard_normal((N, 1) + shape, dtype=np.float32))
    tgt = torch.from_numpy(rng.integers(0, 2, (N,) + shape))
    dm = None
    if variant == "la":
        dm = {"x5": torch.from_numpy((rng.random((N, 256)) < 0.5).astype(np.float32)), "x9": torch.from_numpy((rng.random((N, 16)) < 0.5).astype(np.float32))}
    net = make_vnet(P, dev, ops, variant)
    net.drop_masks = dm
    net._keep_saved = True
    out = net(x.to(dev))[0]
    loss = BU.sup_loss(out, tgt.to(dev))
    loss.backward()
    saved = net._last_saved
    masks = [_pattern(s.y, s.stats, saved.G) for s in saved.layers]
    Pd = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in P.items()}
    Q = O._with_grad(Pd, set(O.trainable_keys(Pd)))
    o64 = O.vnet_forward(Q, x.double(), dm, True, variant, act_masks=masks)
    l64 = O.sup_loss_la(o64, tgt)
    l64.backward()
    assert K.rel_l2(out, o64.detach()) < 1e-4 and abs(float(loss.detach()) - float(l64)) < 1e-5
    params = dict(net.named_parameters())
    worst, n = ("", 0.0), 0
    for k in Q:
        gref = getattr(Q[k], "grad", None)
        if gref is None or is_prenorm_bias(k, params) or float(gref.norm()) < 1e-9:
            continue
        r = K.rel_l2(params[k].grad, gref)
        n += 1
        if r > worst[1]:
            worst = (k, r)
        assert r < bound, (variant, k, r)
    assert n >= 25, n
    return worst


def check_vnet_features(ops, dev, shape=(48, 48, 48)):
    """the LA V-Net's SECOND return value (networks/VNet.py:286-290): pool(features[4]) = MaxPool3d(3, stride=2) of the (dropped-out)
    x5 -- eager path, recorded launch plan and its replay; x5 itself is pinned by the forward parity checks"""
    import torch.nn.functional as F
    rng = np.random.default_rng(77)
    P = O.init_params(O.vnet_param_shapes(), seed=78, random_affine=True)
    x = torch.from_numpy(rng.standard_normal((2, 1) + shape, dtype=np.float32)).to(dev)
    net = make_vnet(P, dev, ops)
    net._keep_saved = True                     # (also keeps this call on the eager path)
    out, feat = net(x)
    idx5 = max(i for i, L in enumerate(net._layers) if L.name.startswith("block_five."))
    x5 = net._last_saved.layers[idx5 + 1].x           # input of block_five_up = x5 after Dropout3d, channels-last
    ref = F.max_pool3d(x5.permute(0, 4, 1, 2, 3), 3, stride=2)
    assert tuple(feat.shape) == (2, 256) + tuple((s // 16 - 3) // 2 + 1 for s in shape), tuple(feat.shape)
    assert torch.equal(feat.contiguous().cpu(), ref.contiguous().cpu())
    net._keep_saved = False
    net.drop_masks = None
    for _ in range(3):                          # record, replay, replay: the pooled features come out of the plan as a copy
        o2, f2 = net(x)
        assert f2 is not None and tuple(f2.shape) == tuple(feat.shape) and bool(torch.isfinite(f2).all())
    net.eval()
    with torch.no_grad():
        o3, f3 = net(x)
    assert tuple(f3.shape) == tuple(feat.shape)
    small = make_vnet(P, dev, ops)
    assert small(x[:, :, :32, :32, :16])[1] is None      # deepest level 2x2x1: smaller than the window (the reference raises there)


def check_unet_pattern_grads(ops, dev, hw=(64, 64), N=2, seed=12, bound=1e-4):
    """the 2-D U-Net (LeakyReLU, elementwise dropout) under the same construction as check_vnet_pattern_grads"""
    rng = np.random.default_rng(seed)
    P = O.init_params(O.unet_param_shapes(), seed=seed + 200, random_affine=True)
    x = torch.from_numpy(rng.random((N, 1) + hw, dtype=np.float32))
    tgt = torch.from_numpy(rng.integers(0, 4, (N,) + hw))
    net = make_unet(P, dev, ops)
    dm = {f"d{i}": torch.from_numpy((rng.random((N, c, hw[0] >> i, hw[1] >> i)) >= p).astype(np.float32))
          for i, (c, p) in enumerate(zip((16, 32, 64, 128, 256), O.UNET_DROP))}
    net.drop_masks = dm
    net._keep_saved = True
    out = net(x.to(dev))
    loss = torch.nn.functional.cross_entropy(out, tgt.to(dev))
    loss.backward()
    saved = net._last_saved
    masks = []
    for tag in [f"e{i}" for i in range(5)] + [f"u{i}" for i in range(1, 5)]:
        h, y1, st1, em, a1, y2, st2, G = saved[tag]
        masks.append(_pattern(y1, st1, G).squeeze(2))
        masks.append(_pattern(y2, st2, G).squeeze(2))
    Pd = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in P.items()}
    Q = O._with_grad(Pd, set(O.trainable_keys(Pd)))
    # max-pool routing is the other discrete choice of this network: ONE window whose two best candidates are closer than the
    # fp32 rounding of the activations moves a gradient tensor of 32 K elements by sqrt(2 / 32768) = 8e-3 -- inject the winners too
    pool_idx = [torch.nn.functional.max_pool2d(a.squeeze(1).permute(0, 3, 1, 2).cpu(), 2, return_indices=True)[1] for a in saved["xs"][:4]]
    o64 = O.unet_forward(Q, x.double(), dm, True, act_masks=masks, pool_idx=pool_idx)
    l64 = torch.nn.functional.cross_entropy(o64, tgt)
    l64.backward()
    assert K.rel_l2(out, o64.detach()) < 1e-4 and abs(float(loss.detach()) - float(l64)) < 1e-5
    params = dict(net.named_parameters())
    worst = ("", 0.0)
    for k in Q:
        gref = getattr(Q[k], "grad", None)
        if gref is None or is_prenorm_bias(k, params) or float(gref.norm()) < 1e-9:
            continue
        r = K.rel_l2(params[k].grad, gref)
        if r > worst[1]:
            worst = (k, r)
        assert r < bound, (k, r)
    return worst


# ------------------------------------------------------------------------------------------ launch plans
def check_plan_hygiene(ops, dev):
    """(1) a training-mode forward whose result is dropped WITHOUT a backward must release its launch plan (it used to stay
    busy for ever and every later pass of the net silently took the eager path); (2) Binding.set_option -- not only Ops.set_option --
    invalidates recorded plans; (3) the plan key carries the switches that change the launch list"""
    from bcp_amd import plan
    plan.ENABLED = True
    try:
        P = O.init_params(O.unet_param_shapes(), seed=51, random_affine=True)
        model = make_unet(P, dev, ops)
        model.train()
        x = O.synth_acdc_batch(4, shape=(32, 32), seed=3)[0].to(dev)
        out = model(x)                                # records the forward plan; saved activations belong to `out`'s graph
        plans = model._plans_for()
        fwd = [pl for k, pl in plans.items() if k[0] == "f"]
        assert len(fwd) == 1 and fwd[0].busy, "a training-mode forward holds its plan until the backward pass"
        del out
        import gc
        gc.collect()
        assert not fwd[0].busy, "the plan must be released when the saved activations die without a backward"
        n0 = fwd[0].n_calls
        out = model(x)                                # replays (not the eager path): no new plan, same launch count
        assert len([k for k in model._plans_for() if k[0] == "f"]) == 1 and fwd[0].n_calls == n0
        out[0].sum().backward() if isinstance(out, (tuple, list)) else out.sum().backward()
        assert not fwd[0].busy
        e0 = plan.epoch()
        ops.b.set_option("splitk", 1)                 # the Binding-level call (bypasses Ops.set_option)
        ops.b.set_option("splitk")
        assert plan.epoch() > e0, "Binding.set_option must invalidate recorded plans"
        model(x)
        keys = [k for k in model._plans_for() if k[0] == "f"]
        model.fuse_c1 = not bool(getattr(model, "fuse_c1", False))
        try:
            model(x)
            keys2 = [k for k in model._plans_for() if k[0] == "f"]
            assert len(keys2) == len(keys) + 1, "a toggled launch-list switch must record its own plan, not replay the other sequence"
        finally:
            model.fuse_c1 = not model.fuse_c1
    finally:
        plan.ENABLED = True


class LoadGenerator:
    """a third stream kept busy beside the step under test: 128 MB copies (HBM / L2), 2048^3 GEMMs (CUs, matrix pipe) and a read-modify-write
    -- the mix under which the round-4 build deviated in 21-35 % of small ACDC runs (tools/probe/replay_stress.py)"""

    def __init__(self, dev):
        self.s = torch.cuda.Stream(device=dev)
        self.a = torch.randn(32 << 20, device=dev)
        self.b = torch.empty_like(self.a)
        self.m = torch.randn(2048, 2048, device=dev)
        self.o = torch.empty_like(self.m)

    def burst(self, n=8):
        with torch.cuda.stream(self.s):
            for _ in range(n):
                self.b.copy_(self.a)
                torch.mm(self.m, self.m, out=self.o)
                self.a[: 1 << 20].add_(1.0)

    def finish(self):
        self.s.synchronize()


def check_partial_packs(ops, dev):
    """round 6 (networks/_hipnet.py PACK_PARTIAL): in front of REPLAYS a network writes only the sections of its weight packs the recorded
    launches were seen reading; everything else must find every section.  (1) after two LA steps on recorded plans the student's and the
    teacher's packs ARE partial and most layers need exactly one section; (2) a pass that reads OTHER sections right behind a replay -- the
    same weights, |max| slots switched off, so every conv takes the three bf16 planes instead of the two fp16 ones -- gets a full repack and
    computes the same logits to conv-arithmetic tolerance (with stale planes it would be garbage); (3) the replayed steps themselves equal
    the eager path bit for bit (check_launch_plans, which runs with partial packs since this round)."""
    from bcp_amd import plan, train_step
    plan.ENABLED = True
    torch.manual_seed(5)
    np.random.seed(5)
    P = O.init_params(O.vnet_param_shapes(), seed=41, random_affine=True)
    model, ema = make_vnet(P, dev, ops, "la"), make_vnet(P, dev, ops, "la")
    model.seed_dropout(11)
    ema.seed_dropout(12)
    for p in ema.parameters():
        p.detach_()
    vol, lab = O.synth_la_batch(4, shape=(32, 32, 16), seed=77)
    vol, lab = vol.to(dev), lab.to(dev)
    opt = train_step.FlatSGD(model, lr=0.01, momentum=0.9, weight_decay=1e-4)
    for _ in range(2):        # step 1 records the passes (eager, full packs, sections noted), step 2 replays them (partial packs)
        train_step.la_self_train_step(model, ema, opt, vol, lab, 2, box=(3, 5, 2, 21, 21, 10), overlap=False)      # (teacher on the caller's stream: the pass below finds its plan)
    for net, name in ((model, "student"), (ema, "teacher")):
        assert type(net).PACK_PARTIAL and net._pack_need, (name, "no section was ever noted")
        assert not net._pack_full, (name, "the last replay did not pack partially")
        single = [m for m in net._pack_need.values() if m in (1, 2, 4)]
        assert len(single) >= len(net._pack_need) // 2, (name, net._pack_need)
    # (2) the teacher's weights as the last replay left them (partial packs of the CURRENT version): an eager forward of the same input
    x = vol[2:].contiguous()
    ema.train()
    with torch.no_grad():
        ema.seed_dropout(99)                                         # (the same Dropout3d draws in both passes)
        ref = ema(x, groups=2, features=False)[0].clone()          # a replay: partial packs, fp16 / observed sections
        assert not ema._pack_full
        amax0 = type(ops).AMAX
        plan.ENABLED = False
        type(ops).AMAX = False                                       # no |max| slots: the convs take three bf16 planes (and the fp32 kernels where they did before)
        try:
            ema.seed_dropout(99)
            out = ema(x, groups=2, features=False)[0].clone()
        finally:
            type(ops).AMAX = amax0
            plan.ENABLED = True
        assert ema._pack_full, "an eager pass behind a partial pack must repack every section"
    d = float((out - ref).abs().max() / (ref.abs().max() + 1e-12))
    print(f"partial packs: eager bf16-plane pass vs replayed fp16-plane pass, max |d| / max |ref| = {d:.2e}; student needs {sorted(set(model._pack_need.values()))}")
    assert d < 2e-3, d        # (same dropout draws; bf16-plane vs fp16-plane arithmetic and the BatchNorm over 4 values at the deepest level: ~1e-4; stale planes: O(1))


def check_launch_plans(ops, dev, steps=3, cases=(("la", True), ("la", False), ("pancreas", True), ("acdc", True)), graphs=None, overlap=True, real_stream=False,
                       load=None, volatile=False):
    """recorded launch plans (bcp_amd/plan.py) == the eager Python path, bit for bit: three self-training steps of the LA V-Net
    (grouped and as the reference's four separate calls -- the second student call must not reuse the busy plan), the pancreas
    V-Net and the ACDC U-Net, live Dropout / Dropout3d (the seeds are patched into the recorded launches), weights, teacher
    weights and running statistics compared after the last step.
    load: a LoadGenerator -- every step of the REPLAYED run starts behind a burst of copies / GEMMs on a third stream (round 5)
    volatile: the replayed run's networks run with volatile_io (round 5, networks/_hipnet.py: logits handed out as aliases of the plans'
    tensors, the copy-paste mix and the loss backward writing straight into the plans' input tensors) as the training scripts and bench.py
    set it -- same bits, and the plans' input tensors must really have been handed out
    graphs (GPU): plan.GRAPHS for the replayed run -- None: the module's default (1 since round 5: forward passes captured when the run
    lives on a real stream), 0 / False: per-launch replays only, 2: the backward pass captured too"""
    from bcp_amd import plan, train_step

    def run(enabled, what, grouped):
        if enabled and (graphs or real_stream):      # (graphs=None with the default >= 1 also captures -- when real_stream puts the run on one)
            # graphs / real_stream (GPU only): the replayed run lives on a real stream as in the training scripts and bench.py; with graphs
            # the first replay of every pass is captured and
            # the later ones are single hipGraphLaunch calls (side-stream weight gradients inside the graph)
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                r = run_(enabled, what, grouped)
            torch.cuda.current_stream(dev).wait_stream(side)
            return r
        return run_(enabled, what, grouped)

    def run_(enabled, what, grouped):
        plan.ENABLED = enabled
        level0 = plan.GRAPHS
        if graphs is not None:
            plan.GRAPHS = int(graphs)      # 0: per-launch replays, 1: forward passes (the default), 2: the backward pass with its side-stream fork / join too
        try:
            torch.manual_seed(5)
            np.random.seed(5)
            if what == "acdc":
                P = O.init_params(O.unet_param_shapes(), seed=51, random_affine=True)
                model, ema = make_unet(P, dev, ops), make_unet(P, dev, ops)
                vol, lab = O.synth_acdc_batch(8, shape=(64, 64), seed=78)
            else:
                shape = (32, 32, 16) if what == "la" else (32, 32, 32)
                P = O.init_params(O.vnet_param_shapes(variant=what), seed=41, random_affine=True)
                model, ema = make_vnet(P, dev, ops, what), make_vnet(P, dev, ops, what)
                vol, lab = O.synth_la_batch(4, shape=shape, seed=77)
            model.seed_dropout(11)
            ema.seed_dropout(12)
            for p in ema.parameters():
                p.detach_()
            if enabled and volatile:
                model.volatile_io = ema.volatile_io = True
            vol, lab = vol.to(dev), lab.to(dev)
            opt = train_step.FlatSGD(model, lr=0.01, momentum=0.9, weight_decay=1e-4)
            losses = []
            for _ in range(steps):
                if load is not None and enabled:
                    load.burst()           # (the eager run is the reference: it runs on an otherwise idle GPU)
                if what == "acdc":
                    r = train_step.acdc_self_train_step(model, ema, opt, vol, lab, 4, box=(9, 13, 42, 42), overlap=overlap)
                else:
                    r = train_step.la_self_train_step(model, ema, opt, vol, lab, 2, box=(3, 5, 2, 21, 21, 10), variant=what,
                                                      connect_mode=2 if what != "la" else None, grouped=grouped, overlap=overlap)
                losses.append(float(r["loss"]))
            if enabled and volatile and grouped:
                half = vol.shape[0] // 2
                buf = model.input_buffer((half,) + tuple(vol.shape[1:]))
                assert buf is not None and r["outputs_l" if what != "acdc" else "out_unl"].data_ptr() != 0, (what, "volatile_io: no input buffer handed out")
                cl_logits = tuple(BU._as_cl(torch.cat([r["outputs_l"], r["outputs_u"]]) if what != "acdc" else torch.cat([r["out_unl"], r["out_l"]])).shape)
                assert model.dout_buffer(cl_logits) is not None, (what, "volatile_io: no backward input buffer")
                # ... and the loss backward really wrote there: autograd runs the backward nodes on its own thread, a provider the step
                # function installs thread-locally never reaches them (round 6: that brought the 16 MB copy back unnoticed)
                assert steps < 3 or model.__dict__.get("_dout_in_place", 0) >= steps - 2, (what, "volatile_io: the logits gradient was copied into the backward plan")
            plans = [p for k, p in model.__dict__.get("_plan_state", (None, {}))[1].items() if k[0] not in ("in", "bin")] + \
                    [p for k, p in ema.__dict__.get("_plan_state", (None, {}))[1].items() if k[0] not in ("in", "bin")]
            n_plans = len([k for k in model.__dict__.get("_plan_state", (None, {}))[1] if k[0] not in ("in", "bin")])
            if enabled and graphs:
                assert steps >= 3
                n_graph = sum(1 for p in plans if p.graph is not None)
                assert n_graph >= 1 + int(graphs), (what, grouped, [p.graph_state for p in plans])      # teacher forward, student forward[, backward]
            return losses, {k: v.detach().clone().cpu() for k, v in model.state_dict().items()}, {k: v.detach().clone().cpu() for k, v in ema.state_dict().items()}, n_plans
        finally:
            plan.ENABLED = True
            plan.GRAPHS = level0

    for what, grouped in cases:
        a, b = run(False, what, grouped), run(True, what, grouped)
        assert a[3] == 0 and b[3] >= 2, (what, a[3], b[3])           # the second run really replayed (forward + backward plans)
        assert a[0] == b[0], (what, grouped, a[0], b[0])
        for k in a[1]:
            assert torch.equal(a[1][k], b[1][k]), (what, "student", k)
        for k in a[2]:
            assert torch.equal(a[2][k], b[2][k]), (what, "teacher", k)


def check_fused_head(ops, dev, steps=2):
    """the head that normalises on its way in (VNet.fuse_head, bcp_pw16_fwd_norm / _bwd_norm) against the separate apply pass, and its
    backward THROUGH that norm (Ops.HEAD_BWD_FUSED, bcp_pw16_bwd_norm_bwd, round 5) against the chain pw16_bwd_norm -> norm_bwd:
    self-training steps of the LA (BatchNorm, Dropout3d live, grouped) and pancreas (InstanceNorm) V-Nets from the same seeds.  The three
    variants differ in instruction contraction and summation order only: after the FIRST step the loss is equal, every gradient tensor
    agrees to 2e-5 of its largest entry and the weights to rounding.  Later steps are compared on the loss only: this 32 x 32 x 16 problem
    normalises 8 values per channel at its deepest level, and one last-bit difference in dy after step 1 (the fused backward's apply pass
    contracts differently from k_norm_bwd_apply: 4.5 % of the elements differ in the last bit at the LA size, tools/probe/head_fusion_diff.py)
    is a 3e-3 relative weight difference after step 2 on the device -- the round-4 path passed two steps at 2e-5 only because its dy was
    BIT-identical to the unfused one."""
    from bcp_amd import train_step
    Opsc = type(ops)

    def run(fuse, head_bwd, what):
        Opsc.HEAD_BWD_FUSED = head_bwd
        torch.manual_seed(5)
        np.random.seed(5)
        shape = (32, 32, 16) if what == "la" else (32, 32, 32)
        P = O.init_params(O.vnet_param_shapes(variant=what), seed=43, random_affine=True)
        model, ema = make_vnet(P, dev, ops, what), make_vnet(P, dev, ops, what)
        model.fuse_head = ema.fuse_head = fuse
        vol, lab = O.synth_la_batch(4, shape=shape, seed=79)
        model.seed_dropout(11)
        ema.seed_dropout(12)
        for p in ema.parameters():
            p.detach_()
        vol, lab = vol.to(dev), lab.to(dev)
        opt = train_step.FlatSGD(model, lr=0.01, momentum=0.9, weight_decay=1e-4)
        losses, grads, weights = [], None, None
        for s in range(steps):
            r = train_step.la_self_train_step(model, ema, opt, vol, lab, 2, box=(3, 5, 2, 21, 21, 10), variant=what,
                                              connect_mode=2 if what != "la" else None, grouped=True)
            losses.append(float(r["loss"]))
            if s == 0:
                grads = {k: p.grad.detach().clone().cpu() for k, p in model.named_parameters() if p.grad is not None}
                weights = {k: v.detach().clone().cpu() for k, v in model.state_dict().items()}
        return losses, grads, weights

    head0 = Opsc.HEAD_BWD_FUSED
    try:
        for what in ("la", "pancreas"):
            a = run(False, False, what)
            assert len(a[1]) > 20 and all(float(g.abs().max()) > 0 for k, g in a[1].items() if k.endswith("conv.0.weight")), "no gradients captured"
            for head_bwd in (False, True):
                b = run(True, head_bwd, what)
                tag = f"{what} fuse_head, head backward through the norm: {head_bwd}"
                assert abs(a[0][0] - b[0][0]) <= 2e-6 * abs(a[0][0]), (tag, a[0], b[0])
                for la_, lb_ in zip(a[0][1:], b[0][1:]):
                    assert abs(la_ - lb_) <= 2e-3 * abs(la_), (tag, a[0], b[0])
                for k in a[1]:
                    d = float((a[1][k] - b[1][k]).abs().max())
                    assert d <= 2e-5 * max(float(a[1][k].abs().max()), 1e-6), (tag, "gradient", k, d, float(a[1][k].abs().max()))
                for k in a[2]:
                    if a[2][k].dtype.is_floating_point:
                        d = float((a[2][k] - b[2][k]).abs().max())
                        assert d <= 1e-6 * max(float(a[2][k].abs().max()), 1e-3), (tag, "weight after one step", k, d)
    finally:
        Opsc.HEAD_BWD_FUSED = head0


def check_fp16_backward_long_run(ops, dev, steps=1000, probes=(0, 10, 100, 300, 600, 999), bound=2e-5, report=None):
    """do the two-plane fp16 instances hold for dgrad / weight-gradient operands (dy is heavy-tailed, the planes' error is
    absolute: 2^-22 of the tensor's |max|) as training moves the gradient distributions?  A small LA V-Net is trained for `steps`
    self-training steps in the product configuration; at every probe the CURRENT state's gradients are computed twice from identical forward
    bits (same kernels, same dropout seeds, forced pseudo-labels: same activation patterns) -- once with fp16 planes for dy (AMAX_BWD, the
    default) and once with three bf16 planes for every launch that reads dy -- and compared per parameter tensor (rel-L2 of the difference).
    Also: the |max| slots never promise less than their tensors hold (Ops.AMAX_CHECK) during the probes."""
    from bcp_amd import plan, train_step
    Opsc = type(ops)
    torch.manual_seed(7); np.random.seed(7)
    P = O.init_params(O.vnet_param_shapes(), seed=91, random_affine=True)
    model, ema = make_vnet(P, dev, ops), make_vnet(P, dev, ops)
    for p in ema.parameters():
        p.detach_()
    model.seed_dropout(21); ema.seed_dropout(22)
    vol, lab = O.synth_la_batch(4, shape=(32, 32, 16), seed=92)
    vol, lab = vol.to(dev), lab.to(dev)
    opt = train_step.FlatSGD(model, lr=0.01, momentum=0.9, weight_decay=1e-4)
    box = (3, 5, 2, 21, 21, 10)

    def grads(bwd16):
        b0, e0, c0 = Opsc.AMAX_BWD, plan.ENABLED, Opsc.AMAX_CHECK
        Opsc.AMAX_BWD, plan.ENABLED, Opsc.AMAX_CHECK = bwd16, False, True
        s0, s1 = model._drop_seed, ema._drop_seed
        try:
            model.mark_grads_stale()
            r = train_step.la_self_train_step(model, ema, None, vol, lab, 2, box=box, plabs=(lab[2:3].to(torch.uint8), lab[3:4].to(torch.uint8)))
            g = model.flat_grads().clone()
            return g, float(r["loss"])
        finally:
            Opsc.AMAX_BWD, plan.ENABLED, Opsc.AMAX_CHECK = b0, e0, c0
            model._drop_seed, ema._drop_seed = s0, s1

    worst = 0.0
    for it in range(steps):
        if it in probes:
            g16, l16 = grads(True)
            gb, lb = grads(False)
            assert l16 == lb, (it, l16, lb)                       # same forward bits
            per = []
            for i, off, q in train_step._opt_param_slices(model):
                a, b = g16[off:off + q.numel()].double(), gb[off:off + q.numel()].double()
                nb = float(b.norm())
                if nb > 0:
                    per.append(float((a - b).norm()) / nb)
            w = max(per)
            worst = max(worst, w)
            if report is not None:
                report.append((it, l16, w, float(np.median(per))))
            assert w <= bound, (it, w)
        train_step.la_self_train_step(model, ema, opt, vol, lab, 2, box=box)
    return worst
