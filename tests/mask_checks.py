"""Checks of the multi-box copy-paste regions (the reference's random / slab masking strategies): the rasteriser bcp_mask_boxes, the
map-driven mix bcp_mix_mask, BU.RegionMask and its dispatch, the four draw functions against the fixture captured from the reference
(tests/golden/mask_strategies.npz, tools/make_golden_masks.py), the loss and the step functions through the region path.  Shared by
tests/test_emu_masks.py (host simulator, CPU tensors) and tests/test_gpu_masks.py (-m gpu), in the style of kernel_checks.py.

Tolerances are the ones the existing checks use for the same comparisons: masks, mixes and anything routed to the box kernels bit-exact;
loss scalars 1e-5 and loss gradients close(rtol=1e-4) against the oracle (kernel_checks.check_mixloss); whole steps loss 1e-5 and gradient
tensors rel-L2 < 3e-2 against the fp32 oracle (net_checks.check_la_step_batch8 / check_pancreas_step)."""
import contextlib
import os

import numpy as np
import torch

import bcp_oracle as O
import kernel_checks as K
import net_checks as NC
from bcp_amd import hip_ops as H
from bcp_amd import train_step
from bcp_amd.utils import BCP_utils as BU


# ------------------------------------------------------------------------------------------ helpers
@contextlib.contextmanager
def count_calls(ops):
    """{entry point: calls} of everything that goes through ops.b.call while the block runs"""
    seen, orig = {}, ops.b.call

    def call(name, *a):
        seen[name] = seen.get(name, 0) + 1
        return orig(name, *a)

    ops.b.call = call
    try:
        yield seen
    finally:
        del ops.b.call


def mask_calls(seen):
    """(rasterise, map mix, box mix) launches of a run"""
    return seen.get("bcp_mask_boxes", 0), seen.get("bcp_mix_mask", 0), seen.get("bcp_mix_box", 0)


def np_mask(boxes6, N, D, H, W, complement=False):
    """numpy restatement of bcp_mask_boxes: ones, zero inside every (clamped) box, optionally swapped, N equal samples"""
    m = np.ones((D, H, W), dtype=np.uint8)
    for d, h, w, sd, sh, sw in boxes6:
        m[max(d, 0):max(d + sd, 0), max(h, 0):max(h + sh, 0), max(w, 0):max(w + sw, 0)] = 0
    if complement:
        m = 1 - m
    return np.broadcast_to(m, (N, D, H, W)).copy()


def _use(ops, dev):
    if dev.type == "cpu":
        BU.set_test_ops(ops)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def strategy_draws(seed=5):
    """[(tag, boxes6, (D, H, W))] of the four strategies at the sizes the three loops run"""
    out = []
    np.random.seed(seed)
    for sp in ((112, 112, 80), (96, 96, 96)):
        img = torch.zeros((2, 1) + sp)
        out.append(("random3d", BU.random_mask(img)[1].boxes6(), sp))
        out.append(("concat3d", BU.concate_mask(img)[1].boxes6(), sp))
    img = torch.zeros(2, 1, 256, 256)
    out.append(("random2d", train_step.random_mask(img)[1].boxes6(), (1, 256, 256)))
    out.append(("contact2d", train_step.contact_mask(img)[1].boxes6(), (1, 256, 256)))
    assert [len(b) for _, b, _ in out] == [27, 1, 27, 1, 9, 1]
    return out


# ------------------------------------------------------------------------------------------ 1. rasteriser
def check_mask_boxes(ops, dev, full_sizes=True):
    rng = np.random.default_rng(11)
    cases = []
    if full_sizes:
        cases += [(tag, b, sp) for tag, b, sp in strategy_draws()]
    small = ((6, 10, 20), (5, 7, 12), (3, 9, 32), (1, 16, 16), (4, 6, 48), (2, 3, 4))
    for sp in small:
        D, Hh, W = sp
        cases.append(("K0", (), sp))
        cases.append(("K1", ((D // 3, 1, 3, max(D // 2, 1), max(Hh - 2, 1), max(W - 5, 1)),), sp))
        k32 = tuple((int(rng.integers(0, D)), int(rng.integers(0, Hh)), int(rng.integers(0, W)), int(rng.integers(0, D + 1)),
                     int(rng.integers(0, Hh // 2 + 1)), int(rng.integers(0, W // 2 + 1))) for _ in range(32))
        cases.append(("K32 (random, overlapping, some empty, some past the far faces)", k32, sp))
        cases.append(("overlap", ((0, 1, 2, D, 4, 7), (0, 3, 5, max(D - 1, 1), 4, 9), (D - 1, 0, 0, 1, Hh, 3)), sp))
        cases.append(("flush with every face", ((0, 0, 0, 1, 2, 3), (D - 1, Hh - 2, W - 3, 1, 2, 3), (0, Hh - 1, 0, D, 1, W), (0, 0, W - 1, D, Hh, 1)), sp))
        cases.append(("whole volume", ((0, 0, 0, D, Hh, W),), sp))
        cases.append(("clamped", ((-2, -1, -3, 4, 3, 8), (D - 1, Hh - 1, W - 2, 5, 5, 5), (D + 1, 0, 0, 2, 2, 2)), sp))
    for tag, boxes, sp in cases:
        for N in (1, 3):
            for complement in (False, True):
                got = ops.mask_boxes(boxes, (N,) + tuple(sp), dev, complement=complement)
                ref = np_mask(boxes, N, *sp, complement=complement)
                assert got.dtype == torch.uint8 and tuple(got.shape) == ref.shape
                assert np.array_equal(got.cpu().numpy(), ref), (tag, sp, N, complement)


def check_mask_boxes_refusals(binding):
    """bad arguments are refused before any launch (no device needed): more than 32 boxes, a negative size, W % 4 != 0, null pointers"""
    import ctypes
    buf = (ctypes.c_ubyte * 4096)()
    out = (ctypes.addressof(buf) + 15) & ~15
    boxes = (ctypes.c_int * (33 * 6))(*([0, 0, 0, 1, 1, 1] * 33))
    fn = binding.cdll.bcp_mask_boxes
    assert fn(out, 1, 2, 4, 8, boxes, 33, 0, None) == -1 and b"33 boxes" in binding.cdll.bcp_last_error()
    neg = (ctypes.c_int * 6)(0, 0, 0, 1, -1, 1)
    assert fn(out, 1, 2, 4, 8, neg, 1, 0, None) == -1 and b"negative" in binding.cdll.bcp_last_error()
    assert fn(out, 1, 2, 4, 6, boxes, 1, 0, None) == -1 and b"multiple of 4" in binding.cdll.bcp_last_error()
    assert fn(None, 1, 2, 4, 8, boxes, 1, 0, None) == -1 and b"null" in binding.cdll.bcp_last_error()
    assert binding.cdll.bcp_mix_mask(None, None, None, None, 1, 1, 4, 4, 0, None) == -1 and b"null" in binding.cdll.bcp_last_error()
    assert not any(buf), "a refused call must not write"


# ------------------------------------------------------------------------------------------ 2. mix
def check_mix_mask(ops, dev):
    _use(ops, dev)
    rng = np.random.default_rng(12)
    for shape in ((2, 6, 8, 12, 1), (3, 1, 16, 16, 1), (2, 5, 7, 20, 1), (1, 3, 9, 80, 1), (4, 2, 3, 4, 1)):
        N, D, Hh, W, _ = shape
        a, b = K.R(rng, *shape), K.R(rng, *shape)
        a.view(-1)[::7] = float("nan")
        b.view(-1)[::5] = -0.0
        a.view(-1)[3::11] = -0.0
        b.view(-1)[2::13] = float("nan")
        ad, bd = a.to(dev), b.to(dev)
        for per_sample in (False, True):
            m = torch.from_numpy((rng.random(((N,) if per_sample else ()) + (D, Hh, W)) < 0.6).astype(np.uint8))
            got = ops.mix_mask(ad, bd, m.to(dev))
            mm = (m if per_sample else m.unsqueeze(0).expand(N, D, Hh, W)).unsqueeze(-1).bool()
            assert torch.equal(_bits(got), _bits(torch.where(mm, a, b))), (shape, per_sample, "mix_mask == torch.where, bit for bit")
            other = ops.mix_mask(bd, ad, m.to(dev))
            sel = mm.expand_as(a)
            assert torch.equal(_bits(got)[sel], _bits(a)[sel]) and torch.equal(_bits(other)[sel], _bits(b)[sel])              # the two complementary
            assert torch.equal(_bits(got)[~sel], _bits(b)[~sel]) and torch.equal(_bits(other)[~sel], _bits(a)[~sel])          # mixes partition a and b
            assert torch.equal(_bits(ops.mix_mask(ad, ad, m.to(dev))), _bits(a)), "mix(a, a) == a"
        for m in (torch.ones(D, Hh, W, dtype=torch.uint8), torch.zeros(D, Hh, W, dtype=torch.uint8), torch.full((D, Hh, W), 255, dtype=torch.uint8)):
            assert torch.equal(_bits(ops.mix_mask(ad, bd, m.to(dev))), _bits(a if int(m[0, 0, 0]) else b)), "any non-zero byte selects a"
    # RegionMask through the scripts' expression and through BU.mix: many boxes -> the map kernels, one launch of the rasteriser per draw
    sp = (8, 12, 16)
    boxes = ((1, 2, 3, 3, 4, 5), (2, 4, 6, 4, 5, 7), (6, 0, 0, 2, 12, 2))
    a, b = K.R(rng, 2, 1, *sp).to(dev), K.R(rng, 2, 1, *sp).to(dev)
    img_mask, loss_mask = BU._region_pair(boxes, sp, 2, dev)
    dense = torch.from_numpy(np_mask(boxes, 1, *sp)[0]).to(dev)
    with count_calls(ops) as seen:
        got = a * img_mask + b * (1 - img_mask)
        got2 = (1 - img_mask) * b + img_mask * a
        loss_mask.u8(ops, 2)
    assert seen == {"bcp_mask_boxes": 1, "bcp_mix_mask": 2}, seen
    ref = torch.where(dense.bool(), a, b)
    assert torch.equal(got, ref) and torch.equal(got2, ref)
    user = BU.RegionMask(boxes, sp)                                                  # built by hand, no device given: the map follows the tensors
    assert torch.equal(a * user + b * (1 - user), ref) and user.u8(ops, 1, dev).device == a.device
    assert torch.equal(img_mask.tensor(dev, torch.uint8), dense) and torch.equal(loss_mask.u8(ops, 2).cpu(), torch.from_numpy(np_mask(boxes, 2, *sp)))
    assert img_mask.count() == int(dense.sum()) and (1 - loss_mask).count() == 2 * int((1 - dense).sum()) and tuple(loss_mask.shape) == (2,) + sp
    # a region of exactly ONE box is served by the box kernels: bit-identical to BoxMask, no map
    box = (2, 3, 5, 4, 6, 7)
    one, _ = BU._region_pair([box], sp, 2, dev)
    with count_calls(ops) as seen:
        got = a * one + b * (1 - one)
    assert seen == {"bcp_mix_box": 1}, seen
    bm = BU.BoxMask(box, sp, None, False, dev)
    assert torch.equal(got, a * bm + b * (1 - bm)) and torch.equal(got.view(2, *sp, 1), ops.mix_box(a.view(2, *sp, 1), b.view(2, *sp, 1), box))
    assert one.count() == bm.count() and torch.equal(one.tensor(dev), bm.tensor(dev))
    # 2-D, and what does not conform (labels, more channels) keeps the dense torch fallback
    boxes2 = ((1, 2, 5, 6), (9, 9, 4, 7), (3, 4, 5, 5))
    a2, b2 = K.R(rng, 3, 1, 16, 20).to(dev), K.R(rng, 3, 1, 16, 20).to(dev)
    m2, _ = BU._region_pair(boxes2, (16, 20), 3, dev)
    d2 = m2.tensor(dev, torch.bool)
    assert torch.equal(a2 * m2 + b2 * (1 - m2), torch.where(d2, a2, b2))
    la, lb = torch.from_numpy(rng.integers(0, 4, (3, 16, 20))).to(dev), torch.from_numpy(rng.integers(0, 4, (3, 16, 20))).to(dev)
    with count_calls(ops) as seen:
        got = la * m2 + lb * (1 - m2)
    assert not seen and torch.equal(got, torch.where(d2, la, lb))


# ------------------------------------------------------------------------------------------ 3. draws vs the reference's
_DRAW = {"random3d": lambda img: BU.random_mask(img), "concat3d": lambda img: BU.concate_mask(img),
         "random2d": lambda img: train_step.random_mask(img), "contact2d": lambda img: train_step.contact_mask(img)}


def check_draws_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "mask_strategies.npz"))
    cases = sorted({k.rsplit("/", 1)[0] for k in g.files})
    assert len(cases) >= 24
    per_fn = {}
    for c in cases:
        fn = c.split("_")[0]
        per_fn[(fn, c.split("/")[0])] = per_fn.get((fn, c.split("/")[0]), 0) + 1
        seed, shape, batch = int(g[c + "/seed"]), tuple(int(v) for v in g[c + "/shape"]), int(g[c + "/batch"])
        ref = np.unpackbits(g[c + "/bits"])[:int(np.prod(shape))].reshape(shape)
        np.random.seed(seed)
        img_mask, loss_mask = _DRAW[fn](torch.zeros((batch, 1) + shape))
        nxt = int(np.random.randint(0, 1 << 30))
        assert nxt == int(g[c + "/next"]), (c, "the call must consume np.random exactly as the reference does")
        assert isinstance(img_mask, BU.RegionMask) and isinstance(loss_mask, BU.RegionMask)
        assert np.array_equal(img_mask.tensor().numpy(), ref), c
        assert tuple(loss_mask.shape) == (batch,) + shape and tuple(img_mask.shape) == shape
        assert img_mask.count() == int(ref.sum()) and int(img_mask.sum()) == int(ref.sum()), c
        assert loss_mask.count() == batch * int(ref.sum()) and (1 - img_mask).count() == int((1 - ref).sum()), c
        lm = loss_mask.tensor().numpy()
        assert all(np.array_equal(lm[i], ref) for i in range(batch)), c
    assert len(per_fn) == 6 and all(v >= 4 for v in per_fn.values()), per_fn
    # patches too small for the grid: np.random.randint raises in the reference, and here
    for fn, shape in (("random3d", (12, 12, 8)), ("random2d", (2, 2))):
        try:
            _DRAW[fn](torch.zeros((1, 1) + shape))
        except ValueError:
            continue
        raise AssertionError(fn + ": expected ValueError from np.random.randint")


# ------------------------------------------------------------------------------------------ 4. loss through the region path
def check_region_loss(ops, dev):
    _use(ops, dev)
    rng = np.random.default_rng(13)
    # ---- LA flavour, 27 boxes
    N, sp = 2, (24, 24, 12)
    np.random.seed(3)
    img_mask, loss_mask = BU.random_mask(torch.zeros((N, 1) + sp, device=dev))
    assert len(loss_mask.boxes) == 27
    dense = loss_mask.tensor(torch.device("cpu"))                                   # int64 [N, X, Y, Z], as the reference's loss_mask
    lo = torch.from_numpy(rng.standard_normal((N, 2) + sp, dtype=np.float32) * 2)
    a, b = torch.from_numpy(rng.integers(0, 2, (N,) + sp)), torch.from_numpy(rng.integers(0, 2, (N,) + sp))
    a8, b8 = a.to(torch.uint8).to(dev), b.to(torch.uint8).to(dev)
    x = torch.zeros((N, 1) + sp, device=dev)
    for unlab in (False, True):
        lr = lo.clone().requires_grad_(True)
        ref = O.mix_loss_la(lr, a, b, dense, u_weight=0.5, unlab=unlab)
        ref.backward()
        lg = lo.clone().to(dev).requires_grad_(True)
        with count_calls(ops) as seen:
            x * img_mask + x * (1 - img_mask)                                        # the step's image mix comes first and rasterises
            loss = BU.mix_loss(lg, a8, b8, loss_mask, u_weight=0.5, unlab=unlab)
            loss.backward()
        assert seen.get("bcp_mask_boxes", 0) <= 1 and "bcp_cast" not in seen, seen   # one map per draw; no int64 -> uint8 pass over the mask
        assert abs(float(loss) - float(ref)) < 1e-5, (float(loss), float(ref))
        K.close(lg.grad, lr.grad, rtol=1e-4, msg="region mix_loss gradient")
        lg2 = lo.clone().to(dev).requires_grad_(True)
        loss2 = BU.mix_loss(lg2, a8, b8, loss_mask.u8(ops, N).clone(), u_weight=0.5, unlab=unlab)      # the dense uint8 map handed in directly
        loss2.backward()
        assert torch.equal(loss2.detach().cpu(), loss.detach().cpu()) and torch.equal(lg2.grad.cpu(), lg.grad.cpu()), "region == dense uint8 map, bit for bit"
    # ---- both calls of a step on one logits tensor (grouped), total on the device
    lo2 = torch.from_numpy(rng.standard_normal((2 * N, 2) + sp, dtype=np.float32) * 2)
    lr = lo2.clone().requires_grad_(True)
    ref1 = O.mix_loss_la(lr[:N], a, b, dense, u_weight=0.5)
    ref2 = O.mix_loss_la(lr[N:], b, a, dense, u_weight=0.5, unlab=True)
    (ref1 + ref2).backward()
    lg = lo2.clone().to(dev).requires_grad_(True)
    with count_calls(ops) as seen:
        total, l1, l2 = BU.mix_loss_pair(lg, (a8, b8, 1.0, 0.5), (b8, a8, 0.5, 1.0), loss_mask, total=True)
        total.backward()
    assert "bcp_cast" not in seen and "bcp_mask_boxes" not in seen, seen              # (the map of this draw exists already)
    assert abs(float(total) - float(ref1 + ref2)) < 1e-5 and abs(float(l1) - float(ref1)) < 1e-5 and abs(float(l2) - float(ref2)) < 1e-5
    K.close(lg.grad, lr.grad, rtol=1e-4, msg="region mix_loss_pair gradient")
    lg2 = lo2.clone().to(dev).requires_grad_(True)
    total2 = BU.mix_loss_pair(lg2, (a8, b8, 1.0, 0.5), (b8, a8, 0.5, 1.0), loss_mask.u8(ops, N).clone(), total=True)[0]
    total2.backward()
    assert torch.equal(total2.detach().cpu(), total.detach().cpu()) and torch.equal(lg2.grad.cpu(), lg.grad.cpu())
    lg3 = lo2[:N].clone().to(dev).requires_grad_(True)
    by_hand = BU.mix_loss(lg3, a8, b8, BU.RegionMask(loss_mask.boxes, sp, N))       # no device given: the map lives with the logits
    assert torch.equal(by_hand.detach().cpu(), BU.mix_loss(lg3, a8, b8, loss_mask).detach().cpu())
    try:
        BU.mix_loss(lg2, a8, b8, 1 - loss_mask)
    except ValueError:
        pass
    else:
        raise AssertionError("the complement of a loss mask must be refused, as for BoxMask")
    # ---- ACDC flavour, 9 boxes
    N, hw = 3, (48, 40)
    np.random.seed(4)
    img_mask, loss_mask = train_step.random_mask(torch.zeros((N, 1) + hw, device=dev))
    assert len(loss_mask.boxes) == 9
    dense = loss_mask.tensor(torch.device("cpu"))
    lo = torch.from_numpy(rng.standard_normal((N, 4) + hw, dtype=np.float32) * 2)
    a, b = torch.from_numpy(rng.integers(0, 4, (N,) + hw)), torch.from_numpy(rng.integers(0, 4, (N,) + hw))
    a8, b8 = a.to(torch.uint8).to(dev), b.to(torch.uint8).to(dev)
    for unlab in (False, True):
        lr = lo.clone().requires_grad_(True)
        rd, rc = O.mix_loss_acdc(lr, a, b, dense, u_weight=0.5, unlab=unlab)
        ((rd + rc) / 2).backward()
        lg = lo.clone().to(dev).requires_grad_(True)
        with count_calls(ops) as seen:
            d, c = train_step.acdc_mix_loss(lg, a8, b8, loss_mask, u_weight=0.5, unlab=unlab)
            ((d + c) / 2).backward()
        assert seen.get("bcp_mask_boxes", 0) <= 1 and "bcp_cast" not in seen, seen
        assert abs(float(d) - float(rd)) < 1e-5 and abs(float(c) - float(rc)) < 1e-5, (float(d), float(rd), float(c), float(rc))
        K.close(lg.grad, lr.grad, rtol=1e-4, msg="region acdc_mix_loss gradient")
        lg2 = lo.clone().to(dev).requires_grad_(True)
        d2, c2 = train_step.acdc_mix_loss(lg2, a8, b8, loss_mask.u8(ops, N).clone().view(N, *hw), u_weight=0.5, unlab=unlab)
        ((d2 + c2) / 2).backward()
        assert torch.equal(d2.detach().cpu(), d.detach().cpu()) and torch.equal(c2.detach().cpu(), c.detach().cpu()) and torch.equal(lg2.grad.cpu(), lg.grad.cpu())
    # one box: the loss's arithmetic box path, the same bits as BoxMask
    box = (5, 7, 20, 17)
    _, one = BU._region_pair([box], hw, N, dev)
    res = []
    for mask in (one, BU.BoxMask(box, hw, N, False, dev)):
        lg = lo.clone().to(dev).requires_grad_(True)
        with count_calls(ops) as seen:
            d, c = train_step.acdc_mix_loss(lg, a8, b8, mask)
            (d + c).backward()
        assert "bcp_mask_boxes" not in seen, seen
        res.append((d.detach().cpu(), c.detach().cpu(), lg.grad.cpu()))
    assert all(torch.equal(p, q) for p, q in zip(*res))


# ------------------------------------------------------------------------------------------ 5. steps
def multi_box_to_mask(box, spatial, batch):
    """oracle.box_to_mask for a LIST of boxes (the tests install it in the oracle with monkeypatch): ones with every box zeroed"""
    boxes = box if isinstance(box[0], (tuple, list)) else [box]
    nd = len(spatial)
    mask = torch.ones(spatial, dtype=torch.int64)
    for b in boxes:
        mask[tuple(slice(b[ax], b[ax] + b[nd + ax]) for ax in range(nd))] = 0
    return mask, mask.unsqueeze(0).repeat(batch, *([1] * nd)).contiguous()


def _grad_errors(params, ref_grads):
    """rel-L2 of every gradient tensor against the oracle's.  Left out, as in net_checks.check_la_step_full: conv biases that feed a norm
    layer -- their exact gradient is 0, which is what the kernels write, while the oracle holds rounding noise (net_checks.is_prenorm_bias)"""
    return sorted(((K.rel_l2(params[k].grad, g), k) for k, g in ref_grads.items() if not NC.is_prenorm_bias(k, params) and float(g.norm()) > 1e-9),
                  reverse=True)


def _la_nets(P, dev, ops, variant):
    model = NC.make_vnet(P, dev, ops, variant=variant, has_dropout=variant == "la")
    ema = NC.make_vnet(P, dev, ops, variant=variant, has_dropout=variant == "la")
    for p in ema.parameters():
        p.detach_()
    return model, ema


def check_la_step_regions(ops, dev, monkeypatch, variant="la", modes=(True, False)):
    """tiny LA / pancreas self-training step with a multi-box region, grouped and as the scripts read, against the oracle's step on the
    dense mask of the same boxes"""
    monkeypatch.setattr(O, "box_to_mask", multi_box_to_mask)
    rng = np.random.default_rng(5)
    if variant == "la":
        shape, sub, seed, kw, okw = (32, 32, 16), 2, 81, {}, {}
        boxes = [(2, 3, 1, 8, 9, 5), (14, 12, 6, 10, 8, 7), (10, 10, 4, 8, 8, 6), (20, 0, 9, 12, 20, 7), (0, 25, 0, 6, 7, 16)]
        drops = {k: {"x5": torch.from_numpy((rng.random((sub, 256)) < 0.5).astype(np.float32)),
                     "x9": torch.from_numpy((rng.random((sub, 16)) < 0.5).astype(np.float32))} for k in ("t_a", "t_b", "s_l", "s_u")}
    else:
        shape, sub, seed, kw, okw = (32, 32, 32), 1, 91, dict(variant="pancreas", connect_mode=2), dict(variant="pancreas", connectivity=2)
        boxes = [(4, 6, 3, 10, 9, 12), (10, 12, 10, 12, 10, 9), (20, 2, 20, 12, 14, 12), (0, 24, 0, 32, 8, 5)]
        drops = {}
    P = O.init_params(O.vnet_param_shapes(variant=variant), seed=seed, random_affine=True)
    vol, lab = O.synth_la_batch(4 * sub, shape=shape, seed=seed + 1)
    ro = O.la_self_train_step({k: v.clone() for k, v in P.items()}, {k: v.clone() for k, v in P.items()}, vol, lab, boxes, drops, sub, **okw)
    for grouped in modes:
        model, ema = _la_nets(P, dev, ops, variant)
        with count_calls(ops) as seen:
            r = train_step.la_self_train_step(model, ema, None, vol.to(dev), lab.to(dev), 2 * sub, box=boxes, drops=drops, grouped=grouped, **kw)
        assert seen.get("bcp_mask_boxes") == 1 and seen.get("bcp_mix_mask") == 2 and "bcp_mix_box" not in seen, (grouped, seen)
        dl = abs(float(r["loss"]) - float(ro["loss"]))
        flips = int((r["plab_a"].cpu().float() != ro["plab_a"]).sum() + (r["plab_b"].cpu().float() != ro["plab_b"]).sum())
        errs = _grad_errors(dict(model.named_parameters()), ro["grads"])
        print(f"[la_step_regions {variant} grouped={grouped}] |dloss| {dl:.3e} flips {flips} worst grad rel-L2 {errs[0][0]:.3e} ({errs[0][1]}) median {errs[len(errs) // 2][0]:.3e}")
        assert dl < 1e-5 and abs(float(r["loss_l"]) - float(ro["loss_l"])) < 1e-5, (grouped, float(r["loss"]), float(ro["loss"]))
        assert flips <= 4
        assert errs[0][0] < 3e-2, (grouped, errs[:5])


def check_la_step_dispatch(ops, dev, one_box_modes=(True, False), strategies=("random", "concat")):
    """a one-box list is the box path (bit-identical to the tuple); mask_strategy draws what the draw function draws"""
    rng = np.random.default_rng(6)
    shape, sub = (32, 32, 16), 1
    P = O.init_params(O.vnet_param_shapes(), seed=83, random_affine=True)
    vol, lab = O.synth_la_batch(4 * sub, shape=shape, seed=84)
    drops = {k: {"x5": torch.from_numpy((rng.random((sub, 256)) < 0.5).astype(np.float32)),
                 "x9": torch.from_numpy((rng.random((sub, 16)) < 0.5).astype(np.float32))} for k in ("t_a", "t_b", "s_l", "s_u")}

    def run(**kw):
        model, ema = _la_nets(P, dev, ops, "la")
        with count_calls(ops) as seen:
            r = train_step.la_self_train_step(model, ema, None, vol.to(dev), lab.to(dev), 2 * sub, drops=drops, **kw)
        return r["loss"].cpu(), model.flat_trainable()[1].detach().cpu().clone(), seen

    box = (3, 5, 2, 21, 21, 10)
    for grouped in one_box_modes:
        l0, g0, s0 = run(box=box, grouped=grouped)
        l1, g1, s1 = run(box=[box], grouped=grouped)
        assert torch.equal(l0, l1) and torch.equal(g0, g1) and mask_calls(s0) == mask_calls(s1) == (0, 0, 2), (grouped, s0, s1)
    for strategy, draw, n in (("random", BU.random_mask, 27), ("concat", BU.concate_mask, 1)):
        if strategy not in strategies:
            continue
        np.random.seed(21)
        l0, g0, s0 = run(mask_strategy=strategy)
        after = np.random.randint(0, 1 << 30)
        np.random.seed(21)
        _, loss_mask = draw(vol[:sub])
        assert len(loss_mask.boxes) == n and after == np.random.randint(0, 1 << 30)
        l1, g1, s1 = run(box=list(loss_mask.boxes))
        assert torch.equal(l0, l1) and torch.equal(g0, g1), strategy
        assert mask_calls(s0) == mask_calls(s1) == ((1, 2, 0) if n > 1 else (0, 0, 2)), (strategy, s0, s1)
    for bad in ("contact", "box", ""):
        try:
            run(mask_strategy=bad)
        except ValueError:
            continue
        raise AssertionError(f"mask_strategy={bad!r} must raise ValueError")


def check_acdc_step_regions(ops, dev, monkeypatch, modes=(True, False), dispatch=True):
    """tiny ACDC self-training step with a 5-box region, grouped and as the script reads, against the oracle (pseudo-labels forced to the
    oracle's, as net_checks.check_acdc_step_full compares gradients); one-box list == tuple; mask_strategy == the draw"""
    monkeypatch.setattr(O, "box_to_mask", multi_box_to_mask)
    rng = np.random.default_rng(7)
    hw, lsub = (64, 64), 2
    P = O.init_params(O.unet_param_shapes(), seed=62, random_affine=True)
    vol, lab = O.synth_acdc_batch(4 * lsub, shape=hw, seed=63)
    drops = {k: NC._rand_unet_drops(rng, lsub, hw) for k in ("t_a", "t_b", "s_unl", "s_l")}
    boxes = [(3, 5, 14, 12), (20, 22, 18, 16), (30, 30, 20, 12), (50, 0, 14, 40), (0, 52, 33, 12)]
    ro = O.acdc_self_train_step({k: v.clone() for k, v in P.items()}, {k: v.clone() for k, v in P.items()}, vol, lab, boxes, drops, lsub, lsub)
    plabs = (ro["plab_a"].to(torch.uint8).to(dev), ro["plab_b"].to(torch.uint8).to(dev))

    def run(**kw):
        model, ema = NC.make_unet(P, dev, ops), NC.make_unet(P, dev, ops)
        for p in ema.parameters():
            p.detach_()
        with count_calls(ops) as seen:
            r = train_step.acdc_self_train_step(model, ema, None, vol.to(dev), lab.to(dev), 2 * lsub, drops=drops, plabs=plabs, **kw)
        return r, model, seen

    for grouped in modes:
        r, model, seen = run(box=boxes, grouped=grouped)
        assert seen.get("bcp_mask_boxes") == 1 and seen.get("bcp_mix_mask") == 2 and "bcp_mix_box" not in seen, (grouped, seen)
        errs = _grad_errors(dict(model.named_parameters()), ro["grads"])
        print(f"[acdc_step_regions grouped={grouped}] |dloss| {abs(float(r['loss']) - float(ro['loss'])):.3e} worst grad rel-L2 {errs[0][0]:.3e} ({errs[0][1]}) "
              f"median {errs[len(errs) // 2][0]:.3e}")
        for k in ("loss", "loss_dice", "loss_ce"):
            assert abs(float(r[k]) - float(ro[k])) < 1e-5, (grouped, k, float(r[k]), float(ro[k]))
        assert errs[0][0] < 3e-2, (grouped, errs[:5])
    try:
        run(mask_strategy="concat")
    except ValueError:
        pass
    else:
        raise AssertionError("mask_strategy='concat' is a 3-D strategy: the 2-D step must raise ValueError")
    if not dispatch:
        return
    box = (7, 9, 42, 42)
    (r0, m0, s0), (r1, m1, s1) = run(box=box), run(box=[box])
    assert torch.equal(r0["loss"].cpu(), r1["loss"].cpu()) and torch.equal(m0.flat_trainable()[1].cpu(), m1.flat_trainable()[1].cpu()) and mask_calls(s0) == mask_calls(s1) == (0, 0, 2)
    for strategy, draw, n in (("random", train_step.random_mask, 9), ("contact", train_step.contact_mask, 1)):
        np.random.seed(22)
        r0, m0, s0 = run(mask_strategy=strategy)
        np.random.seed(22)
        _, loss_mask = draw(vol[:lsub])
        assert len(loss_mask.boxes) == n
        r1, m1, s1 = run(box=list(loss_mask.boxes))
        assert torch.equal(r0["loss"].cpu(), r1["loss"].cpu()) and torch.equal(m0.flat_trainable()[1].cpu(), m1.flat_trainable()[1].cpu()), strategy
        assert mask_calls(s0) == mask_calls(s1) == ((1, 2, 0) if n > 1 else (0, 0, 2)), (strategy, s0, s1)


def check_pre_train_regions(ops, dev, acdc=True):
    """the pre-training steps take the region too: mask_strategy == the draw handed in as box=, both finite"""
    P = O.init_params(O.vnet_param_shapes(), seed=85, random_affine=True)
    vol, lab = O.synth_la_batch(2, shape=(32, 32, 16), seed=86)
    res = []
    for it in range(2):
        model = NC.make_vnet(P, dev, ops, has_dropout=False)
        opt = train_step.FlatSGD(model, lr=0.01)
        np.random.seed(23)
        kw = dict(mask_strategy="random") if it == 0 else dict(box=list(BU.random_mask(vol[:1])[1].boxes))
        res.append(train_step.la_pre_train_step(model, opt, vol.to(dev), lab.to(dev), **kw)["loss"].cpu())
    assert torch.equal(res[0], res[1]) and bool(torch.isfinite(res[0]))
    if not acdc:
        return
    P = O.init_params(O.unet_param_shapes(), seed=64, random_affine=True)
    vol, lab = O.synth_acdc_batch(4, shape=(64, 64), seed=65)
    res = []
    for it in range(2):
        model = NC.make_unet(P, dev, ops)
        model._drop_seed = 9
        opt = train_step.FlatSGD(model, lr=0.01)
        np.random.seed(24)
        kw = dict(mask_strategy="random") if it == 0 else dict(box=list(train_step.random_mask(vol[:2])[1].boxes))
        res.append(train_step.acdc_pre_train_step(model, opt, vol.to(dev), lab.to(dev), **kw)["loss"].cpu())
    assert torch.equal(res[0], res[1]) and bool(torch.isfinite(res[0]))


# ------------------------------------------------------------------------------------------ 6. product sizes (GPU)
def check_full_size_properties(ops, dev):
    """the partition and count properties of test_gpu_kernels.test_full_size_properties (4) / (6) with a 27-box (9-box) region at the sizes the
    three loops run, and the rasteriser against numpy there"""
    g = torch.Generator(device="cpu").manual_seed(3)
    np.random.seed(8)
    for N, sp, draw in ((2, (112, 112, 80), BU.random_mask), (2, (96, 96, 96), BU.random_mask), (12, (256, 256), train_step.random_mask)):
        a, b = torch.randn(N, 1, *sp, generator=g).to(dev), torch.randn(N, 1, *sp, generator=g).to(dev)
        img_mask, loss_mask = draw(a)
        assert len(img_mask.boxes) in (9, 27)
        m1, m2 = a * img_mask + b * (1 - img_mask), b * img_mask + a * (1 - img_mask)
        assert torch.equal(m1 + m2, a + b) and torch.equal(a * img_mask + a * (1 - img_mask), a)
        inside = int((m1 == b).sum()) - int((a == b).sum())
        assert inside == N * (1 - img_mask).count() == (1 - loss_mask).count(), (sp, inside)
        sp3 = sp if len(sp) == 3 else (1,) + sp
        ref = np_mask(img_mask.boxes6(), N, *sp3)
        assert np.array_equal(loss_mask.u8(ops, N).cpu().numpy(), ref)
        assert int(ref.sum()) == loss_mask.count() and np.array_equal(img_mask.tensor().cpu().numpy().reshape(sp3), ref[0])
        for complement in (False, True):
            assert np.array_equal(ops.mask_boxes(img_mask.boxes6(), (N,) + sp3, dev, complement=complement).cpu().numpy(), np_mask(img_mask.boxes6(), N, *sp3, complement))
    torch.cuda.synchronize()


def check_full_size_step(ops, dev, config):
    """one full-size self-training step with mask_strategy="random" (grouped, the product path: rasterised map, bcp_mix_mask, the loss on the
    map) == the same step typed out as the scripts read -- separate network calls, DENSE torch masks from tensor(), torch-expression mixing,
    mix_loss per call -- within the 1e-5 the grouped-vs-separate checks use; the loss is finite"""
    from bcp_amd.train_step import acdc_mix_loss, get_ACDC_masks, get_cut_mask
    rng = np.random.default_rng(31)
    if config == "acdc":
        hw, lsub = (256, 256), 6
        P = O.init_params(O.unet_param_shapes(), seed=66, random_affine=True)
        vol, lab = O.synth_acdc_batch(4 * lsub, shape=hw, seed=67)
        drops = {k: NC._rand_unet_drops(rng, lsub, hw) for k in ("t_a", "t_b", "s_unl", "s_l")}
        make = lambda: NC.make_unet(P, dev, ops)
    else:
        variant = config
        shape, lsub = ((112, 112, 80), 1) if variant == "la" else ((96, 96, 96), 1)
        P = O.init_params(O.vnet_param_shapes(variant=variant), seed=45, random_affine=True)
        vol, lab = O.synth_la_batch(4 * lsub, shape=shape, seed=46)
        drops = {k: {"x5": torch.from_numpy((rng.random((lsub, 256)) < 0.5).astype(np.float32)),
                     "x9": torch.from_numpy((rng.random((lsub, 16)) < 0.5).astype(np.float32))} for k in ("t_a", "t_b", "s_l", "s_u")} if variant == "la" else {}
        make = lambda: NC.make_vnet(P, dev, ops, variant=variant, has_dropout=variant == "la")
    vol, lab = vol.to(dev), lab.to(dev)

    def nets():
        model, ema = make(), make()
        for p in ema.parameters():
            p.detach_()
        return model, ema

    model, ema = nets()
    np.random.seed(33)
    with count_calls(ops) as seen:
        if config == "acdc":
            r = train_step.acdc_self_train_step(model, ema, None, vol, lab, 2 * lsub, drops=drops, mask_strategy="random")
        else:
            kw = {} if config == "la" else dict(variant="pancreas", connect_mode=2)
            r = train_step.la_self_train_step(model, ema, None, vol, lab, 2 * lsub, drops=drops, mask_strategy="random", **kw)
    assert mask_calls(seen) == (1, 2, 0), seen
    loss_fused = float(r["loss"])
    assert np.isfinite(loss_fused)
    # ---- the script form
    model, ema = nets()
    np.random.seed(33)
    lb = 2 * lsub
    img_a, img_b, uimg_a, uimg_b = vol[:lsub], vol[lsub:lb], vol[lb:lb + lsub], vol[lb + lsub:]
    lab_a, lab_b = lab[:lsub], lab[lsub:lb]
    with torch.no_grad():
        if config == "acdc":
            ema.drop_masks = drops["t_a"]
            pre_a = ema(uimg_a)
            ema.drop_masks = drops["t_b"]
            pre_b = ema(uimg_b)
            plab_a, plab_b = get_ACDC_masks(pre_a, nms=1), get_ACDC_masks(pre_b, nms=1)
            rm, rl = train_step.random_mask(img_a)
        else:
            ema.drop_masks = drops.get("t_a")
            ua = ema(uimg_a, features=False)[0]
            ema.drop_masks = drops.get("t_b")
            ub = ema(uimg_b, features=False)[0]
            cm = None if config == "la" else 2
            plab_a, plab_b = get_cut_mask(ua, nms=1, connect_mode=cm), get_cut_mask(ub, nms=1, connect_mode=cm)
            rm, rl = BU.random_mask(img_a)
        img_mask, loss_mask = rm.tensor(dev), rl.tensor(dev)                           # dense int64, as the reference's functions return
    if config == "acdc":
        net_input_unl = uimg_a * img_mask + img_a * (1 - img_mask)
        net_input_l = img_b * img_mask + uimg_b * (1 - img_mask)
        model.drop_masks = drops["s_unl"]
        out_unl = model(net_input_unl)
        unl_dice, unl_ce = acdc_mix_loss(out_unl, plab_a, lab_a, loss_mask, u_weight=0.5, unlab=True)
        model.drop_masks = drops["s_l"]
        out_l = model(net_input_l)
        l_dice, l_ce = acdc_mix_loss(out_l, lab_b, plab_b, loss_mask, u_weight=0.5)
        loss = ((unl_dice + l_dice) + (unl_ce + l_ce)) / 2
    elif config == "la":
        mixl = img_a * img_mask + uimg_a * (1 - img_mask)
        mixu = uimg_b * img_mask + img_b * (1 - img_mask)
        model.drop_masks = drops["s_l"]
        out_l = model(mixl, features=False)[0]
        loss_l = BU.mix_loss(out_l, lab_a, plab_a, loss_mask, u_weight=0.5)
        model.drop_masks = drops["s_u"]
        out_u = model(mixu, features=False)[0]
        loss_u = BU.mix_loss(out_u, plab_b, lab_b, loss_mask, u_weight=0.5, unlab=True)
        loss = loss_l + loss_u
    else:
        mixl = uimg_a * img_mask + img_b * (1 - img_mask)
        mixu = img_a * img_mask + uimg_b * (1 - img_mask)
        out_l = model(mixl, features=False)[0]
        loss_l = BU.mix_loss(out_l, plab_a, lab_b, loss_mask, unlab=True)
        out_u = model(mixu, features=False)[0]
        loss_u = BU.mix_loss(out_u, lab_a, plab_b, loss_mask)
        loss = loss_l + loss_u
    model.drop_masks = ema.drop_masks = None
    loss_script = float(loss.detach())
    torch.cuda.synchronize()
    print(f"[full_size_step {config}] fused {loss_fused:.7f} script {loss_script:.7f} |d| {abs(loss_fused - loss_script):.3e}")
    assert abs(loss_fused - loss_script) < 1e-5, (config, loss_fused, loss_script)
