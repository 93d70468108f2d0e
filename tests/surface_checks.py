"""Checks of the surface distances on the device (bcp_surface_border, bcp_edt_sq, bcp_surface_hist, bcp_amd/utils/surface.py and the opt-in
wiring of the three validation paths).  Shared by tests/test_emu_surface.py (host simulator, CPU tensors) and
tests/test_gpu_surface.py (-m gpu), in the style of mask_checks.py.

The yardstick is a restatement of what medpy.metric.binary.hd95 / asd compute with their default arguments (unit voxel spacing,
connectivity 1), written with the two scipy calls medpy makes:
    border(m) = m ^ binary_erosion(m, generate_binary_structure(3, 1))
    sds(a, b) = distance_transform_edt(~border(b))[border(a)]
    hd95      = np.percentile(np.hstack((sds(a, b), sds(b, a))), 95)
    asd       = sds(a, b).mean()
Tolerances: border maps, squared distances and histograms are integers -- equal element for element.  hd95 is the percentile of the same
multiset of doubles (sqrt of an integer, correctly rounded on both sides) -- exact float equality.  asd is a mean of at most 2^20 such
doubles and differs from the reference by the summation order only -- 1e-12 relative.
"""
import contextlib
import ctypes
import functools
import math
import os

import numpy as np
import torch
from scipy import ndimage

import bcp_oracle as O
import net_checks as NC
from bcp_amd import hip_ops as H
from bcp_amd.utils import BCP_utils as BU
from bcp_amd.utils import surface as S

# all extents odd and W longer than a wave; one slice (every object voxel is border); H past 64 with a tiny W; a line past 128; D past 128
# with several workgroups' worth on every axis; the base case
SHAPES = ((7, 13, 70), (1, 9, 11), (5, 66, 3), (2, 130, 67), (130, 67, 70), (16, 16, 16))
STRUCT = ndimage.generate_binary_structure(3, 1)


def _use(ops, dev):
    if dev.type == "cpu":
        BU.set_test_ops(ops)


# ------------------------------------------------------------------------------------------ the restatement
def ref_border(m):
    m = np.atleast_1d(m.astype(bool))
    return m ^ ndimage.binary_erosion(m, structure=STRUCT, iterations=1)


def ref_d2(sites):
    """squared distance to the nearest site as integers"""
    return np.rint(ndimage.distance_transform_edt(~sites.astype(bool)) ** 2).astype(np.int64)


def ref_sds(a, b):
    if not a.any():
        raise RuntimeError("The first supplied array does not contain any binary object.")
    if not b.any():
        raise RuntimeError("The second supplied array does not contain any binary object.")
    return ndimage.distance_transform_edt(~ref_border(b))[ref_border(a)]


def ref_hd95(a, b):
    return float(np.percentile(np.hstack((ref_sds(a, b), ref_sds(b, a))), 95))


def ref_asd(a, b):
    return float(ref_sds(a, b).mean())


# ------------------------------------------------------------------------------------------ inputs
def _grid(shape):
    return np.meshgrid(*(np.arange(s, dtype=np.float64) for s in shape), indexing="ij")


def _ellipsoid(shape, centre, radii):
    g = _grid(shape)
    return sum(((x - c) / max(r, 0.6)) ** 2 for x, c, r in zip(g, centre, radii)) <= 1.0


def _blobs(shape, rng, n=3, lo=0.12, hi=0.35):
    m = np.zeros(shape, dtype=bool)
    for _ in range(n):
        c = [rng.random() * (s - 1) for s in shape]
        r = [max(1.0, (lo + (hi - lo) * rng.random()) * s) for s in shape]
        m |= _ellipsoid(shape, c, r)
    return m


def _labels(shape, rng):
    """a blocky four-label map: every label forms a few connected pieces with real surfaces"""
    coarse = rng.integers(0, 4, tuple(-(-s // 4) for s in shape))
    return np.kron(coarse, np.ones((4, 4, 4), dtype=np.int64))[:shape[0], :shape[1], :shape[2]].astype(np.uint8)


@functools.lru_cache(maxsize=None)
def cases(shape):
    """[(name, a, b, cls)]: uint8 volumes; the object is `!= 0` (cls 0) or `== cls`.  Built once per shape and never modified."""
    rng = np.random.default_rng(1000 + sum(shape))
    D, Hh, W = shape
    out = []
    a, b = _blobs(shape, rng), _blobs(shape, rng)
    out.append(("ellipsoids", a, b, 0))
    out.append(("same", a, a.copy(), 0))
    c0, c1 = np.zeros(shape, dtype=bool), np.zeros(shape, dtype=bool)
    c0[0, 0, 0] = True
    c1[-1, -1, -1] = True
    out.append(("corners", c0, c1, 0))                                  # the top histogram bin
    out.append(("full", np.ones(shape, dtype=bool), b, 0))              # the border is the six faces
    ctr = [(s - 1) / 2 for s in shape]
    outer = _ellipsoid(shape, ctr, [0.48 * s for s in shape])
    inner = _ellipsoid(shape, ctr, [0.30 * s for s in shape])
    core = _ellipsoid(shape, ctr, [0.15 * s for s in shape])
    out.append(("shell", outer & ~inner, core, 0))                      # a hollow shell around a second object
    lo = _ellipsoid(shape, [0.1 * s for s in shape], [0.12 * s for s in shape])
    hi = _ellipsoid(shape, [0.9 * (s - 1) for s in shape], [0.12 * s for s in shape])
    out.append(("far", lo | hi, lo, 0))                                 # two objects far apart against one of them
    la, lb = _labels(shape, rng), _labels(shape, rng)
    for cls in (1, 2, 3):
        out.append((f"labels{cls}", la, lb, cls))
    res = []
    for name, x, y, cls in out:
        x, y = np.ascontiguousarray(x.astype(np.uint8)), np.ascontiguousarray(y.astype(np.uint8))
        x.setflags(write=False)
        y.setflags(write=False)
        res.append((name, x, y, cls))
    return tuple(res)


def _sel(x, cls):
    return (x == cls) if cls else (x != 0)


@functools.lru_cache(maxsize=None)
def reference(shape):
    """{case name: dict} of the restatement's results, computed once per shape and shared by every check"""
    nb = H.Ops.surface_bins(shape)
    ref = {}
    for name, x, y, cls in cases(shape):
        a, b = _sel(x, cls), _sel(y, cls)
        ba, bb = ref_border(a), ref_border(b)
        r = {"ba": ba, "bb": bb}
        if a.any() and b.any():
            eb, ea = ndimage.distance_transform_edt(~bb), ndimage.distance_transform_edt(~ba)      # the two calls medpy makes
            d2b, d2a = np.rint(eb ** 2).astype(np.int64), np.rint(ea ** 2).astype(np.int64)
            assert np.array_equal(np.sqrt(d2b), eb) and np.array_equal(np.sqrt(d2a), ea)           # unit spacing: sqrt of an integer, bit for bit
            sab, sba = eb[ba], ea[bb]
            r.update(d2a=d2a, d2b=d2b, hab=np.bincount(d2b[ba], minlength=nb), hba=np.bincount(d2a[bb], minlength=nb),
                     hd95=float(np.percentile(np.hstack((sab, sba)), 95)), asd=float(sab.mean()))
        ref[name] = r
    return ref


def _t(x, dev):
    return torch.from_numpy(np.array(x, order="C")).to(dev)      # a copy: the shared inputs are read-only


def _u32(hist):
    assert hist.dtype == torch.int64 and int(hist.min()) >= 0      # Ops.surface_hist widens the library's uint32 bins
    return hist.cpu().numpy()


# ------------------------------------------------------------------------------------------ 1-3. kernels
def check_kernels(ops, dev, shape):
    """border map == the erosion restatement bit for bit and its count; edt_sq == rint(distance_transform_edt ** 2) element for element
    (and == a brute-force minimum over all sites for extents up to 16); histogram == np.bincount of the reference squared distances at
    the reference border voxels, its sum == the border count"""
    _use(ops, dev)
    ref = reference(shape)
    nb = ops.surface_bins(shape)
    assert nb == sum((s - 1) ** 2 for s in shape) + 1
    for name, x, y, cls in cases(shape):
        r = ref[name]
        maps = []
        for key, v in (("ba", x), ("bb", y)):
            border, count = ops.surface_border(_t(v, dev), cls)
            assert border.dtype == torch.uint8 and np.array_equal(border.cpu().numpy(), r[key].astype(np.uint8)), (shape, name, key)
            assert int(count.item()) == int(r[key].sum()), (shape, name, key)
            maps.append(border)
        if "d2a" not in r:
            continue
        d2 = []
        for key, border in (("d2a", maps[0]), ("d2b", maps[1])):
            got = ops.edt_sq(border)
            assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy().astype(np.int64), r[key]), (shape, name, key)
            if max(shape) <= 16:
                assert np.array_equal(got.cpu().numpy(), _brute_d2(r["ba" if key == "d2a" else "bb"])), (shape, name, key)
            d2.append(got)
        for key, border, dist, n in (("hab", maps[0], d2[1], r["ba"].sum()), ("hba", maps[1], d2[0], r["bb"].sum())):
            hist = _u32(ops.surface_hist(border, dist))
            assert hist.shape == (nb,) and np.array_equal(hist, r[key]), (shape, name, key)
            assert int(hist.sum()) == int(n), (shape, name, key)
        if name == "corners":
            assert _u32(ops.surface_hist(maps[0], d2[1]))[nb - 1] == 1, "opposite corners land in the top bin"
    # a general site map (not a border map): sparse random sites, and with a reused scratch volume
    rng = np.random.default_rng(7 + sum(shape))
    sites = (rng.random(shape) < 0.02).astype(np.uint8)
    sites[tuple(rng.integers(0, s) for s in shape)] = 1
    scratch = torch.empty(shape, dtype=torch.int32, device=dev)
    got = ops.edt_sq(_t(sites, dev), scratch).cpu().numpy().astype(np.int64)
    assert np.array_equal(got, ref_d2(sites)), (shape, "random sites")
    if max(shape) <= 16:
        assert np.array_equal(got, _brute_d2(sites)), (shape, "random sites, brute force")


def _brute_d2(sites):
    """independent brute force: the minimum over ALL sites of the integer squared distance"""
    idx = np.argwhere(np.ones(sites.shape, dtype=bool)).astype(np.int64)
    s = np.argwhere(sites).astype(np.int64)
    d2 = ((idx[:, None, :] - s[None, :, :]) ** 2).sum(-1).min(1)
    return d2.reshape(sites.shape)


def check_nosite(ops, dev):
    """a line without a site carries EDT_NOSITE exactly; a volume without a site ends with every value >= EDT_NOSITE (and no overflow);
    sites in one line only still reach every voxel; the histogram of a distance map without sites counts nothing"""
    _use(ops, dev)
    assert H.EDT_NOSITE == 1 << 30
    line = ops.edt_sq(torch.zeros((1, 1, 70), dtype=torch.uint8, device=dev)).cpu().numpy()
    assert (line == H.EDT_NOSITE).all()
    for shape in ((5, 6, 7), (3, 130, 5)):
        vol = ops.edt_sq(torch.zeros(shape, dtype=torch.uint8, device=dev)).cpu().numpy().astype(np.int64)
        assert (vol >= H.EDT_NOSITE).all() and (vol < H.EDT_NOSITE + (1 << 22)).all(), shape
        one = np.zeros(shape, dtype=np.uint8)
        one[shape[0] - 1, 2, 3] = 1                      # every other W line is empty after the first pass
        got = ops.edt_sq(_t(one, dev)).cpu().numpy().astype(np.int64)
        assert np.array_equal(got, ref_d2(one)), shape
        border = torch.ones(shape, dtype=torch.uint8, device=dev)
        hist = _u32(ops.surface_hist(border, ops.edt_sq(torch.zeros(shape, dtype=torch.uint8, device=dev))))
        assert hist.sum() == 0, shape


# ------------------------------------------------------------------------------------------ 4-7. metrics
def check_metrics(ops, dev, shape):
    """hd95 == the restatement exactly, asd within 1e-12 relative, both 0.0 for a == b; the histograms and counts of
    surface_histograms are the reference's"""
    _use(ops, dev)
    ref = reference(shape)
    for name, x, y, cls in cases(shape):
        r = ref[name]
        if "hd95" not in r:
            with _raises_runtime():
                S.hd95_asd(_t(x, dev), _t(y, dev), cls)
            continue
        hab, hba, na, nb_ = S.surface_histograms(_t(x, dev), _t(y, dev), cls)
        assert np.array_equal(hab, r["hab"]) and np.array_equal(hba, r["hba"]), (shape, name)
        assert (na, nb_) == (int(r["ba"].sum()), int(r["bb"].sum())), (shape, name)
        hd, asd = S.hd95_asd(_t(x, dev), _t(y, dev), cls)
        print(f"[surface] {shape} {name}: hd95 {hd!r} (ref {r['hd95']!r})  asd {asd!r} (ref {r['asd']!r})")
        assert hd == r["hd95"], (shape, name, hd, r["hd95"])
        assert abs(asd - r["asd"]) <= 1e-12 * abs(r["asd"]), (shape, name, asd, r["asd"])
        if name == "same":
            assert hd == 0.0 and asd == 0.0, (shape, name, hd, asd)
        if name == "corners":
            assert hd == math.sqrt(sum((s - 1) ** 2 for s in shape)) == asd, (shape, name, hd, asd)


@contextlib.contextmanager
def _raises_runtime():
    try:
        yield
    except RuntimeError as e:
        assert not isinstance(e, H._lib.BcpError), f"a library error, not medpy's refusal: {e}"
        return
    raise AssertionError("an empty object must raise RuntimeError, as medpy does")


def check_empty_raises(ops, dev):
    _use(ops, dev)
    shape = (5, 6, 7)
    full = torch.ones(shape, dtype=torch.uint8, device=dev)
    empty = torch.zeros(shape, dtype=torch.uint8, device=dev)
    for a, b, cls in ((empty, full, 0), (full, empty, 0), (empty, empty, 0), (full, full, 2), (full * 2, full, 2)):
        with _raises_runtime():
            S.hd95_asd(a, b, cls)
    hab, hba, na, nb_ = S.surface_histograms(empty, full, 0)
    assert na == 0 and nb_ == int(ref_border(np.ones(shape, dtype=bool)).sum()) and hab.sum() == 0 and hba.sum() == 0
    # numpy inputs and non-uint8 labels go the same way
    x, y = cases((16, 16, 16))[0][1:3]
    assert S.hd95_asd(_t(x, dev), y.astype(np.float32) * 3.0) == S.hd95_asd(_t(x, dev), _t(y, dev))


# ------------------------------------------------------------------------------------------ 8. refusals
def check_refusals(binding):
    """bad arguments are refused with -1 and a message before any launch (no device needed): null pointers, an extent outside 1..1024,
    cls outside 0..255, too few bins"""
    buf = (ctypes.c_ubyte * 8192)()
    p = (ctypes.addressof(buf) + 15) & ~15
    q = p + 4096
    err = binding.cdll.bcp_last_error
    fb, fe, fh = binding.cdll.bcp_surface_border, binding.cdll.bcp_edt_sq, binding.cdll.bcp_surface_hist
    for args in ((None, 2, 2, 2, 0, q, q + 64, None), (p, 2, 2, 2, 0, None, q + 64, None), (p, 2, 2, 2, 0, q, None, None)):
        assert fb(*args) == -1 and b"null" in err(), args
    for ext in ((0, 2, 2), (2, 1025, 2), (2, 2, -1), (1025, 1, 1)):
        assert fb(p, *ext, 0, q, q + 64, None) == -1 and b"1..1024" in err(), ext
        assert fe(p, *ext, q, q + 1024, None) == -1 and b"1..1024" in err(), ext
        assert fh(p, q, *ext, q + 1024, 1 << 22, None) == -1 and b"1..1024" in err(), ext
    for cls in (-1, 256):
        assert fb(p, 2, 2, 2, cls, q, q + 64, None) == -1 and b"cls" in err(), cls
    for args in ((None, 2, 2, 2, q, q + 1024, None), (p, 2, 2, 2, None, q + 1024, None), (p, 2, 2, 2, q, None, None)):
        assert fe(*args) == -1 and b"null" in err(), args
    assert fe(p, 2, 2, 2, q, q, None) == -1 and b"scratch" in err()
    for args in ((None, q, 2, 2, 2, q + 1024, 4, None), (p, None, 2, 2, 2, q + 1024, 4, None), (p, q, 2, 2, 2, None, 4, None)):
        assert fh(*args) == -1 and b"null" in err(), args
    assert fh(p, q, 2, 3, 4, q + 1024, 14, None) == -1 and b"bins" in err()          # needs 1 + 4 + 9 + 1 = 15
    assert fh(p, q, 2, 3, 4, q + 1024, 0, None) == -1 and b"bins" in err()
    assert not any(buf), "a refused call must not write"


# ------------------------------------------------------------------------------------------ 9. wiring
@contextlib.contextmanager
def count_surface_ops(ops):
    """{op: calls} of the three new Ops methods while the block runs"""
    seen = {}

    def wrap(name):
        real = getattr(ops, name)

        def counting(*a, **k):
            seen[name] = seen.get(name, 0) + 1
            return real(*a, **k)
        return counting

    names = ("surface_border", "edt_sq", "surface_hist")
    for n in names:
        setattr(ops, n, wrap(n))
    try:
        yield seen
    finally:
        for n in names:
            delattr(ops, n)


def check_wiring_percase(ops, dev):
    """surface.calculate_metric_percase and val_2d.calculate_metric_percase(..., surface=True) return the restatement's values with Dice /
    Jaccard identical to the nan-reporting calls; those (test_3d_patch, pancreas.test_util, val_2d's default) still return nan and call
    none of the new ops"""
    from bcp_amd.pancreas import test_util as PT
    from bcp_amd.utils import test_3d_patch as T3
    from bcp_amd.utils import val_2d as V
    _use(ops, dev)
    rng = np.random.default_rng(31)
    shape = (12, 18, 21)
    pred_l, gt_l = _labels(shape, rng), _labels(shape, rng)
    pred, gt = _t((pred_l != 0).astype(np.uint8), dev), _t(gt_l, dev)
    a, b = pred_l != 0, gt_l != 0
    with count_surface_ops(ops) as seen:
        on = S.calculate_metric_percase(pred, gt)
    assert seen == {"surface_border": 2, "edt_sq": 2, "surface_hist": 2}, seen
    assert on[2] == ref_hd95(a, b) and abs(on[3] - ref_asd(a, b)) <= 1e-12 * ref_asd(a, b), on
    for mod in (T3, PT):
        with count_surface_ops(ops) as seen:
            off = mod.calculate_metric_percase(pred, gt)
        assert not seen, (mod.__name__, seen)
        assert len(off) == 4 and math.isnan(off[2]) and math.isnan(off[3])
        assert on[:2] == off[:2], (mod.__name__, on, off)
    pred3, gt3 = _t(pred_l, dev), _t(gt_l, dev)
    for cls in (1, 2, 3):
        with count_surface_ops(ops) as seen:
            off = V.calculate_metric_percase(pred3, gt3, cls)
        assert not seen and math.isnan(off[1])
        on = V.calculate_metric_percase(pred3, gt3, cls, surface=True)
        assert on[0] == off[0] and on[1] == ref_hd95(pred_l == cls, gt_l == cls), (cls, on, off)
    # the reference's guards stay in front: an empty prediction never reaches the metric, an empty label under a prediction raises
    none = torch.zeros(shape, dtype=torch.uint8, device=dev)
    assert V.calculate_metric_percase(none, gt3, 1, surface=True) == (0, 0)
    with _raises_runtime():
        V.calculate_metric_percase(pred3, none, 1, surface=True)
    with _raises_runtime():
        S.calculate_metric_percase(pred, none)
    assert S._all_case(lambda image: none, [(None, gt)], 0)[1] == [(0, 0, 0, 0)]


def _tiny_unet(ops, dev, seed=9):
    """the U-Net of net_checks.check_val_2d"""
    rng = np.random.default_rng(seed)
    P = O.init_params(O.unet_param_shapes(), seed=seed + 50, random_affine=True)
    for k in P:
        if k.endswith("running_mean"):
            P[k] = torch.from_numpy(rng.normal(0.0, 0.2, tuple(P[k].shape)).astype(np.float32))
        elif k.endswith("running_var"):
            P[k] = torch.from_numpy(rng.uniform(0.5, 1.5, tuple(P[k].shape)).astype(np.float32))
    return NC.make_unet(P, dev, ops), rng


def check_wiring_val_2d(ops, dev):
    """val_2d.test_single_volume(..., surface=True): finite hd95 for the classes the net predicts, (0, 0) for the others, Dice equal to
    the default call's; the default call runs none of the new ops and reports nan"""
    from bcp_amd.utils import val_2d as V
    _use(ops, dev)
    net, rng = _tiny_unet(ops, dev)
    shape, patch = (5, 32, 48), (32, 48)
    image = torch.from_numpy(rng.standard_normal((1,) + shape, dtype=np.float32))
    label = torch.from_numpy(_labels(shape, rng)[None])
    with count_surface_ops(ops) as seen:
        off = V.test_single_volume(image, label, net, 4, patch_size=patch, batch=2)
    assert not seen, seen
    with count_surface_ops(ops) as seen:
        on = V.test_single_volume(image, label, net, 4, patch_size=patch, batch=2, surface=True)
    assert len(on) == len(off) == 3
    predicted = 0
    for (d0, h0), (d1, h1) in zip(off, on):
        assert d1 == d0
        if (d0, h0) == (0, 0):                       # the class is not predicted: the reference's guard, no metric call
            assert (d1, h1) == (0, 0)
        else:
            predicted += 1
            assert math.isnan(h0) and math.isfinite(h1) and 0.0 <= h1 <= math.sqrt(sum((s - 1) ** 2 for s in shape)), (h0, h1)
    assert predicted >= 1 and seen == {"surface_border": 2 * predicted, "edt_sq": 2 * predicted, "surface_hist": 2 * predicted}, (predicted, seen)
    assert net.training


def check_wiring_pancreas(ops, dev, golden_dir):
    """surface.pancreas_calculate_metric (through pancreas_all_case) on one small case: four finite averages, Dice / Jaccard those of
    pancreas.test_util.test_all_case, whose surface slots stay nan and which runs none of the new ops"""
    from bcp_amd.pancreas import test_util as PT
    _use(ops, dev)
    g = np.load(os.path.join(golden_dir, "sw_pancreas.npz"))
    P = O.init_params(O.vnet_param_shapes(variant="pancreas"), seed=int(g["seed"]), random_affine=True)
    net = NC.make_vnet(P, dev, ops, variant="pancreas", has_dropout=False)
    patch = tuple(int(v) for v in g["patch"])
    image, label = g["image"][:32, :32, :30], g["label_map"][:32, :32, :30]       # one window position (z padded up to the patch)
    with count_surface_ops(ops) as seen:
        avg0, lst0 = PT.test_all_case(net, [(image, label)], num_classes=2, patch_size=patch, stride_xy=16, stride_z=16)
    assert not seen and math.isnan(avg0[2]) and math.isnan(avg0[3])
    with count_surface_ops(ops) as seen:
        avg1, lst1 = S.pancreas_calculate_metric(net, [(image, label)], num_classes=2, dim=patch, s_xy=16, s_z=16)
    assert seen == {"surface_border": 2, "edt_sq": 2, "surface_hist": 2}, seen
    assert np.isfinite(avg1).all() and len(lst1) == 1, avg1
    assert avg1[0] == avg0[0] > 0 and avg1[1] == avg0[1] and avg1[2] >= 0 and avg1[3] >= 0
    assert net.training


def check_wiring_la(ops, dev, golden_dir):
    """surface.la_all_case on one small case, with and without the largest component: four finite averages, Dice / Jaccard those of
    test_3d_patch.test_all_case, whose surface slots stay nan and which runs none of the new ops"""
    from bcp_amd.utils import test_3d_patch as T3
    _use(ops, dev)
    g = np.load(os.path.join(golden_dir, "sw_la.npz"))
    net = NC.make_vnet(O.eval_params(int(g["seed"])), dev, ops)
    patch = tuple(int(v) for v in g["patch"])
    image, label = g["image"][:, :32, :16], g["label_map"][:, :32, :16]             # one window position (x padded up to the patch)
    for nms in (0, 1):
        kw = dict(patch_size=patch, stride_xy=16, stride_z=8, nms=nms)
        with count_surface_ops(ops) as seen:
            avg0 = T3.test_all_case(net, [(image, label)], 2, **kw)
        assert not seen and math.isnan(avg0[2]) and math.isnan(avg0[3])
        with count_surface_ops(ops) as seen:
            avg1 = S.la_all_case(net, [(image, label)], 2, **kw)
        assert seen == {"surface_border": 2, "edt_sq": 2, "surface_hist": 2}, seen
        assert np.isfinite(avg1).all() and avg1[0] == avg0[0] > 0 and avg1[1] == avg0[1] and avg1[2] >= 0 and avg1[3] >= 0, (nms, avg0, avg1)
    assert net.training


# ------------------------------------------------------------------------------------------ 10. drivers
def check_parser_defaults():
    """--val_surface is off by default in both drivers"""
    from bcp_amd import ACDC_BCP_train as TA
    from bcp_amd.pancreas import train_pancreas as TP
    for parser in (TA.parser, TP.build_parser()):
        assert parser.parse_args([]).val_surface is False
        assert parser.parse_args(["--val_surface"]).val_surface is True
