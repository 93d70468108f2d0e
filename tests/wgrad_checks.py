"""The 3x3(x3) conv's magnitude domain on the two-plane fp16 path, the weight gradient's zero / NaN / Inf semantics, and every
weight-gradient kernel instance against fp64.  Check bodies taking (ops, dev); tests/test_emu_wgrad.py runs them on the host simulator
(CPU tensors), tests/test_gpu_wgrad.py on the device.

check_f16_range: the two-plane fp16 kernels pre-scale each operand by a power of two taken from the tensor's own |max| and undo both on
the accumulator (csrc/conv3_defs.h, which states the guaranteed domain: |max| from 2^-100 to 2^100 on either operand).  One operand is
scaled by 2^k over that whole domain, or both at once (PAIRS), on every kernel that has a scale site of its own; every output element
is held to the suite's elementwise bound against fp64 and the maximum error to the gate check_conv3_f16 uses.  Scaling by a power of
two is exact, so the fp64 reference and its bound are computed once per case at k = 0 and scaled.

check_wgrad_nonfinite: an all-zero operand gives exactly zero; one NaN / Inf voxel poisons exactly the entries of its channel.

check_wgrad_instances: one small row of tests/golden/wgrad_routes.npz per kernel instance the sweep of
tools/make_golden_wgrad_routes.py reaches, picked by program (instance_rows) so that the list follows the fixture; write and +=, the
workspace exactly as large as the query says inside poisoned bands."""
import ctypes as C
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

import product_ops as PO
from bcp_amd import hip_ops as H
from kernel_checks import R, from_cl, to_cl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden_wgrad_routes as G  # noqa: E402

# ---------------------------------------------------------------------------------------------------------------------------------
# the fp16 planes' magnitude domain

K_FULL = tuple(range(-100, 101, 4))
K_DEFAULT = (-100, -84, -68, -64, -60, -32, 0, 32, 64, 72, 76, 100)      # both old cliffs (below 2^-60, above 2^74) and the domain's ends
# both scales far from zero at once, the exact result still a normal fp32 number: (first operand x 2^a, second x 2^b)
PAIRS = ((-90, 90), (60, -100), (-50, -50), (50, 50))

# kernel reached (tests/kernel_checks.py check_conv3_f16's case table), N, Cin, Cout, spatial, KD, options
FWD_CASES = {
    "c3d": (1, 32, 32, (8, 16, 16), 3, {"conv3_b6": 2}),                                        # k_c3d 4x8x8 x 32
    "c3d16p": (2, 16, 16, (8, 8, 24), 3, {"conv3_b6": 3, "conv3_p": 3}),                        # persistent 16-channel kernel
    "c3p": (1, 64, 64, (8, 8, 8), 3, {"conv3_b6": 2, "conv3_b6_flat": 0}),                      # k_c3p: brick tiles below 16 K voxels
    "c3q": (1, 128, 64, (7, 7, 5), 3, {"conv3_b6": 2}),                                         # k_c3q, the flat deep-level pipeline
    "c3b2d": (2, 96, 64, (1, 20, 40), 1, {"conv3_b6": 2, "conv3_b6_cfg2d": 2, "conv3_b6_flat": 0}),      # 2-D k_c3b, 64-channel slab
}
WGRAD_CASES = {
    "w6slabs": (1, 32, 32, (4, 8, 8), 3, {"wgrad_b6": 2}),
    "w6_2d": (2, 32, 32, (1, 16, 32), 1, {"wgrad_b6": 2}),
    "w6direct": (1, 64, 48, (4, 8, 4), 3, {"wgrad_b6": 2}),
}
F16_CASES = tuple(FWD_CASES) + tuple(WGRAD_CASES)


class options:
    """set the library options of a block, put every one of them back"""

    def __init__(self, ops, opts):
        self.ops, self.opts = ops, opts

    def __enter__(self):
        for k, v in self.opts.items():
            self.ops.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.opts:
            self.ops.set_option(k)


def _with_amax(t, dev):
    t._bcp_amax = H.amax_slots(float(t.abs().max()), dev)
    return t


def _wgrad64(x, dy, wshape):
    fn = torch.nn.grad.conv2d_weight if len(wshape) == 4 else torch.nn.grad.conv3d_weight
    return fn(x.double(), wshape, dy.double(), padding=1)


def f16_range_points(ks, pairs=True):
    """grid points (a, b): the exponents the first and the second operand of a path are scaled by"""
    return [(k, 0) for k in ks] + (list(PAIRS) if pairs else [])


def _scaled(t, k):
    return t * float(2.0 ** k)                       # exact: every element stays a normal fp32 number or 0 (|k| <= 100, unit-sized data)


def f16_range_runs(ops, dev, case, points):
    """one case of check_f16_range: yields (tag, out_f16, out_bf16 or None, out_fp32, ref64, cond64, (|max| of the first operand, of
    the second)) per path and grid point, outputs as CPU tensors in the reference's layout.  out_bf16 -- the same launch without |max| slots, three bf16 planes -- comes at k = 0
    only, as the proof that the launch with the slots takes another instance."""
    rng = np.random.default_rng(1207)
    if case in FWD_CASES:
        N, Cin, Cout, sp, KD, opts = FWD_CASES[case]
        two_d = KD == 1
        xs = sp[1:] if two_d else sp
        conv, conv_in = (F.conv2d, torch.nn.grad.conv2d_input) if two_d else (F.conv3d, torch.nn.grad.conv3d_input)
        x = R(rng, N, Cin, *xs).clamp_(min=-0.5)                        # the magnitudes of check_conv3_f16: O(1) activations,
        w = R(rng, Cout, Cin, *((3,) * (2 if two_d else 3))) * 0.05     # 0.05-sized weights,
        dy = R(rng, N, Cout, *xs) * 1e-6                                # backward-sized gradients
        y64, ycond = conv(x.double(), w.double(), padding=1), conv(x.double().abs(), w.double().abs(), padding=1)
        dx64, dxcond = conv_in(x.shape, w.double(), dy.double(), padding=1), conv_in(x.shape, w.double().abs(), dy.double().abs(), padding=1)
        packs = {}

        def pack(b):
            if b not in packs:
                packs[b] = ops.conv3_pack(_scaled(w, b).to(dev).contiguous(), KD)
            return packs[b]

        def run(t, wp, Co, amax, o):
            tcl = to_cl(t).to(dev)
            if amax:
                _with_amax(tcl, dev)
            with options(ops, dict(o, splitk=1)):
                return from_cl(ops.conv3_fwd(tcl, wp, None, Co, KD), two_d).cpu()

        for (a, b) in points:
            s = float(2.0 ** (a + b))
            # forward: x scaled by 2^a, w by 2^b (a single-operand point scales x on one path and w on the other)
            for path, (ea, eb) in (("fwd, x scaled", (a, b)), ("fwd, w scaled", (b, a))) if b == 0 else (("fwd, x and w scaled", (a, b)),):
                xs_, wf = _scaled(x, ea), pack(eb)[0]
                yield (f"{case} {path} 2^{a} 2^{b}", run(xs_, wf, Cout, True, opts), run(xs_, wf, Cout, False, opts) if a == b == 0 else None,
                       run(xs_, wf, Cout, False, {"conv3_b6": 0}), y64 * s, ycond * s, (float(xs_.abs().max()), float(_scaled(w, eb).abs().max())))
            if b == 0:
                ds, wd = _scaled(dy, a), pack(0)[1]
                yield (f"{case} dgrad, dy scaled 2^{a}", run(ds, wd, Cin, True, opts), run(ds, wd, Cin, False, opts) if a == 0 else None,
                       run(ds, wd, Cin, False, {"conv3_b6": 0}), dx64 * s, dxcond * s, (float(ds.abs().max()), float(w.abs().max())))
        return
    N, Cin, Cout, sp, KD, opts = WGRAD_CASES[case]
    two_d = KD == 1
    xs = sp[1:] if two_d else sp
    wshape = (Cout, Cin) + (3,) * (2 if two_d else 3)
    x = R(rng, N, Cin, *xs).clamp_(min=-0.5)
    dy = R(rng, N, Cout, *xs) * 1e-6
    g64, gcond = _wgrad64(x, dy, wshape), _wgrad64(x.abs(), dy.abs(), wshape)

    def run(xx, dd, amax, o):
        xcl, dcl = to_cl(xx).to(dev), to_cl(dd).to(dev)
        if amax:
            _with_amax(xcl, dev), _with_amax(dcl, dev)
        with options(ops, o):
            return ops.conv3_wgrad(xcl, dcl, torch.full(wshape, 3.0, device=dev), KD).cpu()

    for (a, b) in points:
        s = float(2.0 ** (a + b))
        for path, (ea, eb) in (("wgrad, x scaled", (a, b)), ("wgrad, dy scaled", (b, a))) if b == 0 else (("wgrad, x and dy scaled", (a, b)),):
            xx, dd = _scaled(x, ea), _scaled(dy, eb)
            yield (f"{case} {path} 2^{a} 2^{b}", run(xx, dd, True, opts), run(xx, dd, False, opts) if a == b == 0 else None,
                   run(xx, dd, False, {"wgrad_b6": 0}), g64 * s, gcond * s, (float(xx.abs().max()), float(dd.abs().max())))


def check_f16_range(ops, dev, case, ks=K_FULL, pairs=True, report=None):
    """at every grid point: no NaN / Inf from finite inputs; |out - ref64| <= TAU x cond element by element (cond: the same operation on
    the operands' magnitudes in fp64); max error <= 3 x the fp32-MFMA kernel's on the same data + 1e-7 x max |ref64| (check_conv3_f16's
    gate).  The launch with |max| slots must be the fp16 instance: its bits differ from the three-plane result of the same launch
    without them.  All grid points run before the first failure is raised, so that a failing library shows its whole failing grid."""
    failures, proofs = [], 0
    for tag, o16, o3, o32, ref, cond, _ in f16_range_runs(ops, dev, case, f16_range_points(ks, pairs)):
        if o3 is not None:
            proofs += 1
            assert not torch.equal(o16, o3), tag + ": the launch with the |max| slots must take the fp16 instance"
        scale = float(ref.abs().max())
        assert 2.0 ** -126 < scale < 2.0 ** 127, tag       # the grid keeps the exact result a normal fp32 number
        e16, e32 = float((o16.double() - ref).abs().max()), float((o32.double() - ref).abs().max())
        ratio = PO.elementwise_ratio(o16.double(), ref, cond)[0] / PO.TAU
        if report is not None:
            report.append(f"{tag}: ratio/TAU {ratio:.3g}  max err/scale f16 {e16 / scale:.2e} fp32 {e32 / scale:.2e}")
        try:
            assert bool(torch.isfinite(o16).all()), f"{tag}: {int((~torch.isfinite(o16)).sum())} non-finite outputs from finite inputs"
            PO.check_elementwise(o16, ref, cond, PO.TAU, tag)
            assert e16 <= 3.0 * e32 + 1e-7 * scale, f"{tag}: error vs fp64 {e16:.3e} (fp32-MFMA kernel {e32:.3e}, scale {scale:.3e})"
        except AssertionError as e:
            failures.append(str(e))
    assert proofs > 0 or 0 not in ks
    assert not failures, f"{len(failures)} failing grid points:\n" + "\n".join(failures)


# ---------------------------------------------------------------------------------------------------------------------------------
# zero / NaN / Inf operands of the weight gradient


def check_wgrad_nonfinite(ops, dev):
    """1 x (4, 8, 8), 32 -> 32, on the two-plane fp16 kernel (wgrad_b6 = 2, both |max| slots) and on the fp32-MFMA kernel (wgrad_b6 = 0):
    an all-zero operand (|max| slot 0) gives dw == 0 exactly; a NaN voxel of x at channel c (|max| slot NaN) makes the 27 x Cout entries
    dw[:, c] NaN and leaves every other entry as in the clean run, bit for bit; an Inf voxel of dy at channel c does the same to
    dw[c, :]; Inf in x and NaN in dy alike.  (Every tap reaches the poisoned voxel -- it lies in the interior -- so all 27 entries of
    a (c, co) pair see it.)  The clean run is the same launch less the poisoned voxel, |max| slots included: a NaN / Inf slot means
    scale 1 for that operand's fp16 planes, so its planes -- and the low bits of every entry -- are not those of a launch whose slot
    holds the true maximum."""
    rng = np.random.default_rng(77)
    N, Cin, Cout, sp = 1, 32, 32, (4, 8, 8)
    wshape = (Cout, Cin, 3, 3, 3)
    x, dy = R(rng, N, Cin, *sp).clamp_(min=-0.5), R(rng, N, Cout, *sp) * 1e-6

    def run(xx, dd, f16, xmax=None, dmax=None):
        xcl, dcl = to_cl(xx).to(dev), to_cl(dd).to(dev)
        if f16:
            xcl._bcp_amax = H.amax_slots(float(xx.abs().max()) if xmax is None else xmax, dev)
            dcl._bcp_amax = H.amax_slots(float(dd.abs().max()) if dmax is None else dmax, dev)
        with options(ops, {"wgrad_b6": 2 if f16 else 0}):
            return ops.conv3_wgrad(xcl, dcl, torch.full(wshape, 3.0, device=dev), 3).cpu()

    clean16, clean32 = run(x, dy, True), run(x, dy, False)
    with options(ops, {"wgrad_b6": 2}):
        xcl, dcl = to_cl(x).to(dev), to_cl(dy).to(dev)
        three = ops.conv3_wgrad(xcl, dcl, torch.full(wshape, 3.0, device=dev), 3).cpu()
    assert not torch.equal(clean16, three), "the launch with both |max| slots must take the fp16 instance"
    for f16, clean in ((True, clean16), (False, clean32)):
        tag = "fp16 planes" if f16 else "fp32-MFMA"
        assert bool(torch.isfinite(clean).all()) and bool((clean != 3.0).all()), tag
        for which in ("x", "dy"):
            z = run(torch.zeros_like(x) if which == "x" else x, torch.zeros_like(dy) if which == "dy" else dy, f16)
            assert bool((z == 0).all()), f"{tag}: all-zero {which} must give dw == 0 exactly ({int((z != 0).sum())} entries are not)"
        c = 5
        for bad, name in ((float("nan"), "NaN"), (float("inf"), "Inf")):
            xn = x.clone()
            xn[0, c, 2, 3, 4] = bad
            g, clean = run(xn, dy, f16, xmax=bad), run(x, dy, f16, xmax=bad)
            hit = torch.zeros(wshape, dtype=torch.bool)
            hit[:, c] = True
            # Inf x dy is +-Inf where dy != 0, and the sum over the other voxels leaves it; NaN stays NaN
            poisoned = torch.isnan(g) if bad != bad else ~torch.isfinite(g)
            assert torch.equal(poisoned, hit), f"{tag}: {name} in x channel {c}: {int(poisoned.sum())} entries poisoned, {int((poisoned != hit).sum())} off the {27 * Cout} of dw[:, {c}]"
            assert torch.equal(g[~hit].view(torch.int32), clean[~hit].view(torch.int32)), f"{tag}: {name} in x changed entries of other channels"
            dn = dy.clone()
            dn[0, c, 1, 4, 3] = bad
            g, clean = run(x, dn, f16, dmax=bad), run(x, dy, f16, dmax=bad)
            hit = torch.zeros(wshape, dtype=torch.bool)
            hit[c] = True
            poisoned = torch.isnan(g) if bad != bad else ~torch.isfinite(g)
            assert torch.equal(poisoned, hit), f"{tag}: {name} in dy channel {c}: {int(poisoned.sum())} entries poisoned, {int((poisoned != hit).sum())} off the {27 * Cin} of dw[{c}]"
            assert torch.equal(g[~hit].view(torch.int32), clean[~hit].view(torch.int32)), f"{tag}: {name} in dy changed entries of other channels"


# ---------------------------------------------------------------------------------------------------------------------------------
# every reachable weight-gradient kernel instance against fp64

CAP_VOX3, CAP_PIX2 = 40 * 40 * 36, 100 * 100         # the route grid's largest awkward extents: no level-size launch is run
SIM_EXTENDED_VOX = 8 * 1024                          # simulator twin: rows above this many voxels are `extended`
COL = {c: i for i, c in enumerate(G.COLUMNS)}


def _tile_of(symbol):
    """(TD, TH, TW) of a tiled kernel symbol, None for the reduce kernels"""
    if symbol.startswith("bcp::k_wgrad_reduce"):
        return None
    a = symbol[symbol.index("<") + 1:symbol.rindex(">")].split(", ")
    return int(a[1]), int(a[2]), int(a[3])


def instance_rows(golden=G.GOLDEN):
    """-> [(id, row dict, option dict, symbols the row is there for, the row's launch log)]: for each kernel symbol the sweep launches,
    the served row under the cap that reaches it with the most tiled dimensions holding several tiles AND a partial one (a 3 x 3 x 3
    volume is partial everywhere and walks no tile), the cheapest among those (cost: voxels x padded channels); a row that serves
    several symbols is listed once.  (Every row of the grid under the cap has N >= 2: the sweep's
    batches are 2 for volumes and 12 for slices, so no second row is needed for the batch stride.)"""
    rows, logs, names = G.unpack(np.load(golden))
    syms = [[ln.split("|")[1] for ln in t.splitlines()] for t in logs]
    best = {}
    for i, r in enumerate(rows):
        d = {c: int(r[COL[c]]) for c in G.COLUMNS}
        if d["rc"] != 0 or d["D"] * d["H"] * d["W"] > (CAP_VOX3 if d["KD"] == 3 else CAP_PIX2):
            continue
        cost = d["N"] * d["D"] * d["H"] * d["W"] * (-(-d["Cin"] // 16)) * (-(-d["Cout"] // 16))
        for s in syms[d["log"]]:
            t = _tile_of(s)
            ragged = 0 if t is None else sum(e > te and e % te != 0 for e, te in zip((d["D"], d["H"], d["W"]), t) if te > 1)
            key = (-ragged, cost, i)
            if s not in best or key < best[s][0]:
                best[s] = (key, i)
    launched = {s for ss in syms for s in ss}
    assert set(best) == launched, f"kernel instances the sweep reaches only above the cap: {sorted(launched - set(best))}"
    out = {}
    for s, (_, i) in sorted(best.items()):
        out.setdefault(i, []).append(s)
    res = []
    for i, ss in sorted(out.items()):
        d = {c: int(rows[i][COL[c]]) for c in G.COLUMNS}
        ident = f"{names[d['option']]}-{d['N']}x{d['D']}x{d['H']}x{d['W']}-{d['Cin']}to{d['Cout']}-amax{d['amax']}"
        res.append((ident, d, G.parse_options(names[d["option"]]), ss, logs[d["log"]]))
    return res


INSTANCE_ROWS = instance_rows()


def row_voxels(d):
    return d["N"] * d["D"] * d["H"] * d["W"]


class _Log:
    """the simulator's launch log around a call (mode 1: note and execute); on the device there is none"""

    def __init__(self, ops):
        self.cdll = ops.b.cdll if hasattr(ops.b.cdll, "bcpemu_log_mode") else None
        if self.cdll is not None:
            self.cdll.bcpemu_log_mode.restype, self.cdll.bcpemu_log_mode.argtypes = C.c_int, [C.c_int]
            self.cdll.bcpemu_log_take.restype, self.cdll.bcpemu_log_take.argtypes = C.c_long, [C.c_char_p, C.c_long]

    def __enter__(self):
        if self.cdll is not None:
            self.prev = self.cdll.bcpemu_log_mode(1)
            self.take()
        return self

    def take(self):
        buf = C.create_string_buffer(1 << 16)
        assert self.cdll.bcpemu_log_take(buf, len(buf)) <= len(buf)
        return "".join(ln + "\n" for ln in buf.value.decode().splitlines() if ln.startswith("L|"))

    def __exit__(self, *exc):
        if self.cdll is not None:
            self.cdll.bcpemu_log_mode(self.prev)
            self.take()


POISON, BAND = 0xA5, 64 << 10


def check_wgrad_instance(ops, dev, d, opts, symbols, log, report=None):
    """one row: under the row's options, dw (prefilled with 3.0) = wgrad(x, dy), then += the same, each against fp64 conv{2,3}d_weight
    element by element (TAU x cond, cond = the weight gradient of (|x|, |dy|); twice that after the +=).  x is ReLU-like, dy
    backward-sized.  The workspace is exactly bcp_conv3_wgrad_workspace_bytes long, between two bands of 0xA5 bytes that must come back
    untouched.  On the simulator the launch log must be the row's recorded one (so the named instances are what ran); on the device the
    three queries must give the row's recorded answers."""
    N, D, Hh, W, KD, Cin, Cout = (d[c] for c in ("N", "D", "H", "W", "KD", "Cin", "Cout"))
    two_d = KD == 1
    g = torch.Generator().manual_seed(1000 * Cin + Cout + D * Hh * W)
    sp = (Hh, W) if two_d else (D, Hh, W)
    x, dy = PO.activation(g, (N, Cin) + sp), PO.gradient(g, (N, Cout) + sp)
    wshape = (Cout, Cin) + (3,) * len(sp)
    g64, cond = _wgrad64(x, dy, wshape), _wgrad64(x.abs(), dy.abs(), wshape)
    xcl, dcl = to_cl(x).to(dev), to_cl(dy).to(dev)
    xa = H.amax_slots(float(x.abs().max()), dev) if d["amax"] else None
    da = H.amax_slots(float(dy.abs().max()), dev) if d["amax"] else None
    dims = (N, D, Hh, W, Cin, Cout, KD)
    p = lambda t: None if t is None else t.data_ptr()
    with options(ops, opts):
        nbytes = int(ops.b.call("bcp_conv3_wgrad_workspace_bytes", *dims))
        assert (nbytes, int(ops.b.call("bcp_conv3_wgrad_path", *dims)), int(ops.b.call("bcp_conv3_planes", *dims, 1))) == \
            (d["workspace_bytes"], d["path"], d["planes"]), "the queries no longer give the fixture's answers"
        assert nbytes > 0 and nbytes % 16 == 0
        buf = torch.full((BAND + nbytes + BAND,), POISON, dtype=torch.uint8, device=dev)
        off = BAND + (-(buf.data_ptr() + BAND)) % 256
        ws = buf[off:off + nbytes]
        dw = torch.full(wshape, 3.0, device=dev)
        worst = 0.0
        with _Log(ops) as lg:
            for acc in (0, 1):
                if Cin == 1:
                    ops.b.call("bcp_conv3_c1_wgrad", p(xcl), p(dcl), p(dw), N, D, Hh, W, KD, acc, p(ws), ops.stream(xcl))
                else:
                    ops.b.call("bcp_conv3_wgrad", p(xcl), p(dcl), p(dw), *dims, acc, p(ws), p(xa), p(da), ops.stream(xcl))
                if lg.cdll is not None:
                    got = lg.take()
                    assert got == log and all(("L|" + s + "|") in got for s in symbols), f"launched\n{got}the fixture's row holds\n{log}"
                r, _ = PO.check_elementwise(dw, g64 * (1 + acc), cond * (1 + acc), PO.TAU, f"wgrad {symbols} {opts} {dims} amax={d['amax']} accumulate={acc}")
                worst = max(worst, r)
        out = buf.cpu()
        assert bool((out[:off] == POISON).all()) and bool((out[off + nbytes:] == POISON).all()), \
            f"wgrad {symbols} {opts} {dims}: bytes outside the {nbytes}-byte workspace were written"
    if report is not None:
        report.append(f"{symbols} {opts} {dims} amax={d['amax']}: worst ratio/TAU {worst:.3g}")
    return worst


def check_wgrad_instances(ops, dev, report=None):
    """every row of INSTANCE_ROWS (the twins run them one test each)"""
    for _, d, opts, symbols, log in INSTANCE_ROWS:
        check_wgrad_instance(ops, dev, d, opts, symbols, log, report=report)
