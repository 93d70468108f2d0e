"""Drop-in for the reference's utils/BCP_utils.py (the callables LA_BCP_train.py imports at :30):
`context_mask`, `mix_loss`, `sup_loss`, `update_ema_variables` -- same names, argument meaning and
results, running on the gfx950 kernels.

* `context_mask` (reference :18-28) draws the SAME three np.random.randint numbers in the same order
  but returns `BoxMask` objects instead of two dense int64 tensors: they behave like the reference's
  masks in every expression the train scripts use (`a * m + b * (1 - m)`, passing to `mix_loss`,
  `.long()`, `.sum()`), while the kernels only ever see six integers.
* `random_mask` (:30-46) and `concate_mask` (:48-56), the other masking strategies, return `RegionMask` objects (a union of boxes)
  in the same way, with the reference's draws.
* `mix_loss` (:58-69) is ONE fused forward pass + ONE backward pass over the logits (csrc/loss.hip).
* `update_ema_variables` (:78-81) is one launch over the flat parameter buffer (bit-exact arithmetic).
"""
from __future__ import annotations

import numpy as np
import torch

from .. import hip_ops as H
from ..hip_ops import Ops


class BoxMask:
    """The reference's (mask | loss_mask): ones with one zero box.  `batch` is None for the [X,Y,Z]
    image mask and N for the [N,X,Y,Z] loss mask.  `complement` marks `1 - mask`."""

    def __init__(self, box, spatial, batch=None, complement=False, device=None):
        self.box = tuple(int(v) for v in box)          # (w, h, z, pw, ph, pz) ; 2-D: (w, h, pw, ph)
        self.spatial = tuple(int(v) for v in spatial)
        self.batch = batch
        self.complement = complement
        self.device = device

    # ---- tensor-like surface used by the train scripts
    @property
    def shape(self):
        return torch.Size(((self.batch,) if self.batch is not None else ()) + self.spatial)

    def box6(self):
        if len(self.spatial) == 3:
            return self.box
        w, h, pw, ph = self.box
        return (0, w, h, 1, pw, ph)

    def long(self):
        return self

    def unsqueeze(self, _dim):
        """`mask.unsqueeze(1)` of ACDC_BCP_train.py:175-176: the kernels see the box, not a channel axis"""
        return self

    def type(self, *_a, **_k):
        return self

    def __rsub__(self, other):
        if other == 1:
            return BoxMask(self.box, self.spatial, self.batch, not self.complement, self.device)
        return NotImplemented

    def __mul__(self, t):
        return _Masked(t, self)

    __rmul__ = __mul__

    def count(self):
        vol = int(np.prod(self.spatial))
        b = int(np.prod(self.box[len(self.spatial):]))
        n = (vol - b) if not self.complement else b
        return n * (self.batch if self.batch is not None else 1)

    def sum(self):
        return torch.tensor(self.count(), dtype=torch.int64)

    def tensor(self, device=None, dtype=torch.int64):
        """materialise the dense mask (compatibility / visualisation only)"""
        m = torch.ones(self.spatial, dtype=dtype, device=device or self.device)
        if len(self.spatial) == 3:
            w, h, z, pw, ph, pz = self.box
            m[w:w + pw, h:h + ph, z:z + pz] = 0
        else:
            w, h, pw, ph = self.box
            m[w:w + pw, h:h + ph] = 0
        if self.complement:
            m = 1 - m
        if self.batch is not None:
            m = m.unsqueeze(0).repeat(self.batch, *([1] * len(self.spatial)))
        return m


class RegionMask:
    """BoxMask's sibling for a UNION of boxes: the reference's random_mask (27 boxes, :30-46; ACDC_BCP_train.py:142-154, 9 boxes) and
    concate_mask / contact_mask (one slab, :48-56; ACDC_BCP_train.py:156-164).  Same tensor-like surface.  What the kernels see depends on
    the box count: exactly one box goes to the box kernels (bcp_mix_box, the loss's arithmetic box test: bit-identical to a BoxMask, nothing
    rasterised); any other count is rasterised ONCE per draw into a uint8 map (bcp_mask_boxes) that the image mix (bcp_mix_mask) and the
    loss (mask_or_null) both read -- the image mask, the loss mask and their complements of one draw share `_shared`, the map cache."""

    def __init__(self, boxes, spatial, batch=None, complement=False, device=None, _shared=None):
        self.spatial = tuple(int(v) for v in spatial)
        nd = len(self.spatial)
        self.boxes = tuple(tuple(int(v) for v in b) for b in boxes)      # 3-D: (w, h, z, pw, ph, pz); 2-D: (w, h, pw, ph)
        if any(len(b) != 2 * nd for b in self.boxes):
            raise ValueError(f"RegionMask: every box of a {nd}-D region is {2 * nd} integers")
        if any(v < 0 for b in self.boxes for v in b[nd:]):
            raise ValueError("RegionMask: negative box size")
        self.batch = batch
        self.complement = complement
        self.device = device
        self._shared = _shared if _shared is not None else {"n": batch or 1, "maps": {}, "count": None}
        if batch is not None:
            self._shared["n"] = max(self._shared["n"], int(batch))

    def _like(self, batch, complement):
        return RegionMask(self.boxes, self.spatial, batch, complement, self.device, self._shared)

    def with_batch(self, batch):
        """the [N, ...] loss mask of this draw (shares the rasterised map)"""
        return self._like(batch, self.complement)

    # ---- tensor-like surface used by the train scripts
    @property
    def shape(self):
        return torch.Size(((self.batch,) if self.batch is not None else ()) + self.spatial)

    def boxes6(self):
        if len(self.spatial) == 3:
            return self.boxes
        return tuple((0, w, h, 1, pw, ph) for w, h, pw, ph in self.boxes)

    def single(self):
        """the region is exactly one box: the box kernels serve it"""
        return len(self.boxes) == 1

    def long(self):
        return self

    def unsqueeze(self, _dim):
        return self

    def type(self, *_a, **_k):
        return self

    def __rsub__(self, other):
        if other == 1:
            return self._like(self.batch, not self.complement)
        return NotImplemented

    def __mul__(self, t):
        return _Masked(t, self)

    __rmul__ = __mul__

    def _union(self):
        """voxels of the union (boxes clamped to the volume, overlaps counted once): coordinate compression, no dense map"""
        if self._shared["count"] is None:
            nd = len(self.spatial)
            lim = [[(min(max(b[ax], 0), self.spatial[ax]), min(max(b[ax] + b[nd + ax], 0), self.spatial[ax])) for ax in range(nd)] for b in self.boxes]
            edges = [np.unique([0, self.spatial[ax]] + [v for l in lim for v in l[ax]]) for ax in range(nd)]
            cells = np.zeros([len(e) - 1 for e in edges], dtype=bool)
            for l in lim:
                if all(lo < hi for lo, hi in l):
                    cells[tuple(slice(int(np.searchsorted(edges[ax], l[ax][0])), int(np.searchsorted(edges[ax], l[ax][1]))) for ax in range(nd))] = True
            size = np.ones((), dtype=np.int64)
            for ax in range(nd):
                size = size[..., None] * np.diff(edges[ax]).astype(np.int64)
            self._shared["count"] = int((size * cells).sum())
        return self._shared["count"]

    def count(self):
        vol = int(np.prod(self.spatial))
        n = (vol - self._union()) if not self.complement else self._union()
        return n * (self.batch if self.batch is not None else 1)

    def sum(self):
        return torch.tensor(self.count(), dtype=torch.int64)

    def tensor(self, device=None, dtype=torch.int64):
        """materialise the dense mask (compatibility / visualisation only)"""
        m = torch.ones(self.spatial, dtype=dtype, device=device or self.device)
        nd = len(self.spatial)
        for b in self.boxes:
            m[tuple(slice(max(b[ax], 0), max(b[ax] + b[nd + ax], 0)) for ax in range(nd))] = 0
        if self.complement:
            m = 1 - m
        if self.batch is not None:
            m = m.unsqueeze(0).repeat(self.batch, *([1] * nd))
        return m

    def u8(self, ops, N=None, device=None):
        """the device map uint8 [N, D, H, W] (2-D: D = 1) of this mask, 1 = image term: ONE bcp_mask_boxes launch per draw -- the first call
        rasterises for the largest batch the draw's masks were made for, later calls (the loss mask after the image mask, any smaller N)
        get views of the same buffer.  device: where the map is needed (the tensors it is used with); default: the mask's own."""
        n = int(N) if N is not None else (self.batch or 1)
        device = torch.device(device if device is not None else (self.device if self.device is not None else "cpu"))
        if device.type == "cuda" and device.index is None:      # "cuda" and "cuda:0" are one device: one map, one launch
            device = torch.device("cuda", torch.cuda.current_device())
        maps, key = self._shared["maps"], (self.complement, device)
        have = maps.get(key)
        if have is None or have.shape[0] < n:
            sp = self.spatial if len(self.spatial) == 3 else (1,) + self.spatial
            have = maps[key] = ops.mask_boxes(self.boxes6(), (max(n, self._shared["n"]),) + sp, device, self.complement)
        return have[:n]

    def _dense(self, device, dtype):
        """tensor() of the un-complemented [spatial] mask, kept per (device, dtype) for the draw: what the dense torch fallback of mix()
        multiplies with (read-only there) -- materialising it is one slice fill per box"""
        d = self._shared.setdefault("dense", {})
        key = (torch.device(device), dtype)
        if key not in d:
            d[key] = self._like(None, False).tensor(device, dtype)
        return d[key]


def _same_region(m1, m2):
    if isinstance(m1, BoxMask) and isinstance(m2, BoxMask):
        return m1.box == m2.box
    if isinstance(m1, RegionMask) and isinstance(m2, RegionMask):
        return m1.boxes == m2.boxes and m1.spatial == m2.spatial
    return False


class _Masked:
    """`t * mask`; adding the complementary term launches the fused copy-paste kernel"""

    def __init__(self, t, mask):
        self.t, self.mask = t, mask

    def __add__(self, other):
        if not isinstance(other, _Masked) or not _same_region(other.mask, self.mask) or other.mask.complement == self.mask.complement:
            return self.dense() + (other.dense() if isinstance(other, _Masked) else other)
        outside, inside = (self, other) if not self.mask.complement else (other, self)
        return mix(outside.t, inside.t, self.mask)

    def dense(self):
        return self.t * self.mask.tensor(self.t.device, self.t.dtype)

    def sum(self, *a, **k):
        """`(CE(output, img_l) * mask).sum()` of ACDC_BCP_train.py:177-178 with a BoxMask: dense fallback (compatibility; the
        fused step never comes through here)"""
        return self.dense().sum(*a, **k)


def mix(a, b, mask, out=None):
    """a*mask + b*(1-mask) (LA_BCP_train.py:248-251): `a` outside the box (or the union of boxes of a RegionMask), `b` inside."""
    if a.dtype != torch.float32 or a.dim() not in (4, 5) or a.shape[1] != 1:
        if isinstance(mask, RegionMask):
            m = mask._dense(a.device, a.dtype)
        else:
            m = mask.tensor(a.device, a.dtype) if not mask.complement else (1 - mask).tensor(a.device, a.dtype)
        return a * m + b * (1 - m)
    ops = Ops.product() if a.is_cuda else _cpu_ops()
    N = a.shape[0]
    sp = tuple(a.shape[2:])
    cl_shape = (N,) + ((1,) + sp if len(sp) == 2 else sp) + (1,)
    ac, bc, oc = a.contiguous().view(cl_shape), b.contiguous().view(cl_shape), None if out is None else out.view(cl_shape)
    if isinstance(mask, RegionMask) and not mask.single():
        m8 = (mask if not mask.complement else 1 - mask).u8(ops, device=a.device)[0]      # one [D,H,W] map for every sample
        o = ops.mix_mask(ac, bc, m8, out=oc)
    else:
        o = ops.mix_box(ac, bc, mask.boxes6()[0] if isinstance(mask, RegionMask) else mask.box6(), out=oc)
    return o.view(a.shape)


_CPU_OPS = None


def _cpu_ops():
    """CPU tensors reach the kernels only through the simulator handle that TESTS install
    (tests/conftest.py: set_test_ops); the product never has one."""
    if _CPU_OPS is None:
        raise RuntimeError("BCP HIP ops were given CPU tensors: the product path has no CPU fallback (move tensors to the GPU)")
    return _CPU_OPS


def set_test_ops(ops):
    global _CPU_OPS
    _CPU_OPS = ops


def _ops_for(t):
    return Ops.product() if t.is_cuda else _cpu_ops()


def context_mask(img, mask_ratio):
    """reference :18-28.  NB the draw bounds are hard-coded to 112/112/80 there; kept."""
    batch_size, channel, img_x, img_y, img_z = img.shape[0], img.shape[1], img.shape[2], img.shape[3], img.shape[4]
    patch_pixel_x, patch_pixel_y, patch_pixel_z = int(img_x * mask_ratio), int(img_y * mask_ratio), int(img_z * mask_ratio)
    w = np.random.randint(0, 112 - patch_pixel_x)
    h = np.random.randint(0, 112 - patch_pixel_y)
    z = np.random.randint(0, 80 - patch_pixel_z)
    box = (w, h, z, patch_pixel_x, patch_pixel_y, patch_pixel_z)
    sp = (img_x, img_y, img_z)
    return BoxMask(box, sp, None, False, img.device), BoxMask(box, sp, batch_size, False, img.device)


def _region_pair(boxes, spatial, batch_size, device):
    """(img_mask, loss_mask) of one draw: two views of one region, sharing its rasterised map"""
    loss_mask = RegionMask(boxes, spatial, batch_size, False, device)
    return loss_mask._like(None, False), loss_mask


def random_mask(img):
    """reference :30-46: 27 zero boxes, one per cell of a 3x3x3 grid; 81 np.random.randint draws (cells in xs, ys, zs order; w, h, z per
    cell).  Patches too small for the grid make randint raise, as in the reference."""
    batch_size, channel, img_x, img_y, img_z = img.shape[0], img.shape[1], img.shape[2], img.shape[3], img.shape[4]
    patch_pixel_x, patch_pixel_y, patch_pixel_z = int(img_x * 2 / 3), int(img_y * 2 / 3), int(img_z * 2 / 3)
    mask_size_x, mask_size_y, mask_size_z = int(patch_pixel_x / 3) + 1, int(patch_pixel_y / 3) + 1, int(patch_pixel_z / 3)
    size_x, size_y, size_z = int(img_x / 3), int(img_y / 3), int(img_z / 3)
    boxes = []
    for xs in range(3):
        for ys in range(3):
            for zs in range(3):
                w = np.random.randint(xs * size_x, (xs + 1) * size_x - mask_size_x - 1)
                h = np.random.randint(ys * size_y, (ys + 1) * size_y - mask_size_y - 1)
                z = np.random.randint(zs * size_z, (zs + 1) * size_z - mask_size_z - 1)
                boxes.append((w, h, z, mask_size_x, mask_size_y, mask_size_z))
    return _region_pair(boxes, (img_x, img_y, img_z), batch_size, img.device)


def concate_mask(img):
    """reference :48-56: one full-width zero slab along z, int(img_z * 8 / 27) thick; one np.random.randint draw"""
    batch_size, channel, img_x, img_y, img_z = img.shape[0], img.shape[1], img.shape[2], img.shape[3], img.shape[4]
    z_length = int(img_z * 8 / 27)
    z = np.random.randint(0, img_z - z_length - 1)
    return _region_pair([(0, 0, z, img_x, img_y, z_length)], (img_x, img_y, img_z), batch_size, img.device)


def _as_cl(out):
    """logical [N,C,X,Y,Z] (or [N,C,H,W]) -> physical [N,D,H,W,C] without a copy when it already is"""
    if out.dim() == 4:
        out = out.unsqueeze(2)
    cl = out.permute(0, 2, 3, 4, 1)
    return cl if cl.is_contiguous() else cl.contiguous()


def _labels_u8(ops, lab, N, sp):
    lab = ops.to_u8(lab)
    return lab.view((N,) + ((1,) + sp if len(sp) == 2 else sp))


class _MixLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits_cl, img_l, patch_l, box6, mask_u8, flavour, w_img, w_patch):
        ops = _ops_for(logits_cl)
        out3, ws = ops.mixloss_fwd(logits_cl, img_l, patch_l, box6, flavour, w_img, w_patch, mask=mask_u8)
        ctx.save_for_backward(logits_cl, img_l, patch_l, ws)
        ctx.meta = (box6, mask_u8, flavour)
        if flavour == H.LOSS_LA:
            return out3[0]
        return out3[0], out3[1]

    @staticmethod
    def backward(ctx, *gs):
        logits_cl, img_l, patch_l, ws = ctx.saved_tensors
        box6, mask_u8, flavour = ctx.meta
        ops = _ops_for(logits_cl)
        if flavour == H.LOSS_LA:
            g = gs[0].reshape(1).to(torch.float32)
            g_dev = torch.cat([g, g]).contiguous()
            d = ops.mixloss_bwd(logits_cl, img_l, patch_l, box6, flavour, ws, 0.5, 0.5, mask=mask_u8, g_dev=g_dev)
        else:
            z = torch.zeros(1, dtype=torch.float32, device=logits_cl.device)
            gd = gs[0].reshape(1).to(torch.float32) if gs[0] is not None else z
            gc = gs[1].reshape(1).to(torch.float32) if gs[1] is not None else z
            d = ops.mixloss_bwd(logits_cl, img_l, patch_l, box6, flavour, ws, 1.0, 1.0, mask=mask_u8, g_dev=torch.cat([gd, gc]).contiguous())
        return d, None, None, None, None, None, None, None


class _MixLossPairFn(torch.autograd.Function):
    """Both mix_loss terms of a BCP step on the two halves of ONE logits tensor (grouped forward): the backward
    kernels write their halves of a single gradient buffer, so autograd never pads / adds slice gradients."""

    @staticmethod
    def forward(ctx, logits_cl, lab1, plab1, lab2, plab2, box6, mask_u8, flavour, w1, w2):
        ops = _ops_for(logits_cl)
        n = logits_cl.shape[0] // 2
        a, b = logits_cl[:n], logits_cl[n:]
        o1, ws1 = ops.mixloss_fwd(a, lab1, plab1, box6, flavour, w1[0], w1[1], mask=mask_u8)
        o2, ws2 = ops.mixloss_fwd(b, lab2, plab2, box6, flavour, w2[0], w2[1], mask=mask_u8)
        ctx.save_for_backward(logits_cl, lab1, plab1, lab2, plab2, ws1, ws2)
        ctx.meta = (box6, mask_u8, flavour)
        if flavour == H.LOSS_LA:
            return o1[0], o2[0]
        return o1[0], o1[1], o2[0], o2[1]

    @staticmethod
    def backward(ctx, *gs):
        logits_cl, lab1, plab1, lab2, plab2, ws1, ws2 = ctx.saved_tensors
        box6, mask_u8, flavour = ctx.meta
        ops = _ops_for(logits_cl)
        n = logits_cl.shape[0] // 2
        d = torch.empty_like(logits_cl)
        z = torch.zeros(1, dtype=torch.float32, device=logits_cl.device)

        def gv(g):
            return g.reshape(1).to(torch.float32) if g is not None else z

        if flavour == H.LOSS_LA:
            pairs = ((gv(gs[0]), gv(gs[0]), 0.5), (gv(gs[1]), gv(gs[1]), 0.5))
        else:
            pairs = ((gv(gs[0]), gv(gs[1]), 1.0), (gv(gs[2]), gv(gs[3]), 1.0))
        for half, (lab, plab, ws, (gd, gc, k)) in enumerate(((lab1, plab1, ws1, pairs[0]), (lab2, plab2, ws2, pairs[1]))):
            sl = slice(0, n) if half == 0 else slice(n, 2 * n)
            ops.mixloss_bwd(logits_cl[sl], lab, plab, box6, flavour, ws, k, k, mask=mask_u8, g_dev=torch.cat([gd, gc]).contiguous(),
                            out=d[sl])
        return (d,) + (None,) * 9


_GRAD_BUFFER = None      # (volatile_io) callable: the LOGITS tensor a loss is differentiating -> the tensor that network's backward plan reads its input
                         # from, or None.  Installed by train_step._backward for the duration of one backward call (removed in a finally).  It is
                         # a plain module global on purpose: autograd runs the backward nodes on ITS OWN thread, a thread-local installed by the
                         # caller is invisible there (the first fix of ADVICE r05 made it one and silently brought the 16 MB copy back).  What
                         # keeps two models apart is the KEY: the provider only answers for the logits tensor its own network handed out
                         # (HipNet.dout_buffer_for compares the storage pointer), not for "any tensor of that shape".


def set_grad_buffer_provider(fn):
    """the step functions hand the loss backward the student's dout_buffer_for (networks/_hipnet.py volatile_io): the logits gradient is then
    written where the backward plan reads it, no copy in between; None switches it off"""
    global _GRAD_BUFFER
    _GRAD_BUFFER = fn


def _grad_buffer(like):
    fn = _GRAD_BUFFER
    d = fn(like) if fn is not None else None
    if d is None or d.shape != like.shape or d.dtype != like.dtype or d.device != like.device:
        d = torch.empty_like(like)
    return d


class _MixLossPairTotalFn(torch.autograd.Function):
    """_MixLossPairFn whose differentiable output is the step's TOTAL loss -- LA / pancreas loss_l + loss_u, ACDC ((unl_dice + l_dice) +
    (unl_ce + l_ce)) / 2, summed by the second call's finalize in the reference's fp32 order (bcp_mixloss_fwd prev / total) -- so that no
    torch elementwise launch sits between the forward and the backward pass (round 4: the step functions' three adds, the division, their
    autograd twins and two torch.cat calls were ~10 dependent 5 us launches per step).  The individual terms come back detached, for
    logging, exactly as _MixLossPairFn computes them.  d total / d term is 1/2 for every (dice, ce) pair of both flavours."""

    @staticmethod
    def forward(ctx, logits_cl, lab1, plab1, lab2, plab2, box6, mask_u8, flavour, w1, w2):
        ops = _ops_for(logits_cl)
        n = logits_cl.shape[0] // 2
        a, b = logits_cl[:n], logits_cl[n:]
        ctx.pair = bool(ops.MIXLOSS_PAIR and logits_cl.shape[0] == 2 * n and logits_cl.is_contiguous())
        if ctx.pair:        # both calls in one launch pair (bcp_mixloss_pair_fwd): bit-identical results, three launches fewer per step
            o6, total, ws1 = ops.mixloss_pair_fwd(logits_cl, lab1, plab1, lab2, plab2, box6, flavour, w1, w2, mask=mask_u8)
            o1, o2, ws2 = o6[0], o6[1], ws1
        else:
            total = torch.empty(1, dtype=torch.float32, device=logits_cl.device)
            o1, ws1 = ops.mixloss_fwd(a, lab1, plab1, box6, flavour, w1[0], w1[1], mask=mask_u8)
            o2, ws2 = ops.mixloss_fwd(b, lab2, plab2, box6, flavour, w2[0], w2[1], mask=mask_u8, prev=o1, total=total)
        ctx.save_for_backward(logits_cl, lab1, plab1, lab2, plab2, ws1, ws2)
        ctx.meta = (box6, mask_u8, flavour)
        terms = (o1[0], o2[0]) if flavour == H.LOSS_LA else (o1[0], o1[1], o2[0], o2[1])
        ctx.mark_non_differentiable(*terms)
        ctx.set_materialize_grads(False)       # (the terms' gradients are never used: materialised as zeros they were one 1-workgroup fill launch
                                               #  each between the forward and the backward pass -- 13 us of the step's critical path at the LA size)
        return (total.reshape(()),) + terms

    @staticmethod
    def backward(ctx, g, *unused):
        logits_cl, lab1, plab1, lab2, plab2, ws1, ws2 = ctx.saved_tensors
        box6, mask_u8, flavour = ctx.meta
        ops = _ops_for(logits_cl)
        n = logits_cl.shape[0] // 2
        if g is None:                          # (set_materialize_grads(False): the total was not part of what is being differentiated)
            return (None,) * 10
        d = _grad_buffer(logits_cl)
        g1 = g.reshape(1)
        if g1.dtype != torch.float32 or not g1.is_contiguous():
            g1 = g1.to(torch.float32).contiguous()
        if ctx.pair:
            ops.mixloss_pair_bwd(logits_cl, lab1, plab1, lab2, plab2, box6, flavour, ws1, 0.5, 0.5, mask=mask_u8, g_dev=g1, out=d)
            return (d,) + (None,) * 9
        for half, (lab, plab, ws) in enumerate(((lab1, plab1, ws1), (lab2, plab2, ws2))):
            sl = slice(0, n) if half == 0 else slice(n, 2 * n)
            ops.mixloss_bwd(logits_cl[sl], lab, plab, box6, flavour, ws, 0.5, 0.5, mask=mask_u8, g_dev=g1, out=d[sl])
        return (d,) + (None,) * 9


def mix_loss_pair(out, first, second, mask, flavour=H.LOSS_LA, total=False):
    """`out` = logits of a grouped forward over [batch1; batch2]; `first` / `second` = (img_l, patch_l, w_img, w_patch)
    for each half.  LA: returns (loss_1, loss_2); ACDC: (dice_1, ce_1, dice_2, ce_2).  total=True: (total, *terms) with `total` the
    step's loss as the reference sums it and the only differentiable output (_MixLossPairTotalFn)."""
    cl = _as_cl(out)
    ops = _ops_for(cl)
    N, sp = cl.shape[0] // 2, tuple(out.shape[2:])
    box6, m8 = _mask_args(mask, ops, N, sp, cl.device)
    l1, p1, w1a, w1b = first
    l2, p2, w2a, w2b = second
    fn = _MixLossPairTotalFn if total else _MixLossPairFn
    return fn.apply(cl, _labels_u8(ops, l1, N, sp), _labels_u8(ops, p1, N, sp), _labels_u8(ops, l2, N, sp),
                    _labels_u8(ops, p2, N, sp), box6, m8, flavour, (float(w1a), float(w1b)), (float(w2a), float(w2b)))


_ONES = {}


def unit_gradient(like):
    """a cached 0-dim float32 one on `like`'s device: `loss.backward(gradient=unit_gradient(loss))` spares the fill launch autograd would
    make for the implicit gradient of a scalar loss"""
    k = (like.device.type, like.device.index)
    o = _ONES.get(k)
    if o is None:
        o = _ONES[k] = torch.ones((), dtype=torch.float32, device=like.device)
    return o


def _mask_args(mask, ops, N, sp, device=None):
    """-> (box6, dense uint8 mask or None); device: the logits' (where a RegionMask's map has to live)"""
    if isinstance(mask, BoxMask):
        if mask.complement:
            raise ValueError("pass the loss mask itself, not its complement")
        return mask.box6(), None
    if isinstance(mask, RegionMask):
        if mask.complement:
            raise ValueError("pass the loss mask itself, not its complement")
        if mask.single():
            return mask.boxes6()[0], None
        return (0, 0, 0, 0, 0, 0), mask.u8(ops, N, device)      # the draw's one rasterised map: no cast launch between forward and backward
    m = ops.to_u8(mask if mask.dim() == len(sp) + 1 else mask.expand((N,) + sp))
    return (0, 0, 0, 0, 0, 0), m.view((N,) + ((1,) + sp if len(sp) == 2 else sp))


def mix_loss(net3_output, img_l, patch_l, mask, l_weight=1.0, u_weight=0.5, unlab=False):
    """reference :58-69 (LA) / pancreas/losses.py:129-141"""
    image_weight, patch_weight = l_weight, u_weight
    if unlab:
        image_weight, patch_weight = u_weight, l_weight
    cl = _as_cl(net3_output)
    ops = _ops_for(cl)
    N, sp = cl.shape[0], tuple(net3_output.shape[2:])
    box6, m8 = _mask_args(mask, ops, N, sp, cl.device)
    return _MixLossFn.apply(cl, _labels_u8(ops, img_l, N, sp), _labels_u8(ops, patch_l, N, sp), box6, m8, H.LOSS_LA,
                            float(image_weight), float(patch_weight))


def sup_loss(output, label):
    """reference :71-76: (unmasked dice + mean CE) / 2 == mix_loss with an empty box and weight 1"""
    cl = _as_cl(output)
    ops = _ops_for(cl)
    N, sp = cl.shape[0], tuple(output.shape[2:])
    lab = _labels_u8(ops, label, N, sp)
    return _MixLossFn.apply(cl, lab, lab, (0, 0, 0, 0, 0, 0), None, H.LOSS_LA, 1.0, 0.0)


@torch.no_grad()
def update_ema_variables(model, ema_model, alpha):
    """reference :78-81: ema = alpha*ema + (1-alpha)*param over .parameters() -- one launch when both
    models keep their parameters in a flat buffer (networks/_hipnet.py), else one launch per tensor."""
    from ..networks._hipnet import HipNet
    if isinstance(model, HipNet) and isinstance(ema_model, HipNet):
        src, dst = model.flat_params(), ema_model.flat_params()
        if src.numel() == dst.numel():
            _ops_for(dst).ema(dst, src, alpha)
            ema_model.bump()
            return
    for ema_param, param in zip(ema_model.parameters(), model.parameters()):
        _ops_for(param).ema(ema_param.data.view(-1), param.data.contiguous().view(-1), alpha)
