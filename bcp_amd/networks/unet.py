"""2-D U-Net on the MI355X kernels -- drop-in for the reference's networks/unet.py:UNet_2d (ACDC).

Same constructor, same 226 state_dict keys / parameter order, `net(x) -> logits [N,4,H,W]`.  Layout is NHWC
fp32 ([N,1,H,W,C] physically: the 3-D kernels run with D = 1, KD = 1).

Topology (networks/unet.py:15-57, 80-86, 104-116): ConvBlock = conv3x3 -> BN -> LeakyReLU(0.01) -> Dropout(p) ->
conv3x3 -> BN -> LeakyReLU; encoder in_conv(1->16, p=.05), down1..4 = MaxPool2d(2) + ConvBlock (32,64,128,256;
p = .1,.2,.3,.5); decoder up1..4 = conv1x1 (halve C) -> bilinear x2 (align_corners=True) -> cat([skip, up]) ->
ConvBlock(p=0); out_conv 3x3 16->4.

The schedule is planned, then executed, as the V-Net's (networks/VNet.py; the route records live in networks/_hipnet.py).  `plan_forward` /
`plan_backward` decide every conv's route -- which Ops method produces the pre-norm tensor, which normalises, what the dgrad behind it
leaves, and which encoder levels write their output straight into the decoder's concat buffer -- from shapes, mode and switches alone
(host-side shape queries of the library: no tensor, no launch); every exclusion rule stands there, once.  `_forward_impl` / `_backward_impl`
walk those records and call the named op between the fixed launches (pool, 1x1 conv, bilinear upsample, concat copy); what the forward
hands to the backward is a `_Saved`.  Tests read the same records (tests/unet_plan_checks.py, test_plan_product.py).
"""
from __future__ import annotations

import functools

import torch

from .. import hip_ops as H
from ._hipnet import (BNP, ConvP, HipNet, Holder, NetFn, Seq, _BwdRoute, _Plan, _Route, _SavedLayer, _norm_params, contrastive_heads,
                      plan_conv3_dgrad, plan_conv3_fwd)

FT = [16, 32, 64, 128, 256]
DROP = [0.05, 0.1, 0.2, 0.3, 0.5]
TAGS = [f"e{i}" for i in range(5)] + [f"u{i}" for i in range(1, 5)]      # the nine ConvBlocks in launch order


class _Saved:
    """what a saving forward hands to its backward -- one object per pass (launch plans key the backward on its identity): a _SavedLayer per
    conv in launch order (out_conv's last: x is the head's input), the five encoder outputs, the four 1x1 convs' inputs"""
    __slots__ = ("plan", "layers", "xs", "pw_in")

    def __init__(self, plan):
        self.plan, self.layers, self.xs, self.pw_in = plan, [], None, []

    def __getitem__(self, key):
        """read-only view in the dict layout this structure replaced: "e0".."u4" -> (h, y1, st1, em, a1, y2, st2, G), "xs", "out" -> (h,),
        "pw1".."pw4" -> (h,) (tests/net_checks.py reads the activation patterns through it)"""
        if key == "xs":
            return self.xs
        if key == "out":
            return (self.layers[-1].x,)
        if key.startswith("pw"):
            return (self.pw_in[int(key[2:]) - 1],)
        s1, s2 = self.layers[2 * TAGS.index(key):][:2]
        return (s1.x, s1.y, s1.stats, s1.cs, s2.x, s2.y, s2.stats, self.plan.G)


class _CB:
    """one ConvBlock: two (conv, bn) pairs + its dropout probability and mask key"""

    def __init__(self, cin, cout, p, dkey):
        self.cin, self.cout, self.p, self.dkey = cin, cout, p, dkey
        self.c1, self.b1 = ConvP((cout, cin, 3, 3), cin * 9, cout), BNP(cout)
        self.c2, self.b2 = ConvP((cout, cout, 3, 3), cout * 9, cout), BNP(cout)
        self.b1._live = self.b2._live = True

    def module(self):
        h = Holder()
        h.conv_conv = Seq([(0, self.c1), (1, self.b1), (4, self.c2), (5, self.b2)])
        return h


class UNet_2d(HipNet):
    fuse_c1 = True       # first layer: conv + norm + LeakyReLU (+ dropout) with recompute (networks/VNet.py)
    skip_in_concat = True   # encoder outputs are written into the decoder's concat buffers (no torch.cat copy; pool backward joins the skip gradient)
    inline_dropout = True   # nn.Dropout keep bits evaluated inside the norm kernels from a device seed (hip_ops.SeedMask): no mask tensors
    def __init__(self, in_chns, class_num):
        super().__init__()
        assert in_chns == 1, "the ACDC hot path is single-channel"
        self.n_classes = class_num
        enc, dec = Holder(), Holder()
        self._enc = [_CB(in_chns, FT[0], DROP[0], "d0")] + [_CB(FT[i - 1], FT[i], DROP[i], f"d{i}") for i in range(1, 5)]
        enc.in_conv = self._enc[0].module()
        for i in range(1, 5):
            d = Holder()
            d.maxpool_conv = Seq([(1, self._enc[i].module())])
            setattr(enc, f"down{i}", d)
        self._up = []
        for i in range(1, 5):
            c1, c2 = FT[5 - i], FT[4 - i]
            u = Holder()
            pw = ConvP((c2, c1, 1, 1), c1, c2)
            cb = _CB(2 * c2, c2, 0.0, None)
            u.conv1x1 = pw
            u.conv = cb.module()
            setattr(dec, f"up{i}", u)
            self._up.append((pw, cb, c1, c2))
        dec.out_conv = ConvP((class_num, FT[0], 3, 3), FT[0] * 9, class_num)
        self.encoder, self.decoder = enc, dec
        contrastive_heads(self, 4)
        object.__setattr__(self, "_out", dec.out_conv)
        ids = set()
        for cb in self._enc + [u[1] for u in self._up]:
            for m in (cb.c1, cb.b1, cb.c2, cb.b2):
                ids.add(id(m.weight)); ids.add(id(m.bias))
        for pw, _, _, _ in self._up:
            ids.add(id(pw.weight)); ids.add(id(pw.bias))
        ids.add(id(self._out.weight)); ids.add(id(self._out.bias))
        self._opt_param_ids = ids
        self._blocks = list(zip(TAGS, self._enc + [u[1] for u in self._up]))
        for tag, cb in self._blocks:
            if cb.cin != 1:
                self.register_conv3((tag, 1), cb.c1.weight, 1)
            self.register_conv3((tag, 2), cb.c2.weight, 1)
        self.register_conv3(("out", 0), self._out.weight, 1)
        for i, (pw, _, c1, c2) in enumerate(self._up, start=1):
            self.register_k2(("pw", i), pw.weight, c1, c2, H.PACK_PW_FWD, H.PACK_PW_DGRAD)
        self._prenorm_bias_ids = set(id(m.bias) for cb in self._enc + [u[1] for u in self._up] for m in (cb.c1, cb.c2))

    # ------------------------------------------------------------------ public call
    def forward(self, x, groups=1):
        """groups: see networks/VNet.py:forward -- `groups` sub-batches normalised separately, launched together"""
        N = x.shape[0]
        assert N % groups == 0
        self._groups = int(groups)
        assert x.dim() == 4 and x.shape[1] == 1, "expected [N,1,H,W]"
        self._ensure_flat()
        self.refresh_weights_version()
        xcl = x.contiguous().view(N, 1, x.shape[2], x.shape[3], 1)
        anchor = self._enc[0].c1.weight
        if self.training and torch.is_grad_enabled() and anchor.requires_grad:
            out = NetFn.apply(xcl, anchor, self)
        else:
            out, _ = self._run_forward(xcl, False)
        return out.permute(0, 4, 1, 2, 3).squeeze(2)   # logical [N,4,H,W]

    # ------------------------------------------------------------------ schedule: the planner (no tensor, no launch)
    def plan_forward(self, N, Hh, Ww, groups, training, keep_saved=False):
        """every conv's forward route for an input of extents (N, Hh, Ww) -> _Plan: the 18 block convs, then out_conv, in launch order, and
        per encoder level whether the block's output lands in the decoder's concat buffer.  Decided from the shapes, the mode (`training`;
        `keep_saved`: a test wants every pre-norm tensor) and the class switches alone -- the library's host-side shape queries and nothing
        else, so it runs without a GPU.  Every exclusion rule stands here, once."""
        ops, G = self.ops, groups
        routes, direct = [], []
        for bi, (tag, cb) in enumerate(self._blocks):
            lvl = bi if bi < 5 else 8 - bi                 # e0..e4 walk down, u1..u4 back up: extents = input >> level
            sp = (N, 1, Hh >> lvl, Ww >> lvl)
            for ci, cin in enumerate((cb.cin, cb.cout)):
                r = _Route()
                r.xshape, r.yshape, r.act = sp + (cin,), sp + (cb.cout,), H.ACT_LRELU
                r.dropout = r.elem_mask = training and ci == 0 and cb.p > 0      # nn.Dropout(p) behind the block's first activation
                if cin > 1:        # model.eval(): running statistics, the plain conv (val_2d / test scripts)
                    plan_conv3_fwd(ops, r, 1, G, slabs=training, stats=training)
                elif training and self.fuse_c1 and not keep_saved and ops.conv3_c1_norm_ok(r.xshape, 1, G):
                    # conv + norm + LeakyReLU + dropout with recompute (bcp_conv3_c1_norm_fwd): the pre-norm tensor is never written.  (This
                    # fusion carries the block's dropout mask; the V-Net's recompute rule excludes its Dropout3d sites)
                    r.producer = "conv3_c1_norm_fwd"
                elif training:
                    r.producer, r.rows = "conv3_c1_fwd_stats", ops.conv3_c1_stat_rows(r.xshape, 1, G)
                else:
                    r.producer = "conv3_c1_fwd"
                r.norm = (r.producer if r.producer == "conv3_c1_norm_fwd" else "norm_fwd_slabs" if r.nslabs > 1 else
                          "norm_fwd" if training else "norm_eval")
                routes.append(r)
            if bi < 4:
                # torch.cat([skip, up]) without the copy (round 4): the encoder block's last norm writes straight into the leading channels of
                # the concat buffer its decoder block reads (bcp_norm_fwd out_ld), the pool reads it from there (bcp_maxpool2d_fwd ldx) -- the
                # skip tensor exists once.  The raw-slab norm has no such output: that level, like every level in eval mode, copies
                r.out_slab = training and self.skip_in_concat and r.nslabs == 1
                direct.append(r.out_slab)
        r = _Route()
        r.xshape, r.yshape, r.act = (N, 1, Hh, Ww, FT[0]), (N, 1, Hh, Ww, self.n_classes), H.ACT_NONE
        r.producer, r.norm = "conv3_fwd", None
        return _Plan(G, None, routes + [r], G if training else 0, tuple(direct))

    def plan_call(self, N, Hh, Ww):
        """plan_forward in the mode this network is in: what its next (or last) call with such an input takes"""
        return self.plan_forward(N, Hh, Ww, getattr(self, "_groups", 1), self.training, getattr(self, "_keep_saved", False))

    def plan_backward(self, plan):
        """the backward routes behind a saving forward's plan -> (None: no head of its own, [_BwdRoute per conv]); launch-free like plan_forward"""
        ops, out = self.ops, []
        for bi, (tag, cb) in enumerate(self._blocks):
            r1, r2, b1, b2 = plan.layers[2 * bi], plan.layers[2 * bi + 1], _BwdRoute(), _BwdRoute()
            b2.norm = "norm_bwd"
            plan_conv3_dgrad(ops, b2, r2, r1, 1, plan.G)
            if not r1.keeps_y:       # the fused first layer: y is recomputed from the block's input; with C1_BWD_FUSED its weight gradient in the same pass, no dy
                b1.norm = "conv3_c1_norm_bwd_wgrad" if ops.C1_BWD_FUSED else "conv3_c1_norm_bwd"
            else:
                b1.norm, b1.partial = "norm_bwd_slabs" if b2.nslabs > 1 else "norm_bwd", b2.rows > 0
            b1.dgrad = None if cb.cin == 1 else "conv3_fwd"       # (cin == 1: the network's input, the one block nothing in front of asks for dx)
            out += [b1, b2]
        b = _BwdRoute()
        b.norm, b.dgrad = None, "conv3_fwd"
        return None, out + [b]

    # ------------------------------------------------------------------ schedule: the executors (dispatch on the records)
    def _elem_mask(self, cb, shape, like):
        """the block's nn.Dropout keep mask: injected (parity runs: a uint8 tensor), or drawn -- as a SeedMask the norm kernels evaluate in
        place (inline_dropout, round 4: no mask tensor, no launch), else as a uint8 tensor from bcp_bernoulli with the SAME bits"""
        dev = like.device
        if self.drop_masks is not None:
            m = self.drop_masks[cb.dkey]                       # logical [N,C,H,W] keep mask
            return m.to(dev).permute(0, 2, 3, 1).unsqueeze(1).contiguous().to(torch.uint8)
        if self.inline_dropout:
            return self.ops.seed_mask(shape, 1.0 - cb.p, self.next_seed(), like)
        m = torch.empty(shape, dtype=torch.uint8, device=dev)
        return self.ops.bernoulli(m, 1.0 - cb.p, 1.0, self.next_seed())

    def _block_fwd(self, bi, routes, h, G, saved, out):
        """one ConvBlock on its two routes.  out: the concat slab the second norm writes into (route.out_slab)"""
        ops, (tag, cb), save = self.ops, self._blocks[bi], saved is not None
        for ci, conv, bn, r in ((1, cb.c1, cb.b1, routes[0]), (2, cb.c2, cb.b2, routes[1])):
            w, b = conv.weight.data, conv.bias.data
            # (the seed of a drawn mask: one per dropout block, in front of the block's first launch)
            kw = dict(elem_mask=self._elem_mask(cb, r.yshape, h), elem_scale=1.0 / (1.0 - cb.p)) if r.dropout else dict(elem_mask=None, elem_scale=1.0)
            if r.xshape[-1] > 1:
                wf, _ = self.conv3_packed((tag, ci), save)
            y, part, nb, stats = None, None, 0, None
            p, n = r.producer, r.norm           # (the recomputing producer, conv3_c1_norm_fwd, IS the norm op below: nothing here)
            if p == "conv3_c1_fwd_stats":
                y, part, nb = ops.conv3_c1_fwd_stats(h, w, b, 1, G)
            elif p == "conv3_c1_fwd":
                y = ops.conv3_c1_fwd(h, w, b, 1)
            elif p == "conv3_fwd_raw":
                src = ops.conv3_fwd_raw(h, wf, cb.cout, 1, r.nslabs)
            elif p == "conv3_fwd_stats":
                y, part, nb = ops.conv3_fwd_stats(h, wf, b, cb.cout, 1, G)
            elif p == "conv3_fwd":
                y = ops.conv3_fwd(h, wf, b, cb.cout, 1)
            if n == "conv3_c1_norm_fwd":
                a, stats = ops.conv3_c1_norm_fwd(h, w, b, 1, G, *_norm_params(bn), r.act, **kw)
            elif n == "norm_fwd_slabs":
                a, stats, y = ops.norm_fwd_slabs(src, r.nslabs, b, G, *_norm_params(bn), r.act, **kw)
            elif n == "norm_eval":
                a = ops.norm_eval(y, *_norm_params(bn), r.act)
            else:
                a, stats = ops.norm_fwd(y, G, *_norm_params(bn), r.act, partial=part, nb=nb, out=out if r.out_slab else None, **kw)
            if save:
                saved.layers.append(_SavedLayer(h, y, stats, kw["elem_mask"], None, r))
            h = a
        return h

    def _forward_impl(self, xcl, save):
        ops = self.ops
        N, _, Hh, Ww, _ = xcl.shape
        plan = self.plan_call(N, Hh, Ww)
        saved = _Saved(plan) if save else None
        # the concat buffers of the levels whose skip is written in place (plan.direct); level j: extents = input >> j, channels 2 * FT[j]
        cats = [torch.empty((N, 1, Hh >> j, Ww >> j, 2 * FT[j]), dtype=torch.float32, device=xcl.device) if d else None for j, d in enumerate(plan.direct)]
        xs, h = [], xcl
        for bi in range(9):
            if 1 <= bi <= 4:
                # (the pooled tensor carries xs[-1]'s |max| slots; the concat buffer xs[-1] lives in gets slots of its own, started as a copy)
                h = ops.maxpool2d_fwd(xs[-1], concat=cats[bi - 1])
            elif bi > 4:
                i = bi - 4
                pw, _, c1, c2 = self._up[i - 1]
                bp, _ = self.k2_packed(("pw", i), save)
                z = ops.pw_fwd(h, bp, pw.bias.data, c2)
                skip, cat = xs[4 - i], cats[4 - i]     # (a direct level's |max| slots: a copy of the skip's, made by the pool launch; the upsample max-reduces its half into them)
                if cat is None:
                    cat = torch.empty((N, 1, skip.shape[2], skip.shape[3], 2 * c2), dtype=torch.float32, device=xcl.device)
                    ops.copy_channels(skip, cat, c2, 0, 0, carry_amax=True)      # (+ the |max| of the concat buffer: skip's, then the upsampled half's)
                ops.bilinear2x_fwd(z, cat, c2)      # the upsample writes directly into its half of the concat buffer
                if save:
                    saved.pw_in.append(h)
                h = cat
            out = ops.channel_slab(cats[bi], FT[bi]) if bi < 4 and cats[bi] is not None else None
            h = self._block_fwd(bi, plan.layers[2 * bi:2 * bi + 2], h, plan.G, saved, out)
            if bi <= 4:
                xs.append(h)
        wf, _ = self.conv3_packed(("out", 0), save)
        logits = ops.conv3_fwd(h, wf, self._out.bias.data, self.n_classes, 1)
        if getattr(self, "_want_features", False):
            self._last_feature = h
        for _ in range(plan.bn_ticks):
            self._nbt_tick()
        if save:
            saved.layers.append(_SavedLayer(h, None, None, None, None, plan.layers[-1]))
            saved.xs = xs
        return logits, saved

    def _grad_stages(self):
        def cbp(cb):
            return [m_.weight for m_ in (cb.c1, cb.b1, cb.c2, cb.b2)] + [m_.bias for m_ in (cb.c1, cb.b1, cb.c2, cb.b2)]
        st = []
        for i in range(4, 0, -1):
            pw, cb = self._up[i - 1][0], self._up[i - 1][1]
            st.append((pw.weight, [pw.weight, pw.bias] + cbp(cb) + ([self._out.weight, self._out.bias] if i == 4 else [])))
        for i in range(4, 0, -1):
            st.append((self._enc[i].c1.weight, cbp(self._enc[i])))
        return st

    def _final_from(self, p, like):
        if self._grad_bucket_hook is not None:      # (data parallelism: the bucket's weight gradients must be on the side stream before the hook orders behind it)
            self._wgrad_flush()
        self._grads_final_from(p, like)

    def _block_bwd(self, bi, da2, saved, routes):
        """one ConvBlock's backward on its two routes -> the gradient of the block's input (None: nobody asks)"""
        ops, (tag, cb), G = self.ops, self._blocks[bi], saved.plan.G
        (s1, s2), (b1, b2) = saved.layers[2 * bi:2 * bi + 2], routes[2 * bi:2 * bi + 2]
        h, act = s1.x, s1.route.act
        dy2 = ops.norm_bwd(s2.y, da2, G, s2.stats, act, cb.b2.weight.grad, cb.b2.bias.grad, True)
        # weight gradients run underneath the dgrad -> norm backward chain (HipNet._wgrad_later)
        self._wgrad_later(functools.partial(ops.conv3_wgrad, s2.x, dy2, cb.c2.weight.grad, 1, accumulate=True), dy2, s2.x)
        _, wd2 = self.conv3_packed((tag, 2), True)
        bpart, bnb = None, 0
        if b2.dgrad == "conv3_fwd_raw":      # deepest level: raw split-K slabs for the norm backward's statistics pass to sum (bcp_norm_bwd_slabs)
            da1 = ops.conv3_fwd_raw(dy2, wd2, cb.cout, 1, b2.nslabs)
        elif b2.dgrad == "conv3_dgrad_bwdstats":       # no dropout between the two convs: the dgrad epilogue leaves b1's backward statistics
            da1, bpart, bnb = ops.conv3_dgrad_bwdstats(dy2, wd2, cb.cout, 1, s1.y, s1.stats, act, G)
        else:
            da1 = ops.conv3_fwd(dy2, wd2, None, cb.cout, 1)
        w, n = cb.c1.weight, b1.norm
        kw = dict(elem_mask=s1.cs, elem_scale=1.0 / (1.0 - cb.p) if s1.route.dropout else 1.0)
        if n == "conv3_c1_norm_bwd_wgrad":
            ops.conv3_c1_norm_bwd_wgrad(h, w.data, cb.c1.bias.data, 1, G, s1.stats, da1, act, w.grad, cb.b1.weight.grad, cb.b1.bias.grad, True,
                                        dw_accumulate=True, **kw)
            return None
        if n == "conv3_c1_norm_bwd":
            dy1 = ops.conv3_c1_norm_bwd(h, w.data, cb.c1.bias.data, 1, G, s1.stats, da1, act, cb.b1.weight.grad, cb.b1.bias.grad, True, **kw)
        elif n == "norm_bwd_slabs":
            dy1, _ = ops.norm_bwd_slabs(s1.y, da1, b2.nslabs, G, s1.stats, act, cb.b1.weight.grad, cb.b1.bias.grad, True, **kw)
        else:
            dy1 = ops.norm_bwd(s1.y, da1, G, s1.stats, act, cb.b1.weight.grad, cb.b1.bias.grad, True, partial=bpart, nb=bnb, **kw)
        self._wgrad_later(functools.partial(ops.conv3_c1_wgrad if cb.cin == 1 else ops.conv3_wgrad, h, dy1, w.grad, 1, accumulate=True), dy1, h)
        if b1.dgrad is None:
            return None
        _, wd1 = self.conv3_packed((tag, 1), True)
        return ops.conv3_fwd(dy1, wd1, None, cb.cin, 1)

    def _backward_impl(self, saved, dout):
        ops = self.ops
        dlogits = dout if dout.is_contiguous() else dout.contiguous()
        self.begin_backward()
        _, routes = self.plan_backward(saved.plan)
        h_last, xs = saved.layers[-1].x, saved.xs
        self._wg_pend = []

        def out_wgrad():
            ops.conv3_wgrad(h_last, dlogits, self._out.weight.grad, 1, accumulate=True)
            ops.colsum(dlogits, self._out.bias.grad, accumulate=True)
        self._wgrad_later(out_wgrad, dlogits, h_last)
        _, wd = self.conv3_packed(("out", 0), True)
        dh = ops.conv3_fwd(dlogits, wd, None, FT[0], 1)
        skip_grads = {}
        for i in range(4, 0, -1):
            pw, cb, c1, c2 = self._up[i - 1]
            dcat = self._block_bwd(4 + i, dh, saved, routes)                     # [N,1,H,W,2*c2]
            skip_grads[4 - i] = (dcat, c2)                                       # first c2 channels belong to xs[4-i]
            dz = ops.bilinear2x_bwd(dcat, c2, c2)
            h_in = saved.pw_in[i - 1]
            def pw_wgrad(h_in=h_in, dz=dz, pw=pw):
                ops.k2_wgrad(h_in, dz, pw.weight.grad, H.WG_PW, accumulate=True)
                ops.colsum(dz, pw.bias.grad, accumulate=True)
            self._wgrad_later(pw_wgrad, dz, h_in)
            _, bpd = self.k2_packed(("pw", i), True)
            dh = ops.pw_fwd(dz, bpd, None, c1)
            self._final_from(pw.weight, dz)
        # dh = gradient w.r.t. x4; walk the encoder upwards
        for i in range(4, 0, -1):
            dpool = self._block_bwd(i, dh, saved, routes)
            dx = torch.empty(tuple(xs[i - 1].shape), dtype=torch.float32, device=dpool.device)
            dcat, c2 = skip_grads[i - 1]
            # pool backward + the decoder-side skip gradient (the leading c2 channels of dcat) in one pass
            ops.maxpool2d_bwd(xs[i - 1], dpool, dx, add=ops.channel_slab(dcat, c2))
            dh = dx
            self._final_from(self._enc[i].c1.weight, dx)
        self._block_bwd(0, dh, saved, routes)
        self._wgrad_flush()
        self._join_wgrad_stream(dlogits)
        return None


class UNet(UNet_2d):
    """networks/unet.py:148-201 `UNet`: the SAME layers and state_dict keys as `UNet_2d`, but `forward` returns
    `(output, features)` with `features` the decoder's last 16-channel activation (:104-116).  The reference only builds it through
    `net_factory(net_type="unet")` in its offline test / demo scripts (test_ACDC.py:91, under `torch.no_grad()` after `.eval()`);
    no training loop uses the second output, so it is served on the no-grad path only."""

    def forward(self, x, groups=1):
        if self.training and torch.is_grad_enabled() and self._enc[0].c1.weight.requires_grad:
            raise NotImplementedError("UNet (net_factory('unet')): (output, features) is an inference-time interface in BCP; train with "
                                      "BCP_net() / UNet_2d, or call under torch.no_grad()")
        self._want_features, plans, self.use_plans = True, self.use_plans, False      # a replayed pass would not refresh _last_feature
        try:
            out = super().forward(x, groups)
            feat = self._last_feature
        finally:
            self._want_features, self.use_plans = False, plans
            self._last_feature = None
        return out, feat.permute(0, 4, 1, 2, 3).squeeze(2)
