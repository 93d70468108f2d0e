"""3-D V-Net on the MI355X kernels -- drop-in for the reference's networks/VNet.py:VNet (LA, BatchNorm3d +
Dropout3d) and pancreas/Vnet.py:VNet (InstanceNorm3d, `branchs` head), each also with normalization='groupnorm'
(nn.GroupNorm(16, C) after every conv: networks/VNet.py:20-21, pancreas/Vnet.py:22-23).  The LA class with BatchNorm also takes
has_residual=True (ResidualConvBlock, networks/VNet.py:35-65): the last 3x3x3 layer of every block adds the block's input in front of its
ReLU (bcp_norm_fwd_res / _bwd_res / _eval_res); same parameters and keys as the plain net.

Same constructor arguments, same `state_dict()` keys / shapes (259 / 60; groupnorm 172 / 118), same `parameters()` order,
same call result: `(out_seg, features)` for the LA net, `[out]` for the pancreas net.  What differs is
what runs: every layer is a call into libbcp_hip.so (NDHWC fp32, MFMA implicit-GEMM convs, fused
norm+act(+dropout,+skip) streams); autograd sees ONE node per call (networks/_hipnet.py:NetFn).

The schedule is planned, then executed.  `plan_forward` / `plan_backward` decide every layer's route -- which Ops method produces the
pre-norm tensor, which normalises, what the dgrad behind it leaves -- from shapes, mode and switches alone (host-side shape queries of the
library: no tensor, no launch), and every exclusion rule between a fusion and a mode stands there, once.  `_forward_impl` /
`_backward_impl` walk those records and call the named op; what the forward hands to the backward is a `_Saved` (named fields, the routes
included).  Tests read the same records (tests/residual_checks.py, gnorm_seam_checks.py, test_plan_product.py).

Topology (networks/VNet.py:167-186, 213-239): block_one(1->16) dw block_two(2x32) dw block_three(3x64) dw
block_four(3x128) dw block_five(3x256) [Dropout3d] up+x4 block_six(3x128) up+x3 block_seven(3x64) up+x2
block_eight(2x32) up+x1 block_nine(16) [Dropout3d] out_conv(16->n_classes, 1x1x1).
"""
from __future__ import annotations

import functools

import torch
import torch.nn as nn

from .. import hip_ops as H
from ._hipnet import (BNP, GNP, ConvP, HipNet, Holder, NetFn, Seq, _BwdRoute, _Plan, _Route, _SavedLayer, _norm_params, contrastive_heads,
                      plan_conv3_dgrad, plan_conv3_fwd)


class UnsupportedConfiguration(NotImplementedError, AssertionError):
    """a constructor combination that is not built (an AssertionError too: what the constructor raised for these before it had this class)"""


class _Layer:
    __slots__ = ("kind", "conv", "bn", "cin", "cout", "name", "skip_push", "skip_pop", "drop", "closing", "block_first")

    def __init__(self, kind, conv, bn, cin, cout, name):
        self.kind, self.conv, self.bn, self.cin, self.cout, self.name = kind, conv, bn, cin, cout, name
        self.skip_push = False   # the INPUT of this (dw) layer is a skip source
        self.skip_pop = False    # this (up) layer adds the matching skip after its ReLU
        self.drop = None         # 'x5' / 'x9': Dropout3d on this layer's output
        self.closing = False     # has_residual: last 3x3x3 layer of a block -- the block's input is added in front of its ReLU
        self.block_first = False  # has_residual: first 3x3x3 layer of a block -- its input is the block input the closing layer adds


class _Saved:
    """what a saving forward hands to its backward -- one object per pass (launch plans key the backward on its identity)"""
    __slots__ = ("plan", "layers", "head_in")

    def __init__(self, plan):
        self.plan, self.layers, self.head_in = plan, [], None     # head_in: the head's input, None when the head is fused

    G = property(lambda self: self.plan.G)

    def __getitem__(self, i):
        """read-only view in the tuple layout this structure replaced -- (x, y, stats, cs, G[, r_in]) per layer, then (head_in,) -- for
        callers written against it; nothing in the package or its tests reads it"""
        rows = [(s.x, s.y, s.stats, s.cs, self.G) + ((s.r_in,) if s.route.closing else ()) for s in self.layers]
        return (rows + [(self.head_in,)])[i]


class VNet(HipNet):
    UP_RECOMPUTE_GRAD = False   # (round 6) the recomputing transposed conv + norm (library option up_recompute) also in forwards that save for a backward pass: measured slower there (both passes of the norm's backward recompute the conv); forwards WITHOUT a backward pass -- the teacher's -- take it wherever the library serves the shape
    fuse_c1 = True       # first layer: conv + norm + ReLU with recompute (bcp_conv3_c1_norm_fwd / _bwd); False: conv -> y -> norm passes
    fuse_head = True     # the 1x1x1 head applies the last conv's norm + ReLU + Dropout3d itself (bcp_pw16_fwd_norm); False: separate apply pass

    def __init__(self, n_channels=3, n_classes=2, n_filters=16, normalization="none", has_dropout=False, has_residual=False,
                 variant="la"):
        super().__init__()
        assert n_filters == 16, "only the configuration the BCP scripts use is implemented"
        if has_residual and variant != "la":
            raise UnsupportedConfiguration("has_residual: the pancreas V-Net of the reference (pancreas/Vnet.py) has no residual blocks")
        if has_residual and normalization != "batchnorm":
            raise UnsupportedConfiguration("has_residual is built for normalization='batchnorm' only (residual blocks with GroupNorm are not)")
        assert n_channels == 1, "the hot path is single-channel (LA / pancreas); see DESIGN.md"
        la = variant == "la"
        gn = normalization == "groupnorm"
        if la:
            assert normalization == "batchnorm" or gn, "networks/net_factory.py builds the LA V-Net with batchnorm"
        else:
            assert normalization == "instancenorm" or gn
        self.variant = variant
        self.norm = normalization
        self._gn = gn        # GroupNorm(16, C): per-sample statistics, no running buffers, train() and eval() one function
        self.has_dropout = has_dropout
        self.has_residual = bool(has_residual)      # ResidualConvBlock (networks/VNet.py:35-65): same parameters, same keys, another function
        self.n_classes = n_classes
        nf = n_filters
        self._layers = []
        bn = la or gn

        def block(owner, name, n, cin, cout, kind="c3"):
            items = []
            for i in range(n):
                ci = cin if i == 0 else cout
                if kind == "c3":
                    w = (cout, ci, 3, 3, 3)
                    fan = ci * 27
                elif kind == "dw":
                    w = (cout, ci, 2, 2, 2)
                    fan = ci * 8
                else:  # ConvTranspose3d weight [Cin, Cout, 2,2,2]; torch's fan_in uses dim 1
                    w = (ci, cout, 2, 2, 2)
                    fan = cout * 8
                conv = ConvP(w, fan, cout)
                items.append((3 * i, conv))
                b = (GNP(cout) if gn else BNP(cout)) if bn else None
                if b is not None:
                    if not gn:
                        b._live = True
                    items.append((3 * i + 1, b))
                k = "c1" if (kind == "c3" and ci == 1) else kind
                self._layers.append(_Layer(k, conv, b, ci, cout, f"{name}.{3 * i}"))
            h = Holder()
            h.conv = Seq(items)
            setattr(owner, name, h)

        enc = Holder() if la else self
        dec = Holder() if la else self
        block(enc, "block_one", 1, n_channels, nf)
        block(enc, "block_one_dw", 1, nf, 2 * nf, "dw")
        block(enc, "block_two", 2, 2 * nf, 2 * nf)
        block(enc, "block_two_dw", 1, 2 * nf, 4 * nf, "dw")
        block(enc, "block_three", 3, 4 * nf, 4 * nf)
        block(enc, "block_three_dw", 1, 4 * nf, 8 * nf, "dw")
        block(enc, "block_four", 3, 8 * nf, 8 * nf)
        block(enc, "block_four_dw", 1, 8 * nf, 16 * nf, "dw")
        block(enc, "block_five", 3, 16 * nf, 16 * nf)
        if la:
            enc.dropout = nn.Dropout3d(p=0.5, inplace=False)  # parameter-free; kept for module-tree parity
        block(dec, "block_five_up", 1, 16 * nf, 8 * nf, "up")
        block(dec, "block_six", 3, 8 * nf, 8 * nf)
        block(dec, "block_six_up", 1, 8 * nf, 4 * nf, "up")
        block(dec, "block_seven", 3, 4 * nf, 4 * nf)
        block(dec, "block_seven_up", 1, 4 * nf, 2 * nf, "up")
        block(dec, "block_eight", 2, 2 * nf, 2 * nf)
        block(dec, "block_eight_up", 1, 2 * nf, nf, "up")
        if la:
            block(dec, "block_nine", 1, nf, nf)
            dec.out_conv = ConvP((n_classes, nf, 1, 1, 1), nf, n_classes)
            dec.dropout = nn.Dropout3d(p=0.5, inplace=False)
            self.encoder, self.decoder = enc, dec
            self.pool = nn.MaxPool3d(3, stride=2)
            contrastive_heads(self, 2)
            object.__setattr__(self, "_out", dec.out_conv)   # alias without a second registration
        else:
            br = Holder()
            block(br, "b0", 1, nf, nf)
            head = ConvP((n_classes, nf, 1, 1, 1), nf, n_classes)
            self.branchs = nn.ModuleList([Seq([(0, br.b0), (1, head)])])
            object.__setattr__(self, "_out", head)
        for L in self._layers:
            if L.kind == "dw":
                L.skip_push = True
            if L.kind == "up":
                L.skip_pop = True
        if la:
            # Dropout3d sites: after block_five's last conv (x5) and after block_nine (x9)
            idx5 = max(i for i, L in enumerate(self._layers) if L.name.startswith("block_five."))
            self._layers[idx5].drop = "x5"
            self._layers[-1].drop = "x9"
        if self.has_residual:
            # a block = a maximal run of 3x3x3 layers with one block name; its last layer adds the block's input in front of the ReLU
            for i, L in enumerate(self._layers):
                if L.kind in ("c1", "c3"):
                    blk = L.name.rsplit(".", 1)[0]
                    L.block_first = i == 0 or self._layers[i - 1].name.rsplit(".", 1)[0] != blk
                    L.closing = i == len(self._layers) - 1 or self._layers[i + 1].name.rsplit(".", 1)[0] != blk
        # parameters that take part in the optimiser: everything the forward pass touches
        ids = set()
        for L in self._layers:
            ids.add(id(L.conv.weight)); ids.add(id(L.conv.bias))
            if L.bn is not None:
                ids.add(id(L.bn.weight)); ids.add(id(L.bn.bias))
        ids.add(id(self._out.weight)); ids.add(id(self._out.bias))
        self._opt_param_ids = ids
        for li, L in enumerate(self._layers):
            if L.kind == "c3":
                self.register_conv3(("c3", li), L.conv.weight, 3)
            elif L.kind == "dw":
                self.register_k2(("k2", li), L.conv.weight, L.cin, L.cout, H.PACK_DOWN_FWD, H.PACK_DOWN_DGRAD)
            elif L.kind == "up":
                self.register_k2(("k2", li), L.conv.weight, L.cin, L.cout, H.PACK_UP_FWD, H.PACK_UP_DGRAD)

    # ------------------------------------------------------------------ public call
    pool_features = True      # LA variant: also return pool(x5) as the reference does (networks/VNet.py:286-290)

    def forward(self, input, turnoff_drop=False, groups=1, features=None):
        """groups > 1: `input` holds `groups` consecutive sub-batches that the reference would push through the net in
        separate calls (LA_BCP_train.py:241-242, 252-253); they are normalised separately (grouped BatchNorm) but every
        layer is ONE launch over all of them -- identical results, half the launches, twice the work per launch."""
        x = input
        N = x.shape[0]
        assert x.dim() == 5 and x.shape[1] == 1, "expected [N,1,X,Y,Z]"
        self._ensure_flat()
        self.refresh_weights_version()
        xcl = x.contiguous().view(N, x.shape[2], x.shape[3], x.shape[4], 1)
        self._turnoff_drop = bool(turnoff_drop)
        assert N % groups == 0
        self._groups = int(groups)
        self._feat_out = None
        # `features=False` (the fused step functions of train_step.py, which discard it): no max-pool launch, no copy out of the plan
        self._want_feat = bool(self.pool_features if features is None else features) and self.variant == "la"
        if self.training and torch.is_grad_enabled() and any(p.requires_grad for p in (self._layers[0].conv.weight,)):
            out = NetFn.apply(xcl, self._layers[0].conv.weight, self)   # eval() is forward-only (validation, test_3d_patch)
        else:
            out, _ = self._run_forward(xcl, False)
        logits = out.permute(0, 4, 1, 2, 3)  # logical [N,C,X,Y,Z], channels_last_3d strides
        if self.variant == "la":
            # second value: pool(x5) [N,256,3,3,2] at the LA size (networks/VNet.py:286-290; dead in every train script, LA_BCP_train.py:158,252;
            # forward only -- no gradient flows into it).  None when the deepest level is smaller than the 3x3x3 window (the reference raises there).
            f = self._feat_out
            return logits, (None if f is None else f.permute(0, 4, 1, 2, 3))
        return [logits]

    # ------------------------------------------------------------------ schedule: the planner (no tensor, no launch)
    def plan_forward(self, N, D, H, W, groups, save, training, dropout, keep_saved=False):
        """every layer's forward route for an input of extents (N, D, H, W) -> _Plan.  Decided from the layer list, the shapes, the mode
        (`training`; `dropout`: the Dropout3d sites draw; `keep_saved`: a test wants every pre-norm tensor) and the class switches alone --
        it asks the library's host-side shape queries and nothing else, so it runs without a GPU.  Every exclusion rule stands here, once."""
        ops, gn, bnorm = self.ops, self._gn, self.norm == "batchnorm"
        G = groups if bnorm else N
        # GroupNorm evaluates exactly as it trains: every choice that asks "training?" for the sake of batch statistics takes the training
        # answer in both modes, so model.eval() gives the train-mode bits (dropout apart)
        batch_stats = training or gn
        last = len(self._layers) - 1
        Ll = self._layers[last]
        # the head normalises on its way in (bcp_pw16_fwd_norm): block_nine's 16-channel activation is never written (statistics only there)
        fuse_head = self.fuse_head and batch_stats and Ll.kind == "c3" and Ll.cout == 16 and not Ll.skip_pop and N <= 32 and not Ll.closing
        routes, sp = [], (D, H, W)
        for li, L in enumerate(self._layers):
            r = _Route()
            r.xshape = (N,) + sp + (L.cin,)
            sp = tuple(e // 2 for e in sp) if L.kind == "dw" else tuple(2 * e for e in sp) if L.kind == "up" else sp
            r.yshape = (N,) + sp + (L.cout,)
            r.closing, r.dropout, r.stats_only = L.closing, dropout and L.drop is not None, li == last and fuse_head
            # a fusion whose norm reads something else than a plain pre-norm tensor: training-mode BatchNorm / InstanceNorm only, and never
            # where another op reads that tensor -- the closing layer of a residual block (bcp_norm_fwd_res / _eval_res apply relu(z + r)
            # themselves) and the layer in front of the fused head
            fusable = training and not gn and not L.closing and not r.stats_only
            # ... and one that never writes the pre-norm tensor (recompute): not at a Dropout3d site, not when a test wants that tensor
            recompute = fusable and L.drop is None and not keep_saved
            if L.kind == "c1":
                if recompute and self.fuse_c1 and not L.skip_pop and ops.conv3_c1_norm_ok(r.xshape, 3, G):
                    r.producer = "conv3_c1_norm_fwd"      # conv + norm + ReLU with recompute: the 16-channel pre-norm tensor is never written
                elif batch_stats:                         # statistics in the epilogue: no pass over the 16-channel y
                    r.producer, r.rows = "conv3_c1_fwd_stats", ops.conv3_c1_stat_rows(r.xshape, 3, G)
                else:
                    r.producer = "conv3_c1_fwd"
            elif L.kind == "c3":                          # (eval-mode BatchNorm needs no batch statistics)
                plan_conv3_fwd(ops, r, 3, G, slabs=fusable, stats=batch_stats or L.bn is None)
            elif L.kind == "up" and recompute and (not save or self.UP_RECOMPUTE_GRAD) and ops.up_norm_rows(r.xshape, L.cout, G) > 0:
                # (round 6) transposed conv + norm + ReLU + skip add with recompute (bcp_up_fwd_norm): the pre-norm tensor is never written
                r.producer = "up_fwd_norm"
            else:
                # (round 6) the norm's statistics from the GEMM's epilogue where the shape has them (library option k2_stats = 0: never)
                r.rows = ops.k2_stat_rows(int(L.kind == "up"), r.xshape, L.cout, G) if batch_stats else 0
                r.producer = "k2_fwd_stats" if r.rows else "down_fwd" if L.kind == "dw" else "up_fwd"
            if L.closing:
                r.norm = "norm_fwd_res" if training else "norm_eval_res"
            elif r.producer in ("conv3_c1_norm_fwd", "up_fwd_norm"):
                r.norm = r.producer
            elif r.producer == "conv3_fwd_raw":
                r.norm = "norm_fwd_slabs"
            elif gn:        # statistics (the producer's rows, or a pass of its own) -> finalize -> apply; in front of the fused head the table only
                r.norm = "gnorm_fwd"
            else:           # model.eval(): running statistics, no update (validation / sliding-window inference)
                r.norm = "norm_eval" if L.bn is not None and not training else "norm_fwd"
            routes.append(r)
        return _Plan(G, "pw16_fwd_norm" if fuse_head else "pw16_fwd", routes, G if bnorm and training else 0)

    def plan_call(self, N, D, H, W, save):
        """plan_forward in the mode this network is in: what its next (or last) call with such an input and these `forward` arguments takes"""
        return self.plan_forward(N, D, H, W, getattr(self, "_groups", 1), save, self.training,
                                 self.has_dropout and self.training and not getattr(self, "_turnoff_drop", False), getattr(self, "_keep_saved", False))

    def plan_backward(self, plan):
        """the backward routes behind a saving forward's plan -> (the head's backward op, [_BwdRoute per layer]); launch-free like plan_forward"""
        ops, gn, G, R = self.ops, self._gn, plan.G, plan.layers
        last = len(self._layers) - 1
        if plan.head != "pw16_fwd_norm":
            head = "pw16_bwd"
        else:       # the fused head goes THROUGH the last layer's norm (the one-call form makes BatchNorm's backward coefficients itself)
            head = "pw16_bwd_norm_bwd" if ops.HEAD_BWD_FUSED and not self._layers[last].skip_pop and not gn else "pw16_bwd_norm"
        out = [None] * (last + 1)
        nsl, partial = 1, False          # what the dgrad behind the layer leaves: raw split-K slabs (> 1), the layer's backward-statistics rows
        for li in range(last, -1, -1):
            L, r, b = self._layers[li], R[li], _BwdRoute()
            if r.closing:
                b.norm = "norm_bwd_res"
            elif li == last and head == "pw16_bwd_norm_bwd":
                b.norm = head
            elif r.norm == "up_fwd_norm":        # (round 6) y = up(x_in) again, inside both passes of the norm's backward
                b.norm = "up_norm_bwd"
            elif r.norm == "conv3_c1_norm_fwd":  # ... and with C1_BWD_FUSED the layer's weight gradient in the same pass: no dy
                b.norm = "conv3_c1_norm_bwd_wgrad" if ops.C1_BWD_FUSED else "conv3_c1_norm_bwd"
            elif r.norm == "gnorm_fwd":
                b.norm = "gnorm_bwd"
            else:                                # deep levels: the backward-statistics pass sums the dgrad's raw slabs (bcp_norm_bwd_slabs)
                b.norm = "norm_bwd_slabs" if nsl > 1 else "norm_bwd"
            assert b.norm in ("norm_bwd", "gnorm_bwd", "norm_bwd_slabs") or (nsl == 1 and not partial), (L.name, b.norm, nsl, partial)
            b.partial, nsl, partial = partial, 1, False
            # the consumer of this layer's dgrad is the norm backward of the layer in front.  has_residual: the dgrad of a block's FIRST layer
            # is joined with the shortcut's gradient first -- a plain tensor, and no statistics taken from it in front of the join
            prev = R[li - 1] if li > 0 and not L.block_first else None
            if L.kind == "c1":
                b.dgrad = None
            elif L.kind == "c3":
                plan_conv3_dgrad(ops, b, r, prev, 3, G, slabs=not gn)
            else:
                # (round 6) bcp_down_dgrad_bwdstats / bcp_up_dgrad_bwdstats where the shape is served: no k_col_partial<1> pass over (y, da)
                if prev is not None and prev.bwdstats_ok:
                    b.rows = ops.k2_bwdstat_rows(int(L.kind == "up"), r.yshape, L.cin, G)
                b.dgrad = "k2_dgrad_bwdstats" if b.rows else "down_dgrad" if L.kind == "dw" else "up_dgrad"
            nsl, partial = b.nslabs, b.rows > 0
            out[li] = b
        return head, out

    # ------------------------------------------------------------------ schedule: the executors (dispatch on the records)
    def _chan_scale(self, L, N, dev):
        if self.drop_masks is not None:
            m = self.drop_masks[L.drop]
            return (m.to(device=dev, dtype=torch.float32) * 2.0).contiguous()
        cs = torch.empty((N, L.cout), dtype=torch.float32, device=dev)
        return self.ops.bernoulli(cs, 0.5, 2.0, self.next_seed())

    def _forward_impl(self, xcl, save):
        ops = self.ops
        N = xcl.shape[0]
        plan = self.plan_call(N, xcl.shape[1], xcl.shape[2], xcl.shape[3], save)
        G = plan.G
        h = xcl
        skips = []
        saved = _Saved(plan) if save else None
        feat = None
        r_in = None                      # has_residual: the input of the block being walked
        for li, (L, r) in enumerate(zip(self._layers, plan.layers)):
            w, b = L.conv.weight, L.conv.bias
            y, part, nb = None, None, 0
            if L.skip_push:
                skips.append(h)
            if L.block_first:
                r_in = h
            p = r.producer           # (the recomputing producers, conv3_c1_norm_fwd and up_fwd_norm, ARE the norm op below: nothing here)
            if L.kind == "c3":
                wf, _ = self.conv3_packed(("c3", li), save)
            elif L.kind != "c1":
                bp, _ = self.k2_packed(("k2", li), save)
            if p == "conv3_c1_fwd_stats":
                y, part, nb = ops.conv3_c1_fwd_stats(h, w.data, b.data, 3, G)
            elif p == "conv3_c1_fwd":
                y = ops.conv3_c1_fwd(h, w.data, b.data, 3)
            elif p == "conv3_fwd_raw":
                src = ops.conv3_fwd_raw(h, wf, L.cout, 3, r.nslabs)
            elif p == "conv3_fwd_stats":
                y, part, nb = ops.conv3_fwd_stats(h, wf, b.data, L.cout, 3, G)
            elif p == "conv3_fwd":
                y = ops.conv3_fwd(h, wf, b.data, L.cout, 3)
            elif p == "k2_fwd_stats":
                y, part, nb = ops.k2_fwd_stats(int(L.kind == "up"), h, bp, b.data, L.cout, G)
            elif p == "down_fwd":
                y = ops.down_fwd(h, bp, b.data, L.cout)
            elif p == "up_fwd":
                y = ops.up_fwd(h, bp, b.data, L.cout)
            res = skips.pop() if L.skip_pop else None
            cs = self._chan_scale(L, N, xcl.device) if r.dropout else None
            n, stats = r.norm, None
            if n == "norm_fwd_res":
                a, stats = ops.norm_fwd_res(y, G, *_norm_params(L.bn), H.ACT_RELU, r_in, chan_scale=cs, partial=part, nb=nb)
            elif n == "norm_eval_res":
                a = ops.norm_eval_res(y, *_norm_params(L.bn), H.ACT_RELU, r_in)
            elif n == "up_fwd_norm":
                a, stats = ops.up_fwd_norm(h, bp, b.data, L.cout, G, *_norm_params(L.bn), H.ACT_RELU, residual=res)
            elif n == "conv3_c1_norm_fwd":
                a, stats = ops.conv3_c1_norm_fwd(h, w.data, b.data, 3, G, *_norm_params(L.bn), H.ACT_RELU)
            elif n == "norm_fwd_slabs":
                a, stats, y = ops.norm_fwd_slabs(src, r.nslabs, b.data, G, *_norm_params(L.bn), H.ACT_RELU, chan_scale=cs, residual=res)
            elif n == "gnorm_fwd":
                a, stats = ops.gnorm_fwd(y, L.bn.weight.data, L.bn.bias.data, H.ACT_RELU, chan_scale=cs, residual=res, partial=part, nb=nb,
                                         stats_only=r.stats_only)
            elif n == "norm_eval":
                a = ops.norm_eval(y, *_norm_params(L.bn), H.ACT_RELU, residual=res)
            else:
                a, stats = ops.norm_fwd(y, G, *_norm_params(L.bn), H.ACT_RELU, chan_scale=cs, residual=res, partial=part, nb=nb,
                                        stats_only=r.stats_only)
            if save:
                saved.layers.append(_SavedLayer(h, y, stats, cs, r_in if r.closing else None, r))
            h = a
            if L.drop == "x5" and getattr(self, "_want_feat", False) and min(a.shape[1:4]) >= 3:
                feat = ops.maxpool3d_k3s2_fwd(a)      # pool(features[4]): the reference's second return value (networks/VNet.py:286-290)
        for _ in range(plan.bn_ticks):
            self._nbt_tick()
        if plan.head == "pw16_fwd_norm":
            logits = ops.pw16_fwd_norm(y, stats, cs, G, H.ACT_RELU, self._out.weight.data, self._out.bias.data, self.n_classes)
        else:
            logits = ops.pw16_fwd(h, self._out.weight.data, self._out.bias.data, self.n_classes)
        if save:
            saved.head_in = h           # None when the head is fused: the backward recomputes it from the last layer's record
        logits._bcp_feat = feat         # rides on the result object (launch plans keep it; _run_forward hands out a copy)
        return logits, saved

    def _grad_stages(self):
        st = []
        for li in range(len(self._layers) - 1, -1, -1):
            L = self._layers[li]
            ps = [L.conv.weight, L.conv.bias] + ([L.bn.weight, L.bn.bias] if L.bn is not None else [])
            if li == len(self._layers) - 1:
                ps += [self._out.weight, self._out.bias]
            st.append((L.conv.weight, ps))
        return st

    def _backward_impl(self, saved, dout):
        ops = self.ops
        G = saved.G
        dlogits = dout if dout.is_contiguous() else dout.contiguous()
        self.begin_backward()
        head, routes = self.plan_backward(saved.plan)
        s9, dy_head = saved.layers[-1], None
        if head == "pw16_bwd_norm_bwd":      # that layer's dy comes out of the head's call: no norm backward of its own
            bn9 = self._layers[-1].bn
            dg9, db9 = (bn9.weight.grad, bn9.bias.grad) if bn9 is not None else (None, None)
            dy_head = ops.pw16_bwd_norm_bwd(s9.y, s9.stats, s9.cs, G, H.ACT_RELU, dlogits, self._out.weight.data, self._out.weight.grad,
                                            self._out.bias.grad, dg9, db9, norm_accumulate=bn9 is not None, accumulate=True)
            dh = None
        elif head == "pw16_bwd_norm":
            dh = ops.pw16_bwd_norm(s9.y, s9.stats, s9.cs, G, H.ACT_RELU, dlogits, self._out.weight.data, self._out.weight.grad, self._out.bias.grad,
                                   accumulate=True)
        else:
            dh = ops.pw16_bwd(saved.head_in, dlogits, self._out.weight.data, self._out.weight.grad, self._out.bias.grad, accumulate=True)
        skip_grads = []
        self._wg_pend = []
        bpart, bnb = None, 0             # backward-statistics partials of THIS layer's norm, left by the dgrad that produced dh
        for li in range(len(self._layers) - 1, -1, -1):
            L, s, r = self._layers[li], saved.layers[li], routes[li]
            x_in, y, stats, cs = s.x, s.y, s.stats, s.cs
            w = L.conv.weight
            da = dh
            dg, db = (L.bn.weight.grad, L.bn.bias.grad) if L.bn is not None else (None, None)
            n = r.norm
            if n == "norm_bwd_res":
                # g = da * chan_scale * [z + r > 0] feeds the norm backward and, as dres, the gradient of the block input (block_one's r is the
                # network input: no dres)
                dy, dres = ops.norm_bwd_res(y, da, s.r_in, G, stats, H.ACT_RELU, dg, db, True, chan_scale=cs, want_dres=li > 0)
            elif n == "pw16_bwd_norm_bwd":
                dy = dy_head
            elif n == "up_norm_bwd":
                bpf, _ = self.k2_packed(("k2", li), True)      # (the FORWARD pack: y is recomputed)
                dy = ops.up_norm_bwd(x_in, bpf, L.conv.bias.data, L.cout, G, stats, da, H.ACT_RELU, dg, db, L.bn is not None)
            elif n == "conv3_c1_norm_bwd_wgrad":      # no dy, no launch left behind the main stream's last one
                ops.conv3_c1_norm_bwd_wgrad(x_in, w.data, L.conv.bias.data, 3, G, stats, da, H.ACT_RELU, w.grad, dg, db, L.bn is not None,
                                            dw_accumulate=True)
                self._wgrad_flush()
                self._grads_final_from(w, da)
                break
            elif n == "conv3_c1_norm_bwd":      # the fused first layer: its pre-norm tensor is recomputed from the input
                dy = ops.conv3_c1_norm_bwd(x_in, w.data, L.conv.bias.data, 3, G, stats, da, H.ACT_RELU, dg, db, L.bn is not None)
            elif n == "gnorm_bwd":
                # conv biases in front of GroupNorm layers with more than one channel per group receive their gradient (DESIGN.md "bias gradients")
                dy = ops.gnorm_bwd(y, da, stats, L.bn.weight.data, H.ACT_RELU, dg, db, L.conv.bias.grad if L.cout > 16 else None, True,
                                   chan_scale=cs, partial=bpart, nb=bnb)
            elif n == "norm_bwd_slabs":      # dh is the raw split-K slabs of the dgrad that produced it
                dy, da = ops.norm_bwd_slabs(y, da, routes[li + 1].nslabs, G, stats, H.ACT_RELU, dg, db, L.bn is not None, chan_scale=cs)
            else:
                dy = ops.norm_bwd(y, da, G, stats, H.ACT_RELU, dg, db, L.bn is not None, chan_scale=cs, partial=bpart, nb=bnb)
            bpart, bnb = None, 0
            if L.skip_pop:
                skip_grads.append(da)       # d(out)/d(skip) = identity: the skip source gets `da` itself
            # conv biases feed a norm: behind BatchNorm / InstanceNorm their gradient is identically zero (DESIGN.md "bias gradients"); the flat
            # gradient buffer was cleared by begin_backward(), nothing to add.  (GroupNorm: gnorm_bwd above has added it.)
            # The weight gradient goes to the side stream, in batches (HipNet._wgrad_later)
            if L.kind in ("c1", "c3"):
                wgrad, arg = ops.conv3_c1_wgrad if L.kind == "c1" else ops.conv3_wgrad, 3      # (x, dy, dw, KD)
            else:
                wgrad, arg = ops.k2_wgrad, H.WG_DOWN if L.kind == "dw" else H.WG_UP            # (x, dy, dw, kind)
            self._wgrad_later(functools.partial(wgrad, x_in, dy, w.grad, arg, accumulate=True), dy, x_in, final=w)
            d = r.dgrad
            prev = saved.layers[li - 1] if li > 0 else None      # (a *_dgrad_bwdstats epilogue reads its pre-norm tensor and statistics)
            if d is None:
                dh = None
            elif L.kind == "c3":
                _, wd = self.conv3_packed(("c3", li), True)
                if d == "conv3_fwd_raw":
                    dh = ops.conv3_fwd_raw(dy, wd, L.cin, 3, r.nslabs)
                elif d == "conv3_dgrad_bwdstats":
                    dh, bpart, bnb = ops.conv3_dgrad_bwdstats(dy, wd, L.cin, 3, prev.y, prev.stats, H.ACT_RELU, G)
                else:
                    dh = ops.conv3_fwd(dy, wd, None, L.cin, 3)
            else:
                _, bp = self.k2_packed(("k2", li), True)
                sg = skip_grads.pop() if L.kind == "dw" else None      # down conv: x_in is a skip source, the decoder-side gradient is joined in place
                if d == "k2_dgrad_bwdstats":
                    dh, bpart, bnb = ops.k2_dgrad_bwdstats(int(L.kind == "up"), dy, bp, L.cin, prev.y, prev.stats, H.ACT_RELU, G, out=sg,
                                                           accumulate=sg is not None)
                elif d == "down_dgrad":
                    dh = ops.down_dgrad(dy, bp, L.cin, out=sg, accumulate=True)
                else:
                    dh = ops.up_dgrad(dy, bp, L.cin)
            if L.block_first and li > 0:
                # the join: the block input's gradient = the first layer's dgrad + the shortcut's dres.  The joined tensor is what the layer in
                # front consumes (and, behind an up layer, what skip_grads receives)
                dh = ops.axpy(dh, dres, 1.0)
                ops._no_amax(dh)
        self._wgrad_flush()
        self._join_wgrad_stream(dlogits)
        return None

