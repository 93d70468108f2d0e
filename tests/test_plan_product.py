"""The planners (networks/VNet.py and networks/unet.py plan_forward / plan_backward) at PRODUCT shapes against the committed product-op table
(tests/product_ops.py STEP_KEYS, recorded from replayed steps on the device): CPU only, the gfx950 library's host-side shape queries, no
launch.  Every (op, shape of its first tensor operand) the planner emits for the passes a workload's step runs is a row of that workload,
and every row whose op is the schedule's choice is emitted -- so a route that needs product extents (the recomputing transposed conv, the k2
GEMMs' statistics epilogues: tests/residual_checks.py ROUTES_REACHED; the U-Net's served dgrad epilogue and its all-direct concat levels:
tests/unet_plan_checks.py) is pinned here."""
import os

import pytest

import product_ops as P
from bcp_amd import _lib
from bcp_amd.hip_ops import Ops
from bcp_amd.networks.unet import UNet_2d
from bcp_amd.networks.VNet import VNet

# the schedule's vocabulary: the conv, k2, norm and head families, forward and backward.  Packs, weight gradients, the shortcut join, loss,
# optimiser and pseudo-label ops are in the table too and are not the planner's choice
VOCAB = {"conv3_c1_norm_fwd", "conv3_c1_fwd_stats", "conv3_c1_fwd", "conv3_fwd_raw", "conv3_fwd_stats", "conv3_fwd", "up_fwd_norm", "k2_fwd_stats",
         "down_fwd", "up_fwd", "norm_fwd", "norm_fwd_slabs", "norm_fwd_res", "norm_eval", "norm_eval_res", "gnorm_fwd", "pw16_fwd", "pw16_fwd_norm",
         "pw16_bwd", "pw16_bwd_norm", "pw16_bwd_norm_bwd", "norm_bwd", "norm_bwd_slabs", "norm_bwd_res", "gnorm_bwd", "up_norm_bwd",
         "conv3_c1_norm_bwd", "conv3_c1_norm_bwd_wgrad", "conv3_dgrad_bwdstats", "k2_dgrad_bwdstats", "down_dgrad", "up_dgrad"}
ON_INPUT = {"conv3_c1_norm_fwd", "up_fwd_norm", "conv3_c1_norm_bwd", "conv3_c1_norm_bwd_wgrad", "up_norm_bwd"}      # first operand: the layer's input
UNET_VOCAB = VOCAB | {"copy_channels"}      # the U-Net's schedule also decides which concat buffers are filled by a copy
LA, PANCREAS, ACDC = (112, 112, 80), (96, 96, 96), (256, 256)
# workload: (variant, has_residual, extents, passes[, normalization: the variant's own unless given]); a pass: (N, groups, mode) -- "teacher": training mode under no_grad, "student": a
# saving forward with its backward, "eval": model.eval() under no_grad.  Batches and extents are those of product_ops.make_step: a
# self-training step runs teacher and student with groups=2 at half the batch, a pre-training step one saving pass on one sample, a
# validation pass one full chunk of four patches and a remainder chunk of one
WORKLOADS = {
    "la": ("la", False, LA, ((2, 2, "teacher"), (2, 2, "student"))),
    "la8": ("la", False, LA, ((4, 2, "teacher"), (4, 2, "student"))),
    "lares": ("la", True, LA, ((2, 2, "teacher"), (2, 2, "student"))),
    "pancreas": ("pancreas", False, PANCREAS, ((2, 2, "teacher"), (2, 2, "student"))),
    "la_pre": ("la", False, LA, ((1, 1, "student"),)),
    "lares_pre": ("la", True, LA, ((1, 1, "student"),)),
    "pancreas_pre": ("pancreas", False, PANCREAS, ((1, 1, "student"),)),
    "la_val": ("la", False, LA, ((4, 1, "eval"), (1, 1, "eval"))),
    "lares_val": ("la", True, LA, ((4, 1, "eval"), (1, 1, "eval"))),
    "pancreas_val": ("pancreas", False, PANCREAS, ((4, 1, "eval"), (1, 1, "eval"))),
    "lagn": ("la", False, LA, ((2, 2, "teacher"), (2, 2, "student")), "groupnorm"),
    "lagn_pre": ("la", False, LA, ((1, 1, "student"),), "groupnorm"),
    "lagn_val": ("la", False, LA, ((4, 1, "eval"), (1, 1, "eval")), "groupnorm"),
    "pancreasgn": ("pancreas", False, PANCREAS, ((2, 2, "teacher"), (2, 2, "student")), "groupnorm"),
}
# the U-Net's: an ACDC self-training step runs teacher and student on 12 slices grouped 2, a pre-training step one saving pass on 6 slices, a
# validation pass one chunk of 16 slices and a remainder chunk of one (the committed tables' batches)
UNET_WORKLOADS = {"acdc": ((12, 2, "teacher"), (12, 2, "student")), "acdc_pre": ((6, 1, "student"),), "acdc_val": ((16, 1, "eval"), (1, 1, "eval"))}
# the wrappers that run their plain op themselves where their rows query answers 0 (the planner's record holds that answer in `rows`): a
# REPLAYED step keys the launches by the plain op alone, an EAGER pass (validation) keys the wrapper's call and, inside it, the plain op's
FALLBACK = {"conv3_fwd_stats": "conv3_fwd", "conv3_c1_fwd_stats": "conv3_c1_fwd", "conv3_dgrad_bwdstats": "conv3_fwd"}


def _keys(op, rows, shape, eager):
    if op in FALLBACK and rows == 0:
        return {(FALLBACK[op], shape)} | ({(op, shape)} if eager else set())
    return {(op, shape)}


@pytest.fixture(scope="module")
def product_ops():
    assert os.path.exists(_lib.LIB_PATH), "libbcp_hip.so missing -- run __graft_entry__.build()"
    return Ops(_lib.Binding(_lib.LIB_PATH), allow_cpu=True)


def planned_pairs(net, N, sp, groups, mode):
    """the (op, shape of the first tensor operand) pairs of one pass as the profile hooks would key them; stats_only norm calls are not
    profiled (hip_ops._profiled) and stay out"""
    train = mode != "eval"
    if isinstance(net, UNet_2d):
        plan = net.plan_forward(N, *sp, groups, training=train)
    else:
        plan = net.plan_forward(N, *sp, groups, save=mode == "student", training=train, dropout=net.has_dropout and train)
    pairs, last = set(), plan.layers[-1]
    for r in plan.layers:
        if r.keeps_y:
            pairs |= _keys(r.producer, r.rows, r.xshape, not train)
        if r.norm is not None and not r.stats_only:
            pairs.add((r.norm, r.xshape if r.norm in ON_INPUT else ((r.nslabs,) if r.norm == "norm_fwd_slabs" else ()) + r.yshape))
    if plan.head is not None:
        pairs.add((plan.head, last.yshape))
    # (U-Net) an encoder level that is not written into its concat buffer is copied there: the second conv's output of block j
    pairs |= {("copy_channels", plan.layers[2 * j + 1].yshape) for j, d in enumerate(plan.direct) if not d}
    if mode == "student":
        head, routes = net.plan_backward(plan)
        if head is not None:
            pairs.add((head, last.yshape))
        for r, b in zip(plan.layers, routes):
            if b.norm is not None and b.norm != head:
                pairs.add((b.norm, r.xshape if b.norm in ON_INPUT else r.yshape))
            if b.dgrad is not None and b.norm != "conv3_c1_norm_bwd_wgrad":
                pairs |= _keys(b.dgrad, b.rows, r.yshape, False)
    return pairs


def _against_table(net, workload, sp, passes, vocab):
    planned = set()
    for N, groups, mode in passes:
        planned |= planned_pairs(net, N, sp, groups, mode)
    table = {(k[0], tuple(k[1][0])) for k in P.STEP_KEYS[workload] if k[0] in vocab}
    assert {p[0] for p in planned} <= vocab
    assert planned <= table, ("planned, not a row of the table", sorted(planned - table))
    assert table <= planned, ("a row of the table the planner does not emit", sorted(table - planned))


@pytest.mark.parametrize("workload", sorted(WORKLOADS))
def test_planner_against_product_table(product_ops, workload):
    variant, res, sp, passes, *norm = WORKLOADS[workload]
    net = VNet(n_channels=1, n_classes=2, normalization=norm[0] if norm else "batchnorm" if variant == "la" else "instancenorm", has_dropout=variant == "la",
               has_residual=res, variant=variant).set_ops(product_ops)
    _against_table(net, workload, sp, passes, VOCAB)


@pytest.mark.parametrize("workload", sorted(UNET_WORKLOADS))
def test_unet_planner_against_product_table(product_ops, workload):
    """the same two-directional assertion for the 2-D U-Net (ACDC): its 19 convs' routes and its concat copies -- none in the training
    workloads, four per batch in acdc_val"""
    net = UNet_2d(in_chns=1, class_num=4).set_ops(product_ops)
    _against_table(net, workload, ACDC, UNET_WORKLOADS[workload], UNET_VOCAB)
    copies = sorted(k[1][0][0] for k in P.STEP_KEYS[workload] if k[0] == "copy_channels")
    assert copies == ([1] * 4 + [16] * 4 if workload == "acdc_val" else []), copies
