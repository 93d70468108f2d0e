"""The 2-D U-Net's planner (networks/unet.py plan_forward / plan_backward) against what runs: one pass under the spy of
tests/residual_checks.py, on the simulator and on the device -- per conv the producer, the forward norm op, the backward norm op with
':partial', whether a conv3_dgrad_bwdstats epilogue fed it, and the number of concat copies against the plan's non-direct levels."""
import numpy as np
import torch

from bcp_amd.networks.unet import DROP, FT, UNet_2d
from bcp_amd.utils import BCP_utils as BU
from residual_checks import NORM_BWD, NORM_FWD, PRODUCERS, _Spy

NCONV = 18      # block convs: each calls one forward norm op; out_conv (the 19th record) has none
# case: (extents, groups, mode, class switches, injected drop_masks + _keep_saved).  All N = 4.  train: a saving forward and its backward;
# teacher: training mode under no_grad, as the self-training step runs the EMA network; eval: model.eval() under no_grad
CASES = {
    "default": ((64, 64), 2, "train", {}, False),
    "no-fuse-c1": ((64, 64), 2, "train", {"fuse_c1": False}, False),
    "masks-keep-saved": ((64, 64), 2, "train", {}, True),
    "no-skip-in-concat": ((64, 64), 2, "train", {"skip_in_concat": False}, False),
    "slabs": ((32, 32), 1, "train", {"fuse_c1": False}, False),      # <= 4096 rows per group from e0 on: a slab route wherever the conv runs split-K
    "teacher": ((64, 64), 2, "teacher", {}, False),
    "eval": ((64, 64), 1, "eval", {}, False),
}
N = 4


def _case_net(case, dev, ops):
    hw, groups, mode, switches, masks = CASES[case]
    torch.manual_seed(7)
    net = UNet_2d(in_chns=1, class_num=4).to(dev)
    net.flatten_()
    net.use_plans = False
    for k, v in switches.items():
        setattr(net, k, v)          # (an instance attribute over the class switch)
    if masks:
        rng = np.random.default_rng(5)
        net.drop_masks = {f"d{i}": torch.from_numpy((rng.random((N, c, hw[0] >> i, hw[1] >> i)) >= p).astype(np.float32)) for i, (c, p) in enumerate(zip(FT, DROP))}
        net._keep_saved = True
    net.train(mode != "eval")
    net._groups = groups
    return net.set_ops(ops), hw, groups, mode


def planned_routes(net, plan, backward=True):
    """the planner's records in the comparison's vocabulary: per block conv [forward norm op, backward norm op (+ ':partial'), a
    conv3_dgrad_bwdstats epilogue takes this conv's backward statistics], the 19 producers, the number of concat copies"""
    bw = net.plan_backward(plan)[1] if backward else None
    routes = [[r.norm, None, False] for r in plan.layers[:NCONV]]
    for li in range(NCONV if backward else 0):
        routes[li][1] = bw[li].norm + (":partial" if bw[li].partial else "")
        routes[li][2] = bw[li + 1].rows > 0
    return routes, [r.producer for r in plan.layers], sum(not d for d in plan.direct)


def observed_routes(log):
    """the spy's log of one pass, by call order (every block conv calls one forward norm op, behind its producer if it has one of its own;
    out_conv is the conv3_fwd behind the last of them; a backward pass calls one backward norm op per block conv, in block order
    u4 .. u1, e4 .. e0 with the second conv of a block first) -> planned_routes' three values"""
    order = [2 * b + c for b in (8, 7, 6, 5, 4, 3, 2, 1, 0) for c in (1, 0)]
    routes, prods, prod, nb, copies = [], [], None, 0, 0
    for n, a, k, r in log:
        if n == "copy_channels":
            copies += 1
        elif n in NORM_FWD:
            routes.append([n, None, False])
            prods.append(prod or n)
            prod = None
        elif n in PRODUCERS and len(routes) < NCONV:
            assert prod is None, (prod, n)
            prod = n
        elif n == "conv3_fwd" and len(prods) == NCONV:
            prods.append(n)
        elif n in NORM_BWD:
            routes[order[nb]][1] = n + (":partial" if k.get("partial") is not None else "")
            nb += 1
        elif n == "conv3_dgrad_bwdstats" and r[2] > 0:
            routes[order[nb]][2] = True
    assert len(routes) == NCONV and len(prods) == NCONV + 1 and nb in (0, NCONV), (len(routes), len(prods), nb)
    return routes, prods, copies


def check_planned_equals_ran(ops, dev, case):
    spy = _Spy(ops)
    net, hw, groups, mode = _case_net(case, dev, spy)
    if dev.type == "cpu":
        BU.set_test_ops(ops)
    rng = np.random.default_rng(3)
    x = torch.from_numpy(rng.random((N, 1) + hw, dtype=np.float32)).to(dev)
    if mode == "train":
        tgt = torch.from_numpy(rng.integers(0, 4, (N,) + hw)).to(dev)
        torch.nn.functional.cross_entropy(net(x, groups=groups), tgt).backward()
    else:
        with torch.no_grad():
            net(x, groups=groups)
    ran = observed_routes(list(spy.log))
    planned = planned_routes(net, net.plan_call(N, *hw), backward=mode == "train")
    assert ran == planned, (case, [(i, r, p) for i, (r, p) in enumerate(zip(ran[0], planned[0])) if r != p], ran[1:], planned[1:])
    return ran


# every route name the cases above reach, on the simulator and on the gfx950 library alike (u4's dgrad epilogue is served at 64 x 64 and at
# 32 x 32: "norm_bwd:partial"; the levels from 16 x 16 down take the slab routes, so two concat levels copy, one in the "slabs" case).  NOT reached:
#   copies:0            every level direct needs extents at which no encoder level takes the raw-slab norm: the product size, planned against
#                       the product-op table in tests/test_plan_product.py (no copy_channels row in acdc / acdc_pre), which pins it
#   conv3_c1_norm_bwd   only with the measurement switch BCP_C1_BWD_FUSED=0
#   e0's second dgrad as raw slabs (norm_bwd_slabs on the first layer with fuse_c1 off): the rule is carried over, but bcp_conv3_fwd_nslabs
#                       answers 0 for the 16-channel conv at every extent tried (N 1..4, 8 x 8 .. 32 x 32): no extents reach it
ROUTES_REACHED = {
    "conv3_c1_norm_fwd", "conv3_c1_fwd_stats", "conv3_c1_fwd", "conv3_fwd_raw", "conv3_fwd_stats", "conv3_fwd", "norm_fwd", "norm_fwd_slabs", "norm_eval",
    "norm_bwd", "norm_bwd:partial", "norm_bwd_slabs", "conv3_c1_norm_bwd_wgrad", "conv3_dgrad_bwdstats", "copies:1", "copies:2", "copies:4"}


def routes_reached(ops):
    """the planner alone (no launch) over CASES: the set of producer / norm / dgrad names and concat-copy counts --
    check_planned_equals_ran shows case by case that these are the ops that ran"""
    names = set()
    for case in CASES:
        net, hw, groups, mode = _case_net(case, torch.device("cpu"), ops)
        plan = net.plan_call(N, *hw)
        routes, prods, copies = planned_routes(net, plan, backward=mode == "train")
        names |= set(prods) | {n for r in routes for n in r[:2] if n} | {"copies:%d" % copies}
        if mode == "train":
            names |= {b.dgrad for b in net.plan_backward(plan)[1] if b.dgrad}
    return names


def check_routes_reached(ops):
    got = routes_reached(ops)
    assert got == ROUTES_REACHED, (sorted(got - ROUTES_REACHED), sorted(ROUTES_REACHED - got))
