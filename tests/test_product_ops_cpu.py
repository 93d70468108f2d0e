"""Host side of tests/test_gpu_product_ops.py: the elementwise comparator's own test (no kernel), and the same drivers and fp64
references on the host simulator at the in-step shapes divided by 8."""
import pytest
import torch

import product_ops as P
from test_emu_kernels import emu_ops  # noqa: F401  (fixture)


def _exact_output(g):
    """a level-2-sized fp64 'output' (2 M elements) and a conv-like per-element bound magnitude"""
    ref = P.activation(g, (1, 56, 56, 40, 16)).double() * 10
    cond = ref.abs() + 0.1 * float(ref.abs().mean())
    return ref, cond


def test_comparator_rejects_local_errors():
    """an fp64-exact output passes; one wrong corner voxel, one tile-seam plane off by 1e-4 relative, one interior 4x8x8 brick off by
    1e-3 each fail the elementwise bound -- while a rel-L2 bound of 1e-4 accepts the last two"""
    g = torch.Generator().manual_seed(11)
    ref, cond = _exact_output(g)
    assert P.check_elementwise(ref.clone(), ref, cond, P.TAU, "exact")[0] == 0.0
    assert P.check_elementwise(ref.float(), ref, cond, P.TAU, "fp32 rounding")[0] <= 2.0 ** -23 / P.TAU
    corner = ref.clone()
    corner[0, 0, 0, 0, 0] += 1e-2 * cond[0, 0, 0, 0, 0]
    seam = ref.clone()
    seam[:, 4] *= 1 + 1e-4                          # the plane d = 4: a 4x8x8 tile border
    brick = ref.clone()
    brick[:, 20:24, 24:32, 16:24] *= 1 + 1e-3       # one interior 4x8x8 tile
    for name, bad, loc in (("corner", corner, "face"), ("seam", seam, None), ("brick", brick, None)):
        with pytest.raises(AssertionError, match=name):
            P.check_elementwise(bad, ref, cond, P.TAU, name)
        r, k = P.elementwise_ratio(bad, ref, cond)
        assert r > P.TAU
        if loc:
            import numpy as np
            assert P.where(np.unravel_index(k, tuple(ref.shape)), tuple(ref.shape)) == loc, name
    for bad in (seam, brick):
        assert P.rel_l2(bad, ref) < 1e-4, "a rel-L2 1e-4 test accepts this error (that is the gap the elementwise bound closes)"


def test_conv3_cl64_matches_torch():
    g = torch.Generator().manual_seed(12)
    x = torch.randn(2, 5, 6, 7, 3, generator=g, dtype=torch.float64)
    w = torch.randn(4, 3, 3, 3, 3, generator=g, dtype=torch.float64)
    ref = torch.nn.functional.conv3d(x.permute(0, 4, 1, 2, 3), w, padding=1).permute(0, 2, 3, 4, 1)
    assert torch.allclose(P.conv3_cl64(x, w), ref, rtol=1e-12, atol=1e-12)
    w2 = torch.randn(4, 3, 3, 3, generator=g, dtype=torch.float64)
    x2 = x[:, :1]
    ref2 = torch.nn.functional.conv2d(x2[:, 0].permute(0, 3, 1, 2), w2, padding=1).permute(0, 2, 3, 1).unsqueeze(1)
    assert torch.allclose(P.conv3_cl64(x2, w2), ref2, rtol=1e-12, atol=1e-12)
    dy = torch.randn(2, 5, 6, 7, 4, generator=g, dtype=torch.float64)
    gw = torch.nn.grad.conv3d_weight(x.permute(0, 4, 1, 2, 3), w.shape, dy.permute(0, 4, 1, 2, 3), padding=1)
    assert torch.allclose(P.conv3_wgrad64(x, dy), gw, rtol=1e-12, atol=1e-10)


def _reduced_rows():
    seen, rows = set(), []
    for wl, k in P.driven_rows():
        rk = P.reduce_key(k)
        if rk not in seen:
            seen.add(rk)
            rows.append((wl, k, rk))
    return rows


# the LA rows run in the default CPU suite; the pancreas / ACDC rows (same drivers, other shapes) with BCP_EXTENDED=1.
# At the reduced shapes the dispatch may differ from the in-step one: a conv3_fwd_raw row falls back to conv3_fwd where the shape is
# not served raw, and where a conv leaves no fused statistics (rows == 0) the fwd_stats / dgrad_bwdstats rows and the norm rows' "partial"
# epilogue run without them.  These rows check the drivers and references on the simulator; the route itself is asserted on the device
# (tests/test_gpu_product_ops.py: each row must launch its key, and the drivers require the fused routes there).
@pytest.mark.parametrize("wl,key,rkey", [pytest.param(*r, marks=() if r[0] == "la" else pytest.mark.extended) for r in _reduced_rows()],
                         ids=[P.row_id(r[0], r[1]) for r in _reduced_rows()])
def test_product_op_reduced_on_simulator(emu_ops, wl, key, rkey):  # noqa: F811
    g = torch.Generator().manual_seed(5)
    fn = P.DRIVERS[rkey[0]]
    if rkey[0] in P._VARIANT_OPS:
        fn(emu_ops, torch.device("cpu"), rkey, g, P.variants_of(wl, key))
    else:
        fn(emu_ops, torch.device("cpu"), rkey, g)
