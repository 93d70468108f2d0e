"""The 3x3(x3) conv's weight-gradient dispatch, pinned on the CPU: tools/make_golden_wgrad_routes.py sweeps options x shapes x channels x
|max| present or not x accumulate on the HOST simulator with its launches noted and not executed, and tests/golden/wgrad_routes.npz
holds that sweep -- the three query answers and the launch records of bcp_conv3_wgrad / bcp_conv3_c1_wgrad: kernel symbol with its
template arguments, grid, block and dynamic LDS.  Beyond reproducing the file, the tests derive from the records what the queries
promise: the workspace is large enough for the slabs the launch writes, bcp_conv3_planes names the planes of the instance that runs,
and every weight-gradient kernel instance the library holds is reached (tests/wgrad_checks.py then runs each against fp64)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden_conv3_routes as R  # noqa: E402
import make_golden_wgrad_routes as G  # noqa: E402

COL = {c: i for i, c in enumerate(G.COLUMNS)}


@pytest.fixture(scope="module")
def swept():
    lib = R.Lib(R.build_emu())
    rows, logs, names, noise, full = G.sweep(lib)
    return dict(rows=rows, logs=logs, names=names, noise=noise, full=full)


def _launches(text):
    """[(symbol, (gx, gy, gz), dynamic LDS)] of one launch log"""
    return [(f[1], tuple(int(v) for v in f[2].split(",")), int(f[4])) for f in (ln.split("|") for ln in text.splitlines())]


def test_routes_reproduce_the_fixture(swept):
    want_rows, want_logs, want_names = G.unpack(np.load(G.GOLDEN))
    assert swept["names"] == want_names
    assert swept["rows"].shape == want_rows.shape
    plain = [i for i, c in enumerate(G.COLUMNS) if c != "log"]
    bad = np.flatnonzero((swept["rows"][:, plain] != want_rows[:, plain]).any(axis=1))
    assert bad.size == 0, [dict(zip(G.COLUMNS, zip(want_rows[i].tolist(), swept["rows"][i].tolist()))) for i in bad[:3]]
    got = np.array(swept["logs"], dtype=object)[swept["rows"][:, COL["log"]]]
    want = np.array(want_logs, dtype=object)[want_rows[:, COL["log"]]]
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(want_names[want_rows[i, 0]], want_rows[i, 1:10].tolist(), want[i], got[i]) for i in bad[:3]]


def test_queries_launch_nothing(swept):
    """bcp_conv3_wgrad_workspace_bytes / _wgrad_path / _planes answer from the shape and the options: no launch, no HIP runtime call"""
    assert swept["noise"] == ""


def test_large_lds_launches_carry_their_attribute(swept):
    """a launch with more than 48 KB of dynamic LDS fails unless hipFuncSetAttribute raised the limit of THAT kernel to at least that size"""
    assert any(int(ln.split("|")[4]) > 48 * 1024 for text in swept["full"] for ln in text.splitlines() if ln.startswith("L|"))
    assert R.lds_attribute_violations(swept["full"]) == []


def test_every_call_serves_or_is_an_expected_refusal(swept):
    """a served call leaves at least one launch record, a refused one none.  The only refusals: channel counts the entry point does not
    take (multiples of 4: the grid's 16 -> 2), and a forced fp32 tile (wgrad_tile) without an instance for the shape's KD -- the
    instances are 4x4x4 / 4x4x8 / 4x8x8 / 2x8x4 / 4x4x16 for KD = 3 and 8x8 / 16x16 for KD = 1, so every tile of the sweep on a 2-D
    shape -- where the matrix pipe (conv3bw.hip) does not take the shape before the tile is looked at"""
    rows, logs, names = swept["rows"], swept["logs"], swept["names"]
    rc, empty = rows[:, COL["rc"]], np.array([t == "" for t in logs])[rows[:, COL["log"]]]
    assert ((rc != 0) == empty).all()
    assert (rc == 0).any() and (rc != 0).any()
    bad_channels = rows[:, COL["Cout"]] % 4 != 0
    assert bad_channels.any() and (rc[bad_channels] != 0).all()
    tile_forced = np.array(["wgrad_tile" in n for n in names])[rows[:, 0]]
    other = (rc != 0) & ~bad_channels
    assert other.any() and (tile_forced[other] & (rows[other, COL["KD"]] == 1) & (rows[other, COL["path"]] == 0)).all()
    # ... and every 2-D shape the fp32 kernels get under a forced 3-D tile is refused: none runs a tile it was not asked for
    assert (rc[tile_forced & (rows[:, COL["KD"]] == 1) & (rows[:, COL["path"]] == 0) & (rows[:, COL["Cin"]] > 1)] != 0).all()


def test_workspace_holds_every_slab_the_launch_writes(swept):
    """derived from the log: a slab-writing launch (every k_conv3_wgrad, k_conv3_c1_wgrad, and k_w6 without DIR) writes gridDim.x slabs of
    [KD * 9][Cin16][Cout16] floats ([KD * 9][16] at the first layer) at the front of the workspace: bcp_conv3_wgrad_workspace_bytes must
    cover them.  A direct-write launch needs none, and nothing reads slabs after it (no reduce launch follows)"""
    rows, logs = swept["rows"], swept["logs"]
    parsed = [_launches(t) for t in logs]
    n_slab = n_direct = 0
    for r in rows[rows[:, COL["rc"]] == 0]:
        ls = parsed[r[COL["log"]]]
        ci, co, KD = (int(r[COL[c]]) for c in ("Cin", "Cout", "KD"))
        slab = KD * 9 * (16 if ci == 1 else (-(-ci // 16) * 16) * (-(-co // 16) * 16)) * 4
        writers = [l for l in ls if G.writes_slabs(l[0])]
        if writers:
            assert len(writers) == 1 and len(ls) == 2 and ls[1][0].startswith("bcp::k_wgrad_reduce"), ls
            assert writers[0][1][0] * slab <= r[COL["workspace_bytes"]], (swept["names"][r[0]], r.tolist(), ls)
            n_slab += 1
        else:
            assert len(ls) == 1 and G.w6_args(ls[0][0])[6], ls
            n_direct += 1
    assert n_slab and n_direct


def test_planes_query_names_the_instance_that_runs(swept):
    """bcp_conv3_planes(..., 1) answers for a launch that carries both operands' |max|: it is the PL template argument of the k_w6
    instance such a launch runs, and 0 exactly where no k_w6 runs (bcp_conv3_wgrad_path: 1 exactly there).  Without the maxima the same
    shapes run the three-plane instance of the same tile"""
    rows, logs = swept["rows"], swept["logs"]
    n = 0
    for r in rows[(rows[:, COL["rc"]] == 0) & (rows[:, COL["Cin"]] > 1)]:
        w6 = [G.w6_args(ln.split("|")[1]) for ln in logs[r[COL["log"]]].splitlines() if ln.split("|")[1].startswith("bcp::k_w6<")]
        assert len(w6) == (1 if r[COL["path"]] else 0), r.tolist()
        assert (r[COL["planes"]] != 0) == bool(w6), r.tolist()
        if w6:
            assert w6[0][5] == (r[COL["planes"]] if r[COL["amax"]] else 3), (swept["names"][r[0]], r.tolist(), w6)
            n += 1
    assert n


def test_every_wgrad_kernel_is_reached_or_known_dead(swept):
    """census: every exported k_conv3_wgrad / k_w6 / k_conv3_c1_wgrad / k_wgrad_reduce* instance is launched somewhere in the sweep.  In
    particular the deep-level measurement switches select the instances they name: wgrad_b6_deep_tile = 0 the 2x8x4 tiles
    (k_w6<3, 2, 8, 4, ...> with and without DIR; 1, the 4x8x4 tiles, is the default), wgrad_b6_deep_nt = 2 the 32-channel slabs
    (k_w6<3, ., 8, 4, 2, ., true> with one tile group).  Nothing is dead: an instance that stops being reachable has to be listed here
    with its reason, or removed"""
    seen = {ln.split("|")[1] for text in swept["logs"] for ln in text.splitlines()}
    dead = {}                                                   # symbol -> one-line reason
    assert R.exported_kernels(families=G.KERNEL_FAMILIES) - seen == set(dead)
    names = swept["names"]
    by_opt = {}
    for r in swept["rows"]:
        by_opt.setdefault(names[r[0]], set()).update(ln.split("|")[1] for ln in swept["logs"][r[COL["log"]]].splitlines())
    assert any(s.startswith("bcp::k_w6<3, 2, 8, 4, 1, 2, true>") for s in by_opt["wgrad_b6=2,wgrad_b6_deep_tile=0"])
    assert not any(s.startswith("bcp::k_w6<3, 2, 8, 4, 1, 2, true>") for s in by_opt["wgrad_b6=2,wgrad_b6_deep_tile=1"])
    nt2 = "wgrad_b6=2,wgrad_b6_deep_tile=1,wgrad_b6_deep_nt=2,wgrad_b6_deep_slots=1"
    assert "bcp::k_w6<3, 4, 8, 4, 2, 2, true>" in by_opt[nt2] and "bcp::k_w6<3, 4, 8, 4, 2, 2, true>" not in by_opt[nt2.replace("nt=2", "nt=1")]
