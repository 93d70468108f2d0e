"""The k2s2 / transposed / 1x1 conv GEMMs' host dispatch (csrc/gemm.hip), pinned on the CPU: tools/make_golden_gemm_routes.py sweeps options
x shapes x channels x groups x accumulate on the HOST simulator with its launches noted and not executed, and tests/golden/gemm_routes.npz
holds that sweep -- the row-count and workspace answers and, for every entry point of the family, the return code and each launch of the
call in order: kernel symbol with its template arguments, grid, block, LDS and the scalar arguments M, K, N, bias_mod, accumulate (k_gemm_nn)
/ M, K, N, rpg (k_gemm_tn) -- as taken from the commit BEFORE the dispatch was rebuilt around k2_problem() (one problem record),
gemm_route() / tn_route() (decide) and nn_launch() / tn_launch() (execute).  No record of the fixture differs at the refactored code."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden_gemm_routes as R  # noqa: E402


@pytest.fixture(scope="module")
def swept():
    lib = R.Lib(R.build_emu())
    rows, logs, names, noise = R.sweep(lib)
    return dict(rows=rows, logs=logs, names=names, noise=noise)


def _col(rows, name):
    return rows[:, R.COLUMNS.index(name)]


def test_routes_reproduce_the_fixture(swept):
    want_rows, want_logs, want_names = R.unpack(np.load(R.GOLDEN))
    assert swept["names"] == want_names
    assert swept["rows"].shape == want_rows.shape
    log_cols = [i for i, c in enumerate(R.COLUMNS) if c.endswith("_log")]
    plain = [i for i in range(len(R.COLUMNS)) if i not in log_cols]
    bad = np.flatnonzero((swept["rows"][:, plain] != want_rows[:, plain]).any(axis=1))
    assert bad.size == 0, (bad.size, [dict(zip(R.COLUMNS, zip(want_rows[i].tolist(), swept["rows"][i].tolist()))) for i in bad[:3]])
    # the launch records themselves: the two sweeps number their distinct logs in order of first appearance
    got = np.array(swept["logs"] + [""], dtype=object)[swept["rows"][:, log_cols]]
    want = np.array(want_logs + [""], dtype=object)[want_rows[:, log_cols]]
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (bad.size, [(want_names[want_rows[i, 0]], want_rows[i, 1:9].tolist(), want[i].tolist(), got[i].tolist()) for i in bad[:3]])


def test_queries_launch_nothing(swept):
    """bcp_k2_stat_rows / bcp_k2_bwdstat_rows / bcp_up_norm_rows / bcp_up_norm_workspace_bytes / bcp_tn_workspace_bytes answer from the
    route: no launch and no HIP runtime call"""
    assert swept["noise"] == ""


def test_served_calls_launch_and_refusals_are_the_expected_ones(swept):
    """every call the sweep makes either succeeds and leaves at least one launch, or is refused without one; and the only refusals are the
    deliberately bad shapes (an odd extent, channels that are no multiple of 16) and a statistics / recompute entry point called where its
    query answers 0 -- which in turn never refuses where the query promised rows"""
    rows = swept["rows"]
    launches = np.array([text.count("L|") for text in swept["logs"]] + [0])
    odd = ((_col(rows, "D") | _col(rows, "H") | _col(rows, "W")) & 1) != 0
    bad_ch = (_col(rows, "Cin") % 16 != 0) | (_col(rows, "Cout") % 16 != 0)
    for c, query in R.CALLS:
        rc, log = _col(rows, c + "_rc"), _col(rows, c + "_log")
        made = rc != R.SKIPPED
        assert made.any() and (log[~made] == -1).all(), c
        served, refused = made & (rc == 0), made & (rc != 0)
        assert served.any() and refused.any(), c
        assert (launches[log[served]] >= 1).all(), c
        assert (launches[log[refused]] == 0).all() and (rc[refused] == -1).all(), c
        # bcp_k2_wgrad's k2 kinds do not look at the extents' parity (their M rounds down); everyone else refuses an odd extent
        bad_shape = bad_ch if c.startswith("wg_") else (bad_ch if c == "pw_fwd" else bad_ch | odd)
        if query is None:
            assert (refused == (made & bad_shape)).all(), c
        else:
            q = _col(rows, query)
            assert not (refused & ~bad_shape & (q > 0)).any(), c
            assert (bad_shape[made] <= refused[made]).all(), c
            if c in ("up_fwd_norm", "up_norm_bwd"):               # these two ask the query themselves: served exactly where it answers rows
                assert (served == (made & (q > 0))).all(), c
    # the shapes the statistics epilogues cannot serve are in the sweep: M that no 64 * groups divides, and M that groups does not divide
    M = _col(rows, "N") * (_col(rows, "D") // 2) * (_col(rows, "H") // 2) * (_col(rows, "W") // 2)
    G = _col(rows, "groups")
    ok = ~odd & ~bad_ch
    assert (ok & (M % G != 0)).any() and (ok & (M % G == 0) & (M % (64 * G) != 0)).any()
    for c in ("down_fwd_stats", "up_fwd_stats", "down_dgrad_bwdstats", "up_dgrad_bwdstats"):
        made = _col(rows, c + "_rc") != R.SKIPPED
        assert (_col(rows, c + "_rc")[made & ok & (M % (64 * G) != 0)] == -1).all(), c


def test_statistics_entry_points_serve_exactly_what_the_ungated_query_promises(swept):
    """bcp_down_fwd_stats / bcp_up_fwd_stats / bcp_*_dgrad_bwdstats do not look at k2_stats / k2_bwd_stats / fuse_bwd_stats: under EVERY
    option they serve exactly the rows for which the query answers more than 0 where its option gate is open everywhere (k2_stats = 1,
    k2_bwd_stats = 1) -- and refuse all others, the bad shapes among them"""
    rows, names = swept["rows"], swept["names"]
    n_opt = len(names)
    per = rows.reshape(n_opt, -1, rows.shape[1])                  # every option sweeps the same grid in the same order
    assert (per[:, :, 1:9] == per[:1, :, 1:9]).all()
    for c, query, ungated in (("down_fwd_stats", "stat_rows_down", "k2_stats=1"), ("up_fwd_stats", "stat_rows_up", "k2_stats=1"),
                              ("down_dgrad_bwdstats", "bwdstat_rows_down", "k2_bwd_stats=1"), ("up_dgrad_bwdstats", "bwdstat_rows_up", "k2_bwd_stats=1")):
        rc, q = per[:, :, R.COLUMNS.index(c + "_rc")], per[names.index(ungated), :, R.COLUMNS.index(query)]
        made = rc[0] != R.SKIPPED
        assert (q[made] > 0).any() and (q[made] == 0).any(), c
        for o in range(n_opt):
            assert ((rc[o] != R.SKIPPED) == made).all() and ((rc[o][made] == 0) == (q[made] > 0)).all(), (c, names[o])


def test_the_finalize_and_reduce_launches_are_in_the_records(swept):
    """bcp_up_fwd_norm / bcp_up_norm_bwd: statistics GEMM, the norm's finalize, apply GEMM; bcp_k2_wgrad: k_gemm_tn, then k_tn_reduce"""
    rows, logs = swept["rows"], swept["logs"]

    def symbols(c):
        rc, log = _col(rows, c + "_rc"), _col(rows, c + "_log")
        return {tuple(ln.split("|")[1].split("<")[0] for ln in logs[i].splitlines() if ln.startswith("L|")) for i in np.unique(log[rc == 0])}

    assert symbols("up_fwd_norm") == {("bcp::k_gemm_nn", "bcp::k_norm_finalize", "bcp::k_norm_running_only", "bcp::k_gemm_nn")}
    assert symbols("up_norm_bwd") == {("bcp::k_gemm_nn", "bcp::k_norm_bwd_finalize", "bcp::k_norm_bwd_params", "bcp::k_gemm_nn")}
    for c in ("wg_down", "wg_up", "wg_pw"):
        assert symbols(c) == {("bcp::k_gemm_tn", "bcp::k_tn_reduce")}, c


def test_every_gemm_kernel_instance_is_reached(swept):
    """the sweep launches all 24 k_gemm_nn<NT, MODE> (NT 1, 2, 4 x modes 0 .. 7) and all 3 k_gemm_tn<NT> instances the library holds: none is
    dead (an instance that no option can select would have to be named here)"""
    seen = {ln.split("|")[1] for text in swept["logs"] for ln in text.splitlines() if ln.startswith("L|")}
    exported = R.exported_kernels()
    assert exported == {f"bcp::k_gemm_nn<{nt}, {mode}>" for nt in (1, 2, 4) for mode in range(8)} | {f"bcp::k_gemm_tn<{nt}>" for nt in (1, 2, 4)}
    dead = set()
    assert exported - seen == dead
