"""The normalisation family's host dispatch (csrc/norm.hip, csrc/norm_res.hip, csrc/gnorm.hip), pinned on the CPU:
tools/make_golden_norm_routes.py sweeps options x (groups, rows per group, rows per sample) x channels x the flag sets of every entry point
on the HOST simulator with its launches noted and not executed, and tests/golden/norm_routes.npz holds that sweep -- the three queries'
answers and, for every call, the return code and each launch in order: kernel symbol with its template arguments, grid, block, LDS, the
scalar arguments and every pointer argument as "null" or as its byte offset from the sweep's base address (log mode 4: which buffer a launch
reads, which pass gets the |max| slots, where c1 lies in the workspace) -- as taken from the commit BEFORE the dispatch was rebuilt around
norm_problem() (one problem record), norm_route() (decide) and norm_fwd_launch() / norm_bwd_launch() (execute).

The one intended difference from that commit: bcp_norm_workspace_bytes(C = 2048) divided by zero (256 / (C / 4) thread-slots); it answers 0
now, as it does for every other C that no entry point serves below 16.  No launch record differs."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden_norm_routes as R  # noqa: E402

WHATIF = "whatif="


@pytest.fixture(scope="module")
def swept():
    lib = R.Lib(R.build_emu())
    rows, logs, names, noise = R.sweep(lib)
    return dict(rows=rows, logs=logs, names=names, noise=noise)


def _col(rows, name):
    return rows[:, R.COLUMNS.index(name)]


def _symbols(text):
    return tuple(ln.split("|")[1] for ln in text.splitlines() if ln.startswith("L|"))


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
    bad = np.argwhere(got != want)
    assert bad.size == 0, (len(bad), [(want_names[want_rows[i, 0]], want_rows[i, 1:5].tolist(), R.CALLS[j][0], want[i, j], got[i, j]) for i, j in bad[:3]])


def test_queries_launch_nothing(swept):
    """bcp_norm_workspace_bytes / bcp_norm_slabs_ok / bcp_gnorm_workspace_bytes answer from the rules of the route: no launch"""
    assert swept["noise"] == ""


def test_served_calls_launch_and_refusals_are_the_expected_ones(swept):
    """every call the sweep makes either succeeds and leaves at least one launch, or is refused without one; and the refusals are exactly
    the deliberately bad rows (tools/make_golden_norm_routes.py CALLS: a C that is no power of two in 16 .. 1024 (GroupNorm: .. 256), a
    group of 65 samples or of no whole number of them, out_ld = C + 2, 65 slabs, res_channels = 2, dres of a broadcast residual, the slab
    entry points above 4096 rows per group, ...).  Under a whatif option (a measurement switch that LEAVES launches OUT: handed-in rows
    with the finalize and the apply pass both priced away leave none) a served call launches a subsequence of what it launches by default"""
    rows, logs, names = swept["rows"], swept["logs"], swept["names"]
    launches = np.array([text.count("L|") for text in logs] + [0])
    whatif = np.array([n.startswith(WHATIF) for n in names])[_col(rows, "option")]
    cell = [tuple(r) for r in rows[:, 1:5].tolist()]
    default = {c: i for i, c in enumerate(cell) if rows[i, 0] == 0}
    for name, _, _, bad in R.CALLS:
        rc, log = _col(rows, name + "_rc"), _col(rows, name + "_log")
        made = rc != R.SKIPPED
        assert made.any() and (log[~made] == -1).all(), name
        served, refused = made & (rc == 0), made & (rc != 0)
        expected = np.array([bad(*c) for c in cell])
        assert (refused == (made & expected)).all(), name
        assert (launches[log[refused]] == 0).all() and (rc[refused] == -1).all(), name
        assert (launches[log[served & ~whatif]] >= 1).all(), name
        for (got, base), i in {(log[i], log[default[cell[i]]]): i for i in np.flatnonzero(served & whatif)}.items():
            full = iter(_symbols(logs[base]))
            assert all(s in full for s in _symbols(logs[got])), (name, names[rows[i, 0]], cell[i])
        if not name.endswith("_bad") and "_bad_" not in name:
            assert served.any(), name
    # the whatif switches do leave something out somewhere
    for o in np.flatnonzero([n.startswith(WHATIF) for n in names]):
        sub = rows[:, 0] == o
        fewer = 0
        for name, *_ in R.CALLS:
            log = _col(rows, name + "_log")[sub]
            base = np.array([_col(rows, name + "_log")[default[c]] for c, s in zip(cell, sub) if s])
            fewer += int((launches[log] < launches[base]).sum())
        assert fewer > 0, names[o]


def test_slab_entry_points_serve_exactly_where_the_open_query_says_so(swept):
    """bcp_norm_fwd_slabs / bcp_norm_bwd_slabs do not look at norm_slabs: under EVERY option they serve a good flag set exactly where
    bcp_norm_slabs_ok answers 1 with the option open (the default), and the query answers 0 everywhere with norm_slabs = 0"""
    rows, names = swept["rows"], swept["names"]
    cell = [tuple(r) for r in rows[:, 1:5].tolist()]
    ok_default = {c: int(rows[i, R.COLUMNS.index("slabs_ok")]) for i, c in enumerate(cell) if rows[i, 0] == 0}
    ok = np.array([ok_default[c] for c in cell])
    assert (ok == 1).any() and (ok == 0).any()
    closed = _col(rows, "option") == names.index("norm_slabs=0")
    assert (_col(rows, "slabs_ok")[closed] == 0).all() and (_col(rows, "slabs_ok")[~closed] == ok[~closed]).all()
    for name in ("fwds_all", "fwds_bare", "fwds_stat_run", "fwds_stat", "bwds_all", "bwds_acc", "bwds_nograd"):
        assert ((_col(rows, name + "_rc") == 0) == (ok == 1)).all(), name


def test_every_kernel_instance_of_the_family_is_reached(swept):
    """the sweep launches every k_col_partial<MODE, SL>, k_norm_own_fwd / _bwd<P>, k_norm_apply_res / k_col_partial_res /
    k_norm_bwd_apply_res / k_norm_eval_res<RB> instance the library holds: none is dead (an instance that no option can select would have to
    be named here)"""
    seen = {s for text in swept["logs"] for s in _symbols(text)}
    exported = R.exported_kernels()
    tf = ("false", "true")
    assert exported == ({f"bcp::k_col_partial<{m}, {sl}>" for m in (0, 1) for sl in tf} | {f"bcp::k_norm_own_{d}<{p}>" for d in ("fwd", "bwd") for p in (1, 2, 4)} |
                        {f"bcp::{k}<{rb}>" for k in ("k_norm_apply_res", "k_col_partial_res", "k_norm_bwd_apply_res", "k_norm_eval_res") for rb in tf})
    dead = set()
    assert exported - seen == dead
