"""The 3x3(x3) conv's forward / dgrad dispatch, pinned on the CPU: tools/make_golden_conv3_routes.py sweeps options x shapes x channels x
groups x |max| present or not on the HOST simulator with its launches noted and not executed, and tests/golden/conv3_routes.npz holds
that sweep -- the seven query answers and, for each of the four entry points, the kernel symbol with its template arguments, grid, block
and dynamic LDS -- as taken before the dispatch was split into conv3_route() (decide) and conv3_launch() (execute).

The one intended difference from that commit: bcp_conv3_fwd_raw at the 16-channel slabs with the input's |max| given launched the
three-plane staged kernel k_c3b<.., 1, 1, false, 3> with the dynamic LDS of two planes (43520 instead of 64768 bytes at the 3-D tile) and
reported pack section 4 for a launch that reads section 2; the fixture holds the size and the section of the kernel that runs."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden_conv3_routes as R  # noqa: E402


@pytest.fixture(scope="module")
def swept():
    lib = R.Lib(R.build_emu())
    rows, logs, names, noise, full = R.sweep(lib)
    return dict(rows=rows, logs=logs, names=names, noise=noise, full=full)


def test_routes_reproduce_the_fixture(swept):
    want_rows, want_logs, want_names = R.unpack(np.load(R.GOLDEN))
    assert swept["names"] == want_names
    assert swept["rows"].shape == want_rows.shape
    log_cols = [i for i, c in enumerate(R.COLUMNS) if c.endswith("_log")]
    plain = [i for i in range(len(R.COLUMNS)) if i not in log_cols]
    bad = np.flatnonzero((swept["rows"][:, plain] != want_rows[:, plain]).any(axis=1))
    assert bad.size == 0, [dict(zip(R.COLUMNS, zip(want_rows[i].tolist(), swept["rows"][i].tolist()))) for i in bad[:3]]
    # the launch records themselves: the two sweeps number their distinct logs in order of first appearance
    got = np.array(swept["logs"] + [""], dtype=object)[swept["rows"][:, log_cols]]
    want = np.array(want_logs + [""], dtype=object)[want_rows[:, log_cols]]
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, [(want_names[want_rows[i, 0]], want_rows[i, 1:10].tolist(), want[i].tolist(), got[i].tolist()) for i in bad[:3]]


def test_the_sweep_launches_something_everywhere(swept):
    """every entry-point call of the sweep succeeded and left at least one launch record (a fixture of empty logs would pin nothing)"""
    rows = swept["rows"]
    for c in R.CALLS:
        rc, log = rows[:, R.COLUMNS.index(c + "_rc")], rows[:, R.COLUMNS.index(c + "_log")]
        made = log >= 0
        assert made.any(), c
        served = made & (rc == 0)
        assert all(swept["logs"][i].startswith("L|") for i in np.unique(log[served])), c
        # the only refusals: a forced streaming tile (conv3_cfg) without an instance for the shape's KD
        assert all("conv3_cfg" in swept["names"][o] for o in np.unique(rows[made & (rc != 0), 0])), c


def test_queries_launch_nothing(swept):
    """bcp_conv3_stat_rows / _fwd_nslabs / _bwdstat_rows / _fwd_path / _planes / _fwd_workspace_bytes answer from the route: no launch and
    no HIP runtime call (the launcher run dry used to call hipFuncSetAttribute)"""
    assert swept["noise"] == ""


def test_large_lds_launches_carry_their_attribute(swept):
    """a launch with more than 48 KB of dynamic LDS fails unless hipFuncSetAttribute raised the limit of THAT kernel to at least that size"""
    assert any(int(ln.split("|")[4]) > 48 * 1024 for text in swept["full"] for ln in text.splitlines() if ln.startswith("L|"))
    assert R.lds_attribute_violations(swept["full"]) == []


def test_every_conv_forward_kernel_is_reached_or_known_dead(swept):
    """the sweep launches every conv forward kernel instance the library holds, but for those no option can select: the resident kernel's
    one-MFMA-tile-per-wave instances (choose_res leaves them to the streaming kernel) and the one-tile-per-workgroup form of the
    16-channel-slab k_c3d (16-channel slabs are persistent; raw slabs take the staged kernel)"""
    seen = {ln.split("|")[1] for text in swept["logs"] for ln in text.splitlines()}
    dead = {"bcp::k_conv3_res<1, 1, 8, 8, 1>", "bcp::k_conv3_res<3, 4, 4, 4, 1>",
            "bcp::k_c3d<1, 1, 16, 16, 1, false, false, 2, false>", "bcp::k_c3d<1, 1, 16, 16, 1, false, false, 3, false>",
            "bcp::k_c3d<3, 4, 8, 8, 1, false, false, 2, false>", "bcp::k_c3d<3, 4, 8, 8, 1, false, false, 3, false>"}
    assert R.exported_kernels() - seen == dead
