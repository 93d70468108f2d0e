#!/usr/bin/env python3
"""The 3x3(x3) conv's WEIGHT-GRADIENT dispatch as DATA: for a grid of (options, shape, channels, |max| present or not, accumulate) what
bcp_conv3_wgrad_workspace_bytes / bcp_conv3_wgrad_path / bcp_conv3_planes(..., 1) answer and which kernel instances bcp_conv3_wgrad and
bcp_conv3_c1_wgrad launch -- symbol with its template arguments, grid, block, dynamic LDS, and the hipFuncSetAttribute calls in front --
read from the host simulator's launch log in no-execute mode (tools/emu).  The grid, the library handle and the helpers are those of
tools/make_golden_conv3_routes.py.

    python tools/make_golden_wgrad_routes.py            # rewrites tests/golden/wgrad_routes.npz from tests/_emu/libbcp_emu.so
    python tools/make_golden_wgrad_routes.py --coverage # also lists the weight-gradient kernel symbols the sweep never launched

tests/test_emu_wgrad_routes.py runs the same sweep (sweep() below) against the current sources and compares it with the committed file;
tests/wgrad_checks.py picks, from the committed file, one small row per kernel instance and runs it against fp64."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden_conv3_routes as R  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "wgrad_routes.npz")

SHAPES = R.SHAPES_SMALL
# (16, 2) stays in the grid: the entry point takes channel counts that are multiples of 4 and must refuse it without a launch
CHANNELS = R.CHANNELS_SMALL + [(1, 16)]                   # Cin = 1: the first layer, bcp_conv3_c1_wgrad

TILES = ("4,4,4", "4,4,8", "4,8,8", "2,8,4", "4,4,16")
_B6 = [(k, v) for k, vs in (("wgrad_b6_deep", (0,)), ("wgrad_b6_deep_tile", (0, 1)), ("wgrad_b6_deep_nt", (1, 2)), ("wgrad_b6_deep_slots", (16, 4096)),
                            ("wgrad_b6_slots", (64, 4096)), ("wgrad_b6_levels", (0, 3, 7, 11)), ("wgrad_b6_minvox", (1, 100000)),
                            ("wgrad_reduce_flat", (0, 2)), ("conv3_f16", (0,))) for v in vs]
_F32 = [("wgrad_nt", v) for v in (1, 2, 4)] + [("wgrad_tile", v) for v in TILES] + [("wgrad_reduce_flat", v) for v in (0, 2)]
OPTIONS = [{}, {"wgrad_b6": 0}, {"wgrad_b6": 2}]
OPTIONS += [{k: v} for k, v in _B6 + _F32[:-2]]
OPTIONS += [{"wgrad_b6": 2, k: v} for k, v in _B6]        # the matrix-pipe kernels' switches where the pipe is forced at every shape
OPTIONS += [{"wgrad_b6": 0, k: v} for k, v in _F32]       # the fp32 kernels' own where the pipe leaves them every shape
# the deep-level switches together: each tile with each slab width, as slabs (many groups) and as a direct write (one group)
OPTIONS += [{"wgrad_b6": 2, "wgrad_b6_deep_tile": t, "wgrad_b6_deep_nt": n, "wgrad_b6_deep_slots": s} for t in (0, 1) for n in (1, 2) for s in (1, 4096)]
OPTIONS += [{"wgrad_b6": 0, "wgrad_tile": t, "wgrad_nt": n} for t in TILES for n in (1, 2, 4)]

KERNEL_FAMILIES = ("k_conv3_wgrad<", "k_w6<", "k_conv3_c1_wgrad<", "k_wgrad_reduce")
SLAB_WRITERS = ("bcp::k_conv3_wgrad<", "bcp::k_w6<", "bcp::k_conv3_c1_wgrad<")
QUERIES = ("workspace_bytes", "path", "planes")
COLUMNS = ("option", "N", "D", "H", "W", "KD", "Cin", "Cout", "amax", "accumulate") + QUERIES + ("rc", "log")


def w6_args(symbol):
    """(KD, TD, TH, TW, NT, PL, DIR) of a bcp::k_w6<...> symbol"""
    a = symbol[symbol.index("<") + 1:symbol.rindex(">")].split(", ")
    return tuple(int(v) for v in a[:6]) + (a[6] == "true",)


def writes_slabs(symbol):
    return symbol.startswith(SLAB_WRITERS) and not (symbol.startswith("bcp::k_w6<") and w6_args(symbol)[6])


def sweep(lib, coverage=None):
    """-> (rows int32 [n, len(COLUMNS)], logs: the distinct launch records ("L|symbol|grid|block|dynamic LDS" lines of one entry-point
    call) the rows' log column indexes, option_names, query_noise: what the query entry points logged -- must be empty, full: the
    distinct logs with their attribute records ("A|symbol|bytes") in place, for lds_attribute_violations)"""
    c, p = lib.cdll, lib.ptr
    logs, log_id, rows, noise, full = [], {}, [], [], set()
    prev = lib.log_mode(2)
    try:
        for oi, opts in enumerate(OPTIONS):
            lib.set_options(opts)
            try:
                for (N, D, H, W, KD) in SHAPES:
                    for (ci, co) in CHANNELS:
                        dims = (N, D, H, W, ci, co, KD)
                        lib.take()
                        q = [c.bcp_conv3_wgrad_workspace_bytes(*dims), c.bcp_conv3_wgrad_path(*dims), c.bcp_conv3_planes(*dims, 1)]
                        noise.append(lib.take())
                        for amax in ((None,) if ci == 1 else (None, p)):      # the first layer's entry point takes no |max|
                            for acc in (0, 1):
                                if ci == 1:
                                    rc = c.bcp_conv3_c1_wgrad(p, p, p, N, D, H, W, KD, acc, p, None)
                                else:
                                    rc = c.bcp_conv3_wgrad(p, p, p, *dims, acc, p, amax, amax, None)
                                text = lib.take()
                                full.add(text)
                                text = "".join(ln + "\n" for ln in text.splitlines() if ln.startswith("L|"))
                                if coverage is not None:
                                    coverage.update(ln.split("|")[1] for ln in text.splitlines())
                                if text not in log_id:
                                    log_id[text] = len(logs)
                                    logs.append(text)
                                rows.append([oi, N, D, H, W, KD, ci, co, int(amax is not None), acc] + q + [rc, log_id[text]])
            finally:
                lib.set_options(opts, reset=True)
    finally:
        lib.log_mode(prev)
        lib.take()
    names = [",".join(f"{k}={v}" for k, v in o.items()) or "default" for o in OPTIONS]
    return np.asarray(rows, dtype=np.int64), logs, names, "".join(noise), sorted(full)


def pack(rows, logs, names):
    assert int(np.abs(rows).max()) < 2 ** 31                 # (the largest workspace of the grid is a few hundred MB)
    return dict(rows=np.ascontiguousarray(rows.T.astype(np.int32)), columns=np.array(COLUMNS), options=np.array(names),
                logs=np.frombuffer("\x00".join(logs).encode(), dtype=np.uint8))


def unpack(z):
    return z["rows"].T.astype(np.int64), bytes(z["logs"]).decode().split("\x00"), list(z["options"])


def parse_options(name):
    """'wgrad_b6=0,wgrad_tile=4,4,8' -> {'wgrad_b6': '0', 'wgrad_tile': '4,4,8'} (an option name carries a letter, a tile extent none)"""
    out, key = {}, None
    for part in ([] if name == "default" else name.split(",")):
        if "=" in part:
            key, v = part.split("=")
            out[key] = v
        else:
            out[key] += "," + part
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--coverage", action="store_true")
    ap.add_argument("--out", default=GOLDEN)
    ap.add_argument("--lib", default=None, help="a simulator library built elsewhere")
    a = ap.parse_args()
    lib = R.Lib(a.lib or R.build_emu())
    seen = set()
    rows, logs, names, noise, full = sweep(lib, seen)
    np.savez_compressed(a.out, **pack(rows, logs, names))
    print(f"{len(rows)} rows, {len(logs)} distinct launch logs, {os.path.getsize(a.out)} bytes -> {a.out}")
    print(f"query entry points logged {len(noise.splitlines())} records")
    for ln in R.lds_attribute_violations(full):
        print("LDS attribute missing:", ln)
    if a.coverage:
        missing = sorted(R.exported_kernels(a.lib or R.EMU, KERNEL_FAMILIES) - seen)
        print(f"{len(seen)} kernel symbols launched, {len(missing)} exported weight-gradient kernels never launched")
        for m in missing:
            print("  ", m)


if __name__ == "__main__":
    main()
