#!/usr/bin/env python3
"""The k2s2 / transposed / 1x1 conv GEMMs' host dispatch (csrc/gemm.hip) as DATA: for a grid of (options, shape, channels, groups,
accumulate) what the row-count and workspace queries answer and what every entry point of the family launches -- symbol with its template
arguments, grid, block, LDS and the kernel's scalar arguments (M, K, N, bias_mod, accumulate / M, K, N, rpg), every launch of the call in
order -- read from the host simulator's launch log in its no-execute mode with arguments (tools/emu, log mode 3).

    python tools/make_golden_gemm_routes.py            # rewrites tests/golden/gemm_routes.npz from tests/_emu/libbcp_emu.so
    python tools/make_golden_gemm_routes.py --coverage # also lists the k_gemm_nn / k_gemm_tn instances of the library the sweep never launched

tests/test_emu_gemm_routes.py runs the same sweep (sweep() below) against the current sources and compares it with the committed file.
The plumbing (simulator build, library wrapper, packed-log layout) is tools/make_golden_conv3_routes.py's."""
import argparse
import ctypes as C
import os

import numpy as np

import make_golden_conv3_routes as R3
from make_golden_conv3_routes import ROOT, EMU, build_emu, pack as _pack3, unpack  # noqa: F401

GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_routes.npz")

# ---- the grid -------------------------------------------------------------------------------------------------------------------
AWKWARD = ((2, 2, 2), (4, 6, 8), (10, 12, 14), (8, 6, 10), (2, 4, 6), (16, 16, 12), (14, 14, 10))
ODD_EXTENT = (8, 7, 8)                      # refused by every entry point that checks its shape
BAD_CHANNELS = ((24, 32), (32, 40))         # not multiples of 16


def _shapes(batches, batches_awkward):
    """(N, D, H, W): the FINE extents of the product workloads' levels 0 .. 3, then small and awkward even ones, then one odd one.  Among
    them: M = N * D/2 * H/2 * W/2 that is no multiple of 64 * groups, and that groups does not divide (N = 1, (14, 14, 10): M = 245)"""
    out = []
    for ext in R3._levels(R3.LA, 4) + R3._levels(R3.PANCREAS, 4):
        out += [(n, *ext) for n in batches]
    for ext in AWKWARD + (ODD_EXTENT,):
        out += [(n, *ext) for n in batches_awkward]
    return list(dict.fromkeys(out))


SHAPES = _shapes((1, 2, 4, 8), (1, 2))
CHANNELS = [(16, 32), (32, 64), (64, 128), (128, 256), (32, 16), (64, 32), (128, 64), (256, 128), (16, 16)] + list(BAD_CHANNELS)
GROUPS = lambda N: tuple(dict.fromkeys((1, 2, N)))
OPTIONS = [{}] + [{k: v} for k, vs in (("k2_stats", (0, 1)), ("k2_bwd_stats", (1, 2))) for v in vs]
OPTIONS += [{"fuse_bwd_stats": 0, "k2_bwd_stats": 1}]
OPTIONS += [{k: v} for k, vs in (("up_recompute", (1, 2)), ("gemm_pipe", (0,)), ("gemm_stat_r", (1, 4, 16)), ("gemm_walk", (256, 512)),
                                 ("tn_groups", (1, 2))) for v in vs]

KERNEL_FAMILIES = ("k_gemm_nn<", "k_gemm_tn<")
WG_DOWN, WG_UP, WG_PW = 0, 1, 2             # include/bcp_hip.h
SKIPPED = -99                               # the *_rc column of a call this row does not make (BCP_EINVAL is -1)

QUERIES = ("stat_rows_down", "stat_rows_up", "bwdstat_rows_down", "bwdstat_rows_up", "up_norm_rows", "up_norm_ws", "tn_ws_down", "tn_ws_up",
           "tn_ws_pw")
# (entry point, the query column that promises it; None: a plain entry point)
CALLS = (("down_fwd", None), ("up_fwd", None), ("pw_fwd", None), ("down_fwd_stats", "stat_rows_down"), ("up_fwd_stats", "stat_rows_up"),
         ("up_fwd_norm", "up_norm_rows"), ("up_norm_bwd", "up_norm_rows"), ("down_dgrad", None), ("up_dgrad", None),
         ("down_dgrad_bwdstats", "bwdstat_rows_down"), ("up_dgrad_bwdstats", "bwdstat_rows_up"), ("wg_down", None), ("wg_up", None),
         ("wg_pw", None))
COLUMNS = ("option", "N", "D", "H", "W", "Cin", "Cout", "groups", "accumulate") + QUERIES + tuple(f"{c}_{f}" for c, _ in CALLS for f in ("rc", "log"))
K2_ENTRY_POINTS = ("bcp_down_", "bcp_up_", "bcp_pw_fwd", "bcp_k2_", "bcp_tn_")


class Lib(R3.Lib):
    """... with the k2s2 / 1x1 GEMM entry points' signatures added"""

    def __init__(self, path=EMU):
        super().__init__(path)
        from bcp_amd import _lib
        for name, (res, args) in _lib._SIGS.items():
            if name.startswith(K2_ENTRY_POINTS):
                fn = getattr(self.cdll, name)
                fn.restype, fn.argtypes = res, args


def sweep(lib, coverage=None):
    """-> (rows int64 [n, len(COLUMNS)], logs: the distinct launch records of one entry-point call ("L|symbol|grid|block|LDS" and behind
    each "P|scalar arguments"), option_names, query_noise: what the query entry points logged -- must be empty)"""
    c, p = lib.cdll, lib.ptr
    logs, log_id, rows, noise = [], {}, [], []
    prev = lib.log_mode(3)
    f32 = C.c_float

    def call(fn, *args):
        rc = fn(*args)
        text = "".join(ln + "\n" for ln in lib.take().splitlines() if ln.startswith(("L|", "P|")))
        if coverage is not None:
            coverage.update(ln.split("|")[1] for ln in text.splitlines() if ln.startswith("L|"))
        if text not in log_id:
            log_id[text] = len(logs)
            logs.append(text)
        return [rc, log_id[text]]

    skip = [SKIPPED, -1]
    try:
        for oi, opts in enumerate(OPTIONS):
            lib.set_options(opts)
            try:
                for (N, D, H, W) in SHAPES:
                    M, rows_pw = N * (D // 2) * (H // 2) * (W // 2), N * D * H * W
                    for (ci, co) in CHANNELS:
                        dims = (N, D, H, W, ci, co)
                        lib.take()
                        tn = [c.bcp_tn_workspace_bytes(M, 8 * ci, co), c.bcp_tn_workspace_bytes(M, ci, 8 * co), c.bcp_tn_workspace_bytes(rows_pw, ci, co)]
                        for gi, G in enumerate(GROUPS(N)):
                            q = [c.bcp_k2_stat_rows(0, *dims, G), c.bcp_k2_stat_rows(1, *dims, G), c.bcp_k2_bwdstat_rows(0, *dims, G),
                                 c.bcp_k2_bwdstat_rows(1, *dims, G), c.bcp_up_norm_rows(*dims, G), c.bcp_up_norm_workspace_bytes(*dims, G)] + tn
                            noise.append(lib.take())
                            for acc in (0, 1):
                                row = [oi, N, D, H, W, ci, co, G, acc] + q
                                first = gi == 0 and acc == 0          # the plain forwards know neither groups nor accumulate
                                row += call(c.bcp_down_fwd, p, p, p, p, *dims, None) if first else skip
                                row += call(c.bcp_up_fwd, p, p, p, p, *dims, None) if first else skip
                                row += call(c.bcp_pw_fwd, p, p, p, p, rows_pw, ci, co, None) if first else skip
                                row += call(c.bcp_down_fwd_stats, p, p, p, p, *dims, p, G, None) if acc == 0 else skip
                                row += call(c.bcp_up_fwd_stats, p, p, p, p, *dims, p, G, None) if acc == 0 else skip
                                row += call(c.bcp_up_fwd_norm, p, p, p, *dims, G, p, p, p, p, f32(0.1), f32(1e-5), 1, p, p, p, p, p, None) if acc == 0 else skip
                                row += call(c.bcp_up_norm_bwd, p, p, p, p, *dims, G, p, 1, p, p, acc, p, p, None)
                                row += call(c.bcp_down_dgrad, p, p, p, *dims, acc, None) if gi == 0 else skip
                                row += call(c.bcp_up_dgrad, p, p, p, *dims, acc, None) if gi == 0 else skip
                                row += call(c.bcp_down_dgrad_bwdstats, p, p, p, *dims, acc, p, p, 1, p, G, None)
                                row += call(c.bcp_up_dgrad_bwdstats, p, p, p, *dims, acc, p, p, 1, p, G, None)
                                for kind in (WG_DOWN, WG_UP, WG_PW):
                                    row += call(c.bcp_k2_wgrad, p, p, p, *dims, kind, acc, p, None) if gi == 0 else skip
                                rows.append(row)
            finally:
                lib.set_options(opts, reset=True)
    finally:
        lib.log_mode(prev)
        lib.take()
    names = [",".join(f"{k}={v}" for k, v in o.items()) or "default" for o in OPTIONS]
    return np.asarray(rows, dtype=np.int64), logs, names, "".join(noise)


def exported_kernels(path=EMU):
    return R3.exported_kernels(path, KERNEL_FAMILIES)


def pack(rows, logs, names):
    return dict(_pack3(rows, logs, names), columns=np.array(COLUMNS))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--coverage", action="store_true")
    ap.add_argument("--out", default=GOLDEN)
    ap.add_argument("--lib", default=None, help="a simulator library built elsewhere (the parent commit's, to pin a refactor against it)")
    a = ap.parse_args()
    lib = Lib(a.lib or build_emu())
    seen = set()
    rows, logs, names, noise = sweep(lib, seen)
    np.savez_compressed(a.out, **pack(rows, logs, names))
    print(f"{len(rows)} rows, {len(logs)} distinct launch logs, {os.path.getsize(a.out)} bytes -> {a.out}")
    print(f"query entry points logged {len(noise.splitlines())} records")
    if a.coverage:
        missing = sorted(exported_kernels(a.lib or EMU) - seen)
        print(f"{len(seen)} kernel symbols launched, {len(missing)} exported GEMM kernels never launched")
        for m in missing:
            print("  ", m)


if __name__ == "__main__":
    main()
