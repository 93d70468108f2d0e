#!/usr/bin/env python3
"""The 3x3(x3) conv's forward / dgrad dispatch as DATA: for a grid of (options, shape, channels, groups, |max| present or not) what the
shape queries answer and which kernel instances the four entry points launch -- symbol with its template arguments, grid, block, dynamic
LDS, and the hipFuncSetAttribute calls in front -- read from the host simulator's launch log in no-execute mode (tools/emu).

    python tools/make_golden_conv3_routes.py            # rewrites tests/golden/conv3_routes.npz from tests/_emu/libbcp_emu.so
    python tools/make_golden_conv3_routes.py --coverage # also lists the conv forward kernel symbols of the library the sweep never launched

tests/test_emu_conv3_routes.py runs the same sweep (sweep() below) against the current sources and compares it with the committed file:
a change of the dispatch that moves any answer or any launch shows up there, on the CPU."""
import argparse
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EMU = os.path.join(ROOT, "tests", "_emu", "libbcp_emu.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "conv3_routes.npz")

# ---- the grid -------------------------------------------------------------------------------------------------------------------
LA, PANCREAS, ACDC = (112, 112, 80), (96, 96, 96), (256, 256)      # tests/test_plan_product.py


def _levels(extent, n=5):
    return [tuple(e >> k for e in extent) for k in range(n)]


def _shapes(batches3, batches2, batches_awkward):
    """(N, D, H, W, KD): the product workloads' level extents at their batches, then small and awkward ones"""
    out = []
    for ext in _levels(LA) + _levels(PANCREAS):
        out += [(n, *ext, 3) for n in batches3]
    for ext in _levels(ACDC):
        out += [(n, 1, *ext, 1) for n in batches2]
    for ext in ((5, 9, 7), (6, 6, 6), (5, 9, 17), (8, 12, 20), (3, 3, 3), (16, 16, 12), (40, 40, 36)):
        out += [(n, *ext, 3) for n in batches_awkward]
    for ext in ((8, 8), (24, 40), (9, 13), (16, 20), (100, 100)):
        out += [(n, 1, *ext, 1) for n in batches_awkward]
    return list(dict.fromkeys(out))


# the whole grid for the default options and the two settings of conv3_b6 that move every shape (off / forced everywhere) ...
SHAPES = _shapes((1, 2, 4), (1, 6, 12, 16), (1, 2))
CHANNELS = [(ci, co) for ci in (16, 32, 64, 128, 256) for co in (16, 32, 64, 128, 256)] + [(16, 2), (16, 4), (32, 2), (48, 48), (4, 16), (20, 36)]
GROUPS = lambda N: dict.fromkeys((1, 2, N))
FULL = [{}, {"conv3_b6": 0}, {"conv3_b6": 3}]
# ... and a smaller one for each other option alone: every level once at the training step's batch, the awkward extents, groups 1 and 2
SHAPES_SMALL = _shapes((2,), (12,), (2,))
CHANNELS_SMALL = [(16, 16), (32, 16), (32, 32), (64, 32), (64, 64), (128, 64), (128, 128), (256, 256), (16, 2), (16, 4), (48, 48)]
GROUPS_SMALL = lambda N: (1, 2)

OPTIONS = FULL + [{k: v} for k, vs in (
    ("conv3_b6", (2,)), ("conv3_f16", (0,)), ("splitk", (2,)), ("conv3_b6_flat_sk", (1, 2, 8)), ("c3d32_form", (0,)), ("c3d16_form", (0,)),
    ("conv3_b6_pipe", (0,)), ("conv3_b6_w22", (0,)), ("conv3_b6_direct", (0, 2)), ("conv3_b6_flat", (0, 2, 3, 4)), ("conv3_b6_cfg2d", (0, 2)),
    ("fuse_bwd_stats", (0, 2)), ("conv3_p", (3,)), ("res_nt", (1, 2)), ("res_pcu", (1, 2)), ("conv3_cfg", ("4,4,4,2",)),
    ("conv3_sk_elems", (4096,)), ("conv3_xcd", (0,)), ("conv3_b6_levels", (0, 7)), ("conv3_b6_minvox", (100000,)), ("conv3_b6_cin16max", (16,)))
    for v in vs]
# the fp32 kernels' own switches act only where the bf16 pipe leaves them the shape (and conv3_cfg only where the streaming kernel runs) ...
OPTIONS += [{"conv3_b6": 0, k: v} for k, v in (
    ("splitk", 2), ("conv3_p", 3), ("res_nt", 1), ("res_nt", 2), ("res_pcu", 1), ("res_pcu", 2), ("conv3_sk_elems", 4096), ("res_tile2d_vox", 1 << 30))]
OPTIONS += [{"conv3_b6": 0, "conv3_cfg": v} for v in ("4,4,4,2", "4,8,8,1", "4,8,8,2", "2,16,2,4", "8,8,1,2", "8,8,1,4", "4,4,16,1", "4,4,16,4", "2,8,4,1",
                                                      "2,8,4,2", "2,8,4,4", "1,16,16,2", "1,8,8,2", "1,8,8,4")]
# ... and the bf16-pipe kernels' where the pipe is forced at every shape, so that each staged / direct / pipelined twin meets split-K and raw mode
OPTIONS += [{"conv3_b6": 3, k: v} for k, v in (
    ("conv3_b6_direct", 0), ("conv3_b6_direct", 2), ("conv3_b6_pipe", 0), ("conv3_b6_w22", 0), ("conv3_f16", 0), ("conv3_p", 3), ("splitk", 2),
    ("c3d16_form", 0), ("c3d32_form", 0), ("fuse_bwd_stats", 2), ("conv3_b6_cfg2d", 0), ("conv3_b6_cfg2d", 2), ("conv3_b6_flat", 0))]
OPTIONS += [{"conv3_b6": 3, "conv3_b6_direct": 2, "conv3_f16": 0}, {"conv3_b6": 3, "conv3_b6_direct": 2, "splitk": 2},
            {"conv3_b6": 3, "conv3_b6_direct": 0, "splitk": 2}, {"conv3_b6": 3, "conv3_b6_pipe": 0, "splitk": 2},
            {"conv3_b6_pipe": 0, "conv3_b6_flat": 2}, {"conv3_b6_pipe": 0, "conv3_b6_flat": 3}, {"conv3_b6_pipe": 0, "conv3_b6_flat": 4}]

KERNEL_FAMILIES = ("k_conv3_mfma<", "k_conv3_res<", "k_c3b<", "k_c3h<", "k_c3p<", "k_c3d<", "k_c3f<", "k_c3q<")


# ---- the library ----------------------------------------------------------------------------------------------------------------
def build_emu():
    srcs = [os.path.join(ROOT, "bcp_amd", "csrc", f) for f in os.listdir(os.path.join(ROOT, "bcp_amd", "csrc")) if f.endswith((".hip", ".h", ".inc"))]
    srcs += [os.path.join(ROOT, "tools", "emu", "emu_runtime.cpp"), os.path.join(ROOT, "tools", "emu", "hip", "hip_runtime.h")]
    if not os.path.exists(EMU) or any(os.path.getmtime(s) > os.path.getmtime(EMU) for s in srcs):
        subprocess.check_call([os.path.join(ROOT, "tools", "emu", "build_emu.sh")])
    return EMU


class Lib:
    """the simulator library's conv3 entry points with the launch log switched to note-and-do-not-execute"""

    def __init__(self, path=EMU):
        from bcp_amd import _lib
        self.cdll = C.CDLL(path)
        for name, (res, args) in _lib._SIGS.items():
            if name.startswith("bcp_conv3_") or name == "bcp_set_option":
                fn = getattr(self.cdll, name)
                fn.restype, fn.argtypes = res, args
        self.cdll.bcpemu_log_mode.restype, self.cdll.bcpemu_log_mode.argtypes = C.c_int, [C.c_int]
        self.cdll.bcpemu_log_take.restype, self.cdll.bcpemu_log_take.argtypes = C.c_long, [C.c_char_p, C.c_long]
        self._buf = C.create_string_buffer(1 << 16)
        self._mem = C.create_string_buffer(256)                      # "any non-null 16-byte-aligned buffer": nothing reads or writes it
        self.ptr = (C.addressof(self._mem) + 63) & ~63

    def log_mode(self, mode):
        return self.cdll.bcpemu_log_mode(mode)

    def take(self):
        need = self.cdll.bcpemu_log_take(self._buf, len(self._buf))
        if need > len(self._buf):
            self._buf = C.create_string_buffer(2 * need)
            self.cdll.bcpemu_log_take(self._buf, len(self._buf))
        return self._buf.value.decode()

    def set_options(self, opts, reset=False):
        for k, v in opts.items():
            assert self.cdll.bcp_set_option(k.encode(), b"" if reset else str(v).encode()) == 0, k


QUERIES = ("stat_rows_nows", "stat_rows_ws", "fwd_nslabs", "bwdstat_rows", "fwd_path", "planes", "workspace_bytes")
CALLS = ("fwd_ws", "fwd_nows", "fwd_stats_ws", "fwd_stats_nows", "fwd_raw", "dgrad_bwdstats")
COLUMNS = ("option", "N", "D", "H", "W", "KD", "Cin", "Cout", "groups", "amax") + QUERIES + tuple(f"{c}_{f}" for c in CALLS for f in ("rc", "log", "section"))


def sweep(lib, coverage=None):
    """-> (rows int32 [n, len(COLUMNS)], logs: the distinct launch records ("L|symbol|grid|block|dynamic LDS" lines of one entry-point call)
    the rows' *_log columns index, option_names, query_noise: what the query entry points logged -- must be empty, full: the distinct
    logs with their attribute records ("A|symbol|bytes") in place, for lds_attribute_violations)"""
    c, p = lib.cdll, lib.ptr
    logs, log_id, rows, noise, full = [], {}, [], [], set()
    prev = lib.log_mode(2)

    def call(fn, *args):
        rc = fn(*args)
        text = lib.take()
        full.add(text)
        text = "".join(ln + "\n" for ln in text.splitlines() if ln.startswith("L|"))
        if coverage is not None:
            coverage.update(ln.split("|")[1] for ln in text.splitlines() if ln.startswith("L|"))
        if text not in log_id:
            log_id[text] = len(logs)
            logs.append(text)
        return [rc, log_id[text], c.bcp_conv3_last_section()]

    skip = [-1, -1, -1]
    try:
        for oi, opts in enumerate(OPTIONS):
            lib.set_options(opts)
            small = opts not in FULL
            try:
                for (N, D, H, W, KD) in (SHAPES_SMALL if small else SHAPES):
                    for (ci, co) in (CHANNELS_SMALL if small else CHANNELS):
                        dims = (N, D, H, W, ci, co, KD)
                        lib.take()
                        nslabs, path, planes = c.bcp_conv3_fwd_nslabs(*dims), c.bcp_conv3_fwd_path(*dims), c.bcp_conv3_planes(*dims, 0)
                        wsb = c.bcp_conv3_fwd_workspace_bytes(*dims)
                        ws = p if wsb else None
                        for G in (GROUPS_SMALL if small else GROUPS)(N):
                            r0, r1, rb = c.bcp_conv3_stat_rows(*dims, G, 0), c.bcp_conv3_stat_rows(*dims, G, 1), c.bcp_conv3_bwdstat_rows(*dims, G)
                            noise.append(lib.take())
                            for amax in (None, p):
                                row = [oi, N, D, H, W, KD, ci, co, G, int(amax is not None), r0, r1, nslabs, rb, path, planes, wsb]
                                if G == 1:                      # the plain and the raw launch know no groups
                                    row += call(c.bcp_conv3_fwd, p, p, p, p, *dims, 0, ws, amax, None)
                                    row += call(c.bcp_conv3_fwd, p, p, p, p, *dims, 0, None, amax, None) if ws else skip
                                else:
                                    row += skip + skip
                                row += call(c.bcp_conv3_fwd_stats, p, p, p, p, *dims, ws, p, G, amax, None) if (r1 if ws else r0) > 0 else skip
                                row += call(c.bcp_conv3_fwd_stats, p, p, p, p, *dims, None, p, G, amax, None) if ws and r0 > 0 else skip
                                row += call(c.bcp_conv3_fwd_raw, p, p, p, nslabs, *dims, amax, None) if G == 1 and nslabs > 0 else skip
                                row += call(c.bcp_conv3_dgrad_bwdstats, p, p, p, *dims, p, p, 1, ws, p, G, amax, None) if rb > 0 else skip
                                rows.append(row)
            finally:
                lib.set_options(opts, reset=True)
    finally:
        lib.log_mode(prev)
        lib.take()
    names = [",".join(f"{k}={v}" for k, v in o.items()) or "default" for o in OPTIONS]
    return np.asarray(rows, dtype=np.int32), logs, names, "".join(noise), sorted(full)


def lds_attribute_violations(logs):
    """launch records with more than 48 KB of dynamic LDS that no attribute record for the same symbol, with a value at least as large,
    precedes within the same entry-point call"""
    bad = []
    for text in logs:
        granted = {}
        for ln in text.splitlines():
            f = ln.split("|")
            if f[0] == "A":
                granted[f[1]] = max(granted.get(f[1], 0), int(f[2]))
            elif int(f[4]) > 48 * 1024 and granted.get(f[1], 0) < int(f[4]):
                bad.append(ln)
    return sorted(set(bad))


def exported_kernels(path=EMU, families=KERNEL_FAMILIES):
    out = subprocess.run(["nm", "-D", "-C", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    syms = set()
    for ln in out.splitlines():
        name = ln.split(" ", 2)[2]
        name = name[5:] if name.startswith("void ") else name
        name = name.split("(")[0]
        if name.startswith("bcp::") and name[5:].startswith(families):
            syms.add(name)
    return syms


def pack(rows, logs, names):
    return dict(rows=np.ascontiguousarray(rows.T),       # column-major: compresses to a third
                 columns=np.array(COLUMNS), options=np.array(names),
                logs=np.frombuffer("\x00".join(logs).encode(), dtype=np.uint8))


def unpack(z):
    return z["rows"].T, bytes(z["logs"]).decode().split("\x00"), list(z["options"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--coverage", action="store_true")
    ap.add_argument("--out", default=GOLDEN)
    ap.add_argument("--lib", default=None, help="a simulator library built elsewhere (the parent commit's, to pin a refactor against it)")
    a = ap.parse_args()
    lib = Lib(a.lib or build_emu())
    seen = set()
    rows, logs, names, noise, full = sweep(lib, seen)
    np.savez_compressed(a.out, **pack(rows, logs, names))
    print(f"{len(rows)} rows, {len(logs)} distinct launch logs, {os.path.getsize(a.out)} bytes -> {a.out}")
    print(f"query entry points logged {len(noise.splitlines())} records")
    for ln in lds_attribute_violations(full):
        print("LDS attribute missing:", ln)
    if a.coverage:
        missing = sorted(exported_kernels(a.lib or EMU) - seen)
        print(f"{len(seen)} kernel symbols launched, {len(missing)} exported conv forward kernels never launched")
        for m in missing:
            print("  ", m)


if __name__ == "__main__":
    main()
