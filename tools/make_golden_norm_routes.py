#!/usr/bin/env python3
"""The normalisation family's host dispatch (csrc/norm.hip, csrc/norm_res.hip, csrc/gnorm.hip) as DATA: for a grid of (options, groups,
rows per group, rows per sample, channels) what the three queries answer and what every entry point of the family launches under each of
its flag sets -- symbol with its template arguments, grid, block, LDS, the kernel's scalar arguments and every POINTER argument as "null"
or as "@" + its byte offset from a base address, every launch of the call in order -- read from the host simulator's launch log in its
no-execute mode with arguments and pointers (tools/emu, log mode 4).  In this family the route lives in the pointers: which of y / ysum /
partial / partial_in a launch reads, whether a pass gets the |max| slots, where c1 lies in the workspace.  The sweep hands every pointer
parameter an address of its own, 4 GiB apart, with no storage behind it (nothing is executed), so a swapped argument or a moved c1 shows.

    python tools/make_golden_norm_routes.py            # rewrites tests/golden/norm_routes.npz from tests/_emu/libbcp_emu.so
    python tools/make_golden_norm_routes.py --coverage # also lists the kernel instances of the family the sweep never launched

tests/test_emu_norm_routes.py runs the same sweep (sweep() below) against the current sources and compares it with the committed file.
The plumbing (simulator build, library wrapper, packed-log layout) is tools/make_golden_conv3_routes.py's."""
import argparse
import ctypes as C
import os

import numpy as np

import make_golden_conv3_routes as R3
from make_golden_conv3_routes import ROOT, EMU, build_emu  # noqa: F401

GOLDEN = os.path.join(ROOT, "tests", "golden", "norm_routes.npz")

# ---- the grid -------------------------------------------------------------------------------------------------------------------
THRESHOLDS = (1, 255, 256, 257, 512, 513, 4096, 4097, 99999, 100000)
SAMPLES = (1, 2, 4, 64, 65)                # per group, with chan_scale; 65 is refused
BATCH = ((R3.LA, 4), (R3.PANCREAS, 2), (R3.ACDC, 12))


def _cells(workloads):
    """(G, rows_per_group, rows_per_sample): the product workloads' levels at their batches split into 1, 2 and N groups, the thresholds of
    the rules and their neighbours, then groups of 1 .. 65 whole samples and one that its sample does not divide"""
    out = []
    for extent, n in workloads:
        for ext in R3._levels(extent):
            vox = int(np.prod(ext))
            out += [(g, n * vox // g, vox) for g in dict.fromkeys((1, 2, n))]
    out += [(g, r, r) for r in THRESHOLDS for g in (1, 2)]
    out += [(g, s * rps, rps) for rps in (245, 1960) for s in SAMPLES for g in (1, 2)]
    out += [(1, 100, 7), (2, 4100, 1000)]
    return list(dict.fromkeys(out))


CELLS = _cells(BATCH)                      # the default options: every workload
CELLS_SMALL = _cells(BATCH[:1])            # each other option: LA's levels (batch and extent axes thinned; thresholds and samples whole)
CHANNELS = (16, 32, 64, 128, 256, 512, 1024, 8, 24, 2048)
OPTIONS = [{}, {"norm_fuse_fin": 0}, {"norm_fin_rows": 64}, {"norm_fin_rows": 192}, {"norm_own": 1}, {"norm_slabs": 0}, {"norm_apply_cap": 512},
           {"norm_apply_vec": 1}, {"whatif": 1}, {"whatif": 2}, {"whatif": 16}, {"whatif": 32}]

KERNEL_FAMILIES = ("k_col_partial<", "k_norm_own_fwd<", "k_norm_own_bwd<", "k_norm_apply_res<", "k_col_partial_res<", "k_norm_bwd_apply_res<",
                   "k_norm_eval_res<")
SKIPPED = -99                              # the *_rc column of a call this row does not make (BCP_EINVAL is -1)
ENTRY_POINTS = ("bcp_norm_", "bcp_gnorm_")

# ---- pointers: one address per parameter name, 4 GiB apart, all behind BASE ------------------------------------------------------
BASE = 1 << 44
SLOTS = ("y", "da", "gamma", "beta", "rmean", "rvar", "cs", "res", "stats", "ws", "pin", "out", "amax", "dgamma", "dbeta", "dbias", "dy", "dres",
         "slabs", "bias", "sum")
ADDR = {name: BASE + ((i + 1) << 32) for i, name in enumerate(SLOTS)}
f32 = C.c_float


def _p(name, present=1):
    return ADDR[name] if present else None


# ---- the calls: name -> (entry point, arguments(G, R, rps, C), refused on purpose(G, R, rps, C)) ------------------------------------
def _bad_c(C_, top=1024):
    return C_ < 16 or C_ > top or C_ & (C_ - 1) != 0


def _bad_cs(R, rps):
    return R % rps != 0 or R // rps > 64


def _fwd(out=1, run=1, res=0, amax=1, pin=None, cs=0, ld=lambda C_: 0):
    return lambda G, R, rps, C_: (_p("y"), G, R, C_, _p("gamma"), _p("beta"), _p("rmean", run), _p("rvar", run), f32(0.1), f32(1e-5), 1, _p("cs", cs), rps,
                                  None, f32(1.0), None, f32(1.0), _p("res", res), _p("stats"), _p("ws"), _p("pin", pin is not None), pin or 0,
                                  _p("out", out), ld(C_), _p("amax", amax), None)


def _bwd(grad=1, acc=0, amax=1, pin=None, cs=0):
    return lambda G, R, rps, C_: (_p("y"), _p("da"), G, R, C_, _p("stats"), 1, _p("cs", cs), rps, None, f32(1.0), None, f32(1.0), _p("dgamma", grad),
                                  _p("dbeta", grad), acc, _p("ws"), _p("pin", pin is not None), pin or 0, _p("dy"), _p("amax", amax), None)


def _fwd_slabs(nslab=4, bias=0, out=1, run=1, res=0, amax=1, cs=0):
    return lambda G, R, rps, C_: (_p("slabs"), nslab, G * R * C_, _p("bias", bias), _p("sum"), G, R, C_, _p("gamma"), _p("beta"), _p("rmean", run),
                                  _p("rvar", run), f32(0.1), f32(1e-5), 1, _p("cs", cs), rps, None, f32(1.0), None, f32(1.0), _p("res", res), _p("stats"),
                                  _p("ws"), _p("out", out), _p("amax", amax), None)


def _bwd_slabs(nslab=4, grad=1, dbeta=None, acc=0, amax=1, cs=0):
    return lambda G, R, rps, C_: (_p("y"), _p("slabs"), nslab, G * R * C_, _p("sum"), G, R, C_, _p("stats"), 1, _p("cs", cs), rps, None, f32(1.0), None,
                                  f32(1.0), _p("dgamma", grad), _p("dbeta", grad if dbeta is None else dbeta), acc, _p("ws"), _p("dy"), _p("amax", amax), None)


def _fwd_res(rc=lambda C_: C_, run=1, amax=1, pin=None, cs=0):
    return lambda G, R, rps, C_: (_p("y"), G, R, C_, _p("gamma"), _p("beta"), _p("rmean", run), _p("rvar", run), f32(0.1), f32(1e-5), 1, _p("cs", cs), rps,
                                  _p("res"), rc(C_), _p("stats"), _p("ws"), _p("pin", pin is not None), pin or 0, _p("out"), _p("amax", amax), None)


def _bwd_res(rc=lambda C_: C_, grad=1, acc=0, dres=0, amax=1, cs=0):
    return lambda G, R, rps, C_: (_p("y"), _p("da"), _p("res"), rc(C_), G, R, C_, _p("stats"), 1, _p("cs", cs), rps, _p("dgamma", grad), _p("dbeta", grad),
                                  acc, _p("ws"), _p("dy"), _p("dres", dres), _p("amax", amax), None)


def _eval_res(rc=lambda C_: C_):
    return lambda G, R, rps, C_: (_p("y"), G * R, C_, _p("gamma"), _p("beta"), _p("rmean"), _p("rvar"), f32(1e-5), 1, _p("res"), rc(C_), _p("out"), None)


def _gn_fwd(groups=16, cs=0, res=0, out=1, amax=1, pin=None):
    return lambda G, R, rps, C_: (_p("y"), G, R, C_, groups, _p("gamma"), _p("beta"), f32(1e-5), 1, _p("cs", cs), _p("res", res), _p("stats"), _p("ws"),
                                  _p("pin", pin is not None), pin or 0, _p("out", out), _p("amax", amax), None)


def _gn_bwd(groups=16, cs=0, grad=1, dbias=0, acc=0, amax=1, pin=None):
    return lambda G, R, rps, C_: (_p("y"), _p("da"), G, R, C_, groups, _p("stats"), _p("gamma"), 1, _p("cs", cs), _p("dgamma", grad), _p("dbeta", grad),
                                  _p("dbias", dbias), acc, _p("ws"), _p("pin", pin is not None), pin or 0, _p("dy"), _p("amax", amax), None)


_one, _two = (lambda C_: 1), (lambda C_: 2)
_never = lambda G, R, rps, C_: _bad_c(C_)
_always = lambda G, R, rps, C_: True
_cs = lambda G, R, rps, C_: _bad_c(C_) or _bad_cs(R, rps)
_sl = lambda G, R, rps, C_: _bad_c(C_) or R > 4096
_sl_cs = lambda G, R, rps, C_: _bad_c(C_) or R > 4096 or _bad_cs(R, rps)
_gn = lambda G, R, rps, C_: _bad_c(C_, 256)
CALLS = (
    ("fwd_all", "bcp_norm_fwd", _fwd(res=1), _never),
    ("fwd_bare", "bcp_norm_fwd", _fwd(run=0, amax=0, ld=lambda C_: C_), _never),
    ("fwd_stat_run", "bcp_norm_fwd", _fwd(out=0), _never),
    ("fwd_stat", "bcp_norm_fwd", _fwd(out=0, run=0), _never),
    ("fwd_pin", "bcp_norm_fwd", _fwd(pin=7), _never),
    ("fwd_pin_stat", "bcp_norm_fwd", _fwd(out=0, run=0, pin=0), _never),        # (any nb_in: bcp_norm_fwd does not look at it)
    ("fwd_cs", "bcp_norm_fwd", _fwd(cs=1, ld=lambda C_: 2 * C_), _cs),
    ("fwd_bad_ld", "bcp_norm_fwd", _fwd(ld=lambda C_: C_ + 2), _always),
    ("fwd_bad_res", "bcp_norm_fwd", _fwd(out=0, res=1), _always),
    ("bwd_all", "bcp_norm_bwd", _bwd(), _never),
    ("bwd_acc", "bcp_norm_bwd", _bwd(acc=1, amax=0), _never),
    ("bwd_nograd", "bcp_norm_bwd", _bwd(grad=0), _never),
    ("bwd_pin", "bcp_norm_bwd", _bwd(pin=7), _never),
    ("bwd_cs", "bcp_norm_bwd", _bwd(cs=1, acc=1), _cs),
    ("bwd_bad_pin", "bcp_norm_bwd", _bwd(pin=7, cs=1), _always),
    ("fwds_all", "bcp_norm_fwd_slabs", _fwd_slabs(bias=1, res=1), _sl),
    ("fwds_bare", "bcp_norm_fwd_slabs", _fwd_slabs(nslab=1, run=0, amax=0), _sl),
    ("fwds_stat_run", "bcp_norm_fwd_slabs", _fwd_slabs(nslab=64, out=0), _sl),
    ("fwds_stat", "bcp_norm_fwd_slabs", _fwd_slabs(out=0, run=0), _sl),
    ("fwds_cs", "bcp_norm_fwd_slabs", _fwd_slabs(cs=1), _sl_cs),
    ("fwds_bad", "bcp_norm_fwd_slabs", _fwd_slabs(nslab=65), _always),
    ("bwds_all", "bcp_norm_bwd_slabs", _bwd_slabs(), _sl),
    ("bwds_acc", "bcp_norm_bwd_slabs", _bwd_slabs(nslab=64, acc=1, amax=0), _sl),
    ("bwds_nograd", "bcp_norm_bwd_slabs", _bwd_slabs(nslab=1, grad=0), _sl),
    ("bwds_cs", "bcp_norm_bwd_slabs", _bwd_slabs(cs=1), _sl_cs),
    ("bwds_bad", "bcp_norm_bwd_slabs", _bwd_slabs(nslab=65), _always),
    ("bwds_bad_pair", "bcp_norm_bwd_slabs", _bwd_slabs(dbeta=0), _always),
    ("fres_all", "bcp_norm_fwd_res", _fwd_res(), _never),
    ("fres_b", "bcp_norm_fwd_res", _fwd_res(rc=_one, run=0, amax=0), _never),
    ("fres_pin", "bcp_norm_fwd_res", _fwd_res(pin=7), _never),
    ("fres_cs", "bcp_norm_fwd_res", _fwd_res(rc=_one, cs=1), _cs),
    ("fres_bad_rc", "bcp_norm_fwd_res", _fwd_res(rc=_two), _always),
    ("fres_bad_pin", "bcp_norm_fwd_res", _fwd_res(pin=0), _always),
    ("bres_all", "bcp_norm_bwd_res", _bwd_res(dres=1), _never),
    ("bres_b", "bcp_norm_bwd_res", _bwd_res(rc=_one, acc=1, amax=0), _never),
    ("bres_nograd", "bcp_norm_bwd_res", _bwd_res(grad=0), _never),
    ("bres_cs", "bcp_norm_bwd_res", _bwd_res(rc=_one, cs=1), _cs),
    ("bres_bad_rc", "bcp_norm_bwd_res", _bwd_res(rc=_two), _always),
    ("bres_bad_dres", "bcp_norm_bwd_res", _bwd_res(rc=_one, dres=1), _always),
    ("eres_c", "bcp_norm_eval_res", _eval_res(), _never),
    ("eres_b", "bcp_norm_eval_res", _eval_res(rc=_one), _never),
    ("eres_bad_rc", "bcp_norm_eval_res", _eval_res(rc=_two), _always),
    ("gfwd_all", "bcp_gnorm_fwd", _gn_fwd(cs=1, res=1), _gn),
    ("gfwd_stat", "bcp_gnorm_fwd", _gn_fwd(out=0), _gn),
    ("gfwd_pin", "bcp_gnorm_fwd", _gn_fwd(pin=7, amax=0), _gn),
    ("gfwd_bad", "bcp_gnorm_fwd", _gn_fwd(groups=8), _always),
    ("gbwd_all", "bcp_gnorm_bwd", _gn_bwd(cs=1, dbias=1), _gn),
    ("gbwd_acc", "bcp_gnorm_bwd", _gn_bwd(acc=1, amax=0), _gn),
    ("gbwd_pin", "bcp_gnorm_bwd", _gn_bwd(pin=7, grad=0), _gn),
    ("gbwd_bad", "bcp_gnorm_bwd", _gn_bwd(pin=7, cs=1), _always),
)
OPTION_FREE = ("bcp_norm_eval_res",)       # looks at no option: swept under the default set only
QUERIES = ("norm_ws", "slabs_ok", "gnorm_ws")
COLUMNS = ("option", "G", "R", "rps", "C") + QUERIES + tuple(f"{c}_{f}" for c, *_ in CALLS for f in ("rc", "log"))


def refused_on_purpose(name, G, R, rps, C_):
    return {c: bad for c, _, _, bad in CALLS}[name](G, R, rps, C_)


class Lib(R3.Lib):
    """... with the normalisation family's signatures added, log mode 4's base address registered"""

    def __init__(self, path=EMU):
        super().__init__(path)
        from bcp_amd import _lib
        for name, (res, args) in _lib._SIGS.items():
            if name.startswith(ENTRY_POINTS):
                fn = getattr(self.cdll, name)
                fn.restype, fn.argtypes = res, args
        self.cdll.bcpemu_log_base.restype, self.cdll.bcpemu_log_base.argtypes = None, [C.c_void_p]
        self.cdll.bcpemu_log_base(BASE)


def sweep(lib, coverage=None):
    """-> (rows int64 [n, len(COLUMNS)], logs: the distinct launch records of one entry-point call ("L|symbol|grid|block|LDS" and behind
    each "P|scalar and pointer arguments"), option_names, query_noise: what the query entry points logged -- must be empty)"""
    c = lib.cdll
    logs, log_id, rows, noise = [], {}, [], []
    prev = lib.log_mode(4)
    fns = [(getattr(c, entry), args, entry in OPTION_FREE) for _, entry, args, _ in CALLS]
    take = lib.take

    def call(fn, args):
        rc = fn(*args)
        text = take()
        if coverage is not None:
            coverage.update(ln.split("|")[1] for ln in text.splitlines() if ln.startswith("L|"))
        i = log_id.get(text)
        if i is None:
            i = log_id[text] = len(logs)
            logs.append(text)
        return rc, i

    try:
        for oi, opts in enumerate(OPTIONS):
            lib.set_options(opts)
            try:
                for (G, R, rps) in (CELLS_SMALL if oi else CELLS):
                    for C_ in CHANNELS:
                        take()
                        row = [oi, G, R, rps, C_, c.bcp_norm_workspace_bytes(G, R, C_), c.bcp_norm_slabs_ok(G, R, C_), c.bcp_gnorm_workspace_bytes(G, R, C_)]
                        noise.append(take())
                        for fn, args, option_free in fns:
                            row += (SKIPPED, -1) if option_free and oi else call(fn, args(G, R, rps, C_))
                        rows.append(row)
            finally:
                lib.set_options(opts, reset=True)
    finally:
        lib.log_mode(prev)
        take()
    names = [",".join(f"{k}={v}" for k, v in o.items()) or "default" for o in OPTIONS]
    return np.asarray(rows, dtype=np.int64), logs, names, "".join(noise)


def exported_kernels(path=EMU):
    return R3.exported_kernels(path, KERNEL_FAMILIES)


# ---- the file: the launch records as numbers (as text, 33000 distinct call logs deflate to 0.6 MB; so, to 0.2 MB) ------------------------
# A call's log is a sequence of launches; a launch is its kernel symbol and a fixed number of fields: grid, block, LDS, then the "P|" tokens.
# Per symbol one int64 matrix [fields, launches] (token t -> 4 * value + kind; kind 0: integer, 1: null, 2: pointer offset, 3: float32 bits),
# the distinct launches numbered in order of first appearance; a call log refers to launch n as (launches seen so far) - n, or 0 for a new one.
def _token(t):
    if t == "null":
        return 1
    if t.startswith("@"):
        return 4 * int(t[1:]) + 2
    try:
        return 4 * int(t)
    except ValueError:
        return 4 * int(np.float32(t).view(np.uint32)) + 3


def _text(v):
    v, kind = divmod(v, 4)
    return "%.9g" % np.uint32(v).view(np.float32) if kind == 3 else ("%d" % v, "null", "@%d" % v)[kind]


def pack(rows, logs, names):
    assert np.abs(rows).max() < 2 ** 31
    launch_id, symbols, fields, sym_of, refs, count = {}, {}, [], [], [], []
    for text in logs:
        lines = text.splitlines()
        assert len(lines) % 2 == 0 and all(a.startswith("L|") and b.startswith("P|") for a, b in zip(lines[0::2], lines[1::2])), text
        count.append(len(lines) // 2)
        for a, b in zip(lines[0::2], lines[1::2]):
            if (a, b) not in launch_id:
                launch_id[a, b] = len(launch_id)
                _, sym, grid, block, lds = a.split("|")
                k = symbols.setdefault(sym, len(symbols))
                if k == len(fields):
                    fields.append([])
                fields[k].append([_token(t) for t in (grid + "," + block + "," + lds + "," + b[2:]).split(",") if t])
                sym_of.append(k)
                refs.append(0)
            else:
                refs.append(len(launch_id) - launch_id[a, b])
    z = dict(rows=np.ascontiguousarray(rows.T.astype(np.int32)), columns=np.array(COLUMNS), options=np.array(names), symbols=np.array(list(symbols)),
             launch_symbol=np.array(sym_of, dtype=np.int16), log_launches=np.array(count, dtype=np.uint8), log_refs=np.array(refs, dtype=np.int32))
    z.update({f"fields{k}": np.ascontiguousarray(np.array(f, dtype=np.int64).T) for k, f in enumerate(fields)})
    assert unpack(z)[1] == logs
    return z


def unpack(z):
    symbols, next_of = list(z["symbols"]), [0] * len(z["symbols"])
    fields = [z[f"fields{k}"].T.tolist() for k in range(len(symbols))]
    launches = []
    for k in z["launch_symbol"].tolist():
        t = [_text(v) for v in fields[k][next_of[k]]]
        next_of[k] += 1
        launches.append("L|%s|%s|%s|%s\nP|%s\n" % (symbols[k], ",".join(t[0:3]), ",".join(t[3:6]), t[6], ",".join(t[7:])))
    refs = z["log_refs"]
    new = refs == 0
    ids = np.cumsum(new) - new - refs                    # (a new launch: the count before it; an old one: that count - its distance)
    ends = np.cumsum(z["log_launches"].astype(np.int64))
    logs = ["".join(launches[i] for i in ids[b:e]) for b, e in zip(np.r_[0, ends[:-1]], ends)]
    return z["rows"].T.astype(np.int64), logs, list(z["options"])


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
        print(f"{len(seen)} kernel symbols launched, {len(missing)} exported kernels of the family never launched")
        for m in missing:
            print("  ", m)


if __name__ == "__main__":
    main()
