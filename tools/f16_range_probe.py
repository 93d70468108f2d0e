#!/usr/bin/env python3
"""The grid of tests/wgrad_checks.py check_f16_range on a simulator library given by path, as a record: per case, path and grid point the
digest of the fp16 kernel's output bits, whether it is finite, its worst |out - ref64| / cond over TAU, and the two maximum errors of the
3x gate.  Two records compare bit for bit where both operands' maxima lie inside a window:

    python tools/f16_range_probe.py --lib OLD/libbcp_emu.so --out old.json      # e.g. a simulator built from the parent commit
    python tools/f16_range_probe.py --out new.json                              # tests/_emu/libbcp_emu.so of this tree
    python tools/f16_range_probe.py --compare old.json new.json --window 60     # both operands' scale exponents 14 - exponent(|max|)
                                                                                # within +-60, the old clamp: same bits

A change of the scale arithmetic (csrc/conv3_defs.h f16_scale_exp / F16Unscale) must leave every output inside the old domain
bit-identical -- powers of two are exact -- and this is how that is shown."""
import argparse
import hashlib
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)


def record(lib, ks, cases):
    import torch
    import make_golden_conv3_routes as R
    import product_ops as PO
    import wgrad_checks as W
    from bcp_amd import _lib
    from bcp_amd.hip_ops import Ops
    ops = Ops(_lib.Binding(lib or R.build_emu()), allow_cpu=True)
    out = {}
    for case in cases or W.F16_CASES:
        for tag, o16, _, o32, ref, cond, maxima in W.f16_range_runs(ops, torch.device("cpu"), case, W.f16_range_points(ks)):
            scale = float(ref.abs().max())
            finite = bool(torch.isfinite(o16).all())
            e16, e32 = float((o16.double() - ref).abs().max()), float((o32.double() - ref).abs().max())
            ratio = PO.elementwise_ratio(o16.double(), ref, cond)[0] / PO.TAU
            ok = finite and ratio <= 1.0 and e16 <= 3.0 * e32 + 1e-7 * scale
            out[tag] = dict(sha1=hashlib.sha1(o16.contiguous().numpy().tobytes()).hexdigest(), finite=finite, ratio_over_tau=ratio,
                            err16=e16 / scale, err32=e32 / scale, ok=ok, scale_exp=[14 - math.frexp(m)[1] for m in maxima])
            print(f"{'ok  ' if ok else 'FAIL'} {tag}: ratio/TAU {ratio:.3g} err/scale f16 {e16 / scale:.2e} fp32 {e32 / scale:.2e}", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--grid", choices=("full", "default"), default="full")
    ap.add_argument("--case", action="append")
    ap.add_argument("--compare", nargs=2)
    ap.add_argument("--window", type=int, default=60)
    a = ap.parse_args()
    if a.compare:
        x, y = (json.load(open(f)) for f in a.compare)
        assert set(x) == set(y)
        tags = [t for t in x if all(abs(e) <= a.window for e in x[t]["scale_exp"])]
        diff = [t for t in tags if x[t]["sha1"] != y[t]["sha1"]]
        print(f"{len(tags)} of {len(x)} outputs have both scale exponents within +-{a.window}: {len(tags) - len(diff)} bit-identical, {len(diff)} differ")
        for t in diff:
            print("  differs:", t)
        for name, r in zip(a.compare, (x, y)):
            bad = [t for t in r if not r[t]["ok"]]
            print(f"{name}: {len(bad)} of {len(r)} grid points fail check_f16_range's assertions")
        sys.exit(1 if diff else 0)
    import wgrad_checks as W
    rec = record(a.lib, W.K_FULL if a.grid == "full" else W.K_DEFAULT, a.case)
    if a.out:
        json.dump(rec, open(a.out, "w"), indent=0)


if __name__ == "__main__":
    main()
