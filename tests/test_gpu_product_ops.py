"""-m gpu: the ops the LA, pancreas and ACDC steps launch, at their exact in-step shapes and with the step's norm epilogues
(tests/product_ops.py STEP_KEYS / STEP_VARIANTS), element by element against an fp64 host reference; and the checks that the table covers
every key and every norm epilogue a real step uses."""
import time
import zlib

import pytest
import torch

import product_ops as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu_ops():
    from bcp_amd.hip_ops import Ops
    assert torch.cuda.is_available(), "the gpu tests need a GPU"
    return Ops.product()


@pytest.mark.parametrize("wl,key", P.driven_rows(), ids=[P.row_id(wl, k) for wl, k in P.driven_rows()])
def test_product_op(gpu_ops, wl, key):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(zlib.crc32(P.row_id(wl, key).encode()))      # (fixed per row, whatever PYTHONHASHSEED)
    t0 = time.perf_counter()
    # the driver's launches must record exactly the table's key: same op, shapes, int arguments and |max| operands as in the step
    # (statistics-only norm calls are not profiled: a key only they use is checked through its variants alone)
    gpu_ops.profile_begin()
    try:
        res = P.run_row(gpu_ops, dev, wl, key, g)
    finally:
        torch.cuda.synchronize()
        recs = gpu_ops.profile_end()
    seen = {(r[0], tuple(tuple(s) for s in r[1]), tuple(r[2]), int(r[4])) for r in recs}
    if key in P.STEP_KEYS[wl]:
        assert key in seen, f"the driver did not launch the step's key {key}; it launched {sorted(seen)}"
    for tag, (ratio, loc) in res:
        print(f"[product-op] {wl:8s} {tag:28s} {'x'.join(map(str, key[1][0])):22s} worst err/bound {ratio:.3e}  at {loc}  "
              f"({time.perf_counter() - t0:.1f} s)")


@pytest.mark.parametrize("wl", sorted(P.STEP_KEYS))
def test_step_keys_in_table(gpu_ops, wl):
    """one replayed step under the profile hooks: every (op, shapes, ints, namax) it records must be a STEP_KEYS row"""
    t0 = time.perf_counter()
    keys = P.record_step_keys(wl)
    table = set(P.STEP_KEYS[wl])
    missing = sorted(keys - table)
    for k in sorted(table - keys):
        print(f"[product-op] {wl}: table row not used by the step: {k}")
    print(f"[product-op] {wl}: {len(keys)} keys recorded, {time.perf_counter() - t0:.1f} s")
    assert not missing, f"{wl}: {len(missing)} step keys not in tests/product_ops.py STEP_KEYS: {missing[:8]}"


@pytest.mark.parametrize("wl", sorted(P.STEP_KEYS))
def test_step_norm_epilogues_in_table(gpu_ops, wl):
    """the step's eager recording pass: every (norm key, epilogue) it uses must be a STEP_VARIANTS entry, so the drivers run it"""
    t0 = time.perf_counter()
    used = P.record_step_variants(wl)
    table = P.STEP_VARIANTS[wl]
    missing = sorted((k, f) for k, fl in used.items() for f in fl if f not in table.get(k, ()))
    print(f"[product-op] {wl}: {sum(len(v) for v in used.values())} norm epilogues recorded, {time.perf_counter() - t0:.1f} s")
    assert not missing, f"{wl}: norm epilogues not in tests/product_ops.py STEP_VARIANTS: {missing[:6]}"
