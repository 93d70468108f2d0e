"""bench.py's stdout record: compact, parseable, contract keys present (the 24.6 KB line of round 5 reached the driver as
`parsed: null`).  CPU test: the record is built from canned `measure()` results -- the committed full report of round 5 and a minimal one."""
import argparse
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
            "roofline", "cpu_baseline")


def _check(rec, n1=True):
    line = json.dumps(rec, separators=(",", ":"))
    assert len(line) < bench.MAX_LINE_BYTES, len(line)
    back = json.loads(line)
    for k in CONTRACT:
        if k == "cpu_baseline" and not n1:
            continue
        assert k in back, k
    assert set(back["config"]) <= {"workload", "global_batch", "parallelism"} and "workload" in back["config"]
    r = back["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] in ("hbm", "mfma")
    assert r["traffic"] is None or isinstance(r["traffic"], (int, float))
    if n1:
        for k in ("value", "unit", "cores", "kind"):
            assert k in back["cpu_baseline"], k
    return back


def test_record_from_the_round5_full_report():
    fn = os.path.join(ROOT, "profiles", "r05_t8_bench.json")
    if not os.path.exists(fn):
        pytest.skip("no committed full report")
    full = json.load(open(fn))
    assert len(json.dumps(full)) > 20000          # what the driver could not parse
    back = _check(bench.compact_record(full, detail="bench_detail.json"))
    assert back["value"] == full["value"] and back["ms_per_step"] == full["ms_per_step"]
    assert abs(back["roofline"]["frac"] - full["roofline"]["frac"]) < 1e-9
    assert back["roofline"]["frac_in_step_bracket"] < back["roofline"]["frac"]
    assert back["roofline"]["traffic"] == full["roofline"]["traffic"]["bytes_per_launch"]
    for wl in ("acdc", "pancreas"):
        e = back["extra_workloads"][wl]
        assert e["value"] == full["extra_workloads"][wl]["value"]
        assert e["roofline_frac"] == full["extra_workloads"][wl]["roofline"]["frac"]
        assert e["cpu_baseline_value"] == full["extra_workloads"][wl]["cpu_baseline"]["value"]


def test_record_minimal_and_multi_rank_and_failed_extra():
    out = {"metric": "m", "value": 1.0, "unit": "volumes/s", "n_gpus": 2, "steps": 3, "warmup": 1, "ms_per_step": 2.0, "higher_is_better": True,
           "scaling": "weak", "vs_baseline": None, "dtype": bench.DTYPE, "data": "synthetic",
           "config": {"workload": "w", "global_batch": 8, "parallelism": "dp2", "host_path": "x" * 5000, "arithmetic": "y" * 5000},
           "roofline": {"bound": "mfma", "achieved": None, "peak": 157.3, "unit": "TFLOP/s", "frac": None, "traffic": None},
           "kernels": [{"op": "o" * 100}] * 200, "ranks_seen": 2, "exposed_allreduce_ms_per_step": 0.1,
           "extra_workloads": {"acdc": {"error": "RuntimeError: " + "z" * 1000}}}
    back = _check(bench.compact_record(out), n1=False)
    assert back["ranks_seen"] == 2 and "kernels" not in back and "host_path" not in back["config"]
    assert len(back["extra_workloads"]["acdc"]["error"]) <= 120


def test_dump_outputs_of_a_step():
    """--dump-outputs: the step's result dict at the LA shapes (batch 4) plus samples of both networks' state, float32 / float64 host arrays
    within the size budget, the same sample indices every time"""
    g = torch.Generator().manual_seed(0)
    r = {"loss": torch.tensor(0.5), "loss_l": torch.tensor(0.25, dtype=torch.float64),
         "plab_a": (torch.rand(2, 112, 112, 80, generator=g) < 0.5).to(torch.uint8),
         "plab_b": (torch.rand(2, 112, 112, 80, generator=g) < 0.5).to(torch.uint8),
         "outputs_l": torch.randn(2, 2, 112, 112, 80, generator=g), "outputs_u": torch.randn(2, 2, 112, 112, 80, generator=g)}
    big = torch.nn.Sequential(torch.nn.Linear(1024, 1536), torch.nn.BatchNorm1d(1536))       # more state than one sample holds
    small = torch.nn.Linear(4, 3)
    a = bench.snapshot_outputs(r, (big, small))
    assert set(a) == set(r) | {"model_state_sample", "ema_state_sample"}
    assert sum(v.nbytes for v in a.values()) <= bench.DUMP_MAX_BYTES
    assert a["loss_l"].dtype == np.float64 and all(v.dtype == np.float32 for k, v in a.items() if k != "loss_l")
    assert float(a["loss"]) == 0.5 and a["outputs_l"].shape == (2, 2, 112, 112, 80)
    assert np.array_equal(a["plab_a"], r["plab_a"].numpy().astype(np.float32))
    assert a["model_state_sample"].size == bench.DUMP_STATE_SAMPLE and a["ema_state_sample"].size == 4 * 3 + 3
    b = bench.snapshot_outputs(r, (big, small))
    assert all(np.array_equal(a[k], b[k]) for k in a)
    # an output larger than its share of the budget is kept as a fixed sample
    huge = bench.snapshot_outputs({"x": torch.zeros(32 * 10**6)}, ())
    assert huge["x"].nbytes <= bench.DUMP_MAX_BYTES


def _measure_counted(monkeypatch, **flags):
    """bench.measure() with a stand-in workload whose steps are counted and the device calls stubbed out: -> (record, steps run, calls of the
    measurements a plain run leaves to --full)"""
    from bcp_amd.dp import DataParallel
    n = {"step": 0, "profile_steps": 0, "cpu_baseline": 0}

    def make_workload(args, dp, dev):
        def step():
            n["step"] += 1
            return {"loss": torch.tensor(0.5)}
        return step, {"metric": "m", "unit": "volumes/s", "what": "w", "gflop_per_item": 1.0}

    def profile_steps(step, k, only=None):
        n["profile_steps"] += 1
        return [], 1.0

    def cpu_baseline(*a, **k):
        n["cpu_baseline"] += 1
        return {"value": 1.0, "unit": "volumes/s", "cores": 1, "kind": "port", "sample": "s"}

    monkeypatch.setattr(bench, "make_workload", make_workload)
    monkeypatch.setattr(bench, "profile_steps", profile_steps)
    monkeypatch.setattr(bench, "cpu_baseline", cpu_baseline)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)
    monkeypatch.setattr(torch.cuda, "empty_cache", lambda: None)
    args = argparse.Namespace(workload="la", batch_size=4, labeled_bs=2, steps=7, warmup=3, profile_steps=3, no_cpu_baseline=False,
                              dump_outputs=None, opt_late=[], full=False)
    vars(args).update(flags)
    out = bench.measure(args, DataParallel(), torch.device("cpu"))
    return bench.compact_record(out), n.pop("step"), n


def test_plain_run_does_only_the_set_up_warm_up_and_timed_steps(monkeypatch):
    """a plain run: the two set-up steps, W warm-ups and K timed steps, nothing measured after them, the headline keys in the record"""
    rec, steps, more = _measure_counted(monkeypatch)
    assert steps == 2 + 3 + 7 and more == {"profile_steps": 0, "cpu_baseline": 0}
    assert rec["steps"] == 7 and rec["warmup"] == 3 and rec["dtype"] == bench.DTYPE and rec["higher_is_better"] is True
    assert rec["value"] > 0 and rec["ms_per_step"] > 0 and rec["unit"] == "volumes/s"
    assert "cpu_baseline" not in rec and rec["roofline"]["frac"] is None
    # --full: the five empty-queue host steps, the profiled steps and the CPU baseline after the timed region
    rec, steps, more = _measure_counted(monkeypatch, full=True)
    assert steps == 2 + 3 + 7 + 5 and more == {"profile_steps": 1, "cpu_baseline": 1}
    assert rec["cpu_baseline"]["value"] == 1.0
