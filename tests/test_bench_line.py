"""The line `bench.py --full` prints must survive the driver's record: one JSON object, below 4 KB, with the contract keys, `roofline`
and `cpu_baseline` (the 20 KB line of round 4 was cut and parsed as nothing). Built here from canned numbers --
the full record of round 4's last builder run (tests/golden/bench_full_record_r04.json) -- no GPU involved. The same for
the headline line of a plain run and for the arrays of --dump-outputs."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402


CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config", "roofline", "cpu_baseline")


def canned():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "bench_full_record_r04.json")))


def test_line_is_small_and_carries_the_contract():
    full = canned()
    text = bench.compact_line(full)
    assert "\n" not in text and len(text) < bench.MAX_LINE_BYTES <= 4096
    line = json.loads(text)
    for k in CONTRACT:
        assert k in line, k
    assert line["value"] == pytest.approx(full["value"], rel=1e-6)
    assert line["steps"] == full["steps"] and line["warmup"] == full["warmup"] and line["n_gpus"] == 1
    assert isinstance(line["config"]["workload"], str) and "model" not in line["config"]
    rf = line["roofline"]
    assert rf["bound"] in ("hbm", "mfma") and rf["frac"] == pytest.approx(rf["achieved"] / rf["peak"], rel=1e-4)
    assert rf["achieved"] == pytest.approx(1e-6 * rf["algorithmic_bytes_per_launch"] / rf["kernel_ms"], rel=1e-4)
    cb = line["cpu_baseline"]
    assert cb["kind"] in ("port", "reference") and cb["cores"] == 1 and cb["value"] > 0 and cb["sample"]
    # every value of config is a scalar (the driver keeps config whole: prose and nested samples belong in the sidecar)
    assert all(not isinstance(v, (dict, list)) for v in line["config"].values())
    for k in ("hs071_us_per_sqp_iteration_gpu", "sparse10k_s_per_sqp_iteration", "dense_2048x4096_cold_s", "hs0xx_batch_512_ms",
              "roofline_mfma_frac", "roofline_spmv_frac"):
        assert isinstance(line["config"][k], float), k


def test_line_without_extras_and_with_gather_stays_small():
    full = canned()
    for k in ("cpu_baseline", "speedup_vs_cpu_baseline", "large_engine", "roofline_spmv", "hs071_single_qp", "hs071_trajectory_latency"):
        full.pop(k, None)
    full["n_gpus"] = 8
    full["with_gather"] = {"steps": 50, "ms_per_step": 0.1, "value": 5e9, "unit": "QP solves/s", "all_gather_ms": 0.03,
                           "ranks_seen": 8, "note": "x" * 5000, "native_rccl": {"a": "y" * 5000}}
    line = json.loads(bench.compact_line(full))
    assert "cpu_baseline" not in line and line["with_gather"]["ranks_seen"] == 8
    assert len(json.dumps(line)) < 2048


def test_oversized_line_is_refused():
    full = canned()
    full["config"]["workload"] = "w" * 5000
    with pytest.raises(AssertionError):
        bench.compact_line(full)


def test_plain_line_carries_the_headline_keys():
    import argparse
    args = argparse.Namespace(batch_per_gpu=65536, steps=20, warmup=5, keep_state=0)
    line = json.loads(bench.headline_line(bench.headline(args, 1, 0.9, "lane_qp_kernel<2, false, true>")))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus"):
        assert k in line, k
    assert line["metric"] == "QP-subproblem solves/sec" and line["unit"] == "QP solves/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f64" and line["steps"] == 20 and line["warmup"] == 5
    assert line["value"] == pytest.approx(65536 * 20 / 0.9, rel=1e-6)
    assert line["ms_per_step"] == pytest.approx(1e3 * 0.9 / 20, rel=1e-6)
    assert line["config"]["qps_per_gpu"] == 65536 and "roofline" not in line and "extras" not in line


class _FakeBatch:
    def __init__(self, nq):
        rng = np.random.default_rng(7)
        self.res = [dict(x=rng.normal(size=8), y=rng.normal(size=10), ws_b=rng.integers(-1, 2, 8).astype(np.int32),
                         ws_c=rng.integers(-1, 2, 2).astype(np.int32), status=20, nWSR=2, obj=float(q)) for q in range(nq)]

    def results(self):
        return self.res


def test_dump_outputs_writes_one_float64_array_per_field(tmp_path):
    b = _FakeBatch(300)
    names = bench.dump_outputs(b, str(tmp_path))
    assert names == ["nWSR", "obj", "status", "ws_b", "ws_c", "x", "y"]
    x = np.load(tmp_path / "x.npy")
    assert x.dtype == np.float64 and x.shape == (300, 8) and np.array_equal(x[17], b.res[17]["x"])
    assert np.load(tmp_path / "ws_c.npy").shape == (300, 2) and np.array_equal(np.load(tmp_path / "obj.npy"), np.arange(300.0))


def test_dump_outputs_samples_a_large_batch_within_the_cap(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "MAX_DUMP_BYTES", 64 * 1024)
    b = _FakeBatch(2000)
    bench.dump_outputs(b, str(tmp_path / "a"))
    bench.dump_outputs(b, str(tmp_path / "b"))
    total = sum(np.load(p).nbytes for p in (tmp_path / "a").iterdir())
    assert total <= 64 * 1024
    member = np.load(tmp_path / "a" / "member.npy").astype(int)
    assert 0 < len(member) < 2000 and np.array_equal(member, np.sort(member))
    assert np.array_equal(member, np.load(tmp_path / "b" / "member.npy").astype(int))      # the same sample every run
    assert np.array_equal(np.load(tmp_path / "a" / "obj.npy"), member.astype(float))
