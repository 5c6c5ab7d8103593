"""The driver's bench line: round 5's one-line JSON had grown to 24 KB and the driver could not parse
it out of its stdout tail.  bench.compact_line makes the LAST stdout line; these tests feed recorded whole results of earlier
rounds (profiles/r0N_bench.json, copies of what the box printed) through it."""
import copy
import io
import json
import os
import subprocess
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

RECORDED = [p for p in ("r05_bench.json", "r04_bench.json", "r03_o_bench.json") if os.path.exists(os.path.join(ROOT, "profiles", p))]


def _load(name):
    return json.load(open(os.path.join(ROOT, "profiles", name)))


@pytest.mark.parametrize("name", RECORDED)
def test_recorded_results_make_a_small_line_with_the_contract_keys(name):
    full = _load(name)
    line = bench.compact_line(full, "profiles/bench_detail_last.json")
    assert "\n" not in line and len(line) < bench.LINE_LIMIT == 8192
    j = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert k in j and j[k] == full[k], k
    assert "workload" in j["config"] and "model" not in j["config"]
    r = j["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3 and r["frac"] == full["roofline"]["frac"]
    assert r["traffic"] is None or r["traffic"] > 0
    assert abs(r["achieved"] - r["algorithmic_bytes_per_launch"] / (r["avg_launch_ms"] * 1e-3) / 1e9) < 0.01 * r["achieved"]
    c = j["cpu_baseline"]
    assert c["value"] == full["cpu_baseline"]["value"] > 0 and c["cores"] == 1 and c["kind"] in ("reference", "port") and c["sample"]
    for cfg, o in j.get("other_configs", {}).items():
        assert len(json.dumps(o)) < 400, cfg                # a triple (+ the dominant kernel), not a table
        if cfg in ("c5", "c3", "c4_block", "ref_default"):
            assert o["value"] == full["other_configs"][cfg]["value"] and o["ms"] > 0


def test_line_stays_small_whatever_the_legs_return():
    """a leg that returns a huge object (or many legs) cannot push the line over the limit: the optional parts are dropped first"""
    full = copy.deepcopy(_load(RECORDED[0]))
    full["other_configs"] = {"leg%d" % i: {"value": float(i), "unit": "Gbp/s", "ms_per_step": 1.0, "whole_step": {"frac": 0.1},
                                             "roofline": {"kernel": "mgScanKernel", "frac": 0.1}, "junk": "x" * 5000} for i in range(200)}
    full["end_to_end"] = {"leg%d" % i: {"Gbp_per_s": 1.0, "what": "y" * 3000} for i in range(300)}
    line = bench.compact_line(full, None)
    j = json.loads(line)
    assert len(line) < bench.LINE_LIMIT and j["roofline"]["frac"] and j["cpu_baseline"]["value"] and j["value"] == full["value"]


def test_multi_rank_line_keeps_the_checks():
    """the N > 1 line (config 4: a block per GPU + the histogram all-reduce) through the same formatter"""
    full = copy.deepcopy(_load(RECORDED[0]))
    full.pop("cpu_baseline"); full.pop("end_to_end", None)
    full.update(n_gpus=8, collective={"what": "w" * 500, "allreduce_ms": 0.05, "histogram_entries": 8, "entries_all_ranks": 8, "matches_local_sums": True},
                per_rank_parity=True, per_rank_parity_rank0={"ok": True}, single_gpu_block_gbps=1100.0,
                other_configs={"c3_sharded": {"value": 9000.0, "unit": "Gbp/s", "n_gpus": 8, "seed_hit_fraction": 0.34, "ms_each_batch_rank0": [1.0] * 9, "workload": "z" * 600}})
    line = bench.compact_line(full, None)
    j = json.loads(line)
    assert len(line) < 4096
    assert j["n_gpus"] == 8 and j["collective"]["matches_local_sums"] is True and j["per_rank_parity"] is True and j["single_gpu_block_gbps"] == 1100.0
    assert j["roofline"]["frac"] > 0 and j["other_configs"]["c3_sharded"] == {"value": 9000.0, "unit": "Gbp/s", "n_gpus": 8}


def test_emit_prints_the_compact_line_last(tmp_path, monkeypatch):
    full = _load(RECORDED[0])
    monkeypatch.setattr(bench, "HERE", str(tmp_path)); os.makedirs(tmp_path / "profiles")
    buf = io.StringIO()
    with redirect_stdout(buf):
        bench.emit(full)
    lines = buf.getvalue().splitlines()
    assert len(lines) == 2 and lines[0].startswith("BENCH_DETAIL ") and lines[1].startswith("{")
    assert json.loads(lines[0][len("BENCH_DETAIL "):]) == full
    assert json.loads(lines[1])["detail"] == "profiles/bench_detail_last.json" and len(lines[1]) < 8192
    assert json.load(open(tmp_path / "profiles" / "bench_detail_last.json")) == full


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_dumps_what_it_computed(tmp_path):
    """a plain run (no --full): exactly --steps timed steps and the contract's keys, nothing measured beside the headline; --dump-outputs
    writes float32 / float64 arrays, under 64 MB in all, that agree with the line's counts -- the same arrays whatever the number of steps"""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["MODGPU_BENCH_GBP"] = "0.2"
    dumps = []
    for steps in (3, 4):
        out = tmp_path / ("out%d" % steps)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--dump-outputs", str(out)],
                           capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        j = json.loads(r.stdout.rstrip().splitlines()[-1])
        for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "dtype", "config"):
            assert k in j, k
        assert j["steps"] == steps and j["value"] > 0 and j["ms_per_step"] > 0 and j["higher_is_better"] is True
        for k in ("roofline", "scan_only", "cpu_baseline", "other_configs", "end_to_end"):
            assert k not in j, k
        files = sorted(os.listdir(out))
        assert sum(os.path.getsize(out / f) for f in files) < 64 << 20
        a = {f[:-len(".npy")]: np.load(out / f) for f in files}
        assert all(v.dtype in (np.float32, np.float64) for v in a.values())
        n_hash, entries = a["modset_counts"]
        assert n_hash == j["config"]["modimizers_per_gpu"] and entries == j["config"]["modset_entries"] > 0
        h = a["modset_depth_histogram"]                  # every entry's depth: one per entry, one depth count per modimizer
        assert h[0] == 0 and h.sum() == entries and (h * np.arange(65536)).sum() == n_hash
        idx = a["modset_sample_index"]
        assert 0 < len(idx) == len(a["modset_value_sample"]) == len(a["modset_depth_sample"]) and 1 <= idx.min() and idx.max() <= entries
        assert (a["modset_depth_sample"] >= 1).all() and len(np.unique(a["modset_value_sample"])) == len(idx)
        dumps.append(a)
    assert dumps[0].keys() == dumps[1].keys() and all(np.array_equal(dumps[0][k], dumps[1][k]) for k in dumps[0])
