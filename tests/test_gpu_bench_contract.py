"""GPU: bench.py keeps the driver's contract — one JSON line from rank 0 with the metric,
the roofline object of the query kernel and, with --full, (N = 1) the CPU baseline."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check_headline(d):
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
                "roofline", "phases"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 2 and d["higher_is_better"] is True and d["scaling"] == "strong"
    assert d["unit"] == "reads/s" and d["value"] > 0 and d["vs_baseline"] is None and d["data"] == "synthetic" and "workload" in d["config"]
    assert d["metric"] == "reads/s through GoldRush-Path (hash + miBF query)" and d["dtype"] == "u64"
    assert abs(d["value"] - 3 * 4096 / (d["ms_per_step"] * 3e-3)) / d["value"] < 1e-6
    ph = d["phases"]
    assert ph["head"]["reads"] + ph["steady"]["reads"] == 3 * 4096 and d["config"]["reads_timed"] == 3 * 4096


def test_a_plain_run_prints_the_headline_alone():
    """Without --full the run is setup, warm-up, the timed steps and the line: the passes behind the timed steps (CPU
    baseline with the oracle's check, the silver-mode pass) are not run and their fields are not in the line; what the
    timed steps and the setup measured themselves (roofline, phases, aux) is."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "C1", "--steps", "3", "--warmup", "2", "--reads", "60000", "--batch", "4096"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    _check_headline(d)
    assert "cpu_baseline" not in d and "oracle_check" not in d["aux"] and "pipeline_shaped" not in d["aux"]
    assert d["roofline"]["line_rate_Gprobes_per_s"] > 0 and d["aux"]["end_to_end"]["classify_s"] > 0 and d["aux"]["counters"]["reads_committed"] == 3 * 4096


def test_bench_line_has_the_contract_fields():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "1", "--config", "C1", "--steps", "3", "--warmup", "2", "--reads", "60000", "--batch", "4096"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
                "roofline", "cpu_baseline", "phases"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 2 and d["higher_is_better"] is True and d["scaling"] == "strong"
    assert d["unit"] == "reads/s" and d["value"] > 0 and d["vs_baseline"] is None and d["data"] == "synthetic" and "workload" in d["config"]
    assert abs(d["value"] - 3 * 4096 / (d["ms_per_step"] * 3e-3)) / d["value"] < 1e-6
    rf = d["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-9 and 0 < rf["frac"] < 1
    assert rf["traffic"] is None or rf["traffic"] > 0
    assert rf["bytes_per_probe"] == 128 and rf["line_rate_Gprobes_per_s"] > 0
    ph = d["phases"]
    assert ph["head"]["reads"] + ph["steady"]["reads"] == 3 * 4096 and d["config"]["reads_timed"] == 3 * 4096
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["value"] > 0 and cb["cores"] >= 1 and cb["unit"] == "reads/s" and cb["sample"]
    # --full: the oracle replayed the witness reads and agrees; the silver-mode pass ran behind the timed steps
    oc = d["aux"]["oracle_check"]
    assert oc["identical"] is True and oc["head_reads"] > 0
    assert d["aux"]["pipeline_shaped"]["reads_consumed"] > 0


def test_dump_outputs_hold_the_last_step_and_repeat(tmp_path):
    """--dump-outputs DIR: the decisions of the last timed step's reads and a sample of the filter behind them, float64,
    the same files from two runs with the same arguments (the inputs come from fixed seeds, the path is order-exact)."""
    import numpy as np

    args = ["--gpus", "1", "--config", "C1", "--steps", "3", "--warmup", "1", "--reads", "60000", "--batch", "4096", "--no-cpu-baseline", "--no-pipeline-shaped"]
    runs = []
    for tag in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args + ["--dump-outputs", str(tmp_path / tag)], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        arr = {f[:-4]: np.load(tmp_path / tag / f) for f in os.listdir(tmp_path / tag)}
        assert d["steps"] == 3 and d["aux"]["dump_outputs"]["reads_of_last_step"] == [2 * 4096, 3 * 4096]
        assert all(a.dtype == np.float64 for a in arr.values())
        assert sum(os.path.getsize(tmp_path / tag / f) for f in os.listdir(tmp_path / tag)) <= 64 << 20
        assert np.array_equal(arr["commit_read"], np.arange(2 * 4096, 3 * 4096))
        assert set(np.unique(arr["commit_kind"]).tolist()) <= {2, 3, 4, 5}
        assert arr["counters"][-1] == d["aux"]["pop"] and arr["counters"][:-1].tolist() == [d["aux"]["counters"][k] for k in d["aux"]["dump_outputs"]["counters"][:-1]]
        assert arr["mibf_ids"].size == arr["mibf_counts"].size == arr["mibf_pos"].size > 0
        runs.append(arr)
    a, b = runs
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


def test_two_ranks_on_the_one_gpu_end_where_one_rank_ends():
    """The N > 1 path end to end on the one available GPU (two processes share it): sharded fill
    merged by reduce-scatter + all-gather, batches with striped queries, striped streaming
    windows, the shared-memory exchange.  The run's counters (tiles, hits, misses, inserted
    bases, IDs, inserts) and the filter's population must equal the single-rank run's — not
    just agree between the ranks."""
    common = ["--config", "C1", "--steps", "4", "--reads", "120000", "--no-cpu-baseline"]
    one = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + common, capture_output=True, text=True, timeout=900)
    assert one.returncode == 0, one.stderr[-2000:]
    # round 6: no launcher around it — `bench.py --gpus 2` starts its two ranks itself (bench.py launch_ranks)
    env = {k_: v_ for k_, v_ in os.environ.items() if k_ not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    two = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--share-gpu", "--verify-ranks"] + common,
                         capture_output=True, text=True, timeout=900, env=env)
    assert two.returncode == 0, two.stderr[-3000:]
    a = json.loads([l for l in one.stdout.splitlines() if l.startswith("{")][-1])
    b = json.loads([l for l in two.stdout.splitlines() if l.startswith("{")][-1])
    assert b["n_gpus"] == 2 and a["n_gpus"] == 1
    assert a["aux"]["pop"] == b["aux"]["pop"]
    assert a["aux"]["counters"] == b["aux"]["counters"]
    assert a["aux"]["counters"]["inserts"] > 1000 and b["aux"]["timed"]["batches"] > 10
    # round 5: the merge of the sharded fill is the product's (csrc/host/gr_ranks.cpp: staged here, the ranks share the
    # device; RCCL where every rank has its own), and the ranks' striped windows apply inserts inside their launches
    assert b["aux"]["comm"]["world"] == 2 and b["aux"]["comm"]["merge"].startswith("staged"), b["aux"]["comm"]
    assert b["aux"]["timed"]["stream_inserts"] > 0, b["aux"]["timed"]
