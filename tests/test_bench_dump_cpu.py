"""CPU: bench.py --dump-outputs writes what the last timed step computed — its reads' decisions and a sample of the
filter — as float64 .npy files of at most 64 MB, the same files for the same inputs.  The engine is a stand-in here
(export_ids over a known array); tests/test_gpu_bench_contract.py runs the flag end to end on the GPU."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


class _Engine:
    def __init__(self, pop):
        self.pop = pop

    def export_ids(self, first, n):
        assert 0 <= first and first + n <= self.pop, (first, n)
        x = np.arange(first, first + n, dtype=np.uint64)
        return (x * np.uint64(2654435761) % np.uint64(1 << 32)).astype(np.uint32), (x % np.uint64(7)).astype(np.uint32)


def _dump(d, first, count, pop):
    # commits of the reads in front of the step too (the witness keeps them beside it): the dump holds the step's alone
    commits = [(r, 2 + r % 4, 25, 20, r % 5, r % 9, r // 3, 1, 3000 + r % 11, 12) for r in range(max(first - 1000, 0), first + count)]
    st = {k: (i + 1) * 10 ** 9 for i, k in enumerate(bench.COUNTER_NAMES)}
    line = bench.dump_outputs(str(d), _Engine(pop), commits, first, count, st, pop)
    return line, {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_a_small_step_is_dumped_whole(tmp_path):
    line, arr = _dump(tmp_path, 8192, 4096, 100_000)
    assert set(arr) == {"commit_" + f for f in bench.COMMIT_FIELDS} | {"counters", "mibf_pos", "mibf_ids", "mibf_counts"}
    assert all(a.dtype == np.float64 for a in arr.values())
    assert np.array_equal(arr["commit_read"], np.arange(8192, 8192 + 4096)) and not line["sampled"] and line["commits"] == 4096
    assert np.array_equal(arr["commit_kind"], 2 + arr["commit_read"] % 4) and np.array_equal(arr["commit_first_id"], arr["commit_read"] // 3)
    assert arr["counters"].tolist() == [(i + 1) * 10 ** 9 for i in range(len(bench.COUNTER_NAMES))] + [100_000]
    assert line["counters"] == list(bench.COUNTER_NAMES) + ["pop"]
    ids, counts = _Engine(100_000).export_ids(0, 100_000)  # a filter this small goes out whole
    assert np.array_equal(arr["mibf_pos"], np.arange(100_000)) and np.array_equal(arr["mibf_ids"], ids) and np.array_equal(arr["mibf_counts"], counts)


def test_a_large_step_is_a_fixed_sample_under_64_mb(tmp_path):
    runs = [_dump(tmp_path / t, 9_500_000, 500_000, 6_000_000_000) for t in ("a", "b")]
    for t, (line, arr) in zip(("a", "b"), runs):
        assert line["sampled"] and line["commits"] == bench.DUMP_READS == arr["commit_read"].size
        r = arr["commit_read"]
        assert r.min() >= 9_500_000 and r.max() < 10_000_000 and np.all(np.diff(r) > 0)
        pos = arr["mibf_pos"]
        assert pos.size == bench.DUMP_MIBF_RUNS * bench.DUMP_MIBF_RUN and pos.max() < 6_000_000_000
        i0 = int(pos[0])
        assert np.array_equal(arr["mibf_ids"][:bench.DUMP_MIBF_RUN], _Engine(6_000_000_000).export_ids(i0, bench.DUMP_MIBF_RUN)[0])
        assert sum(os.path.getsize(tmp_path / t / f) for f in os.listdir(tmp_path / t)) <= 64 << 20
    (_, a), (_, b) = runs
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
