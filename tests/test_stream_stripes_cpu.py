"""CPU: the stripe arithmetic of a striped streaming window (goldrush_amd/csrc/host/gr_stream_stripes.hpp: who owns a read,
the owner's tile list, its totals, and where its launch carries on behind an insert) against the Python model the GPU tests
hold — stream_striped_scenario.owner_of, the same expression as oracle_engine.py's stream_begin.  tests/stream_stripes_main.cpp
is built with the address and undefined-behaviour sanitizers and run as a child process; integers are compared exactly."""
import itertools
import os
import subprocess

import numpy as np
import pytest

from stream_striped_scenario import owner_of

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def model(tiles, first, count, stripe, n_owners, owner, xs):
    """what the engine needs of a window, from owner_of alone"""
    win = tiles[first:first + count]
    owns = [n_owners == 1 or owner_of(j, stripe, n_owners) == owner for j in range(count)]
    start = np.concatenate(([0], np.cumsum(win))).astype(int)  # window index of a read's first tile
    tile_list = [int(t) for j in range(count) if owns[j] for t in range(start[j], start[j + 1])]
    out = {"n_mine": sum(win[j] for j in range(count) if owns[j]), "n_decidable": sum(1 for j in range(count) if owns[j] and win[j]),
           "max_tiles_read": max(win) if count else 0, "owns": [int(o) for o in owns], "tiles": tile_list, "resume": []}
    for x in xs:
        mine = [j for j in range(x + 1) if owns[j]]
        out["resume"] += [sum(1 for j in mine if win[j]), sum(win[j] for j in mine)]
    return out


def cases():
    rng = np.random.default_rng(7)
    out = []
    for count, stripe, n_owners in itertools.product((1, 7, 64), (1, 3, 100), (1, 2, 3)):
        for first in (0, 5):
            n_reads = first + count + 3
            tiles = [int(t) for t in rng.integers(0, 6, size=n_reads)]  # 0 .. 5 tiles per read
            if count >= 7:  # several reads without a tile, the window's first and last among them
                for j in (0, 2, 3, count - 1):
                    tiles[first + j] = 0
            xs = sorted({0, count // 2, count - 1})  # an insert at the first, a middle and the last read
            for owner in range(n_owners):
                out.append((tiles, first, count, stripe, n_owners, owner, xs))
    # windows whose first / last read does have tiles, and a window of one read without a tile
    out.append(([3, 0, 0, 5, 1, 0, 2], 0, 7, 3, 2, 1, [0, 3, 6]))
    out.append(([0], 0, 1, 1, 1, 0, [0]))
    out.append(([4], 0, 1, 3, 3, 2, [0]))
    return out


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="the sanitizer build is for machines without a GPU (as tests/test_buffers_cpu.py)")
def test_stripe_function_matches_the_python_model(tmp_path):
    exe = str(tmp_path / "stream_stripes")
    cmd = ["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "goldrush_amd", "csrc"), "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-o", exe, os.path.join(HERE, "stream_stripes_main.cpp")]
    cc = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr[-4000:]
    cs = cases()
    assert {c[2] for c in cs} == {1, 7, 64} and {c[3] for c in cs} == {1, 3, 100} and {c[4] for c in cs} == {1, 2, 3}
    assert any(c[0][c[1]] == 0 and c[0][c[1] + c[2] - 1] == 0 and c[2] > 1 for c in cs) and max(max(c[0]) for c in cs) == 5
    path = str(tmp_path / "cases.txt")
    with open(path, "w") as f:
        for tiles, first, count, stripe, n_owners, owner, xs in cs:
            f.write(" ".join(str(v) for v in [first, count, stripe, n_owners, owner, len(xs), *xs, len(tiles), *tiles]) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe, path], capture_output=True, text=True, timeout=120, env=env)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "stripes done: %d cases" % len(cs)
    for c, line in zip(cs, lines):
        head, owns, tile_list, resume = ([int(v) for v in part.split()] for part in line.split("|"))
        exp = model(*c)
        assert head == [exp["n_mine"], exp["n_decidable"], exp["max_tiles_read"]], c
        assert owns == exp["owns"] and tile_list == exp["tiles"] and resume == exp["resume"], c
