"""CPU: gr_classifier_set_settle (include/grpath_host.h) — the Phred sums of the insert commits handed over later than the
commits themselves.  A classifier over the oracle engine is driven twice over the same decisions, once with the sums
returned by the commit callback and once through the settle hook; phred_sum_in_path is compared by its 64 bits after every
piece of the run, across the rollovers of a silver run."""
import struct

import numpy as np
import pytest

from helpers import default_seeds
from test_classifier_cpu import _workload


def _phred(commit):
    """a sum per commit whose additions round (no two orders of them give the same bits for long)"""
    return 0.1 * (commit[0] + 1) + 1e-9 * commit[2] + 1.0 / (3 + commit[0])


def _bits(x):
    return struct.pack("<d", x)


def _run(oracle, host, deferred, piece, monkeypatch=None):
    tile, k, h, block = 500, 22, 3, 4
    seeds = default_seeds(h)
    reads = _workload()
    m = oracle.load().orc_calc_optimal_size(1_500_000, 1, 0.1)
    from oracle_engine import OracleEngine

    eng = OracleEngine(oracle, m, seeds, tile, k, reads)
    pending, calls = [], []

    def commit_phred(c):
        if c[1] in (2, 4):
            pending.append(_phred(c))
        return -1.0e300 if deferred else _phred(c)  # (the deferred form must not look at what the callback returns)

    cls = host.Classifier(None, eng.vt, tile=tile, block=block, k=k, h=h, target_bases=60_000, max_paths=4, silver_path=True, max_window=16, commit_phred=commit_phred)

    def settle(n):
        assert 0 < n <= len(pending)
        calls.append((n, len(cls.rollovers)))
        out = pending[:n]
        del pending[:n]
        return out

    if deferred:
        cls.set_settle(settle)
    lens = np.array([len(r) for r in reads], dtype=np.uint32)
    states = []
    for first in range(0, len(reads), piece):
        finished = cls.run_range(None, lens, first, min(piece, len(reads) - first))
        st = cls.state()
        states.append((_bits(st["phred_sum_in_path"]), st["num_reads_in_path"], st["inserted_bases"], st["curr_path"]))
        if deferred:
            assert not pending  # every run ends settled
        if finished:
            break
    return cls, states, calls


@pytest.mark.parametrize("piece", [1, 7, 60])
def test_settled_sums_are_the_commit_callbacks_sums_bit_for_bit(oracle, native, piece):
    from goldrush_amd import host

    a, states_a, _ = _run(oracle, host, False, piece)
    b, states_b, calls = _run(oracle, host, True, piece)
    assert a.commits == b.commits and a.rollovers == b.rollovers
    assert len(a.rollovers) >= 2, a.rollovers  # across rollovers
    assert states_a == states_b
    inserts = sum(1 for c in a.commits if c[1] in (2, 4))
    assert sum(n for n, _ in calls) == inserts >= 10
    assert any(s[0] != _bits(0.0) for s in states_a)
    if piece == 60:
        # one run: the hook is called at every rollover (in front of the rollover callback: the count of rollovers seen then is
        # the number of the call) and once at the end
        assert [r for _, r in calls[:len(a.rollovers)]] == list(range(len(a.rollovers)))
        assert max(n for n, _ in calls) > 1


def test_without_the_hook_nothing_changes(oracle, native):
    """set_settle(None) after set_settle(fn): the commit callback's return values count again"""
    from goldrush_amd import host

    a, states_a, _ = _run(oracle, host, False, 60)
    tile, k, h, block = 500, 22, 3, 4
    from oracle_engine import OracleEngine

    reads = _workload()
    m = oracle.load().orc_calc_optimal_size(1_500_000, 1, 0.1)
    eng = OracleEngine(oracle, m, default_seeds(h), tile, k, reads)
    cls = host.Classifier(None, eng.vt, tile=tile, block=block, k=k, h=h, target_bases=60_000, max_paths=4, silver_path=True, max_window=16, commit_phred=_phred)
    cls.set_settle(lambda n: [0.0] * n)
    cls.set_settle(None)
    lens = np.array([len(r) for r in reads], dtype=np.uint32)
    cls.run_range(None, lens, 0, len(reads))
    assert _bits(cls.state()["phred_sum_in_path"]) == states_a[-1][0]
