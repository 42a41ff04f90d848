"""GPU: a striped resumable streaming window (grp_classify_stream_begin_striped_resumable + grp_classify_stream_insert),
record by record against the oracle's serial loop (process_read, goldrush_path.cpp:892-1094).  What a multi-GPU run scales
on: every rank's launch owns the tiles of its stripes through an index list, takes EVERY insert of the window — its own
(it has parked at the record) and the other ranks' (the command finds it in the middle of a tile, or idle, all of its own
stripes decided) — and holds the tiles it keeps against the slots the insert changed.  tests/stream_striped_scenario.py
drives one rank at a time; the oracle's commit tuples stand for the ranks' record exchange.

hits / misses of a record DEPEND on the ID state (an empty ID slot is a miss, orc_query_tile), so the oracle's figures are
taken inside the serial loop, at the state the reference queries the read in (serial_reference's `counters`): a reference.
Beside it the records are held against the one-rank window of stream_keep_scenario.run over the same stream: a consistency
check, not a reference."""
import time

import numpy as np
import pytest

from helpers import default_seeds, low_error_reads

pytestmark = pytest.mark.gpu

GEOMETRIES = [(2, 7), (3, 1), (3, 64)]  # (ranks, reads per stripe); (3, 64): rank 0's stripes end at read 255, in front of the last cluster


class Case:
    def __init__(self, oracle, g, seeds, m, reads, count_lists=False):
        from oracle_engine import serial_reference

        self.g, self.seeds, self.m, self.reads = g, seeds, m, reads
        self.counters = []
        self.exp, mf = serial_reference(oracle, m, seeds, g.tile, g.k, reads, block=g.block, counters=self.counters)
        self.ids, self.counts, self.pop = mf.ids().copy(), mf.counts().copy(), mf.pop
        # the count > 2 lists of all tiles at the final state, against the window's list arena (8 entries per tile + 4096,
        # stream_begin_impl): a launch that runs out of it hands the read back (kind 0) — the host's synchronous path, not
        # what these tests are about
        self.list_entries = sum(len(t[2]) for s in reads for t in mf.query_read(s)) if count_lists else None
        self.list_arena = 8 * sum(len(s) // g.tile for s in reads) + 4096
        mf.close()
        self.n_tiles = [len(s) // g.tile for s in reads]
        self.inserts = sum(1 for e in self.exp if e[1] in (2, 4))


@pytest.fixture(scope="module")
def keep_case(oracle):
    import stream_striped_scenario as ss

    m = oracle.load().orc_calc_optimal_size(2_500_000, 1, 0.1)
    return Case(oracle, ss.KEEP_GEOMETRY, default_seeds(ss.KEEP_GEOMETRY.h), m, ss.make_stream())


@pytest.fixture(scope="module")
def one_rank(keep_case, native):
    """the same stream through ONE rank's window: what the striped records' hits / misses are held against beside the oracle's"""
    import stream_keep_scenario as sc

    c = keep_case
    r = sc.run(native, c.seeds, c.m, c.reads, limit=20.0)
    assert [t[:8] for t in r["records"]] == c.exp
    return {t[0]: (t[8], t[9]) for t in r["records"]}


def _run_and_check(native, c, n_owners, stripe, when):
    """every rank of the window, one after the other -> (results, the stream's properties); the assertions every case makes"""
    import stream_striped_scenario as ss

    n = len(c.reads)
    props = ss.stream_properties(c.exp, c.n_tiles, stripe, n_owners)
    for o, p in enumerate(props["owners"]):  # the stream means what the test intends: inserts of its own and of the others for every rank
        assert p["own"] >= 1 and p["not_own"] >= 1, (o, p)
    t0 = time.time()
    res = [ss.run_owner(native, c.g, c.seeds, c.m, c.reads, c.exp, stripe, n_owners, o, when) for o in range(n_owners)]
    print("striped window: %d ranks, stripes of %d, %s: %.2f s (windows alone: %s)" % (n_owners, stripe, when, time.time() - t0, ", ".join("%.2f" % r["window_s"] for r in res)))
    for j in range(n):  # every read is one rank's (or, without a tile, the host's with every rank), and its record is the serial loop's
        if c.n_tiles[j] == 0:
            assert all(r["host"][j] == c.exp[j] for r in res) and not any(j in r["own"] for r in res), j
            continue
        holders = [o for o, r in enumerate(res) if j in r["own"]]
        assert holders == [ss.owner_of(j, stripe, n_owners)], (j, holders)
        rec = res[holders[0]]["own"][j]
        assert rec[:8] == c.exp[j], (j, rec, c.exp[j])
        assert rec[1] != 0
        assert rec[8:10] == c.counters[j], "read %d: hits / misses %s, the oracle's serial loop counts %s" % (j, rec[8:10], c.counters[j])
    for o, r in enumerate(res):
        assert r["pop"] == c.pop
        assert np.array_equal(r["ids"], c.ids) and np.array_equal(r["counts"], c.counts), "rank %d's replica differs from the serial loop's arrays" % o
        assert r["generation"] == 1 + c.inserts
        gens = [rec[10] for _, rec in sorted(r["own"].items())]
        assert gens == sorted(gens) and all(1 <= q <= r["generation"] for q in gens)  # (each was taken at the generation current then: run_owner)
        st = r["stats"]
        assert st["inserts_kept"] + st["inserts_kept_nothing"] == c.inserts, (o, st)  # every insert in the launch, the other ranks' too
        assert st["coop_refused"] == 0
        assert r["decided"] == sum(1 for j in range(n) if c.n_tiles[j] == 0 or ss.owner_of(j, stripe, n_owners) == o)
    return res, props


@pytest.mark.parametrize("when", ["eager", "late"])
@pytest.mark.parametrize("n_owners,stripe", GEOMETRIES)
def test_striped_window_record_by_record(native, keep_case, one_rank, n_owners, stripe, when):
    import stream_striped_scenario as ss

    c = keep_case
    assert c.inserts >= 30
    assert [j for j in range(len(c.reads)) if c.n_tiles[j] == 0] == [at for at, _ in ss.NO_TILE_READS]
    no_tile_owners = {ss.owner_of(at, stripe, n_owners) for at, _ in ss.NO_TILE_READS}
    assert len(no_tile_owners) == min(n_owners, len(ss.NO_TILE_READS)), "the reads without a tile lie in different ranks' stripes"
    res, props = _run_and_check(native, c, n_owners, stripe, when)
    assert any(p["behind_last_own_read"] >= 1 for p in props["owners"]), props  # a launch that has decided all it owns and must stay
    for r in res:
        for j, rec in r["own"].items():
            assert rec[8:10] == one_rank[j], "read %d: hits / misses %s, the one-rank window says %s" % (j, rec[8:10], one_rank[j])
    if when == "late":
        for o, r in enumerate(res):  # a record published under the old state, replaced under the new generation (run_owner checks each)
            assert len(r["stale"]) >= 1 and len(r["stale"]) == props["owners"][o]["not_own_with_own_read_behind"], (o, len(r["stale"]), props["owners"][o])
    assert sum(r["stats"]["tiles_kept"] for r in res) > 0
    assert sum(r["stats"]["tiles_redone_dirty"] for r in res) > 0
    assert any(r["stats"]["inserts_kept"] > 0 for r in res)


def _h5_case(oracle, tile, seed, mean_len):
    import stream_striped_scenario as ss

    g = ss.Geometry(22, 5, tile, 4)
    _, reads = low_error_reads(300_000, 120, seed, mean_len=mean_len)
    m = oracle.load().orc_calc_optimal_size(10_000_000, 1, 0.1)
    c = Case(oracle, g, default_seeds(g.h), m, reads, count_lists=True)
    assert c.inserts >= 10 and len(reads) - c.inserts >= 10
    return c


def test_striped_window_that_can_keep_nothing(oracle, native):
    """A geometry whose LDS has no room for a single fingerprint buffer: every insert hands everything behind its read out
    again (SCT_SCAN_END's STREAM_FULL_RESET), through the stripe's tile list.  h = 5 with tiles of 1500: the count table and
    the seed tables take 49 KB, one buffer of fingerprints (7 passes x 256 lanes x 5 seeds) 36 KB more — 85 KB, above what
    two workgroups per CU leave each other of the 160 KB (launch_query wants min(what fits without, 3) resident).
    (h = 5 with tiles of 1000, where launch_query's comment expects the same, does keep on the MI355X: the test below.)"""
    c = _h5_case(oracle, 1500, 53, 8500)
    assert c.list_entries <= c.list_arena  # the arena starts over at every insert of such a window: one walk's lists fit
    res, _ = _run_and_check(native, c, 2, 7, "eager")
    for r in res:
        assert r["stats"]["inserts_kept"] == 0 and r["stats"]["tiles_kept"] == 0, r["stats"]
        assert r["stats"]["inserts_kept_nothing"] == c.inserts


def test_striped_window_h5_tiles_of_1000(oracle, native):
    """h = 5 with tiles of 1000 (48 KB of count table), striped: the serial loop's records and arrays.  launch_query's
    comment says this geometry keeps nothing; on the MI355X its k_query instance is resident twice per CU, not three
    times, one fingerprint buffer (5 passes: 25 KB) fits beside that, and the window does keep (measured with 40 inserts
    and two ranks: 20 and 31 of them kept tiles) — so nothing is asserted here about what is kept."""
    c = _h5_case(oracle, 1000, 51, 6500)
    assert c.list_entries <= c.list_arena // 4  # kept tiles pin their lists until the arena is three quarters full: the last quarter takes a whole walk
    _run_and_check(native, c, 2, 7, "eager")


def test_a_rank_without_a_stripe(oracle, native):
    """stripes as long as the window: rank 1 owns nothing.  Its window begins, takes no insert (there is no launch), ends
    with no record of its own — and the engine classifies as before."""
    import stream_striped_scenario as ss
    from goldrush_amd.native import GRP_ERR_STATE, GrpError

    g = ss.KEEP_GEOMETRY
    seeds = default_seeds(g.h)
    _, reads = low_error_reads(60_000, 12, 61)
    omf = oracle.MiBF(oracle.load().orc_calc_optimal_size(400_000, 1, 0.1), oracle.Seeds(seeds), g.tile, g.k)
    for s in reads:
        omf.bv_insert_read(s)
    omf.finalize()
    eng = native.Engine(g.k, g.h, g.tile, omf.m, seeds)
    try:
        b = eng.upload(reads)
        eng.bv_insert(b)
        assert eng.finalize() == omf.pop
        n = len(reads)
        v = eng.stream_begin(b, 0, n, 0, stripe=n, n_owners=2, owner=1, resumable=True)
        try:
            assert not eng.stream_resumable(0)
            with pytest.raises(GrpError) as err:
                eng.stream_insert(0, 0, 0, len(reads[0]) // g.tile, g.block, 1, 0)
            assert err.value.code == GRP_ERR_STATE
            t0 = time.time()
            while not eng.stream_poll(0):
                assert time.time() - t0 < 20.0
            assert not v["pad"].any()
        finally:
            decided = eng.stream_end(0)
        assert decided == 0
        # ... and the engine is what it was: the first read's insert the classic way (nothing is inserted yet, it starts
        # the path), and the reads behind it classified against it
        nt0 = len(reads[0]) // g.tile
        assert nt0 >= 5
        for bs in range(0, nt0, g.block):
            omf.insert_read_tiles(reads[0], bs, min(bs + g.block, nt0), 1 + bs // g.block)
        eng.insert_read(b, 0, 0, nt0, g.block, 1, 0)
        exp = []
        for seq in reads[1:]:
            res = omf.query_read(seq)
            na = oracle.smooth_tiles([t[0] for t in res], [t[2] for t in res], 10)[2]
            exp.append((len(res), na, sum(t[3][1] for t in res), sum(t[3][2] for t in res)))
        got = [(int(q["num_tiles"]), int(q["num_assigned"]), int(q["hits"]), int(q["misses"])) for q in eng.classify_reads(b, 1, n - 1)]
        assert got == exp
        assert sum(e[1] for e in exp) > 0  # some of them overlap the first read: its insert is seen
        ids, counts = eng.export_ids()
        assert np.array_equal(ids, omf.ids()) and np.array_equal(counts, omf.counts())
    finally:
        eng.close()
        omf.close()
