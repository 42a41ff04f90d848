"""GPU: seeds whose span exceeds 64 bases (k + h - 1 up to 256; the long-span kernels, grp_kernels.inc seed_hash_long)
against the CPU oracle, bit for bit: tile hashes, fill, inserts, queries and the classification window; ntCard tables;
the order-exact forms (a resumable streaming window that applies inserts itself and keeps tiles, batches) against the
oracle's serial loop (process_read, goldrush_path.cpp:892-1094); spans beyond 256 refused."""
import numpy as np
import pytest

from helpers import compare_queries, default_seeds, keep_stream, low_error_reads, palindromic_preset, random_reads, stream_resumable

pytestmark = pytest.mark.gpu


def _long_seeds(k, h, seed):
    seeds = default_seeds(h, palindromic_preset(k, 30, seed))
    assert [len(s) for s in seeds] == [k + i for i in range(h)]
    assert all(s[-1] == "1" and s.count("1") <= 32 for s in seeds)
    return seeds


@pytest.mark.parametrize("k,h,tile", [(63, 3, 400), (65, 1, 300), (96, 3, 500), (128, 5, 700), (200, 3, 1000), (254, 3, 600), (129, 1, 129)])
def test_long_spans_match_oracle(oracle, native, k, h, tile):
    """(63, 3): the family's spans are 63 - 65, the 64-base boundary inside it; (254, 3): the longest seed is 256 bases;
    (129, 1, 129): a tile of exactly one span.  Reads shorter than the longest span, exactly that long, a tile + span - 2
    long, and reads whose last tile is clipped."""
    from goldrush_amd import host

    seeds = _long_seeds(k, h, 7 + k)
    span = k + h - 1
    m = oracle.load().orc_calc_optimal_size(300_000, 1, 0.1)
    eng = native.Engine(k, h, tile, m, seeds)
    oseeds = oracle.Seeds(seeds)
    omf = oracle.MiBF(m, oseeds, tile, k)
    reads = random_reads(5, 2 * tile + span, 6 * tile + 70, seed=151 + k)
    reads += [reads[0][: 3 * tile // 2 + k - 2], reads[1][: 2 * tile + span - 2], b"ACGT" * (tile // 2 + span // 4 + 1), reads[2][: tile + 3],
              reads[3][: span - 1], reads[4][:span], reads[0][: tile + span - 2], reads[1][: 3 * tile + 1]]
    b = eng.upload(reads)
    n_tiles = 0
    for ri, seq in enumerate(reads):
        for t in range(len(seq) // tile):
            got, exp = eng.tile_hashes(b, ri, t), oseeds.tile_hashes(seq, tile, k, t)
            assert got.shape == exp.shape and np.array_equal(got, exp), (ri, t)
            n_tiles += 1
    assert n_tiles >= 20
    eng.bv_insert(b)
    for sq in reads:
        if len(sq) >= span:  # the fill skips reads shorter than the longest seed (process_read: "too short")
            omf.bv_insert_read(sq)
    assert eng.finalize() == omf.finalize()
    assert np.array_equal(eng.export_bits(), omf.bits())
    for ri in (0, 2, 5, 6):
        nt = len(reads[ri]) // tile
        eng.insert_tiles(b, ri, 0, nt, ri + 1)
        omf.insert_read_tiles(reads[ri], 0, nt, ri + 1)
    ids, counts = eng.export_ids()
    assert np.array_equal(ids, omf.ids()) and np.array_equal(counts, omf.counts())
    assert counts.any()
    assert compare_queries(eng, omf, b, reads)[1] > 0
    # whole reads in ID blocks of 2 tiles (k_insert_collect + k_insert_apply) on top of the tile inserts above
    for ri in (1, 3):
        nt = len(reads[ri]) // tile
        eng.insert_read(b, ri, 0, nt, 2, 40 + ri, 0)
        for bs in range(0, nt, 2):
            omf.insert_read_tiles(reads[ri], bs, min(bs + 2, nt), 40 + ri + bs // 2)
    ids, counts = eng.export_ids()
    assert np.array_equal(ids, omf.ids()) and np.array_equal(counts, omf.counts())
    compare_queries(eng, omf, b, reads)
    # the classification window (hash + query + decisions in one call) against the host decision on the queried tiles
    dp = dict(threshold=2, unassigned_min=2, assigned_max=1 << 30)
    dec = eng.classify_reads(b, 0, len(reads), **dp)
    tiles, lists, _ = eng.query_tiles(b)
    lists_arr = np.ascontiguousarray(lists) if len(lists) else np.zeros(1, dtype=native.id_count_dtype)
    for ri in range(len(reads)):
        a0, e0 = int(b.tile0[ri]), int(b.tile0[ri + 1])
        t = np.ascontiguousarray(tiles[a0:e0]) if e0 > a0 else np.zeros(1, dtype=native.tile_summary_dtype)
        d = host.decide_read(t, lists_arr, e0 - a0, **dp)
        got = dec[ri]
        assert (int(got["kind"]), int(got["num_tiles"]), int(got["num_assigned"]), int(got["hits"]), int(got["misses"])) == (d.kind, d.num_tiles, d.num_assigned, d.hits, d.misses), ri
    eng.close()


@pytest.mark.parametrize("k,h", [(128, 2), (254, 3)])
def test_long_span_ntcard_tables_match_oracle(oracle, native, k, h):
    """grp_ntcard_* at longest spans of 129 and 256 bases against the oracle: zero buckets of every sample table for plain
    reads, reads shorter than the longest span (the iterator rule), ACGT runs with explicit stale repeats; then the
    deferred filter size and the fill."""
    from goldrush_amd import host

    seeds = _long_seeds(k, h, 3 + k)
    span = k + h - 1
    osd = oracle.Seeds(seeds)
    rng = np.random.default_rng(92 + k)
    reads = random_reads(30, 1500, 9000, seed=91 + k)
    reads += [reads[0][:k], reads[1][: k + 1], reads[2][: span - 1], reads[3][:span], reads[4][: span + 1], reads[5][: k - 1]]
    dirty = []
    for i, r in enumerate(random_reads(6, 800, 5000, seed=93 + k)):
        r = bytearray(r)
        for p in rng.integers(0, len(r), size=2 + i):
            r[p] = ord("N")
        dirty.append(bytes(r))
    tile = 500
    eng = native.Engine(k, h, tile, 0, seeds)
    b = eng.upload(reads)
    eng.ntcard_begin(7)
    eng.ntcard_add(b, 0, 13)
    eng.ntcard_add(b, 13)
    runs_all, extra_all = [], []
    for seq in dirty:
        runs, extra = host.ntcard_split(seq, k, h)
        runs_all += [seq[o:o + n] for o, n in runs]
        extra_all.append(extra)
    b2 = eng.upload(runs_all)
    eng.ntcard_add(b2, stale_extra=np.concatenate(extra_all).ravel())
    z = eng.ntcard_finish()
    nc = oracle.NtCard(osd, 1000)
    for seq in reads + dirty:
        nc.add_read(seq)
    assert np.array_equal(z, nc.zero_buckets())
    assert int((z < (1 << 27)).sum()) == 2 * h  # every table was hit
    for s in range(h):
        assert host.load().gr_ntcard_f0(int(z[s][0]), int(z[s][1]), 7) == nc.f0(s)
    m = oracle.load().orc_calc_optimal_size(sum(nc.f0(s) for s in range(h)), 1, 0.1)
    nc.close()
    eng.set_filter_size(m)
    eng.bv_insert(b)
    omf = oracle.MiBF(m, osd, tile, k)
    for seq in reads:
        if len(seq) >= span:
            omf.bv_insert_read(seq)
    assert eng.finalize() == omf.finalize()
    assert np.array_equal(eng.export_bits(), omf.bits())
    eng.close()


# ---- the order-exact forms at a span of 128 bases ----------------------------------------------------------------------
# Reads with few errors (long seeds lose a frame to any error in their span): a covered genome yields hits.

K_LONG, H_LONG = 126, 3  # spans 126 - 128


def test_long_span_window_applies_inserts_itself(oracle, native):
    """The head of a path at spans 124 - 128 (h = 5): most reads insert, in the launch; records and the final ID / count
    arrays equal the serial loop's."""
    from oracle_engine import serial_reference

    k, h, tile, block = 124, 5, 500, 4
    seeds = _long_seeds(k, h, 41)
    _, reads = low_error_reads(150_000, 90, 31)
    reads.insert(7, reads[3][: tile - 1])  # a read without a single tile
    m = oracle.load().orc_calc_optimal_size(2_000_000, 1, 0.1)
    exp, mf_ref = serial_reference(oracle, m, seeds, tile, k, reads, block=block)
    eng = native.Engine(k, h, tile, m, seeds)
    b = eng.upload(reads)
    eng.bv_insert(b)
    assert eng.finalize() == mf_ref.pop
    got = stream_resumable(eng, b, reads, tile, block)
    assert got == exp
    kinds = [g[1] for g in got]
    assert sum(q in (2, 4) for q in kinds) >= 10 and sum(q not in (2, 4) for q in kinds) >= 10
    ids, counts = eng.export_ids()
    assert np.array_equal(ids, mf_ref.ids()) and np.array_equal(counts, mf_ref.counts())
    mf_ref.close()
    eng.close()


def test_long_span_window_keeps_tiles(oracle, native):
    """tests/stream_keep_scenario.py's stream at spans 126 - 128: the in-launch inserts keep the tiles they can (the
    kept-tile path of the streaming kernel) and query the dirty ones again; the serial loop's records and arrays."""
    from oracle_engine import serial_reference

    tile, block = 500, 4
    seeds = _long_seeds(K_LONG, H_LONG, 43)
    reads = keep_stream()
    m = oracle.load().orc_calc_optimal_size(2_500_000, 1, 0.1)
    exp, mf_ref = serial_reference(oracle, m, seeds, tile, K_LONG, reads, block=block)
    eng = native.Engine(K_LONG, H_LONG, tile, m, seeds)
    b = eng.upload(reads)
    eng.bv_insert(b)
    assert eng.finalize() == mf_ref.pop
    got = stream_resumable(eng, b, reads, tile, block)
    assert got == exp
    ids, counts = eng.export_ids()
    assert np.array_equal(ids, mf_ref.ids()) and np.array_equal(counts, mf_ref.counts())
    st = eng.stream_stats()
    n_ins = sum(1 for g in got if g[1] in (2, 4))
    assert n_ins >= 10 and sum(1 for g in got[70:] if g[1] not in (2, 4)) >= 150, "the stream is not what the test means"
    assert st["inserts_kept"] + st["inserts_kept_nothing"] == n_ins
    assert st["inserts_kept"] > 0 and st["tiles_kept"] > 0, st
    assert st["coop_refused"] == 0
    mf_ref.close()
    eng.close()


@pytest.mark.parametrize("window,verify", [(7, None), (32, "check"), (32, "chain")])
def test_long_span_batches_equal_the_serial_loop(oracle, native, window, verify):
    """Windows committed as batches (grp_batch_insert_reads / _classify / _verify / _undo; k_batch_collect, k_batch_delta,
    the batch-view queries) at spans 126 - 128, by tests/test_gpu_batch.py's driver."""
    from oracle_engine import serial_reference
    from test_gpu_batch import batch_commit

    tile, block = 500, 4
    seeds = _long_seeds(K_LONG, H_LONG, 47)
    _, reads = low_error_reads(150_000, 140, 21)
    m = oracle.load().orc_calc_optimal_size(2_000_000, 1, 0.1)
    exp, mf_ref = serial_reference(oracle, m, seeds, tile, K_LONG, reads, block=block)
    eng = native.Engine(K_LONG, H_LONG, tile, m, seeds)
    b = eng.upload(reads)
    eng.bv_insert(b)
    assert eng.finalize() == mf_ref.pop
    stats = {"batches": 0, "undone": 0}
    got = batch_commit(eng, b, reads, tile, block, window, stats, verify)
    assert got == [e[:7] for e in exp]
    ids, counts = eng.export_ids()
    assert np.array_equal(ids, mf_ref.ids()) and np.array_equal(counts, mf_ref.counts())
    assert stats["batches"] > 0 and {e[1] for e in exp} >= {2, 3}
    if verify is not None:
        vs = eng.verify_stats()
        assert vs["fallbacks"] == 0 and vs["impossible_deltas"] == 0, vs
    mf_ref.close()
    eng.close()


def test_spans_beyond_256_are_refused(native):
    with pytest.raises(native.GrpError, match="256"):
        native.Engine(257, 1, 1000, 1 << 20, [palindromic_preset(257, 30, 1)])
    with pytest.raises(native.GrpError, match="256"):
        native.Engine(254, 4, 1000, 1 << 20, default_seeds(4, palindromic_preset(254, 30, 2)))  # longest seed 257
    eng = native.Engine(253, 4, 1000, 1 << 20, default_seeds(4, palindromic_preset(253, 30, 3)))  # longest seed 256: accepted
    eng.close()
