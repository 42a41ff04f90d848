"""GPU: seeds whose span exceeds 64 bases (k + h - 1 up to 256; the long-span kernels, grp_kernels.inc seed_hash_long)
against the CPU oracle, bit for bit: tile hashes, fill, inserts, queries and the classification window; ntCard tables;
the order-exact forms (a resumable streaming window that applies inserts itself and keeps tiles, batches) against the
oracle's serial loop (process_read, goldrush_path.cpp:892-1094); spans beyond 256 refused."""
import time

import numpy as np
import pytest

from helpers import canon_list, default_seeds, random_reads

pytestmark = pytest.mark.gpu


def _symmetric_seed(k, weight, seed):
    """A palindromic care pattern of span k whose ends are care positions (the last one at base k - 1), ~weight ones."""
    rng = np.random.default_rng(seed)
    half = k // 2
    left = np.zeros(half, dtype=bool)
    left[0] = True
    left[rng.choice(np.arange(1, half), size=max(weight // 2 - 1, 0), replace=False)] = True
    s = "".join("1" if b else "0" for b in left)
    return s + ("1" if k % 2 else "") + s[::-1]


def _long_seeds(k, h, seed):
    seeds = default_seeds(h, _symmetric_seed(k, 30, seed))
    assert [len(s) for s in seeds] == [k + i for i in range(h)]
    assert all(s[-1] == "1" and s.count("1") <= 32 for s in seeds)
    return seeds


def _compare_queries(eng, omf, batch, reads):
    tiles, lists, stats = eng.query_tiles(batch)
    ti = q = hh = ms = 0
    for seq in reads:
        for top_id, top_count, lst, ctr in omf.query_read(seq):
            t = tiles[ti]
            assert (int(t["top_id"]), int(t["top_count"])) == (top_id, top_count), ti
            got = [(int(a), int(c)) for a, c in lists[t["list_off"]: t["list_off"] + t["list_n"]]]
            assert got == canon_list(lst), ti
            q += ctr[0]
            hh += ctr[1]
            ms += ctr[2]
            ti += 1
    assert ti == len(tiles)
    assert (stats["queries"], stats["hits"], stats["misses"]) == (q, hh, ms)
    return hh


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
    assert _compare_queries(eng, omf, b, reads) > 0
    # whole reads in ID blocks of 2 tiles (k_insert_collect + k_insert_apply) on top of the tile inserts above
    for ri in (1, 3):
        nt = len(reads[ri]) // tile
        eng.insert_read(b, ri, 0, nt, 2, 40 + ri, 0)
        for bs in range(0, nt, 2):
            omf.insert_read_tiles(reads[ri], bs, min(bs + 2, nt), 40 + ri + bs // 2)
    ids, counts = eng.export_ids()
    assert np.array_equal(ids, omf.ids()) and np.array_equal(counts, omf.counts())
    _compare_queries(eng, omf, b, reads)
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


def _reads(genome_len, n, seed, mean_len=5000):
    from goldrush_amd import synth

    g = synth.random_genome(genome_len, seed)
    return g, [r[1] for r in synth.make_reads(g, n, mean_len=mean_len, min_len=3500, seed=seed + 1, max_len=9000, sub=0.004, ins=0.0005, dele=0.0005)]


def _keep_stream():
    """tests/stream_keep_scenario.py's stream with few errors: reads of a covered genome, and clusters of overlapping reads of
    uncovered islands in between — the first read of a cluster inserts, the ones behind it (queried by the launch BEFORE
    that insert) must be decided against it"""
    from goldrush_amd import synth

    ga = synth.random_genome(160_000, 101)
    mk = lambda n, seed: [r[1] for r in synth.make_reads(ga, n, mean_len=5000, min_len=3500, seed=seed, max_len=9000, sub=0.004, ins=0.0005, dele=0.0005)]
    reads = mk(70, 102) + mk(260, 103)
    rng = np.random.default_rng(104)
    for i, at in enumerate((120, 170, 230, 300)):
        gb = synth.random_genome(9_000, 200 + i)
        cluster = [gb[o:o + 6000].tobytes() for o in (0, 1500, 3000, 700)]
        for j, s in enumerate(cluster):
            reads.insert(at + j + int(rng.integers(0, 2)), s)
    return reads


def _stream_resumable(eng, b, reads, tile, block, limit=120.0):
    """ONE resumable window over all reads; every insert record answered with stream_insert (the IDs the serial loop
    allocates) -> the commit tuples of oracle_engine.serial_reference"""
    n = len(reads)
    v = eng.stream_begin(b, 0, n, 0, resumable=True)
    gen, ids_inserted = 1, 0
    got = []
    for j in range(n):
        t0 = time.time()
        while int(v["pad"][j]) != gen:
            assert time.time() - t0 < limit, "record %d of generation %d never came" % (j, gen)
            assert not eng.stream_poll(0) or int(v["pad"][j]) == gen, "the launch ended without record %d" % j
        d = v[j].copy()
        kind = int(d["kind"])
        assert kind != 0
        first_id = 0
        if kind in (2, 4):
            ids_inserted += 1
            first_id = ids_inserted
            if kind == 2:
                ts, te, off = 0, int(d["num_tiles"]), 0
                ids_inserted += len(reads[j]) // (tile * block)
            else:
                ts, te, off = int(d["trim_start"]), int(d["trim_end"]) + 1, 1
                ids_inserted += (int(d["trim_end"]) - int(d["trim_start"])) // block
            gen = eng.stream_insert(0, j, ts, te, block, first_id, off)
        got.append((j, kind, int(d["num_tiles"]), int(d["num_assigned"]), int(d["trim_start"]) if kind == 4 else 0, int(d["trim_end"]) if kind == 4 else 0, first_id, 1))
    t0 = time.time()
    while not eng.stream_poll(0):
        assert time.time() - t0 < 60
    eng.stream_end(0)
    return got


def test_long_span_window_applies_inserts_itself(oracle, native):
    """The head of a path at spans 124 - 128 (h = 5): most reads insert, in the launch; records and the final ID / count
    arrays equal the serial loop's."""
    from oracle_engine import serial_reference

    k, h, tile, block = 124, 5, 500, 4
    seeds = _long_seeds(k, h, 41)
    _, reads = _reads(150_000, 90, 31)
    reads.insert(7, reads[3][: tile - 1])  # a read without a single tile
    m = oracle.load().orc_calc_optimal_size(2_000_000, 1, 0.1)
    exp, mf_ref = serial_reference(oracle, m, seeds, tile, k, reads, block=block)
    eng = native.Engine(k, h, tile, m, seeds)
    b = eng.upload(reads)
    eng.bv_insert(b)
    assert eng.finalize() == mf_ref.pop
    got = _stream_resumable(eng, b, reads, tile, block)
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
    reads = _keep_stream()
    m = oracle.load().orc_calc_optimal_size(2_500_000, 1, 0.1)
    exp, mf_ref = serial_reference(oracle, m, seeds, tile, K_LONG, reads, block=block)
    eng = native.Engine(K_LONG, H_LONG, tile, m, seeds)
    b = eng.upload(reads)
    eng.bv_insert(b)
    assert eng.finalize() == mf_ref.pop
    got = _stream_resumable(eng, b, reads, tile, block)
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
    _, reads = _reads(150_000, 140, 21)
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
        native.Engine(257, 1, 1000, 1 << 20, [_symmetric_seed(257, 30, 1)])
    with pytest.raises(native.GrpError, match="256"):
        native.Engine(254, 4, 1000, 1 << 20, default_seeds(4, _symmetric_seed(254, 30, 2)))  # longest seed 257
    eng = native.Engine(253, 4, 1000, 1 << 20, default_seeds(4, _symmetric_seed(253, 30, 3)))  # longest seed 256: accepted
    eng.close()
