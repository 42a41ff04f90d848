"""GPU: 9 to 16 spaced seeds per frame (the many-seed kernel form, grp_kernels.inc frame_seeds) against the CPU oracle,
bit for bit: tile hashes, fill, inserts, queries and the classification window; ntCard tables; the order-exact forms (a
resumable streaming window that applies inserts itself, keeping tiles and keeping nothing; batches) against the oracle's
serial loop (process_read, goldrush_path.cpp:892-1094); 17 seeds refused."""
import numpy as np
import pytest

from helpers import SEED22, compare_queries, default_seeds, keep_stream, low_error_reads, palindromic_preset, random_reads, stream_resumable

pytestmark = pytest.mark.gpu


def _seeds(k, h, seed=1):
    preset = SEED22 if k == 22 else palindromic_preset(k, min(30, k - 2 if k % 2 == 0 else k - 1), seed + k)
    seeds = default_seeds(h, preset)
    assert [len(s) for s in seeds] == [k + i for i in range(h)]
    return seeds


# (22, 9): spans 22 - 30; (22, 11): 22 - 32, the 32-base boundary inside the family; (24, 10): 24 - 33; (49, 16): 49 - 64;
# (50, 16): 50 - 65, the 64-base boundary; (200, 16): the long-span form; (22, 16): the default preset at 16 seeds
@pytest.mark.parametrize("k,h,tile", [(22, 9, 500), (22, 11, 300), (24, 10, 400), (22, 12, 1000), (49, 16, 500), (50, 16, 400), (200, 16, 600), (22, 16, 1000)])
def test_many_seeds_match_oracle(oracle, native, k, h, tile):
    """Reads shorter than the longest span, exactly that long, a tile + span - 2 long, and reads whose last tile is
    clipped; the fill of half of the reads only, so that the other half's frames find some of their h bits set and
    some not."""
    from goldrush_amd import host

    seeds = _seeds(k, h)
    span = k + h - 1
    m = oracle.load().orc_calc_optimal_size(150_000, 1, 0.1)
    eng = native.Engine(k, h, tile, m, seeds)
    oseeds = oracle.Seeds(seeds)
    omf = oracle.MiBF(m, oseeds, tile, k)
    reads = random_reads(6, 2 * tile + span, 5 * tile + 70, seed=151 + k + h)
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
    fill = [0, 2, 4, 5, 6, 8, 10, 11, 12]
    b_fill = eng.upload([reads[i] for i in fill])
    eng.bv_insert(b_fill)
    for i in fill:
        if len(reads[i]) >= span:  # the fill skips reads shorter than the longest seed (process_read: "too short")
            omf.bv_insert_read(reads[i])
    assert eng.finalize() == omf.finalize()
    assert np.array_equal(eng.export_bits(), omf.bits())
    for ri in (0, 2, 5, 6):
        nt = len(reads[ri]) // tile
        eng.insert_tiles(b, ri, 0, nt, ri + 1)
        omf.insert_read_tiles(reads[ri], 0, nt, ri + 1)
    ids, counts = eng.export_ids()
    assert np.array_equal(ids, omf.ids()) and np.array_equal(counts, omf.counts())
    assert counts.any()
    _, hits, misses = compare_queries(eng, omf, b, reads)
    assert hits > 0 and misses > 0
    # whole reads in ID blocks of 2 tiles (k_insert_collect + k_insert_apply) on top of the tile inserts above
    for ri in (4, 8):
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


@pytest.mark.parametrize("h,tile,n_ids", [(16, 1000, 3), (16, 1000, 1 << 30), (12, 2000, 1 << 30), (16, 1500, 1 << 30)])
def test_many_seeds_ids_per_frame(oracle, native, h, tile, n_ids):
    """IDs imported straight into the filter.  n_ids = 3: a frame's 16 probes return the same few IDs over and over —
    the frame counts each of them once, across both seed groups of the many-seed form.  n_ids = 2^30: (almost) every
    probe another ID, tile x h distinct IDs: at (16, 1000) the worst-case table fits the LDS and is what the first
    launch takes; at (12, 2000) and (16, 1500) it does not, the first launch's table cannot hold the tiles' IDs, and
    they are flagged and redone with the worst-case table in global memory (k_query's GT form)."""
    k = 22
    seeds = _seeds(k, h)
    m = oracle.load().orc_calc_optimal_size(400_000, 1, 0.1)
    eng = native.Engine(k, h, tile, m, seeds)
    oseeds = oracle.Seeds(seeds)
    omf = oracle.MiBF(m, oseeds, tile, k)
    reads = random_reads(4, 2 * tile + 40, 4 * tile + 300, seed=43 + h)
    b = eng.upload(reads)
    eng.bv_insert(b)
    for s in reads:
        omf.bv_insert_read(s)
    pop = eng.finalize()
    assert pop == omf.finalize()
    rng = np.random.default_rng(8 + h)
    ids = rng.integers(1, n_ids + 1, size=pop, dtype=np.uint32)
    if n_ids == 3:
        ids[rng.random(pop) < 0.05] |= np.uint32(0x80000000)  # a few saturated ones: the bit is stripped before counting
    eng.import_ids(0, ids=ids, counts=np.zeros(pop, dtype=np.uint32))
    omf.ids()[:] = ids
    compare_queries(eng, omf, b, reads)
    dec = eng.classify_reads(b)
    assert all(int(d["num_tiles"]) == len(r) // tile for d, r in zip(dec, reads))
    assert (eng.verify_stats()["window_flagged"] > 0) == (n_ids > 3 and tile >= 1500)
    eng.close()


@pytest.mark.parametrize("h", [9, 16])
def test_many_seeds_ntcard_tables_match_oracle(oracle, native, h):
    """grp_ntcard_* against the oracle: zero buckets of every sample table for plain reads, reads shorter than the longest
    span (the iterator rule), ACGT runs with explicit stale repeats; then the deferred filter size and the fill."""
    from goldrush_amd import host

    k = 22
    seeds = _seeds(k, h)
    span = k + h - 1
    osd = oracle.Seeds(seeds)
    rng = np.random.default_rng(92 + h)
    reads = random_reads(30, 1500, 9000, seed=91 + h)
    reads += [reads[0][:k], reads[1][: k + 1], reads[2][: span - 1], reads[3][:span], reads[4][: span + 1], reads[5][: k - 1]]
    dirty = []
    for i, r in enumerate(random_reads(6, 800, 5000, seed=93 + h)):
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


# ---- the order-exact forms ---------------------------------------------------------------------------------------------
# Reads with few errors: a frame of 16 seeds is lost to an error in any of its spans.


@pytest.mark.parametrize("h,tile,keeps", [(16, 250, True), (12, 250, True), (16, 1000, False)])
def test_many_seeds_window_applies_inserts_itself(oracle, native, h, tile, keeps):
    """tests/stream_keep_scenario.py's stream at h seeds: the in-launch inserts keep the tiles they can where the LDS has
    room for the probes' fingerprints (short tiles), and keep nothing at 1000-base tiles (16 000 probes per tile); either
    way the serial loop's records and the final ID / count arrays.  (The filter grows with h, as -o / -H would make it; at
    1000-base tiles a read inserts with 2 unassigned tiles, so that the stream of 3.5 - 9 kb reads has inserts.)"""
    from oracle_engine import serial_reference

    k, block = 22, 4
    u = 5 if tile < 1000 else 2
    seeds = _seeds(k, h)
    reads = keep_stream()
    m = oracle.load().orc_calc_optimal_size(2_500_000 * h // 3, 1, 0.1)
    exp, mf_ref = serial_reference(oracle, m, seeds, tile, k, reads, block=block, u=u)
    eng = native.Engine(k, h, tile, m, seeds)
    b = eng.upload(reads)
    eng.bv_insert(b)
    assert eng.finalize() == mf_ref.pop
    got = stream_resumable(eng, b, reads, tile, block, u=u)
    assert got == exp
    ids, counts = eng.export_ids()
    assert np.array_equal(ids, mf_ref.ids()) and np.array_equal(counts, mf_ref.counts())
    st = eng.stream_stats()
    n_ins = sum(1 for g in got if g[1] in (2, 4))
    assert n_ins >= (10 if keeps else 4) and sum(1 for g in got[70:] if g[1] not in (2, 4)) >= 150, "the stream is not what the test means"
    assert st["inserts_kept"] + st["inserts_kept_nothing"] == n_ins
    if keeps:
        assert st["inserts_kept"] > 0 and st["tiles_kept"] > 0, st
    else:
        assert st["inserts_kept"] == 0 and st["inserts_kept_nothing"] == n_ins, st
    assert st["coop_refused"] == 0
    mf_ref.close()
    eng.close()


@pytest.mark.parametrize("h,window,verify", [(16, 7, None), (16, 32, "check"), (9, 32, "chain"), (13, 12, None)])
def test_many_seeds_batches_equal_the_serial_loop(oracle, native, h, window, verify):
    """Windows committed as batches (grp_batch_insert_reads / _classify / _verify / _undo; k_batch_collect, k_batch_delta,
    the batch-view queries) by tests/test_gpu_batch.py's driver."""
    from oracle_engine import serial_reference
    from test_gpu_batch import batch_commit

    k, tile, block = 22, 500, 4
    seeds = _seeds(k, h)
    _, reads = low_error_reads(150_000, 140, 21)
    m = oracle.load().orc_calc_optimal_size(2_000_000, 1, 0.1)
    exp, mf_ref = serial_reference(oracle, m, seeds, tile, k, reads, block=block)
    eng = native.Engine(k, h, tile, m, seeds)
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


@pytest.mark.parametrize("mode", ["auto", "batch", "stream"])
def test_many_seeds_classifier(oracle, native, mode, monkeypatch):
    """The product's classifier at 16 seeds (its own choice of windows and batches, batches forced, streaming windows
    forced) on a genome a third of which is repeat copies: the commits, IDs and counts of the oracle's serial loop."""
    from goldrush_amd import host, synth
    from oracle_engine import cached_serial_reference

    for key, val in {"auto": {}, "batch": {"GRP_BATCH": "force"}, "stream": {"GRP_BATCH": "off", "GRP_STREAM": "force"}}[mode].items():
        monkeypatch.setenv(key, val)
    tile, k, h, block = 500, 22, 16, 4
    seeds = _seeds(k, h)
    g = synth.repeat_genome(150_000, 31)
    reads = [r[1] for r in synth.make_reads(g, 160, mean_len=5000, min_len=3500, seed=33, max_len=9000, sub=0.004, ins=0.0005, dele=0.0005)]
    m = oracle.load().orc_calc_optimal_size(4_000_000, 1, 0.1)
    exp, ref_ids, ref_counts, ref_pop = cached_serial_reference("many_seeds_classifier", oracle, m, seeds, tile, k, reads, block=block, silver=True, target_bases=120_000, max_paths=3)
    eng = native.Engine(k, h, tile, m, seeds)
    b = eng.upload(reads)
    eng.bv_insert(b)
    assert eng.finalize() == ref_pop
    cls = host.Classifier(eng._h, host.hip_engine_vt(), tile=tile, block=block, k=k, h=h, target_bases=120_000, max_paths=3, silver_path=True, max_window=4096)
    cls.run(b._h, b.lens)
    eng.sync()
    assert [c[:8] for c in cls.commits] == exp
    assert sum(1 for e in exp if e[1] in (2, 4)) >= 3
    ids, counts = eng.export_ids()
    assert np.array_equal(ids, ref_ids) and np.array_equal(counts, ref_counts)
    eng.close()


def test_seventeen_seeds_are_refused(native):
    with pytest.raises(native.GrpError, match="16"):
        native.Engine(22, 17, 1000, 1 << 20, default_seeds(17))
    eng = native.Engine(22, 16, 1000, 1 << 20, default_seeds(16))  # 16: accepted
    eng.close()
