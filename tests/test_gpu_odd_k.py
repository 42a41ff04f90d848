"""GPU: odd -k.  make_seed_pattern's seeds are then one base shorter than k (left and right halves of k/2 positions,
spaced_seeds.cpp:27-66): seed i spans k - 1 + i, while the tile string stays tile + k - 1 bases (read_hashing.cpp:44-45),
so a full tile has tile + 1 frames (multiLensfrHashIterator.hpp:29-68).  Everything against the CPU oracle, bit for bit:
tile hashes, fill, inserts, queries; the order-exact forms (a resumable streaming window that keeps tiles, batches, the
global-table redo, the classifier) against the oracle's serial loop; ntCard tables; the frames-per-tile limit."""
import numpy as np
import pytest

from helpers import compare_queries, palindromic_preset, random_reads, stream_resumable

pytestmark = pytest.mark.gpu


def _seeds(oracle, k, h):
    """designed seeds (-w 16) where glibc's rand() finds a half of 8 care positions quickly; an odd preset beyond"""
    from goldrush_amd import host

    preset = "" if k <= 65 else palindromic_preset(k, 30, k)
    seeds = host.make_seed_pattern(preset, k, 16, h)
    assert seeds == oracle.make_seed_pattern(preset, k, 16, h)
    assert [len(s) for s in seeds] == [k - 1 + i for i in range(h)]
    return seeds


def _frames(length, tile, k, span0):
    """frames per tile of a read: tile + k - span0 for full tiles, the last one possibly clipped"""
    nt = length // tile
    out = []
    for t in range(nt):
        lp = min(tile + k - 1, length - t * tile)
        out.append(lp - span0 + 1)
    return out


@pytest.mark.parametrize("k,h,tile", [(23, 3, 1000), (21, 1, 300), (33, 3, 500), (33, 1, 400), (65, 1, 300), (65, 3, 400), (129, 2, 500),
                                      (255, 2, 600), (23, 9, 700), (23, 16, 1000), (23, 3, 768)])
def test_odd_k_matches_oracle(oracle, native, k, h, tile):
    """(33, 1): one seed of 32 bases, the 32-base window; (65, 1): one seed of 64, the 64-base window; (65, 3): spans 64 - 66,
    the long form; (255, 2): spans 254 - 255 (k + h - 1 = 256); (23, 3, 768): tile + 1 frames cross a 256-frame unit.
    Reads whose last tile is clipped, and reads exactly span0 + h - 1 long (shorter than k + h - 1: they count in the fill)."""
    seeds = _seeds(oracle, k, h)
    span0, longest = k - 1, k + h - 2
    m = oracle.load().orc_calc_optimal_size(300_000, 1, 0.1)
    eng = native.Engine(k, h, tile, m, seeds)
    oseeds = oracle.Seeds(seeds)
    omf = oracle.MiBF(m, oseeds, tile, k)
    reads = random_reads(5, 2 * tile + longest, 5 * tile + 70, seed=311 + k)
    reads += [reads[0][: 3 * tile // 2 + k - 2], reads[1][: 2 * tile + longest - 2], reads[2][: tile + 3], reads[3][:longest], reads[4][: longest - 1],
              reads[0][: tile + k - 1], reads[1][: tile + k - 2], reads[2][: 3 * tile + 1]]
    b = eng.upload(reads)
    n_full = 0
    for ri, seq in enumerate(reads):
        fr = _frames(len(seq), tile, k, span0)
        for t in range(len(seq) // tile):
            got, exp = eng.tile_hashes(b, ri, t), oseeds.tile_hashes(seq, tile, k, t)
            assert got.shape == exp.shape and np.array_equal(got, exp), (ri, t)
            assert got.size == fr[t] * h, (ri, t)
            if fr[t] == tile + 1:
                n_full += 1
    assert n_full >= 10  # a full tile has tile + 1 frames
    eng.bv_insert(b)
    for sq in reads:
        if len(sq) >= longest:  # reads of span0 + h - 1 bases count, shorter ones do not
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
    compare_queries(eng, omf, b, reads)
    for ri in (1, 3):  # whole reads in ID blocks of 2 tiles (k_insert_collect + k_insert_apply)
        nt = len(reads[ri]) // tile
        eng.insert_read(b, ri, 0, nt, 2, 40 + ri, 0)
        for bs in range(0, nt, 2):
            omf.insert_read_tiles(reads[ri], bs, min(bs + 2, nt), 40 + ri + bs // 2)
    ids, counts = eng.export_ids()
    assert np.array_equal(ids, omf.ids()) and np.array_equal(counts, omf.counts())
    q, hits, _ = compare_queries(eng, omf, b, reads)
    assert hits > 0 and q == sum(sum(_frames(len(s), tile, k, span0)) for s in reads)
    eng.close()


def test_odd_preset_of_23_characters(oracle, native):
    """a 23-character -s preset: its last character is dropped, seeds of 22 - 24 bases at k = 23 (the shared halves cut at 11)"""
    from goldrush_amd import host

    preset = "10110111101101111011011"
    seeds = host.make_seed_pattern(preset, 23, 16, 3)
    assert seeds == oracle.make_seed_pattern(preset, 23, 16, 3) and seeds[0] == preset[:22]
    tile = 500
    m = oracle.load().orc_calc_optimal_size(300_000, 1, 0.1)
    eng = native.Engine(23, 3, tile, m, seeds)
    omf = oracle.MiBF(m, oracle.Seeds(seeds), tile, 23)
    reads = random_reads(8, 1200, 4000, seed=5)
    b = eng.upload(reads)
    eng.bv_insert(b)
    for sq in reads:
        omf.bv_insert_read(sq)
    assert eng.finalize() == omf.finalize()
    for ri in (0, 3):
        nt = len(reads[ri]) // tile
        eng.insert_tiles(b, ri, 0, nt, ri + 1)
        omf.insert_read_tiles(reads[ri], 0, nt, ri + 1)
    compare_queries(eng, omf, b, reads)
    eng.close()


def test_odd_k_global_table_redo(oracle, native):
    """-t 12001 at k = 23: the worst-case table (12 002 frames x 3 seeds) does not fit the LDS and lives in global memory.
    Every probe another ID: the first step's LDS table flags the tiles and the GT launches redo them, in grp_query_tiles
    and in grp_classify_reads; a handful of IDs: the first step alone"""
    k, h, tile = 23, 3, 12001
    seeds = _seeds(oracle, k, h)
    m = oracle.load().orc_calc_optimal_size(600_000, 1, 0.1)
    eng = native.Engine(k, h, tile, m, seeds)
    omf = oracle.MiBF(m, oracle.Seeds(seeds), tile, k)
    reads = random_reads(3, 2 * tile + 300, 3 * tile + 900, seed=73)
    b = eng.upload(reads)
    eng.bv_insert(b)
    for sq in reads:
        omf.bv_insert_read(sq)
    pop = eng.finalize()
    assert pop == omf.finalize()
    rng = np.random.default_rng(9)
    for n_ids, flagged in ((1 << 30, True), (25, False)):
        ids = rng.integers(1, n_ids, size=pop, dtype=np.uint32)
        eng.import_ids(0, ids=ids, counts=np.zeros(pop, dtype=np.uint32))
        omf.ids()[:] = ids
        before = eng.verify_stats()["window_flagged"]
        compare_queries(eng, omf, b, reads)
        dec = eng.classify_reads(b)
        assert all(int(d["num_tiles"]) == len(r) // tile for d, r in zip(dec, reads))
        assert (eng.verify_stats()["window_flagged"] > before) == flagged
    eng.close()


# ---- the order-exact forms at k = 23 -------------------------------------------------------------------------------------

K, H, TILE, BLOCK = 23, 3, 500, 4


def test_odd_k_window_keeps_tiles(oracle, native):
    """ONE resumable streaming window applying its inserts itself and keeping the tiles they leave untouched: the serial
    loop's records and arrays"""
    from oracle_engine import serial_reference
    from stream_keep_scenario import make_stream

    seeds = _seeds(oracle, K, H)
    reads = make_stream()  # (that module fixes K = 22; the stream serves any k)
    m = oracle.load().orc_calc_optimal_size(2_500_000, 1, 0.1)
    exp, mf_ref = serial_reference(oracle, m, seeds, TILE, K, reads, block=BLOCK)
    eng = native.Engine(K, H, TILE, m, seeds)
    b = eng.upload(reads)
    eng.bv_insert(b)
    assert eng.finalize() == mf_ref.pop
    got = stream_resumable(eng, b, reads, TILE, BLOCK)
    assert got == exp
    ids, counts = eng.export_ids()
    assert np.array_equal(ids, mf_ref.ids()) and np.array_equal(counts, mf_ref.counts())
    st = eng.stream_stats()
    n_ins = sum(1 for g in got if g[1] in (2, 4))
    assert n_ins >= 10 and st["inserts_kept"] + st["inserts_kept_nothing"] == n_ins
    assert st["inserts_kept"] > 0 and st["tiles_kept"] > 0, st
    mf_ref.close()
    eng.close()


@pytest.mark.parametrize("window,verify", [(7, None), (32, "check")])
def test_odd_k_batches_equal_the_serial_loop(oracle, native, window, verify):
    from goldrush_amd import synth
    from oracle_engine import serial_reference
    from test_gpu_batch import batch_commit

    seeds = _seeds(oracle, K, H)
    g = synth.random_genome(150_000, 21)
    reads = [r[1] for r in synth.make_reads(g, 140, mean_len=5000, min_len=3500, seed=22, max_len=9000)]
    m = oracle.load().orc_calc_optimal_size(2_000_000, 1, 0.1)
    exp, mf_ref = serial_reference(oracle, m, seeds, TILE, K, reads, block=BLOCK)
    eng = native.Engine(K, H, TILE, m, seeds)
    b = eng.upload(reads)
    eng.bv_insert(b)
    assert eng.finalize() == mf_ref.pop
    stats = {"batches": 0, "undone": 0}
    got = batch_commit(eng, b, reads, TILE, BLOCK, window, stats, verify)
    assert got == [e[:7] for e in exp]
    ids, counts = eng.export_ids()
    assert np.array_equal(ids, mf_ref.ids()) and np.array_equal(counts, mf_ref.counts())
    assert stats["batches"] > 0 and {e[1] for e in exp} >= {2, 3}
    mf_ref.close()
    eng.close()


@pytest.mark.parametrize("mode", ["auto", "stream"])
def test_odd_k_classifier_matches_serial_loop(oracle, native, mode, monkeypatch):
    """the product's classifier at k = 23: records, arrays, and the "Total queries" counter (tile + 1 frames per tile)"""
    from goldrush_amd import host, synth
    from oracle_engine import serial_reference

    if mode == "stream":
        monkeypatch.setenv("GRP_BATCH", "off")
        monkeypatch.setenv("GRP_STREAM", "force")
    seeds = _seeds(oracle, K, H)
    g = synth.random_genome(150_000, 21)
    reads = [r[1] for r in synth.make_reads(g, 120, mean_len=5000, min_len=3500, seed=22, max_len=9000)]
    m = oracle.load().orc_calc_optimal_size(2_000_000, 1, 0.1)
    exp, mf_ref = serial_reference(oracle, m, seeds, TILE, K, reads, block=BLOCK, silver=True, target_bases=120_000, max_paths=3)
    eng = native.Engine(K, H, TILE, m, seeds)
    b = eng.upload(reads)
    eng.bv_insert(b)
    assert eng.finalize() == mf_ref.pop
    cls = host.Classifier(eng._h, host.hip_engine_vt(), tile=TILE, block=BLOCK, k=K, h=H, target_bases=120_000, max_paths=3, silver_path=True, max_window=4096, span0=K - 1)
    cls.run(b._h, b.lens)
    eng.sync()
    assert [c[:8] for c in cls.commits] == exp
    ids, counts = eng.export_ids()
    assert np.array_equal(ids, mf_ref.ids()) and np.array_equal(counts, mf_ref.counts())
    st = cls.state()
    assert st["queries"] == sum(sum(_frames(len(reads[c[0]]), TILE, K, K - 1)) for c in cls.commits)
    mf_ref.close()
    eng.close()


@pytest.mark.parametrize("k,h", [(23, 3), (129, 2)])
def test_odd_k_ntcard_tables_match_oracle(oracle, native, k, h):
    """grp_ntcard_* at odd k: windows of the seeds' own spans, the stale repeats span_s - span_0; plain reads (some shorter
    than k), ACGT runs with explicit repeats; then the deferred filter size and the fill"""
    from goldrush_amd import host

    seeds = _seeds(oracle, k, h)
    span0, longest = k - 1, k + h - 2
    osd = oracle.Seeds(seeds)
    rng = np.random.default_rng(92 + k)
    reads = random_reads(30, 1500, 9000, seed=91 + k)
    reads += [reads[0][:span0], reads[1][:k], reads[2][: longest - 1], reads[3][:longest], reads[4][: span0 - 1]]
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
    eng.ntcard_add(b)
    runs_all, extra_all = [], []
    for seq in dirty:
        runs, extra = host.ntcard_split(seq, span0, h)
        runs_all += [seq[o:o + n] for o, n in runs]
        extra_all.append(extra)
    b2 = eng.upload(runs_all)
    eng.ntcard_add(b2, stale_extra=np.concatenate(extra_all).ravel())
    z = eng.ntcard_finish()
    nc = oracle.NtCard(osd, 1000)
    for seq in reads + dirty:
        nc.add_read(seq)
    assert np.array_equal(z, nc.zero_buckets())
    m = oracle.load().orc_calc_optimal_size(sum(nc.f0(s) for s in range(h)), 1, 0.1)
    nc.close()
    eng.set_filter_size(m)
    eng.bv_insert(b)
    omf = oracle.MiBF(m, osd, tile, k)
    for seq in reads:
        if len(seq) >= longest:
            omf.bv_insert_read(seq)
    assert eng.finalize() == omf.finalize()
    assert np.array_equal(eng.export_bits(), omf.bits())
    eng.close()


def test_frames_per_tile_limit_at_odd_k(oracle, native):
    """a tile holds at most 65 535 frames: -t 65534 at odd k (65 535 frames) is accepted, -t 65535 (65 536) refused; even
    k keeps -t 65535"""
    from helpers import default_seeds

    seeds = _seeds(oracle, 23, 3)
    native.Engine(23, 3, 65534, 1 << 20, seeds).close()
    with pytest.raises(native.GrpError, match="65 535"):
        native.Engine(23, 3, 65535, 1 << 20, seeds)
    native.Engine(22, 3, 65535, 1 << 20, default_seeds(3)).close()


def test_seed_spans_other_than_k_or_k_minus_1_are_refused(native):
    from helpers import default_seeds

    seeds = default_seeds(3)  # spans 22 - 24
    for k in (21, 24, 25):
        with pytest.raises(native.GrpError, match="k-1"):
            native.Engine(k, 3, 1000, 1 << 20, seeds)
    with pytest.raises(native.GrpError, match="k-1"):
        native.Engine(23, 3, 1000, 1 << 20, [seeds[0], seeds[1], seeds[1]])
