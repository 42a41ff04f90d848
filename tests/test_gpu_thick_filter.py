"""GPU: the engine's protocols on a THICKENED filter (tests/thick_scenario.py): between the fill and grp_finalize every
64-bit word that holds a bit becomes all ones, on the device (helpers.thicken_engine) and in the oracle
(serial_reference's plant=).  Most of the reads' own probes then read and write the side tables — the overflow table's IDs
(grp_ovf_get / grp_ovf_put), the far table's count words (grp_far_ptr) — where the hash fill sends under 1 % and about 5 %
of them, too few for a vote over hundreds of frames to notice a wrong one.

Every test first asserts its CONDITION on what the engine built: the geometry grp_debug_filter_geometry reports is the
model's, and of the ranks the reads' own probes (grp_debug_tile_hashes mod m) land on, the shares at in-bucket index >= 13
and >= 8 are at least the scenario's.  A test that cannot meet it fails.  Then the existing drivers run against the oracle
with the same planted filter: queries and inserts (helpers.compare_queries), batches (test_gpu_batch.batch_commit), the
classifier, the streaming window with in-launch inserts (helpers.stream_resumable).  Integers throughout: no tolerance."""
import numpy as np
import pytest

import filter_model as fm
import thick_scenario as ts
from helpers import compare_queries, default_seeds, stream_resumable, thicken_engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def reads():
    return ts.make_reads()


def thick_engine(native, reads, seeds, m, k, least13, least8, W, label):
    """fill, thicken, finalize; the condition, asserted on the engine's own geometry and hashes -> (engine, batch, words)"""
    h = len(seeds)
    eng = native.Engine(k, h, ts.TILE, m, seeds)
    b = eng.upload(reads)
    eng.bv_insert(b)
    words = thicken_engine(eng)
    pop = eng.finalize()
    mod = fm.FilterModel(words, m, keep_bits=False)
    assert pop == mod.pop and eng.filter_geometry() == mod.geometry() and mod.W == W, (label, eng.filter_geometry(), mod.geometry())
    hashes = np.concatenate([eng.tile_hashes(b, ri, t) for ri, s in enumerate(reads) for t in range(len(s) // ts.TILE)])
    s13, s8, n = ts.side_table_shares(mod, hashes)
    pos = np.unique(hashes % np.uint64(m))
    bit, rank = eng.rank(pos)
    assert np.array_equal(bit, mod.bit(pos)) and np.array_equal(rank, mod.rank(pos)), label
    print("%s: W %d, overflow IDs %d, far count words %d of pop %d; %d probed ranks: %.3f at index >= 13, %.3f at index >= 8"
          % (label, mod.W, mod.n_ovf, mod.n_far, pop, n, s13, s8))
    assert s13 >= least13 and s8 >= least8, (label, s13, s8)
    return eng, b, words


def _oracle_filter(oracle, reads, seeds, m, k):
    oseeds = oracle.Seeds(seeds)
    omf = oracle.MiBF(m, oseeds, ts.TILE, k)
    for s in reads:
        omf.bv_insert_read(s)
    ts.plant_thickened(omf)
    return omf


def _query_and_insert(eng, omf, b, reads, block, whole=(0, 3, 5, 1, 7), exports=True):
    """tests/test_gpu_parity.py's test_insert_and_query_match_oracle on the planted filter"""
    compare_queries(eng, omf, b, reads)  # empty ID array: all misses
    next_id = 0
    for ri in whole:
        seq = reads[ri]
        nt = len(seq) // ts.TILE
        next_id += 1
        for bs in range(0, nt, block):
            be = min(bs + block, nt)
            eng.insert_tiles(b, ri, bs, be, next_id + bs // block)
            omf.insert_read_tiles(seq, bs, be, next_id + bs // block)
        next_id += len(seq) // (ts.TILE * block)
        if exports:
            ids, counts = eng.export_ids()
            assert np.array_equal(ids, omf.ids()) and np.array_equal(counts, omf.counts()), ri
    ids, counts = eng.export_ids()
    assert np.array_equal(ids, omf.ids()) and np.array_equal(counts, omf.counts())
    assert counts.max() > 1  # overlapping reads: the reservoir rule ran on shared ranks
    compare_queries(eng, omf, b, reads)
    eng.insert_tiles(b, 6, 1, 3, 77)  # a trimmed insert whose dedup scope does not start at tile 0
    omf.insert_read_tiles(reads[6], 1, 3, 77)
    ids, counts = eng.export_ids()
    assert np.array_equal(ids, omf.ids()) and np.array_equal(counts, omf.counts())
    compare_queries(eng, omf, b, reads)
    eng.reset_ids()
    omf.reset_ids()
    ids, counts = eng.export_ids()
    assert not ids.any() and not counts.any()
    compare_queries(eng, omf, b, reads)


@pytest.mark.parametrize("geometry", list(ts.GEOMETRIES))
def test_thick_insert_and_query_match_oracle(oracle, native, reads, geometry):
    m, W, least13, least8 = ts.GEOMETRIES[geometry]
    seeds = default_seeds(ts.H)
    eng, b, words = thick_engine(native, reads, seeds, m, ts.K, least13, least8, W, geometry)
    try:
        omf = _oracle_filter(oracle, reads, seeds, m, ts.K)
        assert omf.finalize() == eng.pop and np.array_equal(omf.bits(), words)
        _query_and_insert(eng, omf, b, reads, ts.BLOCK)
        omf.close()
    finally:
        eng.close()


@pytest.mark.parametrize("form", list(ts.FORMS))
def test_thick_other_query_forms(oracle, native, reads, form):
    """the many-seed form (h = 16) and the long-span form (k = 128): query and insert only"""
    f = ts.FORMS[form]
    seeds = ts.form_seeds(form)
    sub = reads[: f["n_reads"]]
    eng, b, words = thick_engine(native, sub, seeds, f["m"], f["k"], f["least13"], f["least8"], f["W"], form)
    try:
        omf = _oracle_filter(oracle, sub, seeds, f["m"], f["k"])
        assert omf.finalize() == eng.pop and np.array_equal(omf.bits(), words)
        _query_and_insert(eng, omf, b, sub, ts.BLOCK, exports=False)
        omf.close()
    finally:
        eng.close()


@pytest.mark.parametrize("geometry", list(ts.GEOMETRIES))
@pytest.mark.parametrize("window,verify", [(7, None), (32, "check"), (32, "chain")])
def test_thick_batches_equal_the_serial_loop(oracle, native, reads, geometry, window, verify):
    """revert, undo and the verify delta on overflow ranks: records, final IDs and counts of the serial loop"""
    from oracle_engine import cached_serial_reference
    from test_gpu_batch import batch_commit

    m, W, least13, least8 = ts.GEOMETRIES[geometry]
    seeds = default_seeds(ts.H)
    exp, ref_ids, ref_counts, ref_pop = cached_serial_reference(("thick", geometry), oracle, m, seeds, ts.TILE, ts.K, reads, block=ts.BLOCK, plant=ts.plant_thickened)
    assert {2, 3, 4} <= {e[1] for e in exp}
    eng, b, _ = thick_engine(native, reads, seeds, m, ts.K, least13, least8, W, geometry)
    try:
        assert eng.pop == ref_pop
        stats = {"batches": 0, "undone": 0}
        got = batch_commit(eng, b, reads, ts.TILE, ts.BLOCK, window, stats, verify)
        assert got == [e[:7] for e in exp]
        ids, counts = eng.export_ids()
        assert np.array_equal(counts, ref_counts) and np.array_equal(ids, ref_ids)
        vs = eng.verify_stats()
        print(geometry, window, verify, stats, vs)
        assert vs["impossible_deltas"] == 0 and vs["far_count_words"] == eng.filter_geometry()[3]
        assert stats["batches"] > 0 and stats["undone"] + stats.get("carried", 0) > 0  # revert / undo ran on these ranks
        if verify is not None:
            assert vs["fallbacks"] == 0 and vs["patched"] > 0, vs
    finally:
        eng.close()


@pytest.mark.parametrize("geometry", list(ts.GEOMETRIES))
@pytest.mark.parametrize("mode", ["auto", "batch", "stream"])
def test_thick_classifier_matches_serial_loop(oracle, native, reads, geometry, mode, monkeypatch):
    """the product's classifier, silver with two rollovers: grp_reset_ids mid-run on a thickened filter"""
    from goldrush_amd import host
    from oracle_engine import cached_serial_reference

    for key, val in {"auto": {}, "batch": {"GRP_BATCH": "force"}, "stream": {"GRP_BATCH": "off", "GRP_STREAM": "force"}}[mode].items():
        monkeypatch.setenv(key, val)
    m, W, least13, least8 = ts.GEOMETRIES[geometry]
    seeds = default_seeds(ts.H)
    exp, ref_ids, ref_counts, ref_pop = cached_serial_reference(("thick_silver", geometry), oracle, m, seeds, ts.TILE, ts.K, reads, block=ts.BLOCK, plant=ts.plant_thickened, **ts.SILVER)
    assert {e[7] for e in exp} == {1, 2, 3}
    eng, b, _ = thick_engine(native, reads, seeds, m, ts.K, least13, least8, W, geometry)
    try:
        assert eng.pop == ref_pop
        cls = host.Classifier(eng._h, host.hip_engine_vt(), tile=ts.TILE, block=ts.BLOCK, k=ts.K, h=ts.H, target_bases=ts.SILVER["target_bases"], max_paths=ts.SILVER["max_paths"], silver_path=True, max_window=4096)
        cls.run(b._h, b.lens)
        eng.sync()
        assert [c[:8] for c in cls.commits] == exp
        ids, counts = eng.export_ids()
        assert np.array_equal(ids, ref_ids) and np.array_equal(counts, ref_counts)
        st = cls.state()
        assert st["reads_committed"] == len(exp) and st["inserts"] == sum(1 for e in exp if e[1] in (2, 4))
        if mode == "batch":
            assert st["batches"] >= 1
    finally:
        eng.close()


@pytest.mark.parametrize("geometry,keep", [("w64", None), ("w64", "0"), ("w33", None), ("w33", "0")])
def test_thick_stream_window_applies_inserts_itself(oracle, native, reads, geometry, keep, monkeypatch):
    """ONE resumable streaming window over the reads, every insert applied in the launch (helpers.stream_resumable), with
    GRP_STREAM_KEEP at its default and at 0: the oracle's serial loop either way.  With keeping on, tiles are both kept
    and queried again behind the inserts — the fingerprints of the kept tiles were taken over overflow slots.
    (tests/stream_keep_scenario.py's own stream is 350 reads: thickened, it fills a filter of 10^8 bits to W = 13, where
    no bucket overflows.  These 24 overlapping reads are queried ahead of the first insert in one go, and the reads behind an
    inserting read partly overlap it and partly do not: both counters move.)"""
    from oracle_engine import cached_serial_reference

    if keep is not None:
        monkeypatch.setenv("GRP_STREAM_KEEP", keep)  # (read when the context is created)
    m, W, least13, least8 = ts.GEOMETRIES[geometry]
    seeds = default_seeds(ts.H)
    exp, ref_ids, ref_counts, ref_pop = cached_serial_reference(("thick", geometry), oracle, m, seeds, ts.TILE, ts.K, reads, block=ts.BLOCK, plant=ts.plant_thickened)
    eng, b, _ = thick_engine(native, reads, seeds, m, ts.K, least13, least8, W, geometry)
    try:
        got = stream_resumable(eng, b, reads, ts.TILE, ts.BLOCK)
        assert got == exp
        ids, counts = eng.export_ids()
        assert np.array_equal(ids, ref_ids) and np.array_equal(counts, ref_counts)
        st = eng.stream_stats()
        print(geometry, keep, st)
        n_ins = sum(1 for e in exp if e[1] in (2, 4))
        assert st["coop_refused"] == 0 and st["inserts_kept"] + st["inserts_kept_nothing"] == n_ins
        if keep == "0":
            assert st["tiles_kept"] == 0 and st["inserts_kept"] == 0
        else:
            assert st["tiles_kept"] > 0 and st["tiles_redone_dirty"] > 0, st
    finally:
        eng.close()
