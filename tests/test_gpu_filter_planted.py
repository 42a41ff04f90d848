"""GPU: the filter directory grp_finalize builds — bucket units, width W, super[], the overflow and far side tables —
against the plain model of tests/filter_model.py on PLANTED bit vectors (tests/filter_cases.py), not on what the hash fill
writes.  The vector goes in through grp_bv_import_device from a torch tensor; the model is pinned to the oracle's sdsl-rank
on the same vectors by tests/test_filter_model_cpu.py.

Per case, exact integers: pop; grp_export_bits = the planted words; grp_debug_filter_geometry = the model's {W, buckets,
overflow IDs, far count words}; grp_rank's bit and rank at EVERY position (filters of at most 2 M bits) or at every bucket,
chunk and superbucket edge +-1, 0, m - 1 and 100 000 random positions; a grp_import_ids / grp_export_ids round trip of
random IDs (bit 31 and the bare 0x80000000 among them) and counts over all ranks; the same over windows whose ends fall
inside a bucket at in-bucket indices 7|8 and 12|13 and inside a full bucket; grp_reset_ids leaves nothing, side tables
included, and a second import reads back exact.  One engine per m, grp_rewind between the cases (into another W).

Counts stay below 2^16 and every far key is written by grp_finalize: nothing here comes near the engine's two traps."""
import numpy as np
import pytest

import filter_cases as fc
import filter_model as fm
from helpers import default_seeds, random_reads

pytestmark = pytest.mark.gpu

K, H, TILE = 22, 3, 500
EVERY_POSITION_BELOW = 2_000_000


def plant(eng, words, merge=False):
    """the vector into the engine's phase-1 bit vector, from device memory"""
    import torch

    t = torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint64).view(np.int64).copy()).to("cuda")
    torch.cuda.synchronize()
    assert t.data_ptr() % 16 == 0 and t.numel() * 8 >= eng.bv_words() * 4
    (eng.bv_merge_device if merge else eng.bv_import_device)(t.data_ptr())  # (synchronous: the tensor may go)
    del t


def _random_ids(rng, n):
    ids = rng.integers(0, 1 << 31, size=n, dtype=np.uint32)
    ids[rng.random(n) < 0.2] |= np.uint32(0x80000000)
    ids[rng.random(n) < 0.05] = np.uint32(0x80000000)  # "saturated empty"
    ids[rng.random(n) < 0.05] = 0
    return ids, rng.integers(0, 1 << 16, size=n, dtype=np.uint32)


def _windows(mod, per_kind=3):
    """[first, first + n) whose ends fall inside buckets: first at in-bucket index 8 (7 outside), last at 12 (13 outside),
    both inside a full bucket, and one from inside a bucket with far ranks to inside the next one with overflow ranks"""
    out = []
    r0 = mod.bucket_first_rank.astype(np.int64)

    def some(idx):
        return idx[np.unique(np.linspace(0, idx.size - 1, per_kind).astype(int))] if idx.size else idx

    for b in some(np.flatnonzero(mod.counts > fm.BUCKET_IDS)):
        out.append((int(r0[b]) + 8, 5))                           # 7|8 .. 12|13
        out.append((int(r0[b]) + 13, int(mod.counts[b]) - 13))    # the overflow ranks alone
        out.append((int(r0[b]) + 12, 2))                          # across 12|13
    for b in some(np.flatnonzero(mod.counts > fm.NEAR_CW)):
        out.append((int(r0[b]) + 7, 2))                           # across 7|8
        out.append((int(r0[b]), 8))                               # the near ranks alone
    for b in some(np.flatnonzero(mod.counts == mod.W)):
        out.append((int(r0[b]) + 1, mod.W - 2))
    big = np.flatnonzero(mod.counts > fm.BUCKET_IDS)
    if big.size >= 2:
        a, b = int(big[0]), int(big[-1])
        out.append((int(r0[a]) + 9, int(r0[b]) + 13 - (int(r0[a]) + 9) + 1))
    return [(f, n) for f, n in out if n > 0 and f + n <= mod.pop]


def check_directory(eng, mod, words, name, positions=None, windows=True, seed=1):
    """finalize and everything above; returns the positions compared and the ranks round-tripped"""
    pop = eng.finalize()
    assert pop == mod.pop, name
    assert np.array_equal(eng.export_bits(), words), name
    assert eng.filter_geometry() == mod.geometry(), (name, eng.filter_geometry(), mod.geometry())
    if positions is None and mod.m <= EVERY_POSITION_BELOW:
        positions = np.arange(mod.m, dtype=np.uint64)
        bit, rank = eng.rank(positions)
        assert np.array_equal(bit, mod.all_bits()), name
        assert np.array_equal(rank, mod.all_ranks()), name
    else:
        positions = mod.edge_positions() if positions is None else positions
        bit, rank = eng.rank(positions)
    assert np.array_equal(bit, mod.bit(positions)), name
    assert np.array_equal(rank, mod.rank(positions)), name
    n_ranks = 0
    if pop:
        rng = np.random.default_rng(seed)
        ids, counts = _random_ids(rng, pop)
        eng.import_ids(0, ids=ids, counts=counts)
        gi, gc = eng.export_ids()
        assert np.array_equal(gi, ids) and np.array_equal(gc, counts), name
        n_ranks += pop
        for first, n in (_windows(mod) if windows else []):
            gi, gc = eng.export_ids(first, n)
            assert np.array_equal(gi, ids[first:first + n]) and np.array_equal(gc, counts[first:first + n]), (name, first, n)
            wi, wc = _random_ids(rng, n)
            eng.import_ids(first, ids=wi, counts=wc)
            ids[first:first + n], counts[first:first + n] = wi, wc
            n_ranks += n
        gi, gc = eng.export_ids()
        assert np.array_equal(gi, ids) and np.array_equal(gc, counts), name  # the windows landed, nothing else moved
        # ids alone / counts alone leave the other array as it is
        lo, n = pop // 3, max(pop // 5, 1)
        wi, wc = _random_ids(rng, n)
        eng.import_ids(lo, ids=wi)
        ids[lo:lo + n] = wi
        eng.import_ids(pop - n, counts=wc)
        counts[pop - n:] = wc
        gi, gc = eng.export_ids()
        assert np.array_equal(gi, ids) and np.array_equal(gc, counts), name
        eng.reset_ids()
        gi, gc = eng.export_ids()
        assert not gi.any() and not gc.any(), name
        ids, counts = _random_ids(rng, pop)
        eng.import_ids(0, ids=ids, counts=counts)
        gi, gc = eng.export_ids()
        assert np.array_equal(gi, ids) and np.array_equal(gc, counts), name
        # ... and the geometry and the ranks have not moved under the IDs
        assert eng.filter_geometry() == mod.geometry(), name
        b2, r2 = eng.rank(positions[:: max(positions.size // 5000, 1)])
        assert np.array_equal(r2, mod.rank(positions[:: max(positions.size // 5000, 1)])), name
    return positions.size, n_ranks


def run_cases(native, cases):
    """one engine per m, grp_rewind between the cases of an m"""
    by_m = {}
    for name, m, words in cases:
        by_m.setdefault(m, []).append((name, words))
    n_pos = n_ranks = 0
    widths = []
    for m, group in by_m.items():
        eng = native.Engine(K, H, TILE, m, default_seeds(H))
        try:
            for i, (name, words) in enumerate(group):
                if i:
                    eng.rewind()
                mod = fm.FilterModel(words, m)
                plant(eng, words)
                a, b = check_directory(eng, mod, words, name, seed=i)
                n_pos, n_ranks = n_pos + a, n_ranks + b
                widths.append(mod.W)
        finally:
            eng.close()
    print("%d cases, %d positions and %d ranks compared, widths %s" % (len(cases), n_pos, n_ranks, sorted(set(widths))))
    return widths


@pytest.mark.parametrize("family", ["basic", "exact", "runs", "chunks", "stretch", "smallest", "thickened"])
def test_filter_planted_family(native, family):
    run_cases(native, fc.FAMILIES[family]())


@pytest.mark.parametrize("lo", [13, 26, 39, 52])
def test_filter_planted_widths(native, lo):
    """every width on either side of its threshold; the rewinds walk down through the widths (W, W - 1, W + 1, W, ...)"""
    widths = run_cases(native, fc.width_cases(range(lo, lo + 13)))
    assert set(widths) >= set(range(lo, lo + 13))


@pytest.mark.parametrize("m", [fc.M, 13 * 4096 * 5])
def test_filter_planted_or_path(native, m):
    """grp_bv_merge_device of a planted vector over a hashed fill = the OR of the two (a word count that is and is not a
    multiple of four: the merge kernel's 16-byte body and its tail)"""
    eng = native.Engine(K, H, TILE, m, default_seeds(H))
    try:
        assert (eng.bv_words() % 4 != 0) == (m == fc.M)
        b = eng.upload(random_reads(4, 3000, 5000, seed=5))
        eng.bv_insert(b)
        hashed = eng.export_bits()
        assert 0.05 < fm.FilterModel(hashed, m).pop / m < 0.3
        planted = fm.from_bits(fc.run_bits(m, m // 7, 11))
        planted[-1] |= np.uint64(1) << np.uint64((m - 1) & 63)
        plant(eng, planted, merge=True)
        both = hashed | planted
        assert np.array_equal(eng.export_bits(), both)  # phase 1
        check_directory(eng, fm.FilterModel(both, m), both, "or_path")
    finally:
        eng.close()


def test_filter_planted_prepared_tables(native):
    """The sparse vector with one dense stretch under grp_set_occupancy_hint = its true occupancy: the far table prepared
    for the hint (the binomial expectation) is 30 times too small.  The filter is the same as without the hint, and the
    prepared tables do not count as used.  A uniform vector of the same occupancy is the control: there the prepared
    tables fit (taken where the device had the room to prepare them: printed, as tests/test_gpu_rewind.py does)."""
    (name, m, words), = fc.stretch_cases()
    mod = fm.FilterModel(words, m)
    rng = np.random.default_rng(8)
    uniform = fm.from_bits((rng.random(m) < mod.pop / m * 0.98).astype(np.uint8))
    umod = fm.FilterModel(uniform, m)
    assert umod.W == mod.W == 64 and mod.n_far > 10 * umod.n_far
    positions = mod.edge_positions()
    eng = native.Engine(K, H, TILE, m, default_seeds(H))
    try:
        reads = eng.upload(random_reads(2, 3000, 4000, seed=6))

        def observe(vec, model, hint):
            if hint:
                eng.set_occupancy_hint(hint)
            eng.bv_insert(reads)  # (the tables are prepared beside the first fill launch; the import replaces what it wrote)
            plant(eng, vec)
            check_directory(eng, model, vec, "hint %s" % hint, positions=positions)
            ids, counts = eng.export_ids()
            bit, rank = eng.rank(positions)
            used, pop = eng.finalize_times()["prepared_tables_used"], eng.pop
            eng.rewind()
            return used, (pop, ids.tobytes(), counts.tobytes(), bit.tobytes(), rank.tobytes())

        used0, plain = observe(words, mod, None)
        used1, hinted = observe(words, mod, mod.pop / m)
        used2, _ = observe(uniform, umod, mod.pop / m)
        print("prepared tables used: no hint %s, dense stretch %s, uniform control %s%s" % (used0, used1, used2, "" if used2 else " (the device had no room to prepare, or did not)"))
        assert hinted == plain
        assert not used0
        assert not used1  # (units offered or not: a far table prepared for the binomial expectation does not hold this one)
    finally:
        eng.close()


def test_filter_planted_stray_bits_are_refused(native):
    """Bits at positions >= m in an imported or merged vector (include/grpath.h): grp_finalize fails with a named
    GRP_ERR_INVALID, no pop is handed out, nothing is finalized, and after grp_rewind the engine builds a clean filter."""
    m = fc.M
    clean = fm.from_bits(fc.run_bits(m, m // 9, 21))
    stray = clean.copy()
    stray[-1] |= (np.uint64(1) << np.uint64(m & 63)) | (np.uint64(1) << np.uint64((m & 63) + 2))
    eng = native.Engine(K, H, TILE, m, default_seeds(H))
    try:
        reads = eng.upload(random_reads(1, 3000, 3000, seed=7))
        for merge in (False, True):
            plant(eng, stray, merge=merge)
            with pytest.raises(native.GrpError) as e:
                eng.finalize()
            assert e.value.code == native.GRP_ERR_INVALID and "2 set bits at positions >= m" in str(e.value)
            assert eng.pop == 0 and eng.lib.grp_pop(eng._h) == 0
            for call in (eng.filter_geometry, lambda: eng.rank([0]), lambda: eng.query_tiles(reads, 0, 1), eng.reset_ids):
                with pytest.raises(native.GrpError):
                    call()
            eng.rewind()
            plant(eng, clean, merge=merge)
            check_directory(eng, fm.FilterModel(clean, m), clean, "clean after stray")
            eng.rewind()
    finally:
        eng.close()


def test_filter_planted_rank_refuses_positions_behind_m(native):
    m = fc.M
    words = fm.from_bits(fc.run_bits(m, m // 9, 22))
    mod = fm.FilterModel(words, m)
    eng = native.Engine(K, H, TILE, m, default_seeds(H))
    try:
        with pytest.raises(native.GrpError) as e:  # not finalized
            eng.rank([0])
        assert e.value.code == native.GRP_ERR_STATE
        plant(eng, words)
        eng.finalize()
        for bad in ([m], [0, m - 1, m], [m + 63], [1 << 40], [(1 << 64) - 1]):
            with pytest.raises(native.GrpError) as e:
                eng.rank(bad)
            assert e.value.code == native.GRP_ERR_INVALID and ">= m" in str(e.value)
        bit, rank = eng.rank([m - 1, 0])
        assert [int(x) for x in rank] == [int(mod.rank(m - 1)), 0] and int(bit[0]) == int(mod.bit(m - 1))
    finally:
        eng.close()


def test_filter_planted_sizes_below_the_bound_are_refused(native):
    seeds = default_seeds(H)
    for m in fc.REFUSED:
        with pytest.raises(native.GrpError) as e:
            native.Engine(K, H, TILE, m, seeds)
        assert e.value.code == native.GRP_ERR_INVALID and "m=%d" % m in str(e.value)
    eng = native.Engine(K, H, TILE, 0, seeds)
    try:
        for m in fc.REFUSED:
            with pytest.raises(native.GrpError) as e:
                eng.set_filter_size(m)
            assert e.value.code == native.GRP_ERR_INVALID
        eng.set_filter_size(fc.MIN_M)
        words = np.array([0x8000000000000001], dtype=np.uint64)
        plant(eng, words)
        check_directory(eng, fm.FilterModel(words, fc.MIN_M), words, "m = 64 set late")
    finally:
        eng.close()


def test_filter_planted_full_superbucket(native):
    """The one large case: 3.2 * 10^9 bits at W = 64 whose first 2^28 bits are all ones — ONE full superbucket (rel reaches
    2^28 - 64, super[1] = 2^28, the chunk scan runs twelve rounds of 1024 chunks) — then an empty superbucket, then sparse
    random bits (density 1/256).  pop, geometry, bits, ranks at every chunk and superbucket edge +-1, at the edges +-1 of
    200 000 random buckets and of the buckets round the superbucket edges, at 100 000 random positions, and an ID round trip
    over a window across the first superbucket edge (and what lies behind the empty one)."""
    m = 3_200_000_037
    nw = fm.n_words(m)
    rng = np.random.default_rng(12)
    words = np.zeros(nw, dtype=np.uint64)
    words[: 1 << 22] = np.uint64(0xFFFFFFFFFFFFFFFF)
    tail = rng.integers(0, 1 << 64, size=nw - (1 << 23), dtype=np.uint64)
    for _ in range(7):
        tail &= rng.integers(0, 1 << 64, size=tail.size, dtype=np.uint64)
    words[1 << 23:] = tail
    del tail
    fm.mask_tail(words, m)
    mod = fm.FilterModel(words, m, keep_bits=False)
    assert mod.W == 64 and mod.pop / m < 6 / 64 and mod.n_buckets > 11 * 1024 * 4096
    assert int(mod.counts[: 1 << 22].min()) == 64 and int(mod.counts[1 << 22: 1 << 23].max()) == 0
    assert int(mod.bucket_first_rank[(1 << 22) - 1]) == (1 << 28) - 64 and int(mod.bucket_first_rank[1 << 23]) == 1 << 28
    positions = mod.edge_positions(bucket_sample=200_000)
    eng = native.Engine(K, H, TILE, m, default_seeds(H))
    try:
        plant(eng, words)
        assert eng.finalize() == mod.pop
        assert eng.filter_geometry() == mod.geometry()
        assert np.array_equal(eng.export_bits(), words)
        bit, rank = eng.rank(positions)
        assert np.array_equal(bit, mod.bit(positions)) and np.array_equal(rank, mod.rank(positions))
        edge = 1 << 28
        for first, n in ((edge - 1000, 2000), (edge - 64 - 13, 13 + 8), (0, 70), (mod.pop - 500, 500)):
            ids, counts = _random_ids(rng, n)
            eng.import_ids(first, ids=ids, counts=counts)
            gi, gc = eng.export_ids(first, n)
            assert np.array_equal(gi, ids) and np.array_equal(gc, counts), first
        gi, gc = eng.export_ids(edge - 2000, 1000)  # beside the window: untouched
        assert not gi.any() and not gc.any()
        eng.reset_ids()
        gi, gc = eng.export_ids(edge - 1000, 2000)
        assert not gi.any() and not gc.any()
        print("%d positions compared, pop %d, geometry %s" % (positions.size, mod.pop, mod.geometry()))
    finally:
        eng.close()
