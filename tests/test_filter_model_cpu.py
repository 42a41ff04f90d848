"""CPU: the plain model of the filter directory (tests/filter_model.py) against the oracle on every family of planted
vectors (tests/filter_cases.py), and what the families cover.

The oracle's vector is planted through MiBF.plant_bits before orc_mibf_finalize; its bit / rank (sdsl semantics: the ones in
front of a position, from a 512-bit block table) must equal the model's (a cumulative sum) — at EVERY position of every
case of at most 2 M bits, and at every bucket, chunk and superbucket edge +-1 plus 100 000 random positions of the larger
ones.  The model is what tests/test_gpu_filter_planted.py holds the engine to; here it is held to the oracle, so that the
engine's rank stands against the oracle's on arbitrary vectors.  Integers throughout: no tolerance."""
import numpy as np
import pytest

import filter_cases as fc
import filter_model as fm
from helpers import default_seeds

EVERY_POSITION_BELOW = 2_000_000


@pytest.fixture(scope="module")
def cases():
    return list(fc.all_cases())


@pytest.fixture(scope="module")
def models(cases):
    return {name: fm.FilterModel(words, m) for _, name, m, words in cases}


def test_model_equals_oracle_on_every_family(oracle, cases, models):
    seeds = oracle.Seeds(default_seeds(1))
    n_pos = {}
    for family, name, m, words in cases:
        mod = models[name]
        mf = oracle.MiBF(m, seeds, 500, 22)
        mf.plant_bits(words)
        assert mf.finalize() == mod.pop, name
        assert np.array_equal(mf.bits(), words), name
        if m <= EVERY_POSITION_BELOW:
            pos = np.arange(m, dtype=np.uint64)
            bit, rank = mf.bits_ranks(pos)
            assert np.array_equal(bit, mod.all_bits()), name
            assert np.array_equal(rank, mod.all_ranks()), name
        else:
            pos = mod.edge_positions()
            bit, rank = mf.bits_ranks(pos)
        assert np.array_equal(bit, mod.bit(pos)), name
        assert np.array_equal(rank, mod.rank(pos)), name
        # the single calls the other tests use agree with the array form
        for p in (0, m // 2, m - 1):
            assert (mf.bit(p), mf.rank(p)) == (int(mod.bit(p)), int(mod.rank(p))), name
        mf.close()
        n_pos[family] = n_pos.get(family, 0) + pos.size
    print("positions compared per family:", n_pos)
    assert set(n_pos) == set(fc.FAMILIES)


def test_model_counts_are_consistent(cases, models):
    for _, name, m, words in cases:
        mod = models[name]
        assert mod.counts.sum() == mod.pop and mod.counts.size == mod.n_buckets, name
        assert mod.counts.min() >= 0 and mod.counts.max() <= mod.W, name
        assert 13 <= mod.W <= 64, name
        if m <= EVERY_POSITION_BELOW and mod.pop:
            idx = mod.in_bucket_index()
            setp = mod.set_positions()
            assert idx.size == mod.pop and idx.min() == 0 and idx.max() == mod.counts.max() - 1, name
            assert int((idx >= fm.BUCKET_IDS).sum()) == mod.n_ovf and int((idx >= fm.NEAR_CW).sum()) == mod.n_far, name
            some = np.random.default_rng(3).integers(0, mod.pop, size=min(mod.pop, 2000))
            assert np.array_equal(mod.in_bucket_index(some), idx[some]), name
            assert np.array_equal(mod.in_bucket_index_at(setp[some]), idx[some]), name
            assert np.array_equal(mod.rank(setp[some]), some.astype(np.uint64)), name


def test_every_width_is_chosen(models):
    chosen = {mod.W for mod in models.values()}
    assert chosen >= set(range(13, 65)), sorted(set(range(13, 65)) - chosen)
    # and on either side of its threshold: one bit more takes the width below
    for W in range(13, 65):
        at, over = models["width_%d_at" % W], models["width_%d_over" % W]
        assert over.pop == at.pop + 1
        assert at.W == W and over.W == max(W - 1, 13), W
        assert at.counts.min() == 0 and at.counts.max() == W, W  # the runs spread the counts from empty to full


def test_exact_thresholds(models):
    """pop = 6 m / W: the rule's floor gives W; the quotient in double precision gives 58 at W = 59 (what grp_finalize
    computed until it took the quotient in integers)"""
    exact = {name: mod for name, mod in models.items() if name.endswith("_exact")}
    assert len(exact) >= 30 and {mod.W for mod in exact.values()} >= {13, 14, 59, 63, 64}
    for name, mod in exact.items():
        assert 6 * mod.m == mod.W * mod.pop and name == "width_%d_exact" % mod.W
    m59 = models["width_59_exact"]
    assert int(6.0 / (float(m59.pop) / float(m59.m))) == 58


def test_every_bucket_count_occurs(models):
    seen = set()
    for mod in models.values():
        if mod.W == 64:
            seen |= set(np.unique(mod.counts).tolist())
    assert seen >= set(range(65)), sorted(set(range(65)) - seen)
    runs = models["runs_every_phase"]
    assert runs.W == 64 and set(np.unique(runs.counts).tolist()) >= set(range(65))
    full = np.flatnonzero(runs.counts == 64)
    assert (runs.counts[full + 1] == 0).any()  # a full bucket beside an empty one
    # whole chunks without a bit behind the runs
    per_chunk = np.add.reduceat(runs.counts, np.arange(0, runs.n_buckets, fm.CHUNK_BUCKETS))
    assert (per_chunk == 0).any() and (per_chunk > 0).any()


def test_chunk_edges_and_empty_chunks(models):
    for W, j in ((13, 5), (64, 3)):
        for d in (-1, 0, 1):
            mod = models["chunks_w%d_buckets_%+d" % (W, d)]
            assert mod.W == W and mod.n_buckets == 4096 * j + d
            per_chunk = np.add.reduceat(mod.counts, np.arange(0, mod.n_buckets, fm.CHUNK_BUCKETS))
            assert (per_chunk[1::2][: j // 2] == 0).all() and (per_chunk[0::2] > 0).all()
            assert mod.counts[-1] > 0
    assert models["chunks_w64_buckets_-1"].n_ovf > 0 and models["chunks_w13_buckets_+0"].n_far > 0


def test_far_table_far_above_the_binomial_expectation(models):
    mod = models["sparse_with_dense_stretch"]
    expect = fm.binomial_far_expectation(mod.m, mod.pop)
    print("far count words %d, a uniform vector of the occupancy %.4f gives %.0f" % (mod.n_far, mod.pop / mod.m, expect))
    assert mod.W == 64 and mod.n_far > 10 * expect and expect > 1000
    assert int((mod.counts == 64).sum()) >= 5000


def test_short_last_buckets_with_bits(models):
    last = models["bit_m_minus_1"]
    assert last.W == 64 and last.m % 64 and last.counts[-1] == 1 and last.pop == 1
    ones = models["all_ones"]
    assert ones.W == 13 and ones.m % 13 == 3 and ones.counts[-1] == 3 and ones.n_ovf == 0 and ones.n_far == 5 * (ones.n_buckets - 1)
    assert models["empty"].geometry() == [64, (fc.M + 63) // 64, 0, 0]
    assert sum(1 for mod in models.values() if mod.m % mod.W and mod.counts[-1] > 0) >= 10


def test_thicken(models):
    rng = np.random.default_rng(9)
    for m in (64, 65, 1000, fc.M):
        words = fm.from_bits((rng.random(m) < 0.01).astype(np.uint8))
        t = fc.thicken(words, m)
        bits, tb = fm.to_bits(words, m), fm.to_bits(t, m)
        want = np.repeat(np.add.reduceat(bits, np.arange(0, m, 64)) > 0, 64)[:m]
        assert np.array_equal(tb, want.astype(np.uint8))
        assert np.array_equal(fc.thicken(t, m), t)
    mod = models["thickened_uniform"]
    assert 13 < mod.W < 64 and mod.n_ovf > mod.pop // 4  # full words straddle the buckets; a third of the ranks overflow


def test_smallest_sizes(oracle, models):
    assert fc.MIN_M == 64 and min(fc.SMALLEST) == fc.MIN_M and max(fc.REFUSED) == fc.MIN_M - 1
    for m in fc.SMALLEST:
        assert models["smallest_%d_full" % m].geometry() == [13, -(-m // 13), 0, sum(max(min(13, m - b * 13) - 8, 0) for b in range(-(-m // 13)))]
        assert models["smallest_%d_empty" % m].geometry() == [64, -(-m // 64), 0, 0]


def test_plant_bits_refuses_what_it_cannot_plant(oracle):
    seeds = oracle.Seeds(default_seeds(1))
    mf = oracle.MiBF(100, seeds, 500, 22)
    with pytest.raises(ValueError):
        mf.plant_bits(np.zeros(3, dtype=np.uint64))
    with pytest.raises(ValueError):
        mf.plant_bits(np.array([0, 1 << 36], dtype=np.uint64))  # position 100
    mf.plant_bits(np.array([1, 1 << 35], dtype=np.uint64))
    mf.plant_bits(np.array([2, 0], dtype=np.uint64))  # ORs
    assert mf.finalize() == 3 and [mf.rank(p) for p in (0, 1, 2, 99)] == [0, 1, 2, 2] and mf.bit(99) == 1
    with pytest.raises(ValueError):
        mf.plant_bits(np.zeros(2, dtype=np.uint64))
    mf.close()
