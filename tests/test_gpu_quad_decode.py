"""GPU: the query's quad read in rotated piece order (grp_kernels.inc quad_piece / quad_decode: a probe's header arrives in
the lane that owns the probe, which decodes it once; only the ID word crosses lanes) against the CPU oracle, at the
smallest shapes where the exchange can go wrong: every piece boundary and component of the ID slot, the overflow table,
bit offsets at both ends of a bitmap word, tiles that leave one, two or three live lanes in the last quad, and every
kernel form that decodes a line (h = 1 .. 8, the many-seed groups, an odd k, a long span, the global-table redo, the
batch's collect / delta / batch-view query, a streaming window with in-launch inserts)."""
import numpy as np
import pytest

from helpers import SEED22, compare_queries, default_seeds, palindromic_preset, random_reads, stream_resumable

pytestmark = pytest.mark.gpu

GRP_BUCKET_IDS = 13


def _bucket_width(pop, m):
    """grp_finalize's choice: ~6 set bits per bucket at the measured occupancy, 13 <= W <= 64"""
    w = 6.0 / (pop / m)
    return max(GRP_BUCKET_IDS, min(64 if w >= 64.0 else int(w), 64))


def _probe_cover(omf, oseeds, reads, tile, k, m, W):
    """(bit offset, local rank) of every probe of the reads' tiles whose filter bit is set, from the oracle's bit vector"""
    bits = np.unpackbits(omf.bits().view(np.uint8), bitorder="little")[:m]
    hs = np.concatenate([oseeds.tile_hashes(seq, tile, k, t) for seq in reads for t in range(len(seq) // tile)])
    pos = (hs % np.uint64(m)).astype(np.int64)
    for p in pos[:64]:
        assert int(bits[p]) == omf.bit(int(p))  # (the bit order assumed above)
    below = np.concatenate([[0], np.cumsum(bits, dtype=np.int64)])
    b = pos // W
    lr = below[pos] - below[b * W]
    on = bits[pos] == 1
    return (pos - b * W)[on], lr[on]


def _filled(oracle, native, k, h, tile, seeds, reads, m, fill=None):
    eng = native.Engine(k, h, tile, m, seeds)
    oseeds = oracle.Seeds(seeds)
    omf = oracle.MiBF(m, oseeds, tile, k)
    b = eng.upload(reads)
    span = max(len(s) for s in seeds)
    if fill is None:
        eng.bv_insert(b)
        fill = range(len(reads))
    else:
        eng.bv_insert(eng.upload([reads[i] for i in fill]))
    for i in fill:
        if len(reads[i]) >= span:
            omf.bv_insert_read(reads[i])
    pop = eng.finalize()
    assert pop == omf.finalize()
    return eng, omf, oseeds, b, pop


def _random_ids(eng, omf, pop, seed):
    """every rank another ID (a few saturated): a word taken from the wrong slot, piece or lane is another ID"""
    rng = np.random.default_rng(seed)
    ids = rng.integers(1, 1 << 30, size=pop, dtype=np.uint32)
    ids[rng.random(pop) < 0.05] |= np.uint32(0x80000000)
    eng.import_ids(0, ids=ids, counts=np.zeros(pop, dtype=np.uint32))
    omf.ids()[:] = ids


# occupancy 0.75: W = 13, a dense filter like C1's (ranks up to 12 inside 13 bits; no bucket can overflow);
# occupancy 0.085: W = 64 (bitmap words of 32 bits: offsets 31 / 32; buckets of 14 and more set bits: the overflow table)
@pytest.mark.parametrize("W,load", [(13, 1.39), (64, 0.0888)])
def test_every_slot_of_a_bucket(oracle, native, W, load):
    k, h, tile = 22, 3, 150
    seeds = default_seeds(h)
    reads = random_reads(25, 1900, 2100, seed=300 + W)
    n_hashes = sum(len(r) - k + 1 for r in reads) * h
    m = int(n_hashes / load)
    eng, omf, oseeds, b, pop = _filled(oracle, native, k, h, tile, seeds, reads, m)
    assert _bucket_width(pop, m) == W
    off, lr = _probe_cover(omf, oseeds, reads, tile, k, m, W)
    want_lr = {0, 1, 4, 5, 8, 9, 12}  # first / last slot of each 16-byte piece: dwords 3 | 4, 7 | 8, 11 | 12, 15
    assert want_lr <= set(lr.tolist()), sorted(set(lr.tolist()))
    assert {0, W - 1} <= set(off.tolist())
    if W == 64:
        assert {31, 32} <= set(off.tolist())
        assert (lr >= GRP_BUCKET_IDS).sum() >= 4  # the overflow table
    else:
        assert lr.max() == GRP_BUCKET_IDS - 1
    _random_ids(eng, omf, pop, 5 + W)
    _, hits, misses = compare_queries(eng, omf, b, reads)
    assert hits > 0
    eng.close()


# frames per tile = tile - 21: 65, 66, 67 (1, 2, 3 modulo 4: the last quad has one, two, three live lanes, the clamped ones
# recompute the last frame) and 133 (5 modulo 64: a wave with five live lanes)
@pytest.mark.parametrize("tile", [86, 87, 88, 154])
def test_every_quad_lane_alone(oracle, native, tile):
    k, h = 22, 3
    seeds = default_seeds(h)
    reads = random_reads(5, 2 * tile, 3 * tile + tile // 2, seed=310 + tile)
    m = int(sum(len(r) for r in reads) * h / 0.5)
    eng, omf, oseeds, b, pop = _filled(oracle, native, k, h, tile, seeds, reads, m, fill=[0, 1, 3])
    _random_ids(eng, omf, pop, tile)
    _, hits, misses = compare_queries(eng, omf, b, reads)
    assert hits > 0
    eng.close()


def _form_seeds(oracle, k, h):
    from goldrush_amd import host

    if k == 22:
        return default_seeds(h, SEED22)
    if k % 2:
        return host.make_seed_pattern("", k, 16, h)
    return default_seeds(h, palindromic_preset(k, 30, 7 + k))


# h = 1 .. 8: one group; 9: the many-seed groups; k = 23: odd; k = 66: spans 66 - 68, the long-span instantiation
@pytest.mark.parametrize("k,h,tile", [(22, 1, 100), (22, 2, 101), (22, 3, 130), (22, 5, 123), (22, 8, 110), (22, 9, 150), (23, 3, 131), (66, 3, 200)])
def test_kernel_forms(oracle, native, k, h, tile):
    seeds = _form_seeds(oracle, k, h)
    reads = random_reads(6, 2 * tile, 3 * tile + 40, seed=320 + k + h)
    m = int(sum(len(r) for r in reads) * h / 0.35)
    eng, omf, oseeds, b, pop = _filled(oracle, native, k, h, tile, seeds, reads, m, fill=[0, 1, 2, 4])
    _random_ids(eng, omf, pop, k + h)
    _, hits, misses = compare_queries(eng, omf, b, reads)
    assert hits > 0
    eng.close()


def test_global_table_redo(oracle, native, monkeypatch):
    """GRP_SMALL_HIST: a first-step table too small for a tile's IDs, so the tiles are flagged and redone by the GT form"""
    monkeypatch.setenv("GRP_SMALL_HIST", "840")
    k, h, tile = 22, 3, 200
    seeds = default_seeds(h)
    reads = random_reads(4, 2 * tile, 3 * tile + 30, seed=331)
    m = int(sum(len(r) for r in reads) * h / 0.35)
    eng, omf, oseeds, b, pop = _filled(oracle, native, k, h, tile, seeds, reads, m)
    _random_ids(eng, omf, pop, 41)
    before = eng.verify_stats()["window_flagged"]
    compare_queries(eng, omf, b, reads)
    dec = eng.classify_reads(b)
    assert all(int(d["num_tiles"]) == len(r) // tile for d, r in zip(dec, reads))
    assert eng.verify_stats()["window_flagged"] > before
    eng.close()


def _overlapping_reads(genome_len, n, lo, hi, seed):
    from goldrush_amd import synth

    g = synth.random_genome(genome_len, seed)
    return [r[1] for r in synth.make_reads(g, n, mean_len=(lo + hi) // 2, min_len=lo, seed=seed + 1, max_len=hi, sub=0.004, ins=0.0005, dele=0.0005)]


@pytest.mark.parametrize("verify", ["check", "chain"])
def test_batch_of_reads_that_share_ranks(oracle, native, verify):
    """Windows of 8 reads of a genome covered several times: the inserting reads of one batch overlap, so their ranks are
    shared (k_batch_collect's claims and chains, k_batch_delta, the batch-view query) — the serial loop's records and arrays"""
    from oracle_engine import serial_reference
    from test_gpu_batch import batch_commit

    k, h, tile, block = 22, 3, 150, 2
    seeds = default_seeds(h)
    reads = _overlapping_reads(12_000, 40, 1000, 2000, 341)
    m = oracle.load().orc_calc_optimal_size(200_000, 1, 0.1)
    exp, mf_ref = serial_reference(oracle, m, seeds, tile, k, reads, block=block)
    eng = native.Engine(k, h, tile, m, seeds)
    b = eng.upload(reads)
    eng.bv_insert(b)
    assert eng.finalize() == mf_ref.pop
    stats = {"batches": 0, "undone": 0}
    got = batch_commit(eng, b, reads, tile, block, 8, stats, verify)
    assert got == [e[:7] for e in exp]
    ids, counts = eng.export_ids()
    assert np.array_equal(ids, mf_ref.ids()) and np.array_equal(counts, mf_ref.counts())
    assert stats["batches"] > 0 and sum(1 for e in exp if e[1] in (2, 4)) >= 2
    vs = eng.verify_stats()
    assert vs["fallbacks"] == 0 and vs["impossible_deltas"] == 0, vs
    mf_ref.close()
    eng.close()


def test_streaming_window_with_in_launch_inserts(oracle, native, monkeypatch):
    """ONE resumable window that applies its inserts itself and keeps the tiles whose probes' fingerprints name no slot an
    insert wrote (two buffers per workgroup): the fingerprints are of (bucket, bit offset), whichever lane read the line"""
    from oracle_engine import serial_reference

    monkeypatch.setenv("GRP_STREAM_KEEP", "2")
    k, h, tile, block = 22, 3, 150, 2
    seeds = default_seeds(h)
    reads = _overlapping_reads(15_000, 60, 1000, 2000, 351)
    m = oracle.load().orc_calc_optimal_size(250_000, 1, 0.1)
    exp, mf_ref = serial_reference(oracle, m, seeds, tile, k, reads, block=block)
    eng = native.Engine(k, h, tile, m, seeds)
    b = eng.upload(reads)
    eng.bv_insert(b)
    assert eng.finalize() == mf_ref.pop
    got = stream_resumable(eng, b, reads, tile, block)
    assert got == exp
    ids, counts = eng.export_ids()
    assert np.array_equal(ids, mf_ref.ids()) and np.array_equal(counts, mf_ref.counts())
    st = eng.stream_stats()
    n_ins = sum(1 for g in got if g[1] in (2, 4))
    assert n_ins >= 2 and st["inserts_kept"] + st["inserts_kept_nothing"] == n_ins, st
    mf_ref.close()
    eng.close()
