"""Test infrastructure: the named families of bit vectors the filter-directory tests plant (tests/test_filter_model_cpu.py on
the oracle, tests/test_gpu_filter_planted.py on the engine).  What the hash fill writes is uniform at occupancy 0.1 - 0.35;
these are everything else a directory has to hold: empty and full, one bit, every bucket width on either side of its
threshold and (where 6 m / W is whole) on it, runs at every phase against a word, empty and dense chunks at every bucket count around a chunk edge, a sparse
vector with one dense stretch, the thickened fill, the smallest filters.  No bit at a position >= m is ever set.

A case is (name, m, words): uint64 words, bit i = bit i & 63 of word i >> 6.  Every generator is deterministic."""
import numpy as np

from filter_model import from_bits, mask_tail, n_words

M = 260_003          # a multiple of nothing: the last bucket is short at W = 13 (3 bits) and at W = 64 (35 bits)
M_RUNS = 1_450_007   # the run family needs W = 64 with 133 120 set bits: m > 64 * 133120 / 6
M_STRETCH = 4_000_037
MIN_M = 64           # what grp_create / grp_set_filter_size accept; below: refused (GRP_ERR_INVALID)
SMALLEST = (64, 65, 77, 127, 128, 129)
REFUSED = (1, 5, 13, 63)


def thicken(words, m):
    """every 64-bit word that holds a bit becomes all ones (the tail masked to m): the set bits of the fill move to the
    far ends of their buckets' rank ranges, where the side tables are"""
    out = np.where(np.asarray(words, dtype=np.uint64) != 0, np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(0))
    return mask_tail(out, m)


def run_bits(m, pop, seed, max_run=64):
    """m bits with exactly pop ones laid down as runs of 1 .. max_run ones behind gaps that give the density: buckets of
    every count between empty and full (128 ones and 128 zeros at a fixed place hold a full and an empty bucket of any
    width; the single bits that make the count exact are flipped elsewhere)"""
    rng = np.random.default_rng(seed)
    bits = np.zeros(m, dtype=np.uint8)
    if pop >= m:
        bits[:] = 1
        return bits
    p = pop / m
    mean_run = (1 + max_run) / 2
    mean_gap = max(mean_run * (1 - p) / p, 1.0)
    at = 0
    while at < m:
        at += int(rng.integers(0, int(2 * mean_gap) + 1))
        n = int(rng.integers(1, max_run + 1))
        bits[at:at + n] = 1
        at += n + 1
    free = np.ones(m, dtype=bool)
    if m >= 2048 and 128 <= pop <= m - 128:
        bits[1024:1152] = 1
        bits[1152:1280] = 0
        free[1024:1280] = False
    have = int(bits.sum())
    if have > pop:
        ones = np.flatnonzero((bits == 1) & free)
        bits[rng.choice(ones, size=have - pop, replace=False)] = 0
    elif have < pop:
        zeros = np.flatnonzero((bits == 0) & free)
        bits[rng.choice(zeros, size=pop - have, replace=False)] = 1
    return bits


def basic_cases():
    nw = n_words(M)
    empty = np.zeros(nw, dtype=np.uint64)
    ones = mask_tail(np.full(nw, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64), M)
    first = empty.copy()
    first[0] = 1
    last = empty.copy()
    last[-1] = np.uint64(1) << np.uint64((M - 1) & 63)
    return [("empty", M, empty), ("all_ones", M, ones), ("bit_0", M, first), ("bit_m_minus_1", M, last)]


def width_cases(widths=range(13, 65)):
    """for every width W two vectors: pop = floor(6 m / W), the most set bits that still give W, and one bit more, which
    gives W - 1 (13 stays 13)"""
    out = []
    for W in widths:
        pop = (6 * M) // W
        out.append(("width_%d_at" % W, M, from_bits(run_bits(M, pop, 1000 + W))))
        out.append(("width_%d_over" % W, M, from_bits(run_bits(M, pop + 1, 2000 + W))))
    return out


M_EXACT = 277_200                          # 6 m = 2^5 3^3 5^2 7 11: 27 widths divide it
EXACT_OWN_M = (13, 17, 31, 47, 59, 61, 64)  # widths that do not: m = 4333 W, pop = 6 * 4333


def exact_width_cases():
    """pop = 6 m / W exactly: the threshold itself, where floor(6 m / pop) = W and a quotient taken in floating point may
    come out one below (6.0 / (pop / m) = 58.99999999999999 at W = 59)"""
    out = []
    for W in range(13, 65):
        if (6 * M_EXACT) % W == 0:
            out.append(("width_%d_exact" % W, M_EXACT, from_bits(run_bits(M_EXACT, 6 * M_EXACT // W, 3000 + W))))
    for W in EXACT_OWN_M:
        out.append(("width_%d_exact" % W, 4333 * W, from_bits(run_bits(4333 * W, 6 * 4333, 3000 + W))))
    return out


def run_phase_cases():
    """runs of 1 .. 64 ones at every phase 0 .. 63 against a 64-bit word, one per 128-bit slot, then nothing: at W = 64
    buckets are words, so every count 0 .. 64 occurs, full buckets lie beside empty ones, and whole chunks are empty"""
    bits = np.zeros(M_RUNS, dtype=np.uint8)
    slot = 0
    for n in range(1, 65):
        for phase in range(64):
            bits[slot * 128 + phase: slot * 128 + phase + n] = 1
            slot += 1
    return [("runs_every_phase", M_RUNS, from_bits(bits))]


def chunk_cases():
    """chunks of 4096 buckets alternately dense and empty, the bucket count one below, at and one above a multiple of 4096.
    W = 13 (dense chunks hold runs at density 0.9, chunks 0, 2, 4 of five) and W = 64 (dense chunks hold full words at
    density 0.12, chunks 0 and 2 of three)."""
    out = []
    for W, j, m_list in ((13, 5, (13 * (4096 * 5 - 1) - 5, 13 * 4096 * 5, 13 * 4096 * 5 + 1)),
                         (64, 3, (64 * (4096 * 3 - 1) - 29, 64 * 4096 * 3, 64 * 4096 * 3 + 1))):
        chunk_bits = 4096 * W
        for m in m_list:
            bits = np.zeros(m, dtype=np.uint8)
            for c in range(0, j + 1, 2):
                lo, hi = c * chunk_bits, min((c + 1) * chunk_bits, m)
                if lo >= m:
                    break
                if W == 13:
                    bits[lo:hi] = run_bits(hi - lo, int(0.9 * (hi - lo)), 300 + c)
                else:
                    full = np.random.default_rng(400 + c).random((hi - lo + 63) // 64) < 0.12
                    bits[lo:hi] = np.repeat(full.astype(np.uint8), 64)[: hi - lo]
            bits[m - 1] = 1  # the last bucket is never empty: one bit in a chunk of one bucket where n_buckets = 4096 j + 1
            out.append(("chunks_w%d_buckets_%+d" % (W, (-(-m // W)) - 4096 * j), m, from_bits(bits)))
    return out


def stretch_cases():
    """sparse overall (W = 64) with one stretch of 5000 full buckets: 280 000 far count words and 255 000 overflow IDs
    where a uniform vector of the same occupancy has a few thousand"""
    rng = np.random.default_rng(77)
    bits = (rng.random(M_STRETCH) < 0.004).astype(np.uint8)
    lo = 64 * 20_011
    bits[lo: lo + 64 * 5000] = 1
    return [("sparse_with_dense_stretch", M_STRETCH, from_bits(bits))]


def smallest_cases():
    out = []
    for m in SMALLEST:
        rng = np.random.default_rng(m)
        out.append(("smallest_%d_empty" % m, m, np.zeros(n_words(m), dtype=np.uint64)))
        out.append(("smallest_%d_full" % m, m, mask_tail(np.full(n_words(m), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64), m)))
        out.append(("smallest_%d_last_bit" % m, m, from_bits(np.eye(1, m, m - 1, dtype=np.uint8)[0])))
        out.append(("smallest_%d_sparse" % m, m, from_bits((rng.random(m) < 0.08).astype(np.uint8))))
    return out


def thickened_uniform_case():
    """the thickening on a uniform vector (what the hash fill writes at occupancy 0.01): full words straddle the buckets"""
    rng = np.random.default_rng(5)
    words = from_bits((rng.random(M) < 0.004).astype(np.uint8))
    return [("thickened_uniform", M, thicken(words, M))]


FAMILIES = {
    "basic": basic_cases,
    "widths": width_cases,
    "exact": exact_width_cases,
    "runs": run_phase_cases,
    "chunks": chunk_cases,
    "stretch": stretch_cases,
    "smallest": smallest_cases,
    "thickened": thickened_uniform_case,
}


def all_cases():
    for name, make in FAMILIES.items():
        for case in make():
            yield (name,) + case
