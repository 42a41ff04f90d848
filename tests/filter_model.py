"""Test infrastructure: a plain numpy model of the filter directory grp_finalize builds from a bit vector.

From the vector's 64-bit words and m it states what the documented rule gives — nothing of the device code is restated
here (no reciprocal division, no rel / super, no hashing):

    pop                      the set bits in [0, m)
    bit(pos), rank(pos)      rank = the ones in [0, pos)  (sdsl rank semantics, as the oracle's orc_mibf_rank)
    W                        clamp(floor(6 m / pop), 13, 64), 64 at pop = 0: ~6 set bits per bucket
    n_buckets                ceil(m / W); bucket b holds the positions [b W, min((b + 1) W, m))
    counts                   the set bits of every bucket
    n_ovf                    sum max(c - 13, 0): IDs that live in the overflow table
    n_far                    sum max(c - 8, 0): count words that live in the far table
    in_bucket_index          per rank, how many set bits of its bucket lie in front of it

Bit i of the vector is bit i & 63 of word i >> 6 (the sdsl layout the oracle and the engine share)."""
import numpy as np

BUCKET_IDS = 13  # ID slots of a bucket unit
NEAR_CW = 8      # count words of a bucket unit
CHUNK_BUCKETS = 4096
SUPER_BUCKETS = 1 << 22


def n_words(m):
    return (m + 63) // 64


def mask_tail(words, m):
    """the words with every bit at a position >= m cleared (in place), returned"""
    if m & 63:
        words[-1] &= np.uint64((1 << (m & 63)) - 1)
    return words


def from_bits(bits):
    """uint64 words of a 0/1 array of m entries"""
    m = len(bits)
    padded = np.zeros(n_words(m) * 64, dtype=np.uint8)
    padded[:m] = bits
    return np.packbits(padded, bitorder="little").view("<u8").astype(np.uint64)


def to_bits(words, m):
    return np.unpackbits(np.ascontiguousarray(words, dtype="<u8").view(np.uint8), bitorder="little")[:m]


def width_for(m, pop):
    """the bucket width of a filter of m bits with pop set bits"""
    if pop == 0:
        return 64
    return max(13, min((6 * m) // pop, 64))


class FilterModel:
    def __init__(self, words, m, keep_bits=None):
        words = np.ascontiguousarray(words, dtype=np.uint64)
        assert words.size == n_words(m)
        self.m = m
        self.words = words
        small = m <= (1 << 26) if keep_bits is None else keep_bits
        per_word = _popcount64(words)
        if m & 63:
            assert int(words[-1]) >> (m & 63) == 0, "bits at positions >= m"
        self.pop = int(per_word.sum())
        self.W = width_for(m, self.pop)
        self.n_buckets = (m + self.W - 1) // self.W
        # ones in front of every word: rank at any position comes from here and one masked word
        self._word_rank = np.zeros(words.size + 1, dtype=np.uint64)
        np.cumsum(per_word, out=self._word_rank[1:])
        edges = np.minimum(np.arange(self.n_buckets + 1, dtype=np.uint64) * np.uint64(self.W), np.uint64(m))
        at_edge = self.rank(edges)
        self.bucket_first_rank = at_edge[:-1]
        self.counts = np.diff(at_edge.astype(np.int64))
        self.n_ovf = int(np.maximum(self.counts - BUCKET_IDS, 0).sum())
        self.n_far = int(np.maximum(self.counts - NEAR_CW, 0).sum())
        self._bits = to_bits(words, m) if small else None

    def geometry(self):
        """what grp_debug_filter_geometry reports"""
        return [self.W, self.n_buckets, self.n_ovf, self.n_far]

    def bit(self, pos):
        pos = np.asarray(pos, dtype=np.uint64)
        return ((self.words[(pos >> np.uint64(6)).astype(np.int64)] >> (pos & np.uint64(63))) & np.uint64(1)).astype(np.uint8)

    def rank(self, pos):
        """ones in [0, pos); pos may be m"""
        pos = np.asarray(pos, dtype=np.uint64)
        w = (pos >> np.uint64(6)).astype(np.int64)
        inside = pos & np.uint64(63)
        padded = np.append(self.words, np.uint64(0))  # pos = m at a word edge reads one word behind the vector
        below = padded[w] & ((np.uint64(1) << inside) - np.uint64(1))
        return self._word_rank[w] + _popcount64(below).reshape(pos.shape)

    def all_bits(self):
        assert self._bits is not None, "the model keeps the unpacked bits of small filters only"
        return self._bits

    def all_ranks(self):
        """rank(pos) of every pos in [0, m)"""
        b = self.all_bits()
        r = np.zeros(self.m, dtype=np.uint64)
        np.cumsum(b[:-1], out=r[1:])
        return r

    def set_positions(self):
        """the position of every rank, ascending"""
        return np.flatnonzero(self.all_bits()).astype(np.uint64)

    def in_bucket_index(self, ranks=None):
        """per rank (all of them by default) the set bits of its bucket in front of it"""
        if ranks is None:
            return (np.arange(self.pop, dtype=np.int64) - np.repeat(self.bucket_first_rank.astype(np.int64), self.counts)).astype(np.int64)
        ranks = np.asarray(ranks, dtype=np.uint64)
        b = np.searchsorted(self.bucket_first_rank, ranks, side="right") - 1
        # (empty buckets share their first rank with the next one: side="right" lands on the last of them, which holds the rank)
        return (ranks - self.bucket_first_rank[b]).astype(np.int64)

    def in_bucket_index_at(self, pos):
        """for positions whose bit is set: the in-bucket index of their rank"""
        pos = np.asarray(pos, dtype=np.uint64)
        start = (pos // np.uint64(self.W)) * np.uint64(self.W)
        return (self.rank(pos) - self.rank(start)).astype(np.int64)

    def edge_positions(self, n_random=100_000, seed=1, bucket_sample=None):
        """where a directory goes wrong first: every bucket edge +-1, every chunk and superbucket edge +-1, 0, m - 1, and
        n_random positions.  bucket_sample: of the bucket edges only that many random ones (and those within two buckets
        of a superbucket edge) — a filter of 10^7 buckets and more"""
        W, m = self.W, self.m
        rng = np.random.default_rng(seed)
        if bucket_sample is None or bucket_sample >= self.n_buckets:
            b = np.arange(self.n_buckets + 1, dtype=np.int64)
        else:
            sb = np.arange(0, self.n_buckets + SUPER_BUCKETS, SUPER_BUCKETS, dtype=np.int64)
            b = np.concatenate([rng.integers(0, self.n_buckets + 1, size=bucket_sample, dtype=np.int64)] + [sb + d for d in range(-2, 3)])
        e = b * W
        parts = [e - 1, e, e + 1]
        for step in (CHUNK_BUCKETS, SUPER_BUCKETS):
            c = np.arange(0, self.n_buckets + step, step, dtype=np.int64) * W
            parts += [c - 1, c, c + 1]
        parts.append(np.array([0, m - 1], dtype=np.int64))
        parts.append(rng.integers(0, m, size=n_random, dtype=np.int64))
        p = np.unique(np.concatenate(parts))
        return p[(p >= 0) & (p < m)].astype(np.uint64)


_POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.uint8)


def _popcount64(a):
    a = np.ascontiguousarray(a, dtype="<u8")
    return _POP8[a.view(np.uint8)].reshape(a.shape + (8,)).sum(axis=-1, dtype=np.uint64)


def binomial_far_expectation(m, pop, W=None):
    """the far count words a uniform vector of the same m and pop would give: n_buckets E[max(c - 8, 0)], c ~ B(W, pop/m)"""
    W = W or width_for(m, pop)
    p = pop / m
    if p <= 0.0 or p >= 1.0:
        return 0.0 if p <= 0.0 else ((m + W - 1) // W) * max(W - NEAR_CW, 0)
    pk = (1.0 - p) ** W
    tail = 0.0
    for k in range(W + 1):
        if k > NEAR_CW:
            tail += pk * (k - NEAR_CW)
        pk = pk * (W - k) / (k + 1) * p / (1.0 - p)
    return tail * ((m + W - 1) // W)
