"""DEFLATE streams that neither zlib's compressor nor libdeflate writes, for the device inflate (csrc/grp_inflate.inc;
tests/test_gpu_inflate_generated.py, test_deflate_gen_cpu.py, tools/dev/inflate_host_cases.py --generated): random
complete prefix codes up to 15 bits (7 for the code length code) over random token blocks, every (distance, length) pair
of the match copy, members that carry the text across the decoder's flush thresholds from every offset, and segments
with hand-made histories.  Built on the bit writer and the block writers of tests/bgzf_cases.py.

The rule of bgzf_cases.py holds: the generator computes the text of a stream itself, from its own tokens; the stream is
then inflated by zlib.decompress(p, -15), and where the two differ the module raises AssertionError — never a skip.  All
randomness comes from seeded numpy generators: stream i of a corpus is a function of (SEED, corpus, i) alone."""
import functools
import struct
import zlib
from collections import namedtuple

import numpy as np

import bgzf_cases as B
import gzip_cases as G

SEED = 1951
N_MEMBERS, N_STREAMS = 400, 40
BIG_EVERY, BIG_TEXT, SMALL_TEXT = 20, 65536, 3000  # one member in twenty may hold up to 64 KiB of text
BIASES = (0.0, 0.5, 0.95)                           # how often a code's deepest leaf is the one that is split
STORED_LENGTHS = (0, 1, 5, 8191, 8192, 8193, 20000, 65535)
STREAM_TEXT = (1, 2000, 50001, 70000, 140000, 260000)

# name: where the stream comes from; seed: what its generator was seeded with (None: deterministic); info: what the
# coverage assertions of test_deflate_gen_cpu.py count (new_info())
Stream = namedtuple("Stream", "name payload text seed info")


def new_info():
    return dict(lit_bits=set(), dist_bits=set(), cl_bits=set(), hlit=set(), hdist=set(), n_cl=set(), repeats=set(), crossing=0, len_syms=set(),
                dist_syms=set(), kinds=set(), empty=set(), stored=set(), blocks=0)


def merge_info(infos):
    out = new_info()
    for i in infos:
        for k, v in i.items():
            out[k] = out[k] | v if isinstance(v, set) else out[k] + v
    return out


# ---- random complete prefix codes ------------------------------------------------------------------------------------
def random_depths(rng, n, max_len, bias):
    """The depths of the n >= 2 leaves of a random binary tree no deeper than max_len, in random order: two leaves of depth
    1, then a leaf of depth < max_len is split until there are n — the deepest such leaf with probability `bias`, any of
    them otherwise.  The code is complete by construction; bias 1 would give 1, 2, ..., n - 1, n - 1."""
    assert 2 <= n <= 1 << max_len
    cnt = [0] * (max_len + 2)
    cnt[1] = 2
    for _ in range(n - 2):
        elig = [d for d in range(1, max_len) if cnt[d]]
        d = elig[-1]
        if rng.random() >= bias:
            r = int(rng.integers(0, sum(cnt[e] for e in elig)))
            for d in elig:
                r -= cnt[d]
                if r < 0:
                    break
        cnt[d] -= 1
        cnt[d + 1] += 2
    depths = [d for d in range(1, max_len + 1) for _ in range(cnt[d])]
    assert len(depths) == n and sum(1 << (max_len - d) for d in depths) == 1 << max_len
    return [depths[i] for i in rng.permutation(n)]


def random_lengths(rng, used, size_min, size_max, max_len, bias, single_ok):
    """Code lengths over an alphabet whose size is drawn between the largest used symbol + 1 (at least size_min) and
    size_max — a third of the time each end, else anything between: a complete random code over the used symbols (and
    now and then a few that stay unused).  One used symbol: the single code of length 1 where `single_ok`, else a second
    symbol joins it.  None: no code at all."""
    used = sorted(used)
    lo = max(size_min, used[-1] + 1 if used else 0)
    how = int(rng.integers(0, 3))
    size = lo if how == 0 else size_max if how == 1 else int(rng.integers(lo, size_max + 1))
    lens = [0] * size
    if not used:
        return lens
    if len(used) == 1 and single_ok and rng.random() < 0.5:
        lens[used[0]] = 1
        return lens
    extra = int(rng.integers(0, 4)) if rng.random() < 0.3 else 0
    taken = set(used)
    free = [s for s in range(size) if s not in taken]
    extra = min(max(extra, 2 - len(used)), len(free))
    syms = used + [free[i] for i in rng.permutation(len(free))[:extra]]
    if len(syms) < 2:  # (an alphabet of one symbol)
        lens[syms[0]] = 1
        return lens
    for s, d in zip(syms, random_depths(rng, len(syms), max_len, bias)):
        lens[s] = d
    return lens


# ---- random token blocks ---------------------------------------------------------------------------------------------
def token_length(t):
    return 1 if isinstance(t, int) else t[1] if t[0] == "m" else B.LEN_BASE[t[1]] + t[2]


def token_distance(t):
    return t[2] if t[0] == "m" else B.DIST_BASE[t[3]] + t[4]


def apply_tokens(text, tokens):
    """what the tokens stand for, appended to the bytearray `text`: the generator's own inflate"""
    for t in tokens:
        if isinstance(t, int):
            text.append(t)
            continue
        n, d = token_length(t), token_distance(t)
        assert 3 <= n <= 258 and 1 <= d <= min(len(text), 32768)
        at = len(text) - d
        text += text[at:at + n] if d >= n else (text[at:] * (n // d + 1))[:n]


def random_tokens(rng, have, room, n):
    """At most n tokens that hold at most `room` bytes of text behind `have` bytes: literals from a random subset of the
    bytes, matches drawn by length symbol and extra value and by distance symbol and extra value — uniformly over the
    symbols, so that each of the 29 and of the 30 occurs, and with it both spellings of 258 (symbol 285; symbol 284
    with the extra value 31).  A match whose distance exceeds the text so far is redrawn."""
    alphabet = rng.permutation(256)[:int(rng.choice([1, 2, 4, 20, 100, 256]))]
    p_match = float(rng.choice([0.0, 0.05, 0.5, 0.9, 1.0]))
    short = rng.random() < 0.4  # lengths 3 .. 10 only: many matches in little text
    is_match = rng.random(n) < p_match
    lits = alphabet[rng.integers(0, len(alphabet), n)]
    ls_all = rng.integers(0, 8 if short else 29, n)
    u = rng.random((n, 3))
    toks, made = [], 0
    for i in range(n):
        if room - made < 1:
            break
        pos = have + made
        if is_match[i] and pos > 0 and room - made >= 3:
            ls = int(ls_all[i])
            while B.LEN_BASE[ls] > room - made:
                ls -= 1
            le = min(int(u[i, 0] * (1 << B.LEN_EXTRA[ls])), room - made - B.LEN_BASE[ls])
            if u[i, 0] > 0.9:  # the largest extra value of the symbol
                le = min((1 << B.LEN_EXTRA[ls]) - 1, room - made - B.LEN_BASE[ls])
            top = max(s for s in range(30) if B.DIST_BASE[s] <= min(pos, 32768))
            ds, de = int(u[i, 1] * (top + 1)), int(u[i, 2] * (1 << B.DIST_EXTRA[int(u[i, 1] * (top + 1))]))
            while B.DIST_BASE[ds] + de > pos:  # redrawn
                ds = int(rng.integers(0, top + 1))
                de = int(rng.integers(0, 1 << B.DIST_EXTRA[ds]))
            toks.append(("d", ls, le, ds, de))
            made += B.LEN_BASE[ls] + le
        else:
            toks.append(int(lits[i]))
            made += 1
    return toks


def _note_tokens(info, tokens, lit_lens=None, dist_lens=None):
    """the symbols the tokens use and, under a dynamic block's codes, how long the codes are"""
    for t in tokens:
        if not isinstance(t, int):
            info["len_syms"].add((t[1], t[2]) if t[1] >= 27 else t[1])
            info["dist_syms"].add(t[3])
        if lit_lens is not None:
            info["lit_bits"].add(lit_lens[t if isinstance(t, int) else 257 + t[1]])
            if not isinstance(t, int):
                info["dist_bits"].add(dist_lens[t[3]])


def random_dynamic_block(rng, w, last, tokens, bias, info):
    """the tokens as a dynamic block under random codes; counts what it used into `info`"""
    lit_used = {256} | {t if isinstance(t, int) else 257 + t[1] for t in tokens}
    dist_used = {t[3] for t in tokens if not isinstance(t, int)}
    lit_lens = random_lengths(rng, lit_used, 257, 286, 15, bias, True)
    dist_lens = random_lengths(rng, dist_used, 1, 30, 15, bias, True)
    seq = B.rle_lengths(lit_lens + dist_lens, rng if rng.random() < 0.5 else None)
    assert B.expand_lengths(seq) == lit_lens + dist_lens
    cl_lens = random_lengths(rng, {s for s, _, _ in seq}, 19, 19, 7, bias, False)
    B.dynamic_block(w, last, lit_lens, dist_lens, tokens, cl_lens=cl_lens, seq=seq)
    _note_tokens(info, tokens, lit_lens, dist_lens)
    info["hlit"].add(len(lit_lens))
    info["hdist"].add(len(dist_lens))
    info["n_cl"].add(max(max(i for i, s in enumerate(B.CL_ORDER) if cl_lens[s]) + 1, 4))
    info["cl_bits"] |= {cl_lens[s] for s, _, _ in seq}
    at = 0
    for s, ev, _ in seq:
        n = 1 if s < 16 else (3 if s < 18 else 11) + ev
        if s >= 16:
            info["repeats"].add((s, ev))
            info["crossing"] += at < len(lit_lens) < at + n
        at += n


def random_stream(rng, max_text, bias, force_stored=None):
    """One raw DEFLATE stream of 1 to 11 stored, fixed and dynamic blocks, some of them without text, that holds at most
    max_text bytes -> (payload, text, info).  force_stored: a stored block of this length is one of the blocks, on top
    of max_text."""
    n_blocks = int(rng.integers(1, 12))
    forced_at = int(rng.integers(0, n_blocks)) if force_stored is not None else -1
    reserve = force_stored or 0
    max_text += reserve
    w, text, info = B.BitWriter(), bytearray(), new_info()
    for b in range(n_blocks):
        last = b == n_blocks - 1
        if b == forced_at:
            reserve = 0
        room = max_text - len(text) - reserve
        kind = 0 if b == forced_at else int(rng.integers(0, 3))
        empty = rng.random() < 0.12
        info["blocks"] += 1
        if kind == 0:
            fit = [n for n in STORED_LENGTHS if n <= room]
            n = force_stored if b == forced_at else 0 if empty else fit[int(rng.integers(0, len(fit)))]
            data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
            B.stored_block(w, last, data)
            text += data
            info["stored"].add(n)
            info["kinds"].add("stored")
            if n == 0:
                info["empty"].add("stored")
            continue
        budget = 0 if empty else min(room, int(rng.integers(1, max(2, 3 * max_text // n_blocks))))
        tokens = random_tokens(rng, len(text), budget, min(budget, 30000)) if budget else []
        apply_tokens(text, tokens)
        if not tokens:
            info["empty"].add("fixed" if kind == 1 else "dynamic")
        if kind == 1:
            B.fixed_block(w, last, tokens)
            info["kinds"].add("fixed")
            _note_tokens(info, tokens)
        else:
            random_dynamic_block(rng, w, last, tokens, bias, info)
            info["kinds"].add("dynamic")
    assert len(text) <= max_text
    return w.done(), bytes(text), info


def _confirmed(name, payload, text, seed=None, info=None):
    got = zlib.decompress(payload, -15)
    assert got == text, "%s (seed %s): zlib inflates %d bytes, the generator computed %d — or other bytes" % (name, seed, len(got), len(text))
    return Stream(name, payload, text, seed, info or new_info())


@functools.lru_cache(maxsize=None)
def members():
    """the N_MEMBERS random members: raw DEFLATE streams of at most 65536 bytes of text"""
    out = []
    for i in range(N_MEMBERS):
        seed = (SEED, 1, i)
        rng = np.random.default_rng(seed)
        cap = BIG_TEXT if i % BIG_EVERY == BIG_EVERY - 1 else SMALL_TEXT
        max_text = cap if rng.random() < 0.3 else int(rng.integers(1, cap + 1))
        payload, text, info = random_stream(rng, max_text, BIASES[i % 3])
        out.append(_confirmed("member%d" % i, payload, text, seed, info))
    return out


def gzip_wrap(raw, text):
    return b"\x1f\x8b\x08\0\0\0\0\0\0\x03" + raw + struct.pack("<II", zlib.crc32(text), len(text) & 0xffffffff)


@functools.lru_cache(maxsize=None)
def gzip_streams():
    """the N_STREAMS random multi-block streams of any length, each wrapped as one gzip member (Stream.payload: the file)"""
    out = []
    for i in range(N_STREAMS):
        seed = (SEED, 2, i)
        rng = np.random.default_rng(seed)
        raw, text, info = random_stream(rng, STREAM_TEXT[i % len(STREAM_TEXT)], BIASES[i % 3], force_stored=STORED_LENGTHS[i % len(STORED_LENGTHS)])
        s = _confirmed("stream%d" % i, raw, text, seed, info)
        out.append(s._replace(payload=gzip_wrap(raw, text)))
    return out


# ---- the match sweep -------------------------------------------------------------------------------------------------
SWEEP_DISTANCES = list(range(1, 131)) + [255, 256, 257, 258, 259, 4095, 4096, 16383, 16384, 32767, 32768]
SWEEP_LENGTHS = list(range(3, 71)) + list(range(127, 132)) + list(range(191, 195)) + list(range(255, 259))


@functools.lru_cache(maxsize=None)
def match_sweep():
    """Every distance of SWEEP_DISTANCES with every length of SWEEP_LENGTHS (258 in both spellings), a random literal between
    two matches, in members of at most 65536 bytes: a stored block of random bytes as long as the member's longest
    distance, then one fixed block.  -> (members, the set of (distance, length) pairs they hold)"""
    rng = np.random.default_rng((SEED, 3))
    per_distance = sum(SWEEP_LENGTHS) + 258 + len(SWEEP_LENGTHS) + 1
    groups, cur = [], []
    for d in SWEEP_DISTANCES:  # (ascending: the last distance of a group is its longest)
        if cur and d + (len(cur) + 1) * per_distance > 65536:
            groups.append(cur)
            cur = []
        cur.append(d)
    groups.append(cur)
    out, pairs = [], set()
    for k, group in enumerate(groups):
        head = rng.integers(0, 256, group[-1], dtype=np.uint8).tobytes()
        tokens = []
        for d in group:
            for n in SWEEP_LENGTHS:
                tokens += [B.match_symbols(n, d), int(rng.integers(0, 256))]
                pairs.add((d, n))
            tokens += [B.match_symbols(258, d, long_258=True), int(rng.integers(0, 256))]
        w, text = B.BitWriter(), bytearray(head)
        B.stored_block(w, False, head)
        B.fixed_block(w, True, tokens)
        apply_tokens(text, tokens)
        assert len(text) <= 65536
        out.append(_confirmed("sweep%d(distances %d..%d)" % (k, group[0], group[-1]), w.done(), bytes(text), (SEED, 3)))
    return out, pairs


# ---- members that cross the decoder's thresholds ---------------------------------------------------------------------
THRESHOLDS = (16384, 32768, 49152)  # the first flush (INF_FLUSH), the ring's wrap, the second flush behind the wrap
BELOW = (1, 2, 3, 257)
STEPS = ("literal", "match258", "stored_piece", "stored8193")


def _reads_across(p, q, n, d):
    """a match of n bytes at text position q with distance d has its source on both sides of p, or (its source ends where p
    begins) reads the last byte in front of p for the first byte behind it"""
    return q - d < p < q - d + n or (q == p and d <= n)


@functools.lru_cache(maxsize=None)
def threshold_members():
    """For every threshold p, every producing step and every offset of BELOW: a member whose step begins that many bytes
    below p and carries the text across it (literal: literals up to p exactly; match258: one match of 258 bytes, at
    distance 1 or 200; stored_piece: the second 8192-byte piece of a stored block begins there; stored8193: a stored
    block of 8193 bytes).  Behind the step the text reads back across p: where the step ends at p, a match at distance 1
    whose source is the last byte in front of p; where it ends less than 64 bytes behind p, a match at distance 64 whose
    source lies on both sides of p; and, behind stored filler, a match at distance 16384 and one at 32768 whose sources
    lie on both sides of p, where 65536 bytes of text have room for them.
    -> [(member, the set of distances that read across p)]"""
    rng = np.random.default_rng((SEED, 4))
    out = []
    for p in THRESHOLDS:
        for step in STEPS:
            for k in BELOW:
                start = p - k - (8192 if step == "stored_piece" else 0)
                head = rng.integers(0, 256, start, dtype=np.uint8).tobytes()
                w, text, across = B.BitWriter(), bytearray(head), set()
                B.stored_block(w, False, head)

                def fixed(tokens, last=False):
                    for t in tokens:
                        if not isinstance(t, int) and _reads_across(p, len(text), t[1], t[2]):
                            across.add(t[2])
                        apply_tokens(text, [t])
                    B.fixed_block(w, last, tokens)

                if step == "literal":
                    fixed([int(x) for x in rng.integers(0, 256, k)])
                elif step == "match258":
                    fixed([("m", 258, 1 if k in (2, 257) else 200)])
                else:
                    data = rng.integers(0, 256, 8193 if step == "stored8193" else 8192 + 300, dtype=np.uint8).tobytes()
                    B.stored_block(w, False, data)
                    text += data
                assert len(text) >= p
                near = [("m", 10, 1)] if len(text) == p else []
                if len(text) + 10 < p + 64:
                    near.append(("m", 100, 64))
                fixed(near + [int(x) for x in rng.integers(0, 256, 70)] + [("m", 10, 1), ("m", 100, 64), ("m", 3, 64)])
                for d in (16384, 32768):
                    q = p + d - 129
                    if q >= len(text) and q + 258 + 400 <= 65536:
                        data = rng.integers(0, 256, q - len(text), dtype=np.uint8).tobytes()
                        B.stored_block(w, False, data)
                        text += data
                        fixed([("m", 258, d)] + [int(x) for x in rng.integers(0, 256, 30)])
                fixed([int(x) for x in rng.integers(0, 256, 300)], last=True)
                assert p < len(text) <= 65536
                out.append((_confirmed("threshold %d, %s from %d below" % (p, step, k), w.done(), bytes(text), (SEED, 4)), frozenset(across)))
    return out


# ---- hand-made segments ----------------------------------------------------------------------------------------------
HISTORY_LENGTHS = (0, 1, 2, 3, 5, 32767, 32768)


def _segment(rng, phase, hist_len, first_distance, final, too_far=0):
    """-> (file, segment as gzip_index gives it, its text by zlib): blocks without text up to bit `phase` modulo 8, then the
    segment: a fixed block whose first token is a match at first_distance (none: a literal), a stored block — padded to a
    byte of the FILE — and a dynamic block under a random code.  too_far: the first match is WRITTEN that much farther back"""
    history = rng.integers(0, 256, hist_len, dtype=np.uint8).tobytes()
    pv, pn = G._empty_blocks()[phase]
    w = B.BitWriter()
    for at in range(0, pn, 16):
        w.bits(pv >> at, min(16, pn - at))
    comp_bit = pn
    text = bytearray(history)
    tokens = ([("m", 11, first_distance)] if first_distance else []) + [int(x) for x in rng.integers(65, 91, 40)]
    if len(text) + 11 >= 64:
        tokens += [("m", 70, 64)]
    apply_tokens(text, tokens)
    if too_far:
        tokens[0] = ("m", 11, first_distance + too_far)
    B.fixed_block(w, False, tokens)
    data = rng.integers(0, 256, 37, dtype=np.uint8).tobytes()
    B.stored_block(w, False, data)
    text += data
    tokens = random_tokens(rng, len(text), 500, 200)
    apply_tokens(text, tokens)
    random_dynamic_block(rng, w, final, tokens, 0.5, new_info())
    n_bits = 8 * len(w.out) + w.n - comp_bit
    f = w.done() + b"\0" * 8
    own = bytes(text[hist_len:])
    g = dict(comp_bit=comp_bit, n_bits=n_bits, dict=history, text_len=len(own), crc32=zlib.crc32(own), flags=1 if final else 0)
    return f, g, own


@functools.lru_cache(maxsize=None)
def hand_segments():
    """[(name, file, segment, text)]: histories of HISTORY_LENGTHS bytes, each at every bit phase 0 .. 7; the first token is a
    match that reaches exactly the first byte of the history.  The text is zlib's (gzip_cases.inflate_segment) and must
    be the generator's own."""
    rng = np.random.default_rng((SEED, 5))
    out = []
    for n in HISTORY_LENGTHS:
        for phase in range(8):
            f, g, own = _segment(rng, phase, n, n, final=(phase + n) % 2 == 1)
            text, eof = G.inflate_segment(f, g["comp_bit"], g["n_bits"], g["dict"])
            assert text == own and eof == bool(g["flags"]) and g["comp_bit"] % 8 == phase, (n, phase)
            out.append(("history %d, bit phase %d" % (n, phase), f, g, text))
    return out


@functools.lru_cache(maxsize=None)
def refused_segments():
    """name -> (file, segment, the reason zlib names): segments whose first match reaches one byte in front of the history"""
    out = {}
    rng = np.random.default_rng((SEED, 6))
    for n, phase in ((5, 3), (32767, 6)):
        f, g, _ = _segment(rng, phase, n, n, final=False, too_far=1)
        try:
            G.inflate_segment(f, g["comp_bit"], g["n_bits"], g["dict"])
        except zlib.error as e:
            out["first_match_in_front_of_a_history_of_%d" % n] = (f, g, str(e).split(": ", 1)[1])
        else:
            raise AssertionError("zlib accepts a segment whose first match reaches in front of its history")
    return out
