"""Raw DEFLATE streams and BGZF files for the tests of the device inflate (tests/test_gpu_bgzf.py, test_gpu_cli_bgzf.py,
test_bgzf_cpu.py).  The expectation is Python's zlib everywhere: a good stream is inflated with zlib.decompress(payload, -15)
first and THAT text (with its zlib.crc32) is what the device must return; a stream meant to be bad must raise zlib.error
there.  A crafted stream that zlib does not confirm either way is an error of the test (AssertionError), never a skip."""
import functools
import struct
import zlib

import numpy as np


# ---- a bit writer for the streams zlib cannot produce (RFC 1951: data elements LSB first, Huffman codes MSB first) ----
class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, value, n):
        self.acc |= (value & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, n):
        """a Huffman code: its first bit first"""
        if n:
            self.bits(int(format(code & ((1 << n) - 1), "0%db" % n)[::-1], 2), n)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def done(self):
        self.align()
        return bytes(self.out)


def canonical(lengths):
    """{symbol: (code, length)} of the canonical Huffman code with these lengths (0: no code)"""
    codes, code = {}, 0
    for l in range(1, 16):
        for s, sl in enumerate(lengths):
            if sl == l:
                codes[s] = (code, l)
                code += 1
        code <<= 1
    return codes


def complete_lengths(symbols, size):
    """lengths of a complete prefix code over `symbols` (at least two) in an alphabet of `size` symbols"""
    u = len(symbols)
    assert u >= 2
    L = (u - 1).bit_length()
    x = (1 << L) - u  # codes of length L - 1
    lens = [0] * size
    for i, s in enumerate(sorted(symbols)):
        lens[s] = L - 1 if i < x else L
    return lens


LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def rle_lengths(lens, rng=None):
    """the code length symbols [(symbol, extra value, extra bits)] of a sequence of code lengths, repeats taken greedily
    over the WHOLE sequence — a run that spans the literal/length and the distance lengths becomes one repeat.  With a
    numpy generator `rng` every repeat is as long as it may be, of a random length, or written out as plain lengths
    (a third each): the forms an encoder may choose among."""
    def pick(lo, hi):  # the length of one repeat out of lo .. hi; 0: none, one plain length instead
        if rng is None:
            return hi
        how = int(rng.integers(0, 3))
        return hi if how == 0 else int(rng.integers(lo, hi + 1)) if how == 1 else 0

    out, i = [], 0
    while i < len(lens):
        v, r = lens[i], 1
        while i + r < len(lens) and lens[i + r] == v:
            r += 1
        i += r
        if v == 0:
            while r >= 3:
                if r >= 11 and (rng is None or rng.integers(0, 4)):
                    k = pick(11, min(r, 138))
                    sym = (18, k - 11, 7)
                else:
                    k = pick(3, min(r, 10))
                    sym = (17, k - 3, 3)
                if k == 0:
                    out.append((0, 0, 0))
                    r -= 1
                else:
                    out.append(sym)
                    r -= k
            out += [(0, 0, 0)] * r
        else:
            out.append((v, 0, 0))
            r -= 1
            while r >= 3:
                k = pick(3, min(r, 6))
                if k == 0:
                    out.append((v, 0, 0))
                    r -= 1
                else:
                    out.append((16, k - 3, 2))
                    r -= k
            out += [(v, 0, 0)] * r
    return out


def expand_lengths(seq):
    """the code lengths that the code length symbols of rle_lengths stand for"""
    lens = []
    for s, ev, _ in seq:
        lens += [s] if s < 16 else [lens[-1]] * (3 + ev) if s == 16 else [0] * ((3 if s == 17 else 11) + ev)
    return lens


def match_symbols(length, dist, long_258=False):
    """("d", length symbol, length extra value, distance symbol, distance extra value) of a match; long_258: a length of 258
    as symbol 284 with the extra value 31, the spelling no compressor chooses"""
    ls = 28 if length == 258 and not long_258 else max(i for i in range(28) if LEN_BASE[i] <= length)
    ds = max(i for i in range(30) if DIST_BASE[i] <= dist)
    return ("d", ls, length - LEN_BASE[ls], ds, dist - DIST_BASE[ds])


def stored_block(w, last, data):
    w.bits(1 if last else 0, 1)
    w.bits(0, 2)
    w.align()
    w.bits(len(data), 16)
    w.bits(len(data) ^ 0xffff, 16)
    w.out += data


def fixed_block(w, last, symbols, eob=True):
    """One fixed-Huffman block of the symbols of dynamic_block"""
    w.bits(1 if last else 0, 1)
    w.bits(1, 2)
    for sym in list(symbols) + ([256] if eob else []):
        if isinstance(sym, int):
            fixed_code(w, sym)
            continue
        if sym[0] == "m":
            sym = match_symbols(sym[1], sym[2])
        _, ls, le, ds, de = sym
        fixed_code(w, 257 + ls)
        w.bits(le, LEN_EXTRA[ls])
        w.code(ds, 5)
        w.bits(de, DIST_EXTRA[ds])


def dynamic_block(w, last, lit_lens, dist_lens, symbols, cl_lens=None, seq=None, eob=True):
    """One dynamic-Huffman block.  symbols: ints (literals), ("m", length, distance) or ("d", length symbol, length extra
    value, distance symbol, distance extra value); the end-of-block symbol is appended (eob).  cl_lens: the code length
    code's lengths (default: a complete code over the symbols used); seq: the code length symbols, where they are not
    rle_lengths' (another choice of repeats, or a sequence that is not valid)."""
    if seq is None:
        seq = rle_lengths(list(lit_lens) + list(dist_lens))
    if cl_lens is None:
        used = {s for s, _, _ in seq}
        if len(used) < 2:
            used.add(0 if 0 not in used else 1)
        cl_lens = complete_lengths(used, 19)
    n_cl = max(i for i, s in enumerate(CL_ORDER) if cl_lens[s]) + 1
    n_cl = max(n_cl, 4)
    w.bits(1 if last else 0, 1)
    w.bits(2, 2)
    w.bits(len(lit_lens) - 257, 5)
    w.bits(len(dist_lens) - 1, 5)
    w.bits(n_cl - 4, 4)
    for s in CL_ORDER[:n_cl]:
        w.bits(cl_lens[s], 3)
    clc = canonical(cl_lens)
    for s, ev, eb in seq:
        w.code(*clc[s])
        w.bits(ev, eb)
    lc, dc = canonical(lit_lens), canonical(dist_lens)
    for sym in list(symbols) + ([256] if eob else []):
        if isinstance(sym, int):
            w.code(*lc[sym])
            continue
        if sym[0] == "m":
            sym = match_symbols(sym[1], sym[2])
        _, ls, le, ds, de = sym
        w.code(*lc[257 + ls])
        w.bits(le, LEN_EXTRA[ls])
        w.code(*dc[ds])
        w.bits(de, DIST_EXTRA[ds] if ds < 30 else 0)


def fixed_code(w, sym):
    if sym < 144:
        w.code(0x30 + sym, 8)
    elif sym < 256:
        w.code(0x190 + sym - 144, 9)
    elif sym < 280:
        w.code(sym - 256, 7)
    else:
        w.code(0xC0 + sym - 280, 8)


def deflate(text, level=6, mem_level=8, strategy=zlib.Z_DEFAULT_STRATEGY, flushes=()):
    """raw DEFLATE of `text`; flushes: [(offset, zlib flush mode)] — the member is written in pieces"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem_level, strategy)
    out, at = b"", 0
    for off, mode in flushes:
        out += c.compress(text[at:off]) + c.flush(mode)
        at = off
    return out + c.compress(text[at:]) + c.flush()


def confirm_good(payload):
    text = zlib.decompress(payload, -15)
    return text, zlib.crc32(text)


def confirm_bad(payload, text_len=None, trailing=None):
    """zlib must refuse the stream (or, with text_len, inflate it to another length; or, with trailing, leave exactly these
    bytes behind the stream's end as unused_data).  -> the reason zlib names (the text of its zlib.error), or None"""
    d = zlib.decompressobj(-15)
    try:
        text = d.decompress(payload)
    except zlib.error as e:
        assert trailing is None, "zlib refuses a stream that was meant to be good up to its trailing bytes"
        return str(e).split(": ", 1)[1]
    if trailing is not None:
        assert d.eof and d.unused_data == trailing and len(trailing) > 0, "zlib does not leave the trailing bytes unused"
        return None
    assert not d.eof or (text_len is not None and len(text) != text_len), "zlib accepts a stream that was meant to be bad"
    return None


def texts():
    """name -> text of one member (every one at most 65536 bytes)"""
    from helpers import random_reads

    rng = np.random.default_rng(7)
    reads = random_reads(40, 500, 3000, 11)
    fq = b"".join(b"@read%d some comment\n%s\n+\n%s\n" % (i, r, bytes(rng.integers(35, 75, len(r), dtype=np.uint8))) for i, r in enumerate(reads))
    t = {"fastq": fq[:65280], "bytes": bytes(rng.integers(0, 256, 50001, dtype=np.uint8)), "run_of_A": b"A" * 60000,
         "period3": b"ACG" * 20001, "period258": bytes(rng.integers(65, 85, 258, dtype=np.uint8)) * 200}
    head = bytes(rng.integers(0, 256, 32768, dtype=np.uint8))
    t["longest_distance"] = head + head[:300]
    for n in (0, 1, 2, 257, 258, 259, 32768, 32769, 65280, 65535, 65536):
        t["len%d" % n] = (fq * 2)[:n]
    return t


FORMS = {
    "level0": dict(level=0), "level1": dict(level=1), "level6": dict(level=6), "level9": dict(level=9),
    "fixed": dict(strategy=zlib.Z_FIXED), "huffman_only": dict(strategy=zlib.Z_HUFFMAN_ONLY), "rle": dict(strategy=zlib.Z_RLE),
}


def flushed(text):
    """written in pieces: several blocks per member, empty stored blocks at odd bit positions"""
    n = len(text)
    offs = sorted({n // 7, n // 3, n // 3 + 1, n // 2, (4 * n) // 5})
    return deflate(text, 6, flushes=[(o, zlib.Z_SYNC_FLUSH if i % 2 == 0 else zlib.Z_FULL_FLUSH) for i, o in enumerate(offs)])


def hand_written():
    """name -> payload of the dynamic blocks zlib never writes (all good streams)"""
    out = {}
    # one distance code of length 1 (an incomplete distance code: libdeflate writes these)
    lit = complete_lengths([97, 98, 256, 257, 258], 259)
    w = BitWriter()
    dynamic_block(w, True, lit, [1], [97, 98, ("m", 3, 1), 97, ("m", 4, 1)])
    out["one_distance_code"] = w.done()
    # no distance code at all, literals only
    w = BitWriter()
    dynamic_block(w, True, complete_lengths([120, 121, 122, 256], 257), [0], [120, 121, 122, 122, 121] * 9)
    out["no_distance_code"] = w.done()
    # a zero run (code 18) from the literal/length lengths into the distance lengths
    w = BitWriter()
    dynamic_block(w, True, complete_lengths([65, 67, 71, 84, 256, 257], 286), [0] * 10 + [1, 1], [65, 67, 71, 84] * 30 + [("m", 3, 40), 65, ("m", 3, 50)])
    out["repeat18_across"] = w.done()
    # a short zero run (code 17) across
    w = BitWriter()
    dynamic_block(w, True, complete_lengths([65, 66, 256, 257], 260), [0, 0, 1, 1], [65, 66, 65, 65, ("m", 3, 3), 66, ("m", 3, 4)])
    out["repeat17_across"] = w.done()
    # the previous length repeated (code 16) across: ... 2 2 | 2 2 2 2
    lit = [0] * 259
    lit[97], lit[256], lit[98], lit[257], lit[258] = 2, 3, 3, 2, 2
    w = BitWriter()
    dynamic_block(w, True, lit, [2, 2, 2, 2], [97, 98, 97, 97, ("m", 3, 2), ("m", 4, 4), 98, ("m", 3, 1)])
    out["repeat16_across"] = w.done()
    # the fewest code length code lengths a good block can have, 5 (16 17 18 0 8): 256 codes of length 8, zeros, no more
    w = BitWriter()
    dynamic_block(w, True, [8] * 255 + [0, 8], [0], list(range(255)) + [7, 7, 200])
    out["five_code_length_lengths"] = w.done()
    assert (int.from_bytes(out["five_code_length_lengths"][:3], "little") >> 13) & 15 == 1
    return out


def refused():
    """name -> (payload, text_len, crc32): inputs a checking decoder turns down; zlib turns each of them down too.  Every
    one has exactly one defect, so that the order of a decoder's checks cannot change the reason it gives."""
    return dict(_refused()[0])


def refused_reasons():
    """name -> the reason zlib names for refused()[name] (the text of its zlib.error), None where zlib has no word for
    it: a stream that is good by itself and holds another amount of text, ends early, or has bytes behind its end"""
    return dict(_refused()[1])


@functools.lru_cache(maxsize=None)
def _refused():
    good = deflate(texts()["fastq"][:20000], 6)
    text, crc = confirm_good(good)
    out = {"wrong_crc": (good, len(text), crc ^ 0x10), "text_len_plus_1": (good, len(text) + 1, crc), "text_len_minus_1": (good, len(text) - 1, crc),
           "cut_by_5": (good[:-5], len(text), crc)}
    assert zlib.crc32(text) != crc ^ 0x10
    reasons = {"wrong_crc": None, "text_len_plus_1": confirm_bad(good, len(text) + 1), "text_len_minus_1": confirm_bad(good, len(text) - 1),
               "cut_by_5": confirm_bad(good[:-5])}
    crafted = {}
    w = BitWriter()
    w.bits(1, 1)
    w.bits(3, 2)
    crafted["block_type_3"] = w.done() + b"\0\0\0\0"
    w = BitWriter()
    w.bits(1, 1)
    w.bits(0, 2)
    w.align()
    crafted["stored_len_mismatch"] = w.done() + struct.pack("<HH", 5, 0xFFFA ^ 1) + b"hello"
    # an over-subscribed code length code: three codes of length 1
    w = BitWriter()
    w.bits(1, 1)
    w.bits(2, 2)
    w.bits(0, 5)
    w.bits(0, 5)
    w.bits(0, 4)
    for l in (1, 1, 1, 0):
        w.bits(l, 3)
    w.bits(0, 32)
    crafted["oversubscribed_code_lengths"] = w.done()
    # an incomplete literal/length code: two codes of length 2 and nothing else
    lit = [0] * 257
    lit[97], lit[256] = 2, 2
    w = BitWriter()
    dynamic_block(w, True, lit, [0], [97, 97, 97])
    crafted["incomplete_literal_set"] = w.done()
    # fixed Huffman: a match as the first symbol — its distance lies in front of the member
    w = BitWriter()
    w.bits(1, 1)
    w.bits(1, 2)
    fixed_code(w, 257)
    w.code(0, 5)
    fixed_code(w, 256)
    crafted["match_at_position_0"] = w.done()
    # fixed Huffman: distance symbol 30 has a code but no meaning
    w = BitWriter()
    w.bits(1, 1)
    w.bits(1, 2)
    for ch in b"abcd":
        fixed_code(w, ch)
    fixed_code(w, 257)
    w.code(30, 5)
    fixed_code(w, 256)
    crafted["distance_symbol_30"] = w.done()
    # HLIT = 287 and HDIST = 31, one more symbol than the alphabets have (the block is well-formed apart from that), and
    # HDIST = 32, the largest the 5-bit field can say
    w = BitWriter()
    dynamic_block(w, True, complete_lengths([97, 98, 256, 257], 287), [1], [97, 98, ("m", 3, 1)])
    crafted["hlit_287"] = w.done()
    for n_dist in (31, 32):
        w = BitWriter()
        dynamic_block(w, True, complete_lengths([97, 98, 256, 257], 258), [1] + [0] * (n_dist - 1), [97, 98, ("m", 3, 1)])
        crafted["hdist_%d" % n_dist] = w.done()
        assert (int.from_bytes(crafted["hdist_%d" % n_dist][:2], "little") >> 3) & 1023 == 1 | (n_dist - 1) << 5  # HLIT 258
    assert (int.from_bytes(crafted["hlit_287"][:2], "little") >> 3) & 1023 == 30 | 0 << 5
    # The first code length symbol repeats a previous length that does not exist.  The three lengths it stands for are
    # those of the symbols 0, 1 and 2, which are zero: the sequence holds exactly HLIT + HDIST lengths, and a decoder
    # that took a zero from in front of its table would find a good block
    lit = complete_lengths([97, 98, 99, 256], 257)
    assert lit[:3] == [0, 0, 0] and 3 + len(expand_lengths(rle_lengths(lit[3:] + [0]))) == 258
    w = BitWriter()
    dynamic_block(w, True, lit, [0], [97, 98, 99], seq=[(16, 0, 2)] + rle_lengths(lit[3:] + [0]))
    crafted["repeat16_first"] = w.done()
    # a repeat that runs past the HLIT + HDIST lengths, by each of the three repeat symbols
    lit = complete_lengths(list(range(97, 104)) + [256], 257)
    for sym, dist, tail in ((16, [2, 2, 2, 2], [(2, 0, 0), (16, 3, 2)]), (17, [1, 1, 0, 0, 0], [(1, 0, 0), (1, 0, 0), (17, 7, 3)]),
                            (18, [1, 1, 0, 0, 0], [(1, 0, 0), (1, 0, 0), (18, 0, 7)])):
        assert len(expand_lengths(rle_lengths(lit) + tail)) > len(lit) + len(dist)
        w = BitWriter()
        dynamic_block(w, True, lit, dist, [97, 98, 99], seq=rle_lengths(lit) + tail)
        crafted["repeat%d_past_the_end" % sym] = w.done()
    # a complete literal/length code without the end-of-block symbol
    lit = [0] * 257
    lit[97], lit[98] = 1, 1
    w = BitWriter()
    dynamic_block(w, True, lit, [0], [97, 98, 97, 97], eob=False)
    crafted["no_end_of_block_code"] = w.done()
    # ... and no code at all: 258 zero lengths by two repeats, a code length code of 0 and 18 alone.  The only way to the
    # smallest number of code length code lengths, 4: a valid block gives symbol 256 a length, and the lengths 1 .. 15
    # come from the fifth on
    w = BitWriter()
    dynamic_block(w, True, [0] * 257, [0], [], seq=[(18, 127, 7), (18, 109, 7)], cl_lens=[1] + [0] * 17 + [1], eob=False)
    crafted["no_code_at_all"] = w.done()
    # distance codes: three of length 1 (over-subscribed), two of length 2 (incomplete, and not the one code zlib accepts)
    lit = complete_lengths([97, 98, 256, 257], 258)
    for name, dist in (("oversubscribed_distance_set", [1, 1, 1]), ("incomplete_distance_set", [2, 2])):
        w = BitWriter()
        dynamic_block(w, True, lit, dist, [97, 98, 97])
        crafted[name] = w.done()
    # one literal/length code of length 1 that is not the end-of-block symbol (zlib looks for symbol 256 first)
    lit = [0] * 257
    lit[97] = 1
    w = BitWriter()
    dynamic_block(w, True, lit, [0], [97, 97, 97], eob=False)
    crafted["single_literal_code"] = w.done()
    # fixed Huffman: the literal/length symbols 286 and 287 have codes but no meaning
    for sym in (286, 287):
        w = BitWriter()
        fixed_block(w, True, [97, 98, 99, 100], eob=False)
        fixed_code(w, sym)
        w.code(0, 5)
        fixed_code(w, 256)
        crafted["fixed_symbol_%d" % sym] = w.done()
    # one distance code of length 1 (a good set), and a match whose distance bit is the other one
    lit = complete_lengths([97, 98, 99, 256, 257], 258)
    w = BitWriter()
    dynamic_block(w, True, lit, [1], [97, 98, 99], eob=False)
    w.code(*canonical(lit)[257])
    w.bits(1, 1)
    w.code(*canonical(lit)[256])
    crafted["single_distance_code_other_bit"] = w.done()
    for name, p in crafted.items():
        reasons[name] = confirm_bad(p)
        assert reasons[name], name
        out[name] = (p, 3 if name == "match_at_position_0" else 7 if name == "distance_symbol_30" else 5, 0)
    # a good member with bytes behind its end inside comp_len
    for tail in (b"\0", b"\1\2\3\4"):
        name = "trailing_%d_byte%s" % (len(tail), "s" if len(tail) > 1 else "")
        reasons[name] = confirm_bad(good + tail, trailing=tail)
        out[name] = (good + tail, len(text), crc)
    # good streams whose last step goes one byte beyond text_len: a stored block, a match (text_len_minus_1: a literal)
    w = BitWriter()
    fixed_block(w, False, list(b"abc"))
    stored_block(w, True, b"ACGTACGTAC")
    w2 = BitWriter()
    fixed_block(w2, True, list(b"abcdef") + [("m", 7, 5)])
    for name, p in (("stored_block_beyond_text_len", w.done()), ("match_beyond_text_len", w2.done())):
        t = confirm_good(p)[0]
        assert len(t) == 13
        reasons[name] = confirm_bad(p, len(t) - 1)
        out[name] = (p, len(t) - 1, zlib.crc32(t[:-1]))
    return out, reasons


# ---- BGZF files ---------------------------------------------------------------
def bgzf_member(text, level=6, extra=b"", payload=None):
    """one BGZF member; extra: subfields in front of the BC subfield"""
    payload = deflate(text, level) if payload is None else payload
    xlen = len(extra) + 6
    bsize = 12 + xlen + len(payload) + 8 - 1
    assert bsize < 65536 and len(text) <= 65536
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", xlen) + extra + b"BC" + struct.pack("<HH", 2, bsize) + payload +
            struct.pack("<II", zlib.crc32(text), len(text)))


BGZF_EOF = bgzf_member(b"")
assert len(BGZF_EOF) == 28


def bgzf_file(text, sizes, level=1, eof=True):
    """text cut into members of the given text sizes (cycled)"""
    out, at, i = [], 0, 0
    while at < len(text):
        n = sizes[i % len(sizes)]
        out.append(bgzf_member(text[at:at + n], level))
        at += n
        i += 1
    return b"".join(out) + (BGZF_EOF if eof else b"")


def walk_members(buf):
    """the members of a BGZF byte string as (payload offset, payload length, ISIZE, CRC32), by the format's definition;
    stops like gr_bgzf_scan: -> (blocks, consumed, why)"""
    blocks, pos = [], 0
    while True:
        if pos == len(buf):
            return blocks, pos, 1
        head = buf[pos:pos + 12]
        want = b"\x1f\x8b\x08\x04"
        if head[:4] != want[:len(head[:4])]:
            return blocks, pos, 2
        if len(head) < 12:
            return blocks, pos, 0
        xlen = struct.unpack_from("<H", head, 10)[0]
        if len(buf) - pos < 12 + xlen:
            return blocks, pos, 0
        bsize, at = None, pos + 12
        while at + 4 <= pos + 12 + xlen:
            slen = struct.unpack_from("<H", buf, at + 2)[0]
            if buf[at:at + 2] == b"BC" and slen == 2 and at + 6 <= pos + 12 + xlen:
                bsize = struct.unpack_from("<H", buf, at + 4)[0]
                break
            at += 4 + slen
        if bsize is None or bsize + 1 < 12 + xlen + 8:
            return blocks, pos, 2
        if len(buf) - pos < bsize + 1:
            return blocks, pos, 0
        crc, isize = struct.unpack_from("<II", buf, pos + bsize + 1 - 8)
        if isize > 65536:
            return blocks, pos, 2
        blocks.append((pos + 12 + xlen, bsize + 1 - 12 - xlen - 8, isize, crc))
        pos += bsize + 1
