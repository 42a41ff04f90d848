"""Plain gzip streams for the tests of the gzip index (csrc/host/gr_gzidx.cpp) and of grp_gzip_inflate (csrc/grp_inflate.inc:
the segment form of the decoder), all built with Python's zlib, and what the tests check them with WITHOUT the code under
test: a walk over the DEFLATE blocks of a member in Python (walk_blocks: every block boundary's bit position and text
offset) and the inflate of one segment by zlib from a copy of its bits with its history as the preset dictionary
(inflate_segment).

  python tests/gzip_cases.py DIR     writes every stream to DIR/<name>.gz (for tools/dev/inflate_host_check.cpp)"""
import gzip
import os
import struct
import sys
import zlib

import bgzf_cases as B

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SPANS = (1, 50000, 10 ** 9)


def member(text, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_every=0, flushes=(zlib.Z_SYNC_FLUSH, zlib.Z_FULL_FLUSH), mem_level=8):
    """one gzip member; flush_every: a flush (alternating `flushes`) behind every so many bytes of text — an empty stored
    block (and, at a full flush, a compressor that forgets its history) at whatever bit the block in front of it ends on"""
    c = zlib.compressobj(level, zlib.DEFLATED, 31, mem_level, strategy)
    out = []
    if flush_every:
        for k, a in enumerate(range(0, len(text), flush_every)):
            out.append(c.compress(text[a:a + flush_every]))
            out.append(c.flush(flushes[k % len(flushes)]))
    else:
        out.append(c.compress(text))
    out.append(c.flush())
    return b"".join(out)


def tiny():
    return open(os.path.join(GOLD, "tiny.fq"), "rb").read()


# ---- a walk over the blocks of a raw DEFLATE stream ------------------------------------------------------------------
class _Bits:
    def __init__(self, buf, bit):
        self.buf, self.bit = buf, bit

    def take(self, n):
        v = 0
        for i in range(n):
            v |= ((self.buf[(self.bit + i) >> 3] >> ((self.bit + i) & 7)) & 1) << i
        self.bit += n
        return v


def _table(lengths):
    """(length, code with its first bit first) -> symbol"""
    return {(l, c): s for s, (c, l) in B.canonical(lengths).items()}


def _symbol(r, table):
    code = 0
    for l in range(1, 16):
        code = code << 1 | r.take(1)
        s = table.get((l, code))
        if s is not None:
            return s
    raise ValueError("no code")


_FIXED = None


def walk_blocks(buf, bit):
    """The blocks of the raw DEFLATE stream that starts at `bit` of buf: [(first bit, bit behind it, text offset at its start,
    text behind it, final)] — by decoding every symbol, in Python."""
    global _FIXED
    if _FIXED is None:
        _FIXED = (_table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), _table([5] * 30))
    r, n, out = _Bits(buf, bit), 0, []
    while True:
        start, n0 = r.bit, n
        last, typ = r.take(1), r.take(2)
        if typ == 0:
            r.bit = (r.bit + 7) & ~7
            ln, nl = r.take(16), r.take(16)
            assert ln ^ 0xffff == nl
            r.bit += 8 * ln
            n += ln
        else:
            assert typ != 3
            if typ == 1:
                lit, dist = _FIXED
            else:
                n_lit, n_dist, n_cl = r.take(5) + 257, r.take(5) + 1, r.take(4) + 4
                cl = [0] * 19
                for i in range(n_cl):
                    cl[B.CL_ORDER[i]] = r.take(3)
                clt, lens = _table(cl), []
                while len(lens) < n_lit + n_dist:
                    s = _symbol(r, clt)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + r.take(2))
                    elif s == 17:
                        lens += [0] * (3 + r.take(3))
                    else:
                        lens += [0] * (11 + r.take(7))
                lit, dist = _table(lens[:n_lit]), _table(lens[n_lit:n_lit + n_dist])
            while True:
                s = _symbol(r, lit)
                if s < 256:
                    n += 1
                elif s == 256:
                    break
                else:
                    n += B.LEN_BASE[s - 257] + r.take(B.LEN_EXTRA[s - 257])
                    r.take(B.DIST_EXTRA[_symbol(r, dist)])
        out.append((start, r.bit, n0, n, bool(last)))
        if last:
            return out


def payload_bit(buf, at=0):
    """the first bit behind the gzip header that starts at byte `at`"""
    assert buf[at:at + 3] == b"\x1f\x8b\x08"
    flg, p = buf[at + 3], at + 10
    if flg & 4:
        p += 2 + struct.unpack_from("<H", buf, p)[0]
    for f in (8, 16):
        if flg & f:
            p = buf.index(b"\0", p) + 1
    if flg & 2:
        p += 2
    return 8 * p


def expected_segments(buf, span, blocks=None):
    """The index a walk over the blocks in Python gives for ONE member at the start of buf (the rules of
    csrc/host/gr_gzidx.hpp): [(comp_bit, n_bits, text offset, text_len, flags)]"""
    blocks = blocks or walk_blocks(buf, payload_bit(buf))
    segs, start_bit, start_text = [], blocks[0][0], 0
    for (b0, b1, t0, t1, final) in blocks:
        if final:
            if t1 > start_text:
                segs.append((start_bit, b1 - start_bit, start_text, t1 - start_text, 1))
            elif segs:
                a = segs[-1]
                segs[-1] = (a[0], b1 - a[0], a[2], a[3], 1)
        elif t1 - start_text >= span:
            segs.append((start_bit, b1 - start_bit, start_text, t1 - start_text, 0))
            start_bit, start_text = b1, t1
    return segs


def _empty_blocks():
    """phase -> (bits, their number) of non-final blocks without text whose number of bits is `phase` modulo 8: an empty fixed
    block has 10 bits, so the odd phases need an empty dynamic block with an odd number of bits"""
    def bits_of(write):
        w = B.BitWriter()
        write(w)
        n = 8 * len(w.out) + w.n
        return int.from_bytes(bytes(w.out), "little") | w.acc << (8 * len(w.out)), n

    def fixed(w):
        w.bits(0, 1)
        w.bits(1, 2)
        B.fixed_code(w, 256)

    odd = None
    for extra in range(1, 40):
        lit = B.complete_lengths(set(range(extra)) | {256}, 257)
        v, n = bits_of(lambda w: B.dynamic_block(w, False, lit, [0], []))
        if n % 2:
            odd = (v, n)
            break
    assert odd
    out = {}
    for phase in range(8):
        parts = ([odd] if phase % 2 else [])
        while sum(n for _, n in parts) % 8 != phase:
            parts.append(bits_of(fixed))
        v = n = 0
        for pv, pn in parts:
            v |= pv << n
            n += pn
        out[phase] = (v, n)
    return out


_EMPTY = None


def inflate_segment(buf, comp_bit, n_bits, history):
    """(the text of the n_bits from comp_bit on, whether they end with a final block), by zlib.  The bits are moved to the
    front of a copy, the history is the preset dictionary.  A stored block is padded to a byte of the FILE, so the copy
    keeps the file's bit phase: blocks without text that zlib itself accepts fill the comp_bit % 8 bits in front."""
    global _EMPTY
    if _EMPTY is None:
        _EMPTY = _empty_blocks()
    v = int.from_bytes(buf[comp_bit >> 3:(comp_bit + n_bits + 7) >> 3], "little") >> (comp_bit & 7)
    v &= (1 << n_bits) - 1
    pv, pn = _EMPTY[comp_bit & 7]
    n = pn + n_bits
    d = zlib.decompressobj(-15, zdict=history) if history else zlib.decompressobj(-15)
    text = d.decompress((pv | v << pn).to_bytes((n + 7) // 8, "little"))
    assert d.unused_data == b""
    return text, d.eof


def streams():
    """name -> (gzip file, its text)"""
    t = tiny()
    out = {}
    for lv in (1, 6, 9):
        out["tiny_level%d" % lv] = (member(t, lv), t)
    out["fixed"] = (member(t[:60000], 6, zlib.Z_FIXED), t[:60000])
    out["stored"] = (member(t, 0), t)
    out["acgt"] = (member(b"ACGT" * 50000), b"ACGT" * 50000)
    out["distance_32768"] = distance_32768()
    a, b = t[:70001], t[70001:]
    out["two_members_and_an_empty_one"] = (member(a, 6) + member(b"", 6) + member(b, 1), t)
    out["bgzf"] = (B.bgzf_file(t, [1, 65280, 7, 3000, 40000, 2, 12345]), t)
    out["flushed"] = flushed_all_phases()
    return out


def distance_32768():
    """A text whose bytes from 32 768 on repeat its first 32 768, every match at the distance of exactly 32 768: the first of
    them, at the start of the second block, copies the FIRST byte of a history of 32 768 bytes.  zlib's compressor stays 262
    bytes short of that distance, so the member is written here: a stored block, then a fixed block of matches."""
    first = bytes((i * 7 + (i >> 8) * 13 + (i >> 3)) & 0xff for i in range(32768))
    text = first + first + first[:5000]
    w = B.BitWriter()
    w.bits(0, 1)
    w.bits(0, 2)
    w.align()
    w.bits(32768, 16)
    w.bits(32768 ^ 0xffff, 16)
    w.out += first
    w.bits(1, 1)
    w.bits(1, 2)
    left = len(text) - 32768
    while left:
        n = min(left, 258) if left - min(left, 258) == 0 or left - min(left, 258) >= 3 else left - 3
        ls = 28 if n == 258 else max(i for i in range(28) if B.LEN_BASE[i] <= n)
        B.fixed_code(w, 257 + ls)
        w.bits(n - B.LEN_BASE[ls], B.LEN_EXTRA[ls])
        w.code(29, 5)  # distances 24 577 .. 32 768: 13 more bits
        w.bits(32768 - B.DIST_BASE[29], 13)
        left -= n
    B.fixed_code(w, 256)
    raw = w.done()
    assert zlib.decompress(raw, -15) == text
    return b"\x1f\x8b\x08\0\0\0\0\0\0\x03" + raw + struct.pack("<II", zlib.crc32(text), len(text)), text


def flushed_all_phases():
    """tiny.fq's first bytes with a sync or a full flush every ~1000 bytes, made longer 1000 bytes at a time until the
    blocks that hold text end on all eight bit phases (so that, at span 1, segments start on all eight)"""
    t = tiny()
    for n in range(8000, len(t), 1000):
        text = t[:n]
        f = member(text, 6, flush_every=997)
        phases = {b1 % 8 for (b0, b1, t0, t1, final) in walk_blocks(f, payload_bit(f)) if t1 > t0 and not final}
        if len(phases) == 8:
            return f, text
    raise AssertionError("no prefix of tiny.fq gives all eight bit phases")


if __name__ == "__main__":
    os.makedirs(sys.argv[1], exist_ok=True)
    for name, (f, text) in streams().items():
        assert gzip.decompress(f) == text
        open(os.path.join(sys.argv[1], name + ".gz"), "wb").write(f)
