"""Concatenated gzip files for the tests of the walk's members switch (csrc/host/gr_gzwalk.cpp: GzWalkMembers), built from
tests/gzip_cases.py's member() and tiny(): files of many members (M1 ragged, M2 equal, M5 several files), files in which
`1f 8b 08` stands where no member begins (M3), and files the walk leaves to zlib (M6).  Every case is a Case: the file, its
text (None: zlib does not read the file to its end) and the number of members a chain from byte 0 passes through.

  python tests/gzip_member_cases.py DIR     writes every file to DIR/<name>.gz (for tools/dev/inflate_host_check.cpp --members)"""
import collections
import gzip
import os
import struct
import sys
import zlib

import gzip_cases as G

SPANS = G.SPANS
Case = collections.namedtuple("Case", "data text members")


def header(flg=0, extra=b"", name=b"", comment=b""):
    """a gzip header with the given FLG and its optional fields in RFC 1952's order (FHCRC: the right CRC16)"""
    h = bytes([0x1f, 0x8b, 8, flg]) + struct.pack("<IBB", 1234567, 0, 3)
    if flg & 4:
        h += struct.pack("<H", len(extra)) + extra
    if flg & 8:
        assert b"\0" not in name
        h += name + b"\0"
    if flg & 16:
        assert b"\0" not in comment
        h += comment + b"\0"
    if flg & 2:
        h += struct.pack("<H", zlib.crc32(h) & 0xffff)
    return h


def member(text, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, head=None, **kw):
    """gzip_cases.member with another header in the place of zlib's ten bytes (head: header()'s arguments)"""
    f = G.member(text, level, strategy, **kw)
    if head is None:
        return f
    assert f[:4] == b"\x1f\x8b\x08\0"
    return header(**head) + f[10:]


def _text(n, skip=0):
    t = G.tiny()
    t = t * (1 + (n + skip) // len(t))
    return t[skip:skip + n]


def _join(parts):
    return Case(b"".join(f for f, _ in parts), b"".join(t for _, t in parts), len(parts))


def m1_ragged():
    """12 members at levels 0, 1, 6, 9 and Z_FIXED, texts of 0, 1, 32 768, 70 001 and about 200 000 bytes among them, one
    header each with FEXTRA, FNAME, FCOMMENT and FHCRC"""
    specs = [(200003, 6, {}), (0, 6, {}), (1, 1, dict(head=dict(flg=4, extra=b"AB\x03\0xyz"))), (32768, 9, dict(head=dict(flg=8, name=b"cell3.fastq"))), (70001, 0, {}),
             (5000, 6, dict(strategy=zlib.Z_FIXED, head=dict(flg=16, comment=b"a comment"))), (70001, 1, dict(head=dict(flg=2))), (32768, 0, {}), (1, 9, {}), (200003, 1, {}), (0, 0, {}),
             (12345, 6, dict(strategy=zlib.Z_FIXED))]
    parts = []
    for i, (n, level, kw) in enumerate(specs):
        t = _text(n, 1000 * i)
        parts.append((member(t, level, **kw), t))
    assert len(parts) == 12
    return _join(parts)


def m2_equal(n=8):
    """(n equal members of about 200 000 bytes of text in one file, one of them alone)"""
    t = _text(200000)
    one = G.member(t, 6)
    return Case(one * n, t * n, n), Case(one, t, 1)


def m3_false_candidates():
    """name -> Case: `1f 8b 08` with a clean flag byte where no member of the chain begins"""
    a, b, c = _text(30000), _text(20000, 500), _text(10000, 900)
    inner = G.member(b"@inner\nACGT\n+\n!!!!\n" * 20, 9)
    fake = bytes([0x1f, 0x8b, 8, 1, 1, 1, 1, 1, 2, 3])
    out = {}
    # (a) a true header whose FEXTRA field holds a complete valid small gzip member
    out["a_member_in_fextra"] = _join([(G.member(a, 6), a), (member(b, 6, head=dict(flg=4, extra=inner)), b), (G.member(c, 1), c)])
    # (b) an FNAME that holds a NUL-free header and bytes behind it
    out["b_header_in_fname"] = _join([(G.member(a, 6), a), (member(b, 9, head=dict(flg=8, name=fake + b"\x4b\x4c\x4d\x01\x02 reads")), b), (G.member(c, 1), c)])
    # (c) a stored member whose text is a complete three-member gzip file, and one more true member: the inner members
    # decode, their trailers match, and they are no members of this file
    three = G.member(a[:9000], 6) + G.member(a[9000:9100], 1) + G.member(a[9100:20000], 9)
    assert gzip.decompress(three) == a[:20000] and len(three) < 65535
    out["c_gzip_file_in_stored_text"] = _join([(G.member(three, 0), three), (G.member(c, 6), c)])
    # (d) a stored member whose text holds the four bytes 2000 times
    many = b"".join(b"\x1f\x8b\x08\0" + bytes([65 + i % 26]) * (i % 7) for i in range(2000))
    out["d_2000_magics_in_stored_text"] = _join([(G.member(many, 0), many)])
    # (e) a member of 559 903 bytes of text: its ISIZE bytes are 1f 8b 08 00
    e = _text(559903)
    f = G.member(e, 6)
    assert f[-4:] == b"\x1f\x8b\x08\0"
    out["e_isize_is_a_magic"] = _join([(f, e), (G.member(c, 6), c)])
    return out


def m5_several_files():
    """10 files of 1 to 6 members"""
    out = {}
    for i in range(10):
        parts = []
        for j in range(1 + (i * 5) % 6):
            t = _text(3000 + 7919 * ((i + 3 * j) % 9), 100 * (i + j))
            parts.append((G.member(t, (0, 1, 6, 9)[(i + j) % 4]), t))
        out["several%d" % i] = _join(parts)
    assert sorted({c.members for c in out.values()}) == [1, 2, 3, 4, 5, 6]
    return out


def m6_left_to_zlib():
    """name -> Case with text None: one fault each, behind a good first member"""
    a, b, c = _text(40000), _text(30000, 700), _text(8000, 300)
    ma, mb, mc = G.member(a, 6), G.member(b, 0), G.member(c, 9)
    out = {}
    out["trailing_bytes"] = Case(ma + mc + b"\0\0\0", None, 2)
    out["method_9"] = Case(ma + b"\x1f\x8b\x09" + mc[3:], None, 1)
    flipped = bytearray(mb)
    flipped[len(mb) // 2] ^= 0x10  # (a stored member: a byte of text)
    out["crc"] = Case(ma + bytes(flipped) + mc, None, 1)
    deep = G.member(b, 6)
    out["truncated"] = Case(ma + deep[:len(deep) * 2 // 3], None, 1)
    out["isize"] = Case(ma + mb[:-4] + struct.pack("<I", len(b) + 1) + mc, None, 1)
    return out


def all_cases():
    out = {"m1_ragged": m1_ragged()}
    out["m2_equal"], out["m2_one"] = m2_equal()
    out.update(("m3_" + k, v) for k, v in m3_false_candidates().items())
    out.update(("m5_" + k, v) for k, v in m5_several_files().items())
    out.update(("m6_" + k, v) for k, v in m6_left_to_zlib().items())
    return out


if __name__ == "__main__":
    os.makedirs(sys.argv[1], exist_ok=True)
    for name, case in all_cases().items():
        if case.text is not None:
            assert gzip.decompress(case.data) == case.text, name
        assert len(case.data) < 3 << 20, name
        open(os.path.join(sys.argv[1], name + ".gz"), "wb").write(case.data)
