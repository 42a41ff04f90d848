"""Unaligned BAM byte strings for the tests of the BAM input (csrc/host/gr_bam.hpp, grp_bam_parse): a writer that takes every
field of a record from the test, the FASTQ twin of what it writes, and a walk of the bytes by the format's definition (SAM
specification §4.2) that the C++ walk is compared with."""
import struct

import bgzf_cases as B

CODES = b"=ACMGRSVTWYHKDBN"
CODE_OF = {c: i for i, c in enumerate(CODES)}
REFUSED_FLAGS = 0x10 | 0x100 | 0x800


def header(text=b"", refs=()):
    """the BAM header: magic, l_text, text, n_ref, then (l_name, name NUL-terminated, l_ref) per reference"""
    out = [b"BAM\1", struct.pack("<i", len(text)), text, struct.pack("<i", len(refs))]
    for name, length in refs:
        out += [struct.pack("<i", len(name) + 1), name + b"\0", struct.pack("<i", length)]
    return b"".join(out)


def pack_bases(bases, pad=0):
    """4-bit codes, the first base in the high half of a byte; `pad`: the code behind an odd length"""
    codes = [CODE_OF[c] for c in bases.upper()]
    if len(codes) & 1:
        codes.append(pad)
    return bytes((codes[i] << 4) | codes[i + 1] for i in range(0, len(codes), 2))


def record(name, bases, quals, flag=4, cigar=(), tags=b"", pad=0, block_size=None, l_read_name=None, nul=True, l_seq=None):
    """one alignment record.  name: bytes without the NUL; bases: bytes over CODES; quals: raw Phred bytes (len(bases) of
    them); cigar: uint32 operations; tags: bytes.  block_size / l_read_name / nul / l_seq let a test write a broken one."""
    assert len(quals) == len(bases)
    nm = name + (b"\0" if nul else b"")
    body = nm + b"".join(struct.pack("<I", c) for c in cigar) + pack_bases(bases, pad) + bytes(quals) + tags
    fixed = struct.pack("<iiBBHHHIiii", -1, -1, len(nm) if l_read_name is None else l_read_name, 0, 4680, len(cigar), flag,
                        len(bases) if l_seq is None else l_seq, -1, -1, 0)
    assert len(fixed) == 32
    return struct.pack("<I", len(fixed) + len(body) if block_size is None else block_size) + fixed + body


def twin_record(name, bases, quals):
    """the four lines the program reads in place of the record (a quality above 93 has no character: such a record has
    no twin, and what stands here for it is never compared)"""
    return b"@" + name + b"\n" + bases.upper() + b"\n+\n" + bytes((q + 33) & 255 for q in quals) + b"\n"


def stream(records, text=b"", refs=()):
    """records: dicts of record()'s arguments -> (the decompressed BAM stream, where its records begin, its FASTQ twin)"""
    hdr = header(text, refs)
    body = b"".join(record(**r) for r in records)
    twin = b"".join(twin_record(r["name"], r["bases"], r["quals"]) for r in records)
    return hdr + body, len(hdr), twin


def bam_file(records, sizes=(65280,), text=b"", refs=(), level=1, eof=True):
    """-> (the BGZF file, its FASTQ twin)"""
    raw, _, twin = stream(records, text, refs)
    return B.bgzf_file(raw, list(sizes), level=level, eof=eof), twin


def walk(buf, final=True):
    """The record chain of `buf` (which begins at a record) by the definition: -> (records, consumed, bad_offset or None).
    records: dicts of off, name (up to the NUL, cut at the first whitespace), l_seq, seq_off, qual_off, end, flag.
    bad_offset: the first record that the program refuses, or that the buffer ends in when it is the final one."""
    recs, pos, n = [], 0, len(buf)
    while pos < n:
        if n - pos < 4:
            break
        (bs,) = struct.unpack_from("<I", buf, pos)
        if bs < 32:
            return recs, pos, pos
        if n - pos - 4 < bs:
            break
        l_name, _, _, n_cig, flag, l_seq = struct.unpack_from("<BBHHHI", buf, pos + 4 + 8)
        if 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq > bs or l_name == 0 or buf[pos + 36 + l_name - 1] != 0 or flag & REFUSED_FLAGS:
            return recs, pos, pos
        name = buf[pos + 36:pos + 36 + l_name - 1].split(b"\0")[0]
        for i, ch in enumerate(name):
            if ch == 32 or 9 <= ch <= 13:
                name = name[:i]
                break
        seq_off = pos + 36 + l_name + 4 * n_cig
        recs.append(dict(off=pos, name=name, l_seq=l_seq, seq_off=seq_off, qual_off=seq_off + (l_seq + 1) // 2, end=pos + 4 + bs, flag=flag))
        pos += 4 + bs
    return recs, pos, (pos if final and pos < n else None)
