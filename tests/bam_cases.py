"""Unaligned BAM byte strings for the tests of the BAM input (csrc/host/gr_bam.hpp, grp_bam_parse): a writer that takes every
field of a record from the test, the FASTQ twin of what it writes, and a walk of the bytes by the format's definition (SAM
specification §4.2) that the C++ walk is compared with."""
import struct

import numpy as np

import bgzf_cases as B
import ingest_cases as IC

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


# ---- the edge sweeps (tests/test_gpu_bam_edges.py; ingest_cases.py has the FASTQ side and the kernels' geometry) --------------
# the lengths of the FASTQ sweep, and those whose code bytes (half as many as the bases) end round 1024 and 2048
SWEEP_LENGTHS = IC.S1_LENGTHS + [2079, 2080, 2081, 4128]
BAD_CODES = [c for c in range(16) if c not in (1, 2, 4, 8)]  # the 12 codes that are none of A, C, G, T
BAD_SHORT = list(range(1, 50))
BAD_LONG = [2047, 2048, 2049, 2063, 2064, 2065, 2079, 2080, 2081, 4128]
BAD_KINDS = IC.S2_KINDS + ["odd"]  # "odd": the last base of an odd length, the high half of the byte behind the whole bytes
BAD_CASE = np.dtype([("rec", "<i8"), ("twin", "<i8"), ("len", "<i4"), ("align", "<i4"), ("pos", "<i4"), ("code", "<i4"), ("kind", "<i4")])
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def steered_name(i, pos, want):
    """a name for the record at byte `pos` of the stream (no CIGAR) that puts its bases at want (mod 16)"""
    k = (want - (pos + 37)) % 16
    n = k if k >= 4 else k + 16
    name = (b"s%d" % i).ljust(n, b"_")[:n]
    assert (pos + 36 + len(name) + 1) % 16 == want
    return name


def record_size(r):
    return 36 + len(r["name"]) + 1 + 4 * len(r.get("cigar", ())) + (len(r["bases"]) + 1) // 2 + len(r["bases"]) + len(r.get("tags", b""))


def sweep_records(seed=201, lengths=None, aligns=range(16)):
    """length x alignment: every length at all 16 values of seq_off % 16 (qual_off % 16 follows), random A / C / G / T,
    qualities 0..93; the padding code behind an odd length takes all 16 values (it is the alignment)"""
    rng = np.random.default_rng(seed)
    recs, pos = [], 0
    for L in SWEEP_LENGTHS if lengths is None else lengths:
        for a in aligns:
            quals = bytes(rng.integers(0, 94, size=L).astype(np.uint8)) if len(recs) % 7 else b"\x5d" * L
            r = dict(name=steered_name(len(recs), pos, a), bases=_ACGT[rng.integers(0, 4, size=L)].tobytes(), quals=quals, pad=a, flag=4)
            recs.append(r)
            pos += record_size(r)
    return recs


def bad_code_records(seed=202, short=None, long=None, aligns=range(16)):
    """-> (records, cases[BAD_CASE]): as ingest_cases.s2_text — a clean record per (length, alignment) and behind it one
    copy per planted base with that one code replaced.  Short records: every base.  Long ones: both halves of the code
    bytes at the swept positions of the aligned middle, and the last base of an odd length."""
    rng = np.random.default_rng(seed)
    recs, cases, pos, turn = [], [], 0, 0

    def put(bases, a, pad):
        nonlocal pos
        r = dict(name=steered_name(len(recs), pos, a), bases=bytes(bases), quals=b"\x28" * len(bases), pad=pad, flag=4)
        recs.append(r)
        pos += record_size(r)
        return len(recs) - 1

    for lengths, every in ((BAD_SHORT if short is None else short, True), (BAD_LONG if long is None else long, False)):
        for L in lengths:
            for a in aligns:
                clean = bytearray(_ACGT[rng.integers(0, 4, size=L)].tobytes())
                twin = put(clean, a, a)  # (the padding code behind an odd length: every value on clean records)
                if every:
                    planted = [("every", p) for p in range(L)]
                else:
                    planted = [(k, 2 * b + half) for k, b in IC.edge_positions(a, L // 2) for half in (0, 1)] + ([("odd", L - 1)] if L & 1 else [])
                for kind, p in planted:
                    bases = bytearray(clean)
                    code = BAD_CODES[turn % len(BAD_CODES)]
                    bases[p] = CODES[code]
                    cases.append((put(bases, a, turn % 16), twin, L, a, p, code, BAD_KINDS.index(kind)))
                    turn += 1
    return recs, np.array(cases, dtype=BAD_CASE)


QUAL_REFUSED = (94, 127, 128, 0xFF)
QUAL_CASE = np.dtype([("rec", "<i8"), ("pos", "<i4"), ("kind", "U12")])


def qual_sweep_records(seed=203):
    """-> (records, positions[QUAL_CASE]): one small stream for the range test over the qualities, a byte of which is patched
    per case: records of 2100 bases (an aligned middle of two rounds), of 40 and of 5 (no middle) at four alignments of the
    quality bytes, on either strand; the swept positions of ingest_cases.edge_positions and the four byte lanes of a word"""
    rng = np.random.default_rng(seed)
    recs, at, pos = [], [], 0
    for qa in (0, 1, 7, 14):
        for L in (2100, 40, 5):
            a = (qa - (L + 1) // 2) % 16
            r = dict(name=steered_name(len(recs), pos, a), bases=_ACGT[rng.integers(0, 4, size=L)].tobytes(), quals=bytes(rng.integers(0, 60, size=L).astype(np.uint8)),
                     pad=3, flag=(4, 0x10)[len(recs) % 2])
            f = IC.middle(qa, L)[0]
            where = [("every", p) for p in range(L)] if L == 5 else IC.edge_positions(qa, L)
            if L == 2100:
                where += [("lane", f + j) for j in (1, 2, 3)] + [("lane-1024", f + 1024 + j) for j in (1, 2, 3)]
            at += [(len(recs), p, k) for k, p in where]
            recs.append(r)
            pos += record_size(r)
    return recs, np.array(at, dtype=QUAL_CASE)
