"""Aligned BAM for the tests of GRP_BAM_ALIGNED (csrc/host/gr_bam.hpp, grp_bam_parse_ex): the aligned twin — the FASTQ that
`samtools fastq -n` writes for a BAM file with its default filters, written down from the SAM specification and samtools'
documented behaviour (no samtools is at hand: nothing here is pinned against its output) — and a walk of the bytes by the
format's definition that takes the mask of accepted flags.  bam_cases.py writes the records."""
import struct

import bam_cases as BC

REVERSE, SECONDARY, SUPPLEMENTARY = 0x10, 0x100, 0x800
SKIPPED = SECONDARY | SUPPLEMENTARY
ALL = REVERSE | SKIPPED
# the complement of a base, IUPAC codes included; '=' has none
COMPLEMENT = bytes.maketrans(b"=ACMGRSVTWYHKDBN", b"=TGKCYSBAWRDMHVN")
assert all(BC.CODES[int("{:04b}".format(i)[::-1], 2)] == BC.CODES.translate(COMPLEMENT)[i] for i in range(16))  # ... is the bit reversal of its 4-bit code


def twin_read(bases, quals, flag):
    """(bases, quality characters) of one record as the aligned twin has them; None: the record is no read of the twin"""
    if flag & SKIPPED:
        return None
    bases, qual = bases.upper(), bytes((q + 33) & 255 for q in quals)
    if flag & REVERSE:
        bases, qual = bases.translate(COMPLEMENT)[::-1], qual[::-1]
    return bases, qual


def aligned_twin(records):
    """records: dicts of bam_cases.record()'s arguments -> the FASTQ text the program reads in their place"""
    out = []
    for r in records:
        t = twin_read(r["bases"], r["quals"], r.get("flag", 4))
        if t is not None:
            out.append(b"@" + r["name"] + b"\n" + t[0] + b"\n+\n" + t[1] + b"\n")
    return b"".join(out)


def model_table(body, records, accept, sum_phred):
    """The record table that grp_bam_parse[_ex] reports for `body` (the records written one behind the other), by the
    definitions alone: the offsets and lengths of walk(), the ACGT flag and the Phred sums of the twin's lines (sum_phred:
    the host library's gr_sum_phred), GRP_FQ_REVERSED where an accepted 0x10 is set.  ingest_cases.RECORD_DTYPE."""
    import numpy as np

    import ingest_cases as IC

    recs, used, bad, _ = walk(body, True, accept)
    reads = [r for r in records if not r.get("flag", 4) & SKIPPED]
    assert bad is None and used == len(body) and len(recs) == len(reads)
    table = np.zeros(len(recs), dtype=IC.RECORD_DTYPE)
    for i, (w, r) in enumerate(zip(recs, reads)):
        bases, qual = twin_read(r["bases"], r["quals"], r.get("flag", 4))
        flags = (IC.NON_ACGT if bases.strip(b"ACGT") else 0) | (2 if w["flag"] & accept & REVERSE else 0)
        n = w["l_seq"]
        table[i] = (w["off"] + 36, w["seq_off"], w["qual_off"], len(w["name"]), n, n, flags, sum_phred(qual), sum_phred(qual[:n // 2]) if n >= 2 else 0.0)
    return table


def counts(records):
    """(records skipped, records read in reverse)"""
    flags = [r.get("flag", 4) for r in records]
    return sum(1 for f in flags if f & SKIPPED), sum(1 for f in flags if f & REVERSE and not f & SKIPPED)


def walk(buf, final=True, accept=0):
    """bam_cases.walk with the mask: -> (records emitted, consumed, bad_offset or None, records skipped).  A flag bit of
    0x910 outside `accept` refuses the record; an accepted 0x100 / 0x800 is checked, consumed, counted and not emitted."""
    recs, pos, n, skipped = [], 0, len(buf), 0
    while pos < n:
        if n - pos < 4:
            break
        (bs,) = struct.unpack_from("<I", buf, pos)
        if bs < 32:
            return recs, pos, pos, skipped
        if n - pos - 4 < bs:
            break
        l_name, _, _, n_cig, flag, l_seq = struct.unpack_from("<BBHHHI", buf, pos + 4 + 8)
        if 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq > bs or l_name == 0 or buf[pos + 36 + l_name - 1] != 0 or flag & ALL & ~accept:
            return recs, pos, pos, skipped
        if flag & SKIPPED:
            skipped += 1
        else:
            name = buf[pos + 36:pos + 36 + l_name - 1].split(b"\0")[0]
            for i, ch in enumerate(name):
                if ch == 32 or 9 <= ch <= 13:
                    name = name[:i]
                    break
            seq_off = pos + 36 + l_name + 4 * n_cig
            recs.append(dict(off=pos, name=name, l_seq=l_seq, seq_off=seq_off, qual_off=seq_off + (l_seq + 1) // 2, end=pos + 4 + bs, flag=flag))
        pos += 4 + bs
    return recs, pos, (pos if final and pos < n else None), skipped
