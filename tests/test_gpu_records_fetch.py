"""GPU: grp_records_fetch (csrc/grp_inflate.inc, k_emit_records) at the C ABI — records of a compressed input inflated,
cut and formatted on the device.  The expectation is a Python model of what the host program's commit_sink writes for an
inserted read (csrc/host/gr_writer.cpp) and the host library's gr_sum_phred of the quality characters it writes: bytes are
compared as bytes, sums by their 64 bits.  Every refusal here is one of the table checks or a unit with a wrong CRC32:
both are turned down before the emit kernel is launched, and the caller's buffer is untouched."""
import struct
import zlib

import numpy as np
import pytest

import bam_cases as BC
import bgzf_cases as B
import gzip_cases as G
from helpers import default_seeds
from test_gpu_bgzf import _pack as _pack_members
from test_gpu_gzip import _pack as _pack_segments

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 15, 16, 17, 63, 64, 65, 4097, 70001)
BASES = b"ACGTacgtNnRYxy*-"


@pytest.fixture(scope="module")
def eng(native):
    e = native.Engine(22, 3, 1000, 1 << 20, default_seeds())
    yield e
    e.close()


@pytest.fixture(scope="module")
def hl(native):
    from goldrush_amd import host as h

    h.load()
    return h


# ---- the model: commit_sink (gr_writer.cpp) ------------------------------------------------------------------------------
def slice_of(seq_len, qual_len, trim, tile=1):
    """(off, n_seq, qoff, n_qual) of a committed read; trim = None (inserted whole) or (trim_start, trim_end, num_tiles)"""
    off, n_seq, n_qual = 0, seq_len, qual_len
    if trim is not None:
        ts, te, nt = trim
        off = ts * tile
        end_pos = (1 << 62) if te == nt - 1 else (te - ts + 1) * tile
        n_seq = min(end_pos, seq_len - off)
        n_qual = min(end_pos, qual_len - off) if off <= qual_len else 0
    return off, n_seq, min(off, qual_len), n_qual


def written(rec, trim, fastq):
    """rec: dict(id, bases, quals) with bases as the text the program sees (a BAM record: its twin's) and quals as quality
    CHARACTERS -> (the bytes commit_sink writes, the quality characters it sums)"""
    off, n_seq, qoff, n_qual = slice_of(len(rec["bases"]), len(rec["quals"]), trim)
    seq = bytes(c - 32 if 97 <= c <= 122 else c for c in rec["bases"][off:off + n_seq])
    qual = rec["quals"][qoff:qoff + n_qual]
    out = (b"@" if fastq else b">") + rec["id"] + (b"_untrimmed\n" if trim is None else b"_trimmed\n") + seq + b"\n"
    if fastq:
        out += b"+\n" + qual + b"\n"
    return out, qual


# ---- inputs ----------------------------------------------------------------------------------------------------------
def _records(rng, bam):
    recs = []
    for i, n in enumerate(LENGTHS):
        name = b"r%d" % i
        if n == 15:
            name = b"x"  # an id of one character ...
        if n == 16:
            name = bytes(rng.integers(48, 123, 254 if bam else 255).astype(np.uint8))  # ... and one of 255 (BAM: 254 and the NUL fill l_read_name)
        if bam:
            bases = bytes(rng.choice(np.frombuffer(BC.CODES, dtype=np.uint8), n))
            quals = bytes(rng.integers(0, 94, n).astype(np.uint8))
        else:
            bases = bytes(rng.choice(np.frombuffer(BASES, dtype=np.uint8), n))
            quals = bytes(rng.integers(33, 127, n).astype(np.uint8))
        recs.append(dict(id=name, bases=bases, quals=quals))
    if not bam:  # qualities shorter than the bases: qoff is clamped, n_qual 0 behind their end
        recs.append(dict(id=b"shortq", bases=bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 100)), quals=bytes(rng.integers(33, 127, 40).astype(np.uint8))))
    return recs


def _fastq_text(recs):
    """the records as FASTQ text (headers with a comment; the last line without its newline: the last record ends at the
    text's last byte) -> (text, [dict(id_off, seq_off, qual_off)])"""
    text, where = bytearray(), []
    for r in recs:
        w = dict(id_off=len(text) + 1)
        text += b"@" + r["id"] + b" a comment\n"
        w["seq_off"] = len(text)
        text += r["bases"] + b"\n+\n"
        w["qual_off"] = len(text)
        text += r["quals"] + b"\n"
        where.append(w)
    assert recs[-1]["quals"]
    return bytes(text[:-1]), where


def _bam_text(recs):
    raw, hdr, _ = BC.stream([dict(name=r["id"], bases=r["bases"], quals=r["quals"], tags=b"" if i == len(recs) - 1 else b"XYZ\0") for i, r in enumerate(recs)], text=b"@HD\tVN:1.6\n")
    walked, used, bad = BC.walk(raw[hdr:])
    assert bad is None and len(walked) == len(recs) and walked[-1]["qual_off"] + walked[-1]["l_seq"] + hdr == len(raw)
    where = [dict(id_off=hdr + w["off"] + 36, seq_off=hdr + w["seq_off"], qual_off=hdr + w["qual_off"]) for w in walked]
    # the model sees the twin: bases as text, qualities as characters
    twins = [dict(id=r["id"], bases=r["bases"], quals=bytes(q + 33 for q in r["quals"])) for r in recs]
    return raw, where, twins


def _plan(recs):
    """(record, trim) pairs: every record whole; slices from bases 0, 1, 15, 16 (and an odd base of a record of odd length)
    up to the end and up to a base in the middle; the record with short qualities cut inside and behind them"""
    plan = [(i, None) for i in range(len(recs))]
    big = LENGTHS.index(4097)
    for start in (0, 1, 15, 16, 33):
        plan.append((big, (start, 4096, 4097)))          # to the end (trim_end is the last tile)
        plan.append((big, (start, start + 1000, 4097)))  # 1001 bases
    plan.append((LENGTHS.index(70001), (65279, 69999, 70001)))
    plan.append((LENGTHS.index(17), (3, 3, 17)))
    if len(recs) > len(LENGTHS):
        s = len(recs) - 1
        plan += [(s, (20, 99, 100)), (s, (20, 29, 100)), (s, (50, 99, 100)), (s, (40, 60, 100))]
    return plan


def _table(nat, recs, where, plan, fastq, gap=19):
    """the fetch table with the outputs at every residue modulo 16 and `gap`+ bytes between them (gap 0: back to back); the
    last output ends the buffer -> (table, out_cap)"""
    tab = np.zeros(len(plan), dtype=nat.fetch_record_dtype)
    at = gap
    for k, (i, trim) in enumerate(plan):
        r, w = recs[i], where[i]
        off, n_seq, qoff, n_qual = slice_of(len(r["bases"]), len(r["quals"]), trim)
        while gap and at % 16 != k % 16:
            at += 1
        tab[k] = (w["id_off"], w["seq_off"], w["qual_off"], at, len(r["id"]), off, n_seq, qoff, n_qual, 0 if trim is None else nat.FETCH_REC_TRIMMED)
        at += len(written(r, trim, fastq)[0]) + (gap if k + 1 < len(plan) else 0)
    return tab, at


def _sentinel(n):
    return ((np.arange(n, dtype=np.uint32) * 7 + 3) % 251).astype(np.uint8) | 0x80  # (no byte of it is text)


def _check(hl, recs, plan, tab, out, sums, fastq):
    keep = _sentinel(out.size)
    mask = np.ones(out.size, dtype=bool)
    for k, (i, trim) in enumerate(plan):
        exp, qual = written(recs[i], trim, fastq)
        a = int(tab[k]["out_off"])
        assert out[a:a + len(exp)].tobytes() == exp, (k, i, trim)
        assert struct.pack("<d", float(sums[k])) == struct.pack("<d", hl.load().gr_sum_phred(qual, len(qual))), (k, i, trim)
        mask[a:a + len(exp)] = False
    assert np.array_equal(out[mask], keep[mask]), "a byte outside the records' output ranges was written"
    assert mask.sum() > 0 and not mask[-1]


@pytest.fixture(scope="module")
def inputs(tmp_path_factory, hl):
    """kind -> (unit kind, comp, dict, units, records as the model sees them, where they are in the text, the text)"""
    from goldrush_amd import native as nat

    rng = np.random.default_rng(11)
    out = {}
    fq = _records(rng, bam=False)
    text, where = _fastq_text(fq)
    f = B.bgzf_file(text, [65280, 1, 40000, 513])
    blocks, used, why = B.walk_members(f)
    assert why == 1 and sum(b[2] for b in blocks) == len(text) and len(blocks) >= 6
    out["fastq-bgzf"] = (nat.FETCH_UNITS_BGZF, f, b"", np.array([b + (0,) for b in blocks], dtype=nat.bgzf_block_dtype), fq, where, text)
    # ... with an empty member in the middle (the EOF marker is one at the end already)
    cut = 3
    at = blocks[cut][0] - 18
    f2 = f[:at] + B.BGZF_EOF + f[at:]
    blocks2, _, why = B.walk_members(f2)
    assert why == 1 and blocks2[cut][2] == 0 and len(blocks2) == len(blocks) + 1
    out["fastq-bgzf-empty-member"] = (nat.FETCH_UNITS_BGZF, f2, b"", np.array([b + (0,) for b in blocks2], dtype=nat.bgzf_block_dtype), fq, where, text)
    p = tmp_path_factory.mktemp("fetch") / "reads.fq.gz"
    gz = G.member(text, 6)
    p.write_bytes(gz)
    segs = hl.gzip_index(p, 50000)["segments"]
    assert sum(g["text_len"] for g in segs) == len(text) and len(segs) >= 3 and max(len(g["dict"]) for g in segs) == 32768
    comp, hist, table = _pack_segments([(gz, g) for g in segs], gap=1)
    out["fastq-gzip"] = (nat.FETCH_UNITS_GZIP, comp, hist, np.array(table, dtype=nat.gzip_segment_dtype), fq, where, text)
    raw, bwhere, twins = _bam_text(_records(rng, bam=True))
    fb = B.bgzf_file(raw, [65280, 1, 40000, 513])
    bblocks, _, why = B.walk_members(fb)
    assert why == 1
    out["bam-bgzf"] = (nat.FETCH_UNITS_BGZF, fb, b"", np.array([b + (0,) for b in bblocks], dtype=nat.bgzf_block_dtype), twins, bwhere, raw)
    return out


@pytest.mark.parametrize("fastq", [True, False], ids=["fastq-out", "fasta-out"])
@pytest.mark.parametrize("kind", ["fastq-bgzf", "fastq-bgzf-empty-member", "fastq-gzip", "bam-bgzf"])
def test_records_are_what_commit_sink_writes(eng, native, hl, inputs, kind, fastq):
    unit_kind, comp, hist, units, recs, where, text = inputs[kind]
    plan = _plan(recs)
    tab, cap = _table(native, recs, where, plan, fastq)
    assert {int(o) % 16 for o in tab["out_off"]} == set(range(16))
    assert any(int(t["n_seq"]) > 65536 for t in tab)  # (more than one member)
    if kind.startswith("bam"):
        assert any(int(t["seq_from"]) % 2 == 1 and len(recs[i]["bases"]) % 2 == 1 for t, (i, _) in zip(tab, plan))
    else:
        assert any(int(t["n_qual"]) == 0 and int(t["qual_from"]) == 40 for t in tab)  # qoff clamped to the qualities' end
        last = max(range(len(tab)), key=lambda k: int(tab[k]["qual_off"]) + int(tab[k]["qual_from"]) + int(tab[k]["n_qual"]))
        assert int(tab[last]["qual_off"]) + int(tab[last]["qual_from"]) + int(tab[last]["n_qual"]) == len(text)  # the text's last byte
    out = _sentinel(cap)
    flags = (native.FETCH_FASTQ if fastq else 0) | (native.FETCH_BAM if kind.startswith("bam") else 0)
    sums = eng.records_fetch(unit_kind, comp, hist, units, tab, flags, out)
    _check(hl, recs, plan, tab, out, sums, fastq)
    # the same records in another order of the table, packed back to back
    order = np.random.default_rng(5).permutation(len(plan))
    plan2 = [plan[i] for i in order]
    tab2, cap2 = _table(native, recs, where, plan2, fastq, gap=0)
    out2 = _sentinel(cap2 + 5)  # (the buffer is larger than the capacity the call is told)
    sums2 = eng.records_fetch(unit_kind, comp, hist, units, tab2, flags, out2, out_cap=cap2)
    assert out2[:cap2].tobytes() == b"".join(written(recs[i], t, fastq)[0] for i, t in plan2)
    assert np.array_equal(out2[cap2:], _sentinel(cap2 + 5)[cap2:])
    assert [struct.pack("<d", float(s)) for s in sums2] == [struct.pack("<d", float(sums[i])) for i in order]


def test_no_records_and_no_units(eng, native, hl, inputs):
    unit_kind, comp, hist, units, recs, where, text = inputs["fastq-bgzf"]
    none = np.zeros(0, dtype=native.fetch_record_dtype)
    out = _sentinel(64)
    assert len(eng.records_fetch(unit_kind, comp, hist, units, none, native.FETCH_FASTQ, out)) == 0
    assert len(eng.records_fetch(unit_kind, b"", b"", units[:0], none, native.FETCH_FASTQ, out)) == 0
    assert np.array_equal(out, _sentinel(64))
    # no unit, no text: a record of nothing is its fixed characters
    one = np.zeros(1, dtype=native.fetch_record_dtype)
    one[0]["out_off"] = 7
    sums = eng.records_fetch(unit_kind, b"", b"", units[:0], one, native.FETCH_FASTQ, out)
    exp = b"@_untrimmed\n\n+\n\n"
    assert out[7:7 + len(exp)].tobytes() == exp and float(sums[0]) == 0.0
    keep = _sentinel(64)
    assert np.array_equal(out[:7], keep[:7]) and np.array_equal(out[7 + len(exp):], keep[7 + len(exp):])


def _stats(eng):
    return eng.bgzf_stats(), eng.gzip_stats()


def test_every_table_check_refuses_before_a_launch(eng, native, hl, inputs):
    unit_kind, comp, hist, units, recs, where, text = inputs["fastq-bgzf"]
    plan = [(0, None), (4, None), (8, (1, 4096, 4097))]
    good, cap = _table(native, recs, where, plan, True, gap=0)
    total = len(text)
    before = _stats(eng)

    def refused(tab, flags=native.FETCH_FASTQ, bad_record=None, bad_unit=None, out_cap=cap, u=units, c=comp, kind=unit_kind):
        out = _sentinel(cap + 16)
        with pytest.raises(native.GrpError) as e:
            eng.records_fetch(kind, c, hist, u, tab, flags, out, out_cap=out_cap)
        assert e.value.code == native.GRP_ERR_INVALID, str(e.value)
        assert (e.value.bad_record, e.value.bad_unit) == (bad_record, bad_unit), str(e.value)
        assert np.array_equal(out, _sentinel(cap + 16))

    def with_(k, **kw):
        t = good.copy()
        for name, v in kw.items():
            t[k][name] = v
        return t

    refused(with_(1, id_off=total - 1), bad_record=1)                      # the id ends behind the text
    refused(with_(1, id_off=total + 1, id_len=0), bad_record=1)
    refused(with_(2, seq_off=total - 500), bad_record=2)                   # the bases do
    refused(with_(2, seq_from=0xFFFFFFFF), bad_record=2)
    refused(with_(2, n_seq=0xFFFFFFFF), bad_record=2)
    refused(with_(0, seq_off=1 << 63), bad_record=0)
    refused(with_(2, qual_off=total - 500), bad_record=2)                  # the qualities do
    refused(with_(2, qual_from=0xFFFFFFFF, n_qual=0xFFFFFFFF), bad_record=2)
    refused(with_(1, flags=2), bad_record=1)                               # an unknown flag
    refused(good, bad_record=2, out_cap=cap - 1)                           # the last output ends one byte behind the capacity
    refused(with_(0, out_off=cap), bad_record=0)
    refused(with_(0, out_off=(1 << 64) - 4), bad_record=0)
    refused(with_(1, out_off=int(good[0]["out_off"]) + 3), bad_record=1)   # overlaps record 0's: the one that begins later
    refused(with_(2, out_off=int(good[1]["out_off"])), bad_record=2)       # the same begin: the later entry
    refused(good, flags=4)                                                 # an unknown output flag
    refused(good, kind=2)                                                  # an unknown kind of unit
    assert _stats(eng) == before  # nothing was launched for any of them
    # BAM: two bases to a byte — the last base's byte must lie inside the text
    bkind, bcomp, _, bunits, brecs, bwhere, braw = inputs["bam-bgzf"]
    btab, bcap = _table(native, brecs, bwhere, [(8, None)], True, gap=0)
    assert bcap <= cap
    t = btab.copy()
    t[0]["seq_off"] = len(braw) - 2048
    t[0]["n_seq"] = 4097                                                   # 2049 bytes
    t[0]["n_qual"] = 0
    out = _sentinel(cap + 16)
    with pytest.raises(native.GrpError) as e:
        eng.records_fetch(bkind, bcomp, b"", bunits, t, native.FETCH_FASTQ | native.FETCH_BAM, out)
    assert e.value.bad_record == 0 and "bases" in str(e.value)
    t[0]["n_seq"] = 4096                                                   # 2048 bytes: inside (the call runs)
    eng.records_fetch(bkind, bcomp, b"", bunits, t, native.FETCH_FASTQ | native.FETCH_BAM, out)
    after_bam = _stats(eng)
    assert after_bam[0]["blocks"] - before[0]["blocks"] == len(bunits) and after_bam[1] == before[1]
    # the unit table's checks are grp_bgzf_inflate's
    bad = units.copy()
    bad[2]["comp_len"] = len(comp)
    refused(good, bad_unit=2, u=bad)
    bad = units.copy()
    bad[1]["text_len"] = 65537
    refused(good, bad_unit=1, u=bad)
    assert _stats(eng) == after_bam  # nothing was launched for any of them


def test_a_unit_with_a_wrong_crc_is_refused_and_the_engine_goes_on(eng, native, hl, inputs):
    for kind in ("fastq-bgzf", "fastq-gzip"):
        unit_kind, comp, hist, units, recs, where, text = inputs[kind]
        plan = [(3, None), (5, (1, 30, 63))]
        tab, cap = _table(native, recs, where, plan, True)
        bad = units.copy()
        bad[1]["crc32"] ^= 1
        out = _sentinel(cap)
        with pytest.raises(native.GrpError) as e:
            eng.records_fetch(unit_kind, comp, hist, bad, tab, native.FETCH_FASTQ, out)
        assert e.value.code == native.GRP_ERR_INVALID and e.value.bad_unit == 1 and e.value.bad_record is None and "CRC32" in str(e.value)
        assert np.array_equal(out, _sentinel(cap))
        sums = eng.records_fetch(unit_kind, comp, hist, units, tab, native.FETCH_FASTQ, out)
        _check(hl, recs, plan, tab, out, sums, True)


def test_the_inflate_calls_still_return_their_text(eng, native, inputs):
    """the fetch shares the launcher and the pool of grp_bgzf_inflate / grp_gzip_inflate: the text still comes down from them"""
    unit_kind, comp, hist, units, recs, where, text = inputs["fastq-bgzf"]
    assert eng.bgzf_inflate(comp, units) == text
    unit_kind, comp, hist, units, recs, where, text = inputs["fastq-gzip"]
    assert eng.gzip_inflate(comp, hist, units) == text
    assert zlib.crc32(text) == zlib.crc32(inputs["fastq-bgzf"][6])
