"""GPU: grp_records_fetch with GRP_FETCH_REC_REVERSED (csrc/grp_inflate.inc: k_emit_records' backward forms) — the written
records of reverse-strand reads of an aligned BAM file.  The BAM case of tests/test_gpu_records_fetch.py with every entry of
its plan fetched twice, as it is stored and reversed: the table names the STORED range, the expectation is the model of
commit_sink on the aligned twin's read (tests/bam_aligned_cases.py), bytes compared as bytes and sums by their 64 bits
against the host library's gr_sum_phred of the written quality characters."""
import struct

import numpy as np
import pytest

import bam_aligned_cases as BA
import bgzf_cases as B
import test_gpu_records_fetch as RF
from test_gpu_records_fetch import eng, hl  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

REVERSED = 2  # GRP_FETCH_REC_REVERSED


@pytest.fixture(scope="module")
def bam(native):
    rng = np.random.default_rng(23)
    stored = RF._records(rng, bam=True)
    raw, where, twins = RF._bam_text(stored)
    # the same records as the aligned twin has them when their flag 0x10 is set
    turned = []
    for r in stored:
        seq, qual = BA.twin_read(r["bases"], r["quals"], 0x10)
        turned.append(dict(id=r["id"], bases=seq, quals=qual))
    f = B.bgzf_file(raw, [65280, 1, 40000, 513])
    blocks, _, why = B.walk_members(f)
    assert why == 1 and len(blocks) >= 4
    return f, np.array([b + (0,) for b in blocks], dtype=native.bgzf_block_dtype), twins, turned, where, raw


def _plan(recs):
    """(record, trim, reversed): the plan of test_gpu_records_fetch.py — every record whole, slices of the record of 4097
    bases (odd) from bases 0, 1, 15, 16 and 33, one slice across a member boundary — and the same slices of the record of
    64 bases (even), each entry as it is stored and reversed"""
    plan = RF._plan(recs)
    even = RF.LENGTHS.index(64)
    for start in (0, 1, 15, 16, 33):
        plan.append((even, (start, 63, 64)))
        plan.append((even, (start, start + 20, 64)))
    plan.append((RF.LENGTHS.index(70001), (0, 66000, 70001)))  # reversed: the stored bases 4000 ... 70000, across the members' boundaries
    return [(i, trim, rev) for rev in (True, False) for i, trim in plan]  # (each half meets every residue of 16 in the output)


def _table(nat, twins, turned, where, plan, fastq, gap=19):
    tab = np.zeros(len(plan), dtype=nat.fetch_record_dtype)
    at = gap
    for k, (i, trim, rev) in enumerate(plan):
        r, w = (turned if rev else twins)[i], where[i]
        L = len(r["bases"])
        off, n_seq, qoff, n_qual = RF.slice_of(L, len(r["quals"]), trim)
        if rev:  # the stored range of the twin's slice
            off, qoff = L - off - n_seq, L - qoff - n_qual
        while gap and at % 16 != k % 16:
            at += 1
        tab[k] = (w["id_off"], w["seq_off"], w["qual_off"], at, len(r["id"]), off, n_seq, qoff, n_qual, (0 if trim is None else nat.FETCH_REC_TRIMMED) | (REVERSED if rev else 0))
        at += len(RF.written(r, trim, fastq)[0]) + (gap if k + 1 < len(plan) else 0)
    return tab, at


def _check(hl, twins, turned, plan, tab, out, sums, fastq):
    keep = RF._sentinel(out.size)
    mask = np.ones(out.size, dtype=bool)
    for k, (i, trim, rev) in enumerate(plan):
        exp, qual = RF.written((turned if rev else twins)[i], trim, fastq)
        a = int(tab[k]["out_off"])
        assert out[a:a + len(exp)].tobytes() == exp, (k, i, trim, rev)
        assert struct.pack("<d", float(sums[k])) == struct.pack("<d", hl.load().gr_sum_phred(qual, len(qual))), (k, i, trim, rev)
        mask[a:a + len(exp)] = False
    assert np.array_equal(out[mask], keep[mask]), "a byte outside the records' output ranges was written"
    assert mask.sum() > 0 and not mask[-1]


@pytest.mark.parametrize("fastq", [True, False], ids=["fastq-out", "fasta-out"])
def test_reversed_records_are_what_commit_sink_writes_for_the_aligned_twin(eng, native, hl, bam, fastq):
    comp, units, twins, turned, where, raw = bam
    assert native.FETCH_REC_REVERSED == REVERSED
    plan = _plan(twins)
    tab, cap = _table(native, twins, turned, where, plan, fastq)
    rev = [k for k, p in enumerate(plan) if p[2]]
    assert len(rev) * 2 == len(plan) and {int(tab[k]["out_off"]) % 16 for k in rev} == set(range(16))
    assert {len(twins[plan[k][0]]["bases"]) % 2 for k in rev if plan[k][1] is not None} == {0, 1}
    assert {int(tab[k]["seq_from"]) % 2 for k in rev} == {0, 1} and {(int(tab[k]["seq_from"]) + int(tab[k]["n_seq"])) % 2 for k in rev} == {0, 1}
    assert any(int(tab[k]["n_seq"]) > 65536 for k in rev)  # (more than one member)
    out = RF._sentinel(cap)
    flags = (native.FETCH_FASTQ if fastq else 0) | native.FETCH_BAM
    sums = eng.records_fetch(native.FETCH_UNITS_BGZF, comp, b"", units, tab, flags, out)
    _check(hl, twins, turned, plan, tab, out, sums, fastq)
    # the same records in another order of the table, packed back to back
    order = np.random.default_rng(5).permutation(len(plan))
    plan2 = [plan[i] for i in order]
    tab2, cap2 = _table(native, twins, turned, where, plan2, fastq, gap=0)
    out2 = RF._sentinel(cap2 + 5)
    sums2 = eng.records_fetch(native.FETCH_UNITS_BGZF, comp, b"", units, tab2, flags, out2, out_cap=cap2)
    assert out2[:cap2].tobytes() == b"".join(RF.written((turned if rev_ else twins)[i], t, fastq)[0] for i, t, rev_ in plan2)
    assert np.array_equal(out2[cap2:], RF._sentinel(cap2 + 5)[cap2:])
    assert [struct.pack("<d", float(s)) for s in sums2] == [struct.pack("<d", float(sums[i])) for i in order]


def test_the_flag_is_refused_without_a_launch_where_the_text_is_not_bam(eng, native, hl, bam):
    comp, units, twins, turned, where, raw = bam
    plan = [(3, None, False), (5, None, True), (4, None, False)]
    tab, cap = _table(native, twins, turned, where, plan, True, gap=0)
    before = RF._stats(eng)
    for flags in (native.FETCH_FASTQ, 0):
        out = RF._sentinel(cap + 16)
        with pytest.raises(native.GrpError) as e:
            eng.records_fetch(native.FETCH_UNITS_BGZF, comp, b"", units, tab, flags, out, out_cap=cap)
        assert e.value.code == native.GRP_ERR_INVALID and (e.value.bad_record, e.value.bad_unit) == (1, None) and "flag" in str(e.value), str(e.value)
        assert np.array_equal(out, RF._sentinel(cap + 16))
    with pytest.raises(native.GrpError) as e:  # ... and no other bit with it
        t = tab.copy()
        t[2]["flags"] = 4
        eng.records_fetch(native.FETCH_UNITS_BGZF, comp, b"", units, t, native.FETCH_FASTQ | native.FETCH_BAM, RF._sentinel(cap + 16), out_cap=cap)
    assert e.value.bad_record == 2
    assert RF._stats(eng) == before  # nothing was launched for any of them
    # a stored range that leaves the text is refused like any other
    t = tab.copy()
    t[1]["seq_from"] = 0xFFFFFFF0
    with pytest.raises(native.GrpError) as e:
        eng.records_fetch(native.FETCH_UNITS_BGZF, comp, b"", units, t, native.FETCH_FASTQ | native.FETCH_BAM, RF._sentinel(cap + 16), out_cap=cap)
    assert e.value.bad_record == 1 and RF._stats(eng) == before
    # the engine stays usable, and with GRP_FETCH_BAM the same table is served
    spaced, cap = _table(native, twins, turned, where, plan, True)
    out = RF._sentinel(cap)
    sums = eng.records_fetch(native.FETCH_UNITS_BGZF, comp, b"", units, spaced, native.FETCH_FASTQ | native.FETCH_BAM, out)
    _check(hl, twins, turned, plan, spaced, out, sums, True)
