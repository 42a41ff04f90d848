"""GPU: the BAM ingest kernels (csrc/grp_ingest.inc: k_bam_records, k_fq_phred forwards and backwards, k_bam_pack in both
forms; the word functions of csrc/host/gr_bam.hpp) over the edge sweeps of tests/bam_cases.py, bit for bit against the
model of tests/bam_aligned_cases.py: the whole record table, and every packed word read back with grp_reads_download
against native.pack_reads of the twin's strings.  Each sweep runs once on the forward strand (flag 4) and once reversed
(flag 0x10 under accept = 0x10).  tests/test_ingest_cases_cpu.py asserts what the sweeps cover."""
import numpy as np
import pytest

import bam_aligned_cases as BA
import bam_cases as BC
import ingest_cases as IC
from helpers import default_seeds
from test_gpu_ingest_edges import _same_pack

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(native):
    e = native.Engine(22, 4, 25, 1 << 20, default_seeds(4))
    yield e
    e.close()


@pytest.fixture(scope="module")
def sum_phred(native):
    from goldrush_amd import host

    hl = host.load()
    return IC.PhredCache(lambda q: hl.gr_sum_phred(q, len(q)))


def _parse(eng, body, flag):
    if flag & 0x10:
        fq, rec, used, skipped = eng.bam_parse(body, accept=0x10)
        assert skipped == 0
    else:
        fq, rec, used = eng.bam_parse(body)
    assert used == len(body)
    return fq, rec


def _twin_strings(records):
    return [BA.twin_read(r["bases"], r["quals"], r["flag"])[0] for r in records]


@pytest.mark.parametrize("flag", [4, 0x10])
def test_every_length_at_every_alignment(native, eng, sum_phred, flag):
    records = [dict(r, flag=flag) for r in BC.sweep_records()]
    body = b"".join(BC.record(**r) for r in records)
    exp = BA.model_table(body, records, flag & 0x10, sum_phred)
    fq, rec = _parse(eng, body, flag)
    assert IC.table_diff(rec, exp) is None, IC.table_diff(rec, exp)
    print("BAM lengths x alignments, flag 0x%x: %d records compared" % (flag, len(rec)))
    assert len(rec) == len(records) == 16 * 347 and not (rec["flags"] & 1).any() and ((rec["flags"] & 2) != 0).all() == bool(flag & 0x10)
    # one pack of all of them: the padding code behind an odd length (all 16 values) reaches no word, forward or reversed
    batch = eng.fastq_pack(fq, np.arange(len(rec)), rec["seq_len"])
    n_words = _same_pack(native, eng, batch, _twin_strings(records))
    print("BAM lengths x alignments, flag 0x%x: %d packed words compared" % (flag, n_words))
    batch.free()
    eng.fastq_free(fq)


@pytest.mark.parametrize("flag", [4, 0x10])
def test_one_bad_code_per_record(native, eng, sum_phred, flag):
    records, cases = BC.bad_code_records()
    records = [dict(r, flag=flag) for r in records]
    body = b"".join(BC.record(**r) for r in records)
    exp = BA.model_table(body, records, flag & 0x10, sum_phred)
    fq, rec = _parse(eng, body, flag)
    assert IC.table_diff(rec, exp) is None, IC.table_diff(rec, exp)
    print("BAM bad codes, flag 0x%x: %d records compared, %d of them with a planted code" % (flag, len(rec), len(cases)))
    assert len(rec) == len(records) == len(cases) + len(np.unique(cases["twin"])) and len(cases) > 20_000
    # the bad record is flagged, its clean twin is not — whatever padding code stands behind an odd length
    assert (rec["flags"][cases["rec"]] & 1).all() and not (rec["flags"][cases["twin"]] & 1).any()
    flagged = np.flatnonzero(rec["flags"] & 1)
    assert len(flagged) == len(cases)
    for i in flagged[:: len(flagged) // 40]:
        for sel in ([i], sorted({0, int(i), len(rec) - 1})):
            with pytest.raises(native.GrpError) as e:
                eng.fastq_pack(fq, sel, rec["seq_len"][sel])
            assert e.value.code == native.GRP_ERR_INVALID
    clean = np.flatnonzero((rec["flags"] & 1) == 0)
    batch = eng.fastq_pack(fq, clean, rec["seq_len"][clean])
    strings = _twin_strings(records)
    _same_pack(native, eng, batch, [strings[i] for i in clean])
    batch.free()
    eng.fastq_free(fq)


def test_the_range_test_over_the_qualities(native, eng):
    """93 parses at every swept position; 94, 127, 128 and 0xFF are refused, with bad_offset on that record: one byte of one
    shared stream is patched per case"""
    records, at = BC.qual_sweep_records()
    body = b"".join(BC.record(**r) for r in records)
    walked, _, _, _ = BA.walk(body, True, 0x10)
    where = np.array([walked[c["rec"]]["qual_off"] + int(c["pos"]) for c in at])
    buf = np.frombuffer(body, dtype=np.uint8).copy()
    fq, ref, used, _ = eng.bam_parse(buf, accept=0x10)
    eng.fastq_free(fq)
    assert used == len(body) and len(ref) == len(records)
    buf[where] = 93
    fq, rec, used, _ = eng.bam_parse(buf, accept=0x10)
    eng.fastq_free(fq)
    assert used == len(body) and all(np.array_equal(rec[f], ref[f]) for f in ("id_off", "seq_off", "qual_off", "id_len", "seq_len", "qual_len", "flags"))
    assert (rec["phred_sum"] != ref["phred_sum"]).any()
    n = 0
    for c, w in zip(at, where):
        for q in BC.QUAL_REFUSED:
            buf[:] = np.frombuffer(body, dtype=np.uint8)
            buf[w] = q
            with pytest.raises(native.GrpError) as e:
                eng.bam_parse(buf, accept=0x10)
            assert e.value.code == native.GRP_ERR_INVALID and e.value.bad_offset == walked[c["rec"]]["off"], (c, q, e.value.bad_offset)
            n += 1
    print("BAM qualities: %d positions, %d refusals compared" % (len(at), n))
    assert n == 4 * len(at) and len(at) > 100
    fq, rec, used, _ = eng.bam_parse(body, accept=0x10)  # the engine stays usable
    assert np.array_equal(rec, ref)
    eng.fastq_free(fq)
