"""GPU: the FASTQ ingest kernels (csrc/grp_ingest.inc: k_nl_count / k_nl_scatter, k_fq_records, k_fq_phred, k_fq_pack) over
the edge sweeps of tests/ingest_cases.py, bit for bit against its host model: the whole record table (offsets, lengths,
flags, both Phred sums as bit patterns), the bytes consumed, and every packed word read back with grp_reads_download
against native.pack_reads.  tests/test_ingest_cases_cpu.py asserts that the sweeps hit the edges they are named after and
pins the model to the oracle's reader."""
import numpy as np
import pytest

import bam_cases as BC
import ingest_cases as IC
from helpers import default_seeds

pytestmark = pytest.mark.gpu

FRONT = 16 << 20  # GRP_FASTQ_PREFETCH_FRONT (include/grpath_ingest.h): a prefetched body lies this far into its device buffer


@pytest.fixture(scope="module")
def eng(native):
    e = native.Engine(22, 3, 1000, 1 << 20, default_seeds(3))
    yield e
    e.close()


@pytest.fixture(scope="module")
def sum_phred(native):
    from goldrush_amd import host

    hl = host.load()
    return IC.PhredCache(lambda q: hl.gr_sum_phred(q, len(q)))


@pytest.fixture(scope="module")
def s1(sum_phred):
    text, lengths, _ = IC.s1_text()
    table, used, stopped = IC.model_table(text, sum_phred)
    assert len(table) == len(lengths) == 343 * 16 and used == len(text) and not stopped and not table["flags"].any()
    return text, table


def _same_pack(native, eng, batch, strings):
    """reads_download of the batch == pack_reads of the strings: word_off, len and every word (the unused high bits of a
    read's last word are zero in pack_reads)"""
    packed, word_off, lens = eng.reads_download(batch)
    exp_packed, exp_word_off, exp_lens = native.pack_reads(strings)
    assert np.array_equal(word_off, exp_word_off) and np.array_equal(lens, exp_lens)
    d = np.flatnonzero(packed != exp_packed)
    if d.size:
        r = int(np.searchsorted(exp_word_off, d[0], side="right")) - 1
        raise AssertionError("%d words differ; the first: word %d of read %d (%d bases): %08x, expected %08x" % (d.size, d[0] - exp_word_off[r], r, exp_lens[r], packed[d[0]], exp_packed[d[0]]))
    return packed.size


def test_s1_every_length_at_every_alignment(native, eng, s1):
    text, exp = s1
    fq, rec, used, stopped = eng.fastq_parse(text)
    assert IC.table_diff(rec, exp) is None and (used, stopped) == (len(text), False)
    print("S1: %d records compared" % len(rec))
    assert len(rec) == len(exp) == 5488  # no record is skipped
    # one pack of all of them, those of 0 and of 1..15 bases included
    sel = np.arange(len(rec))
    batch = eng.fastq_pack(fq, sel, rec["seq_len"])
    n_words = _same_pack(native, eng, batch, IC.upper_strings(text, exp))
    print("S1: %d packed words compared" % n_words)
    batch.free()
    eng.fastq_free(fq)


def test_s1_uploaded_ahead_behind_a_tail_of_5_mod_16(native, s1, sum_phred):
    """grp_fastq_prefetch: the body goes up first, the parse gets [the carried tail | body] with a tail of 21 bytes, so the text
    begins 11 bytes into a 16-byte group of the device buffer (`lead`).  A record of 11 bytes in front of S1 puts a newline
    into that first group.  The same table, 11 bytes on, and the same packed words.  All three device buffers are first
    filled with a text whose bytes in front of that place are newlines: what lies in front of the text in its first group
    is no text, whatever it holds."""
    first = b"@a\nAC\n+\nII\n"
    text = first + s1[0]
    exp, exp_used, exp_stopped = IC.model_table(text, sum_phred)
    shifted = s1[1].copy()
    for f in ("id_off", "seq_off", "qual_off"):
        shifted[f] += len(first)
    assert IC.table_diff(exp[1:], shifted) is None and b"\n" in text[:5]
    eng = native.Engine(22, 3, 1000, 1 << 20, default_seeds(3))
    tail = 21
    prime = b"@p\n" + b"A" * (FRONT - 256 - 3) + b"\n" * 256 + b"A" * (len(text) + 64)
    for _ in range(3):
        fq, rec, _, stopped = eng.fastq_parse(prime)
        assert stopped and len(rec) == 1 and rec[0]["seq_len"] == FRONT - 256 - 3
        eng.fastq_free(fq)
    room = 4096
    buf = np.zeros(room + len(text) - tail, dtype=np.uint8)
    buf[room:] = np.frombuffer(text[tail:], dtype=np.uint8)
    assert eng.fastq_prefetch(buf[room:], buf.size - room)
    buf[room - tail:room] = np.frombuffer(text[:tail], dtype=np.uint8)
    view = buf[room - tail:]
    fq, rec, used, stopped = eng.fastq_parse_at(view, view.size)
    assert IC.table_diff(rec, exp) is None, IC.table_diff(rec, exp)
    assert (used, stopped) == (exp_used, exp_stopped) == (len(text), False) and len(rec) == 5489
    batch = eng.fastq_pack(fq, np.arange(len(rec)), rec["seq_len"])
    _same_pack(native, eng, batch, IC.upper_strings(text, exp))
    eng.fastq_free(fq)
    assert eng.fastq_prefetch(None, 0)
    eng.close()


def test_s2_one_bad_byte_per_record(native, eng, sum_phred):
    text, cases = IC.s2_text()
    exp, exp_used, exp_stopped = IC.model_table(text, sum_phred)
    fq, rec, used, stopped = eng.fastq_parse(text)
    assert IC.table_diff(rec, exp) is None and (used, stopped) == (exp_used, exp_stopped) == (len(text), False)
    print("S2: %d records compared, %d of them with a planted byte" % (len(rec), len(cases)))
    assert len(rec) == len(cases) + len(np.unique(cases["twin"])) and len(cases) > 20_000
    # the bad record is flagged and its clean twin is not; a white-space byte at the end is trimmed instead
    trimmed = np.isin(cases["byte"], [32, 9, 13]) & (cases["pos"] == cases["len"] - 1)
    assert np.array_equal(rec["flags"][cases["rec"]], np.where(trimmed, 0, 1)) and not rec["flags"][cases["twin"]].any()
    assert np.array_equal(rec["seq_len"][cases["rec"]], cases["len"] - trimmed) and np.array_equal(rec["seq_len"][cases["twin"]], cases["len"])
    assert 0 < trimmed.sum() < 1000
    # packing a flagged record is refused, alone or among clean ones; the clean ones pack like the strings
    flagged = np.flatnonzero(rec["flags"] & 1)
    for i in flagged[:: len(flagged) // 40]:
        for sel in ([i], sorted({0, int(i), len(rec) - 1} | {int(cases["twin"][0])})):
            with pytest.raises(native.GrpError) as e:
                eng.fastq_pack(fq, sel, rec["seq_len"][sel])
            assert e.value.code == native.GRP_ERR_INVALID
    clean = np.flatnonzero((rec["flags"] & 1) == 0)
    batch = eng.fastq_pack(fq, clean, rec["seq_len"][clean])
    strings = IC.upper_strings(text, exp)
    _same_pack(native, eng, batch, [strings[i] for i in clean])
    batch.free()
    eng.fastq_free(fq)


def test_s3_degenerate_lines(native, eng, sum_phred):
    text, what = IC.s3_text()
    exp, exp_used, exp_stopped = IC.model_table(text, sum_phred)
    fq, rec, used, stopped = eng.fastq_parse(text)
    assert IC.table_diff(rec, exp) is None, IC.table_diff(rec, exp)
    assert (used, stopped) == (exp_used, exp_stopped) == (len(text), False) and len(rec) == len(what)
    print("S3: %d records compared" % len(rec))
    clean = np.flatnonzero((rec["flags"] & 1) == 0)
    batch = eng.fastq_pack(fq, clean, rec["seq_len"][clean])
    strings = IC.upper_strings(text, exp)
    _same_pack(native, eng, batch, [strings[i] for i in clean])
    batch.free()
    eng.fastq_free(fq)
    # the same with CR LF line ends, and cut in front of its last newline
    for other in (text.replace(b"\n", b"\r\n"), text[:-1]):
        exp, exp_used, exp_stopped = IC.model_table(other, sum_phred)
        fq, rec, used, stopped = eng.fastq_parse(other)
        assert IC.table_diff(rec, exp) is None and (used, stopped) == (exp_used, exp_stopped) == (len(other), False) and len(rec) == len(what)
        eng.fastq_free(fq)


def test_s4_newlines_round_the_block_boundaries(native, eng, sum_phred):
    cases = IC.s4_small()
    records = expected = 0
    for what, text, final in cases:
        exp, exp_used, exp_stopped = IC.model_table(text, sum_phred, final)
        fq, rec, used, stopped = eng.fastq_parse(text, final_chunk=final)
        assert IC.table_diff(rec, exp) is None, what + ": " + IC.table_diff(rec, exp)
        assert (used, stopped) == (exp_used, exp_stopped), what
        records += len(rec)
        expected += len(exp)
        eng.fastq_free(fq)
    print("S4: %d texts, %d records compared" % (len(cases), records))
    assert len(cases) == 3 * len(IC.S4_CUTS) + 6 and records == expected > 80_000


def test_s4_eight_mebibytes_two_carries_of_the_scan(native, eng, sum_phred):
    text = IC.s4_big()
    assert len(text) > 2 * IC.SCAN_ROUND * IC.NL_BLOCK
    exp, exp_used, exp_stopped = IC.table_np(text, sum_phred)
    fq, rec, used, stopped = eng.fastq_parse(text)
    assert IC.table_diff(rec, exp) is None and (used, stopped) == (exp_used, exp_stopped) == (len(text), False)
    print("S4, 8 MiB: %d records compared" % len(rec))
    assert len(rec) == len(exp) > 4000
    eng.fastq_free(fq)


@pytest.mark.parametrize("kind", ["fastq", "bam"])
def test_a_record_of_length_zero_in_a_selection(native, eng, kind):
    """grp_fastq_pack takes a record without bases like any other (reads_index: no word, no tile, no fill chunk): its
    word_off is its neighbour's, its len is 0 — for a FASTQ and for a BAM handle alike"""
    seqs = [b"", b"ACGTACGTACGTACGTA", b"", b"", b"GATTACA", b""]
    if kind == "fastq":
        fq, rec, _, _ = eng.fastq_parse(b"".join(b"@z%d\n" % i + s + b"\n+\n" + b"I" * len(s) + b"\n" for i, s in enumerate(seqs)))
    else:
        fq, rec, _ = eng.bam_parse(b"".join(BC.record(b"z%d" % i, s, b"\x28" * len(s)) for i, s in enumerate(seqs)))
    assert list(rec["seq_len"]) == [len(s) for s in seqs] and not rec["flags"].any()
    for sel in ([0], [2, 3], [0, 2, 3, 5], list(range(6)), [1, 2], [3, 4]):
        batch = eng.fastq_pack(fq, sel, rec["seq_len"][sel])
        packed, word_off, lens = eng.reads_download(batch)
        exp_packed, exp_word_off, exp_lens = native.pack_reads([seqs[i] for i in sel])
        assert np.array_equal(packed, exp_packed) and np.array_equal(word_off, exp_word_off) and np.array_equal(lens, exp_lens), sel
        assert packed.size == sum((len(seqs[i]) + 15) // 16 for i in sel) and list(batch.tile0) == [0] * (len(sel) + 1)
        batch.free()
    eng.fastq_free(fq)
