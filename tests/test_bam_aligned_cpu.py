"""CPU: aligned BAM input read as `samtools fastq` reads it (GRP_BAM_ALIGNED=on).  The walk with its mask of accepted flags
(gr_bam_walk_ex) against a Python walk by the format's definition at every prefix of small streams, the twin decoder whole
and sliced, and the product's whole host program over the oracle engine: an aligned BAM file against its aligned twin —
the host reader, the chunked source with a Python stand-in for grp_bam_parse_ex, an engine without that entry point, and
GRP_RESIDENT=all with the host formatting the written records.  The aligned twin is written down from the SAM
specification and samtools' documented behaviour (tests/bam_aligned_cases.py); it is not pinned against samtools' output."""
import os
import subprocess
import sys

import pytest

import bam_aligned_cases as BA
import bam_cases as BC
import resident_runner as RR
import test_bam_cpu as TB

ROOT = TB.ROOT
ACCEPTS = (0, 0x10, 0x100, 0x800, 0x910)


def _rec(name, bases, quals=None, **kw):
    return dict(name=name, bases=bases, quals=bytes([(7 * i + len(bases)) % 60 for i in range(len(bases))]) if quals is None else quals, **kw)


SEC = _rec(b"sec", b"", cigar=(16,), flag=0x100)                             # a secondary record without bases
SEC_FF = _rec(b"sec ff", b"ACGTA", quals=b"\xff" * 5, flag=0x100 | 0x10)     # ... with absent qualities, on the reverse strand
SUP = _rec(b"sup", b"ACGTNACGT", flag=0x800 | 4, tags=b"SAZx\0")
REV_ODD = _rec(b"rev odd", b"ACGTNRYKMSWBDHV=A", flag=0x10, pad=9)           # every code, an odd length
REV_EVEN = _rec(b"rev_even", b"AACCGGTTACGTAC", flag=0x10 | 1 | 64, cigar=(32, 48))
REV_ONE = _rec(b"r1", b"C", flag=0x10)
REV_NONE = _rec(b"r0", b"", flag=0x10)
FWD = _rec(b"fwd", b"ACGTACGTAA", flag=4)
FWD2 = _rec(b"fwd2 x", b"TTGCA", flag=0x400 | 0x200)
STREAMS = {
    "skipped first": [SEC, FWD, REV_ODD, FWD2],
    "skipped last": [FWD, REV_EVEN, SUP],
    "two skipped in a row": [REV_ONE, SEC_FF, SUP, REV_NONE, FWD, SEC, SEC, REV_ODD],
    "a skipped record alone": [SEC_FF],
    "none of the three": [FWD, FWD2],
}


# ---- the walk ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", sorted(STREAMS))
def test_walk_ex_at_every_prefix_for_every_mask(native, what):
    from goldrush_amd import host

    body = b"".join(BC.record(**r) for r in STREAMS[what])
    for accept in ACCEPTS:
        for cut in range(len(body) + 1):
            for final in (False, True):
                want, used, bad, skipped = BA.walk(body[:cut], final, accept)
                rc, recs, n, consumed, bad_off, why, n_skipped = host.bam_walk_ex(body[:cut], final, accept, cap=16)
                assert (rc, n, consumed, n_skipped) == (0 if bad is None else -1, len(want), used, skipped), (accept, cut, final, why)
                if bad is not None:
                    assert bad_off == bad and why, (accept, cut, why)
                for w, r in zip(want, recs):
                    assert (r.off, r.seq_off, r.qual_off, r.end, r.l_seq, r.flag, r.id_len) == (w["off"], w["seq_off"], w["qual_off"], w["end"], w["l_seq"], w["flag"], len(w["name"]))
                if accept == 0:  # ... is today's walk
                    t = host.bam_walk(body[:cut], final, cap=16)
                    assert (rc, n, consumed, bad_off, why) == (t[0], t[2], t[3], t[4], t[5]), (cut, final)
    # what the full mask reads of the whole stream
    recs, used, bad, skipped = BA.walk(body, True, 0x910)
    assert bad is None and used == len(body) and (skipped, sum(1 for r in recs if r["flag"] & 0x10)) == BA.counts(STREAMS[what])


def test_walk_ex_refuses_what_its_mask_does_not_hold(native):
    from goldrush_amd import host

    good = b"".join(BC.record(**r) for r in (FWD, FWD2))
    for flag in (0x10, 0x100, 0x800, 0x110, 0x900, 0x910):
        buf = good + BC.record(**dict(FWD, flag=flag)) + BC.record(**FWD)
        for accept in ACCEPTS:
            rc, recs, n, used, bad_off, why, skipped = host.bam_walk_ex(buf, True, accept)
            if flag & ~accept:
                assert (rc, n, used, bad_off, skipped) == (-1, 2, len(good), len(good), 0) and "samtools fastq" in why and "GRP_BAM_ALIGNED=on" in why, (flag, accept, why)
            else:
                assert (rc, used, n, skipped) == (0, len(buf), 3 if flag & 0x900 else 4, 1 if flag & 0x900 else 0), (flag, accept)
    assert host.bam_walk_ex(good, True, 0x1)[0] == -1 and host.bam_walk_ex(good, True, 0x911)[0] == -1  # no mask of the walk's


@pytest.mark.parametrize("broken", [dict(block_size=31), dict(block_size=32 + 4 + 4 - 1), dict(l_seq=1000), dict(nul=False), dict(l_read_name=0, nul=False, name=b"")])
def test_a_skipped_record_that_is_broken_is_refused_at_its_offset(native, broken):
    from goldrush_amd import host

    good = b"".join(BC.record(**r) for r in (FWD, SEC, REV_ODD))
    buf = good + BC.record(**dict(dict(name=b"nm", bases=b"ACGT", quals=b"\xff" * 4, flag=0x100), **broken)) + BC.record(**FWD)
    for final in (False, True):
        rc, recs, n, used, bad_off, why, skipped = host.bam_walk_ex(buf, final, 0x910)
        assert (rc, n, used, bad_off, skipped) == (-1, 2, len(good), len(good), 1) and why, (broken, why)
        assert BA.walk(buf, final, 0x910)[1:] == (len(good), len(good), 1)
    # ... and one that ends the stream early is the truncation error, skipped or not
    cut = good + BC.record(**SUP)[:-3]
    assert host.bam_walk_ex(cut, False, 0x910)[:4:3] == (0, len(good)) and host.bam_walk_ex(cut, True, 0x910)[4] == len(good)
    assert "truncated" in host.bam_walk_ex(cut, True, 0x910)[5]


# ---- the twin decoder ----------------------------------------------------------------------------------------------------
def test_twin_decoder_whole_and_sliced(native):
    from goldrush_amd import host

    src = [REV_ODD, REV_EVEN, REV_ONE, REV_NONE, FWD, FWD2, _rec(b"long", b"ACGTTGCAN" * 9, flag=0x10), _rec(b"long2", b"CATG" * 16, flag=0x10 | 4)]
    body = b"".join(BC.record(**r) for r in src)
    rc, recs, n, used, _, _, skipped = host.bam_walk_ex(body, True, 0x910)
    assert rc == 0 and n == len(src) and used == len(body) and skipped == 0
    assert {r.l_seq % 2 for r in recs if r.flag & 0x10} == {0, 1}
    for r, s in zip(recs, src):
        seq, qual = BA.twin_read(s["bases"], s["quals"], s["flag"])
        assert host.bam_decode_twin(body, r) == (0, seq, qual), s["name"]
        L = len(seq)
        for start in sorted({0, 1, 2, 15, 16, 17, L // 2, max(L - 1, 0), L} & set(range(L + 1))):
            for k in sorted({0, 1, 2, 16, 33, L - start} & set(range(L - start + 1))):
                assert host.bam_decode_twin(body, r, start, k) == (0, seq[start:start + k], qual[start:start + k]), (s["name"], start, k)
        assert host.bam_decode_twin(body, r, L, 1)[0] == -1 and host.bam_decode_twin(body, r, L + 1, 0)[0] == -1  # a slice outside the record
        if not s["flag"] & 0x10:
            assert host.bam_decode(body, r) == (0, seq, qual)
    # a quality without a character, met only where the slice holds it
    b = BC.record(b"q", b"ACGTAC", b"\x01\x02\x5e\x03\x04\x05", flag=0x10)
    r = host.bam_walk_ex(b, True, 0x10)[1][0]
    assert host.bam_decode_twin(b, r)[0] == -1 and host.bam_decode_twin(b, r, 0, 3)[0] == 0 and host.bam_decode_twin(b, r, 3, 1)[0] == -1 and host.bam_decode_twin(b, r, 4, 2)[0] == 0


# ---- the whole host program ------------------------------------------------------------------------------------------------
# The runner of tests/resident_runner.py (the oracle engine, grp_bam_parse restated, zlib stand-ins for the inflates) with
# grp_bam_parse_ex restated beside it: the walk with the mask, a table entry per emitted record with GRP_FQ_REVERSED and the
# sums of the twin's quality line, the twin's bases behind fastq_pack.
_EX = '''
    n_ex = [0, 0, 0]  # calls, calls that consumed bytes and returned no record, records skipped

    def bam_parse_ex(ctx, bytes_p, n, final, accept, out_pp, nrec_p, used_p, bad_p, skipped_p):
        import bam_aligned_cases as BA
        n_ex[0] += 1
        buf = C.string_at(bytes_p, n) if n else b""
        recs, used, bad, skipped = BA.walk(buf, bool(final), accept)
        rows, seqs = [], []
        for r in recs if bad is None else []:
            packed = buf[r["seq_off"]:r["qual_off"]]
            stored = bytes(BC.CODES[(packed[j >> 1] >> (0 if j & 1 else 4)) & 15] for j in range(r["l_seq"]))
            raw = buf[r["qual_off"]:r["qual_off"] + r["l_seq"]]
            if any(q > 93 for q in raw):
                bad = r["off"]
                break
            seq, qual = BA.twin_read(stored, raw, r["flag"])
            half = qual[:len(qual) // 2]
            rows.append((r["off"] + 36, r["seq_off"], r["qual_off"], len(r["name"]), r["l_seq"], r["l_seq"], (1 if seq.translate(None, b"ACGT") else 0) | (2 if r["flag"] & 16 else 0),
                         hl.gr_sum_phred(qual, len(qual)), hl.gr_sum_phred(half, len(half)) if len(qual) >= 2 else 0.0))
            seqs.append(seq)
        if bad is not None:
            bad_p[0] = bad
            return -1
        n_ex[1] += 1 if used and not rows else 0
        n_ex[2] += skipped
        hnd = eng._next
        eng._next += 1
        mine[hnd] = (np.array(rows, dtype=rec_dtype), seqs)
        out_pp[0], nrec_p[0], used_p[0], skipped_p[0] = hnd, len(rows), used, skipped
        return 0

    keep_ex = host.BAM_PARSE_EX_FN(bam_parse_ex)
    ext.bam_parse_ex = keep_ex
'''
_KEEP = "    keep = [host.BAM_PARSE_FN(bam_parse)]\n"
_CHECK = '''
if os.environ.get("EXPECT_BAM_PARSE_EX"):
    want = int(os.environ["EXPECT_BAM_PARSE_EX"])  # the records a pass over the whole file skips
    assert n_ex[0] > 0 and n_bam[0] == 0 and eng.n_parse == 0 and n_ex[2] >= want and n_ex[2] % want == 0, (n_ex, n_bam, eng.n_parse)
    assert n_ex[1] > 0 or not os.environ.get("EXPECT_EMPTY_CHUNK"), n_ex
'''
_TAIL = '\nif os.environ.get("FETCH_OUT"):'
_FORMATTED = RR.RUNNER.format(root=ROOT)
assert _FORMATTED.count(_KEEP) == 1 and _FORMATTED.count(_TAIL) == 1
RUNNER = _FORMATTED.replace(_KEEP, _EX + _KEEP).replace(_TAIL, _CHECK + _TAIL)
RUNNER_OLD = RUNNER.replace("    ext.bam_parse_ex = keep_ex\n", "")  # an engine from before the entry point: bam_parse alone

COMMON, MODES, KEEP = TB.COMMON, TB.MODES, TB.KEEP


def _aligned_records():
    """the reads of tests/golden/tiny.fq as an aligned BAM file: every third record on the reverse strand (stored as the
    reverse complement of the read, as an aligner stores it), secondary and supplementary copies in between — two in a row,
    with and without bases, one with absent qualities — and one reversed record with other codes than A, C, G, T"""
    lines = open(os.path.join(TB.GOLD, "tiny.fq"), "rb").read().split(b"\n")
    recs = []
    for i in range(len(lines) // 4):
        name, seq, qual = lines[4 * i][1:], lines[4 * i + 1], lines[4 * i + 3]
        if i == 9:
            seq = seq[:5] + b"N" + seq[6:300] + b"R" + seq[301:]
        if i % 9 == 7:
            seq, qual = seq[:-1], qual[:-1]
        raw = bytes(q - 33 for q in qual)
        flag = (0, 1 | 64, 1 | 128 | 0x400)[i % 3]
        kw = dict(cigar=(16 * 7,) * (i % 3), tags=b"NMC\x02" * (i % 4), pad=i % 16)
        if i % 3 == 0:  # the aligner stored the reverse complement; the twin gives the read back
            recs.append(_rec(name, seq.translate(BA.COMPLEMENT)[::-1], raw[::-1], flag=flag | 0x10, **kw))
        else:
            recs.append(_rec(name, seq, raw, flag=flag | (4 if i % 2 else 0), **kw))
        if i % 5 == 1:
            recs.append(_rec(name, seq, raw, flag=0x100 | (0x10 if i % 2 else 0)))
            recs.append(_rec(name, seq[100:900], b"\xff" * 800, flag=0x800))
        if i == 20:
            recs.append(_rec(name, b"", flag=0x100))
    return recs


HEADER = dict(text=b"@HD\tVN:1.6\tSO:coordinate\n@CO\t" + b"c" * 70000 + b"\n", refs=[(b"chr1", 100000)])


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("bam_aligned_cpu")
    recs = _aligned_records()
    bam, _ = BC.bam_file(recs, sizes=(1, 65280, 7, 30011, 2, 513), **HEADER)
    paths = {"bam": str(d / "aligned.bam"), "twin": str(d / "aligned.fq")}
    open(paths["bam"], "wb").write(bam)
    open(paths["twin"], "wb").write(BA.aligned_twin(recs))
    (d / "runner.py").write_text(RUNNER)
    (d / "runner_old.py").write_text(RUNNER_OLD)
    n_skipped, n_reversed = BA.counts(recs)
    assert n_skipped >= 10 and n_reversed == 12 and any(r["flag"] & 0x10 and r["bases"].strip(b"ACGT") for r in recs if not r["flag"] & 0x900)
    return d, paths, recs


def _run(files, tag, mode, path, runner="runner.py", **env):
    d = files[0] / tag
    d.mkdir()
    e = dict(os.environ, OMP_NUM_THREADS="2", **env)
    for k in ("GRP_HOST_INGEST", "GRP_INGEST_CHUNK", "GRP_BATCH_RECORDS", "GRP_BGZF", "GRP_RESIDENT", "GRP_BAM_ALIGNED", "FETCH_STAND_IN", "FETCH_OUT"):
        if k not in env:
            e.pop(k, None)
    rp = subprocess.run([sys.executable, str(files[0] / runner)] + COMMON + MODES[mode] + ["-i", path, "-p", str(d / "out")], capture_output=True, text=True, timeout=900, env=e)
    return rp, {f: open(d / f, "rb").read() for f in sorted(os.listdir(d))}


def _pick(rp):
    return [l for l in rp.stderr.splitlines() if l.startswith(KEEP)]


def _said(rp):
    return [l for l in rp.stderr.splitlines() if l.startswith("GRP_BAM_ALIGNED:")]


def _line_is_right(files, rp):
    n_skipped, n_reversed = BA.counts(files[2])
    said = _said(rp)
    assert len(said) == 1, rp.stderr[-3000:]
    words = said[0].split()
    assert files[1]["bam"] in said[0] and str(n_skipped) in words and str(n_reversed) in words and words.index(str(n_skipped)) < words.index(str(n_reversed)), said


@pytest.fixture(scope="module")
def twin_runs(oracle, native, files):
    out = {}
    for mode in MODES:
        rp, fo = _run(files, "twin_" + mode, mode, files[1]["twin"], GRP_BAM_ALIGNED="on")
        assert rp.returncode == 0 and fo and any(fo.values()) and not _said(rp), rp.stderr[-3000:]
        out[mode] = (rp, fo)
    return out


@pytest.mark.parametrize("mode,env", [("silver", {}), ("golden", {"GRP_BATCH_RECORDS": "1"}), ("debug", {"GRP_BATCH_RECORDS": "11"})])
def test_host_reader_on_an_aligned_file_equals_its_aligned_twin(files, twin_runs, mode, env):
    rp, fo = _run(files, "host_%s" % mode, mode, files[1]["bam"], GRP_BAM_ALIGNED="on", **env)
    assert rp.returncode == 0, rp.stderr[-3000:]
    assert fo == twin_runs[mode][1]
    assert _pick(rp) == _pick(twin_runs[mode][0]) and len(_pick(rp)) > 5
    _line_is_right(files, rp)


@pytest.mark.parametrize("mode,env", [("silver", {}), ("golden", {"GRP_INGEST_CHUNK": "3000"}), ("silver", {"GRP_BGZF": "off", "GRP_INGEST_CHUNK": "2500", "EXPECT_EMPTY_CHUNK": "1"}),
                                      ("debug", {"GRP_INGEST_CHUNK": "9000"})])
def test_chunked_source_on_an_aligned_file_equals_its_aligned_twin(files, twin_runs, mode, env):
    """the chunked source with grp_bam_parse_ex restated in Python; through zlib (GRP_BGZF=off: a BGZF feed's chunk holds
    whole members) the chunks are small enough that a parse consumes skipped records alone and hands out no record"""
    rp, fo = _run(files, "chunked_%s_%d" % (mode, len(env)), mode, files[1]["bam"], GRP_BAM_ALIGNED="on", BAM_STAND_IN="1", GRP_RESIDENT="off",
                  EXPECT_BAM_PARSE_EX=str(BA.counts(files[2])[0]), **env)
    assert rp.returncode == 0, rp.stderr[-3000:]
    assert fo == twin_runs[mode][1]
    assert _pick(rp) == _pick(twin_runs[mode][0])
    _line_is_right(files, rp)


def test_an_engine_without_bam_parse_ex_takes_the_host_reader(files, twin_runs):
    """bam_parse, but no bam_parse_ex in the second table: with the switch on, the BAM file is read by the host"""
    rp, fo = _run(files, "old_engine", "golden", files[1]["bam"], runner="runner_old.py", GRP_BAM_ALIGNED="on", BAM_STAND_IN="1")
    assert rp.returncode == 0, rp.stderr[-3000:]
    assert fo == twin_runs["golden"][1] and _pick(rp) == _pick(twin_runs["golden"][0])
    _line_is_right(files, rp)


@pytest.mark.parametrize("mode,env", [("silver", {}), ("golden", {"GRP_INGEST_CHUNK": "20000"}), ("silver", {"GRP_INGEST_CHUNK": "3000"})])
def test_resident_all_with_the_host_formatting_the_records(files, twin_runs, mode, env):
    """GRP_RESIDENT=all: the reads stay on the device, the written records are fetched through the file's BGZF members and
    formatted by the host — reversed records through the twin decoder"""
    rp, fo = _run(files, "resident_%s_%d" % (mode, len(env)), mode, files[1]["bam"], GRP_BAM_ALIGNED="on", BAM_STAND_IN="1", GRP_RESIDENT="all", GRP_TRACE_INGEST="1", **env)
    assert rp.returncode == 0, rp.stderr[-3000:]
    assert "GRP_TRACE_INGEST resident fetch" in rp.stderr and "formatted on the host" in rp.stderr and "not kept on the device" not in rp.stderr, rp.stderr[-3000:]
    assert fo == twin_runs[mode][1]
    assert _pick(rp) == _pick(twin_runs[mode][0])
    _line_is_right(files, rp)


def test_the_switch(files, twin_runs):
    # unset and off: the aligned file is refused with today's message, at the first record that has one of the flags
    raw, hb, _ = BC.stream(files[2], **HEADER)
    first = hb + BA.walk(raw[hb:], True, 0)[2]
    for tag, env in (("unset", {}), ("off", {"GRP_BAM_ALIGNED": "off"}), ("off_chunked", {"GRP_BAM_ALIGNED": "off", "BAM_STAND_IN": "1"})):
        rp, _ = _run(files, "switch_" + tag, "golden", files[1]["bam"], **env)
        assert rp.returncode == 1 and "failed" in rp.stderr and not _said(rp), rp.stderr[-2000:]
        if "BAM_STAND_IN" not in env:
            assert "samtools fastq" in rp.stderr and "BAM record at byte %d " % first in rp.stderr, rp.stderr[-2000:]
    # any other value ends the run before the first pass, with a line that names the switch
    for bad in ("1", "ON", ""):
        rp, fo = _run(files, "switch_bad_%s" % (bad or "empty"), "golden", files[1]["twin"], GRP_BAM_ALIGNED=bad)
        assert rp.returncode == 1 and "GRP_BAM_ALIGNED" in rp.stderr and "Calculating" not in rp.stderr and not any(fo.values()), rp.stderr[-2000:]
    # on, and an unaligned file or text: nothing changes and nothing is said
    assert not _said(twin_runs["golden"][0])
