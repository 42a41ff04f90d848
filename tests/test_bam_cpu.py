"""CPU: the host side of unaligned BAM input.  gr_bam_header and the shared walk (csrc/host/gr_bam.hpp) against a Python
restatement of the format, the decoder against the twin's text, and the product's whole host program over the oracle
engine: a BAM file against its FASTQ twin — the host reader, and the chunked source with a Python stand-in for
grp_bam_parse in the second engine table."""
import os
import subprocess
import sys
import textwrap

import pytest

import bam_cases as BC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _rec(name, bases, quals=None, **kw):
    return dict(name=name, bases=bases, quals=bytes([30] * len(bases)) if quals is None else quals, **kw)


SMALL = [_rec(b"r0", b"ACGTACGTA", pad=7), _rec(b"read one  comment", b"", cigar=(16, 32)), _rec(b"x" * 40, b"ACGTN=RYACGTAC", tags=b"NMC\x05zz"),
         _rec(b"p", b"A", flag=4 | 1 | 64, quals=b"\x00"), _rec(b"q\tr", b"ACGT" * 40 + b"C", quals=bytes([93] * 161))]


# ---- the header and the walk ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l_text,n_ref", [(0, 0), (0, 3), (200_000, 0), (200_000, 3)])
def test_header_of_any_length(native, l_text, n_ref):
    from goldrush_amd import host

    refs = [(b"chr%d" % i * (i + 1), 1000 * i) for i in range(n_ref)]
    raw, hb, _ = BC.stream(SMALL, text=b"@HD\tVN:1.6\n".ljust(l_text, b"x")[:l_text], refs=refs)
    assert host.bam_header(raw) == (1, hb)
    assert host.bam_header(raw[:hb]) == (1, hb)
    for cut in (0, 1, 3, 4, 7, 8, 11, hb - 1, max(hb - 5, 0), l_text + 8, l_text + 11):
        if cut < hb:
            assert host.bam_header(raw[:cut])[0] == 0, cut
    for bad in (b"@read0\nACGT\n", b"BAM\2" + raw[4:], b"\x1f\x8b", b"BAM\1\xff\xff\xff\xff"):
        assert host.bam_header(bad)[0] == -1, bad


def test_every_prefix_of_a_small_stream(native):
    """'need more' up to each boundary, never a wrong answer: the header function and the walk at every length"""
    from goldrush_amd import host

    raw, hb, _ = BC.stream(SMALL, text=b"@CO\tsmall\n", refs=[(b"ref", 5)])
    for cut in range(hb):
        assert host.bam_header(raw[:cut])[0] == 0, cut
    body = raw[hb:]
    want_all, _, _ = BC.walk(body)
    assert len(want_all) == len(SMALL) and want_all[-1]["end"] == len(body)
    for cut in range(len(body) + 1):
        for final in (False, True):
            want, used, bad = BC.walk(body[:cut], final)
            rc, recs, n, consumed, bad_off, why = host.bam_walk(body[:cut], final)
            assert (rc, n, consumed) == (0 if bad is None else -1, len(want), used), (cut, final, why)
            if bad is not None:
                assert bad_off == bad and "truncated" in why, (cut, why)
            for w, r in zip(want, recs):
                assert (r.off, r.seq_off, r.qual_off, r.end, r.l_seq, r.flag, r.id_len) == (w["off"], w["seq_off"], w["qual_off"], w["end"], w["l_seq"], w["flag"], len(w["name"]))
                assert body[r.name_off:r.name_off + r.id_len] == w["name"]


def test_decoder_gives_the_twins_text(native):
    from goldrush_amd import host

    raw, hb, twin = BC.stream(SMALL)
    body = raw[hb:]
    rc, recs, n, used, _, _ = host.bam_walk(body)
    assert rc == 0 and n == len(SMALL) and used == len(body)
    lines = twin.split(b"\n")
    for i, r in enumerate(recs):
        rc, seq, qual = host.bam_decode(body, r)
        assert rc == 0 and seq == lines[4 * i + 1] and qual == lines[4 * i + 3]
        assert lines[4 * i] == b"@" + SMALL[i]["name"] and lines[4 * i].split()[0][1:] == body[r.name_off:r.name_off + r.id_len]
    for q in (b"\xff" * 4, b"\x00\x5e\x00\x00"):  # absent qualities, a quality of 94
        b = BC.record(b"n", b"ACGT", q)
        rc, recs, *_ = host.bam_walk(b)
        assert rc == 0 and host.bam_decode(b, recs[0])[0] == -1


REFUSALS = {
    "block_size below the fixed part": dict(block_size=31),
    "block_size below the fields": dict(block_size=32 + 3 + 2 + 4 - 1),
    "l_seq beyond the block": dict(l_seq=1000),
    "l_read_name 0": dict(l_read_name=0, nul=False, name=b""),
    "name without NUL": dict(nul=False),
    "reverse strand": dict(flag=16),
    "secondary": dict(flag=256 | 4),
    "supplementary": dict(flag=2048),
}


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_each_refusal_at_its_exact_offset(native, what):
    from goldrush_amd import host

    good = b"".join(BC.record(**r) for r in SMALL[:3])
    bad = BC.record(**dict(dict(name=b"nm", bases=b"ACGT", quals=b"\x10" * 4), **REFUSALS[what]))
    tail = BC.record(**SMALL[3])
    buf = good + bad + tail
    assert BC.walk(buf)[2] == len(good)
    for final in (False, True):
        rc, recs, n, used, bad_off, why = host.bam_walk(buf, final)
        assert rc == -1 and bad_off == len(good) and n == 3 and why, (what, why)
        if "strand" in what or "ary" in what:
            assert "samtools fastq" in why
    assert host.bam_walk(good + tail)[0] == 0
    # paired-end flags are not refused, an ending inside a record is — but only at the end of the stream
    assert host.bam_walk(BC.record(b"p", b"AC", b"\x01\x02", flag=1 | 64 | 128 | 4 | 8 | 32))[0] == 0
    assert host.bam_walk(buf[:len(good) - 1], False)[:1] == (0,) and host.bam_walk(buf[:len(good) - 1], True)[4] == len(b"".join(BC.record(**r) for r in SMALL[:2]))


# ---- the whole host program ------------------------------------------------------------------------------------------------
RUNNER = textwrap.dedent("""
    import ctypes as C, os, sys
    import numpy as np
    sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests")); sys.path.insert(0, os.path.join({root!r}, "oracle"))
    import orc
    import bam_cases as BC
    from goldrush_amd import host
    from oracle_engine import OracleCliEngine
    stand_in = bool(os.environ.get("BAM_STAND_IN"))
    eng = OracleCliEngine(orc, ingest=stand_in)
    ext = host.grp_engine_ext()
    ext.struct_size = C.sizeof(host.grp_engine_ext)
    n_bam = [0]
    if stand_in:
        # grp_bam_parse restated (include/grpath_ingest.h) beside the oracle engine's FASTQ ingest: the walk by the format's
        # definition, the table with offsets from `bytes`, the sums of the twin's quality line; its handles are served by
        # wrappers around the table's fastq_records / fastq_pack / fastq_free
        rec_dtype = np.dtype([("id_off", "<u8"), ("seq_off", "<u8"), ("qual_off", "<u8"), ("id_len", "<u4"), ("seq_len", "<u4"),
                              ("qual_len", "<u4"), ("flags", "<u4"), ("phred_sum", "<f8"), ("phred_first", "<f8")])
        mine, hl = {{}}, host.load()
        orig = {{n: dict(host.VT_TYPES)[n](C.cast(getattr(eng.vt, n), C.c_void_p).value) for n in ("fastq_records", "fastq_pack", "fastq_free")}}  # (by value: a field read is a view of the table)

        def bam_parse(ctx, bytes_p, n, final, out_pp, nrec_p, used_p, bad_p):
            n_bam[0] += 1
            buf = C.string_at(bytes_p, n) if n else b""
            recs, used, bad = BC.walk(buf, bool(final))
            rows, seqs = [], []
            for r in recs if bad is None else []:
                packed = buf[r["seq_off"]:r["qual_off"]]
                seq = bytes(BC.CODES[(packed[j >> 1] >> (0 if j & 1 else 4)) & 15] for j in range(r["l_seq"]))
                raw = buf[r["qual_off"]:r["qual_off"] + r["l_seq"]]
                if any(q > 93 for q in raw):
                    bad = r["off"]
                    break
                qual = bytes(q + 33 for q in raw)
                half = qual[:len(qual) // 2]
                rows.append((r["off"] + 36, r["seq_off"], r["qual_off"], len(r["name"]), r["l_seq"], r["l_seq"], 1 if seq.translate(None, b"ACGT") else 0,
                             hl.gr_sum_phred(qual, len(qual)), hl.gr_sum_phred(half, len(half)) if len(qual) >= 2 else 0.0))
                seqs.append(seq)
            if bad is not None:
                bad_p[0] = bad
                return -1
            hnd = eng._next
            eng._next += 1
            mine[hnd] = (np.array(rows, dtype=rec_dtype), seqs)
            out_pp[0], nrec_p[0], used_p[0] = hnd, len(rows), used
            return 0

        def fastq_records(fq, out_p):
            if fq not in mine:
                return orig["fastq_records"](fq, out_p)
            C.memmove(out_p, mine[fq][0].ctypes.data, mine[fq][0].nbytes)
            return 0

        def fastq_pack(ctx, fq, sel_p, n_sel, out_pp):
            if fq not in mine:
                return orig["fastq_pack"](ctx, fq, sel_p, n_sel, out_pp)
            sel = np.ctypeslib.as_array(C.cast(sel_p, C.POINTER(C.c_uint32)), shape=(max(n_sel, 1),))[:n_sel]
            hnd = eng._next
            eng._next += 1
            eng.batches[hnd] = [mine[fq][1][int(i)] for i in sel]
            out_pp[0] = hnd
            return 0

        def fastq_free(fq):
            if mine.pop(fq, None) is None:
                orig["fastq_free"](fq)

        keep = [host.BAM_PARSE_FN(bam_parse)]
        ext.bam_parse = keep[0]
        for name, fn in (("fastq_records", fastq_records), ("fastq_pack", fastq_pack), ("fastq_free", fastq_free)):
            keep.append(dict(host.VT_TYPES)[name](fn))
            setattr(eng.vt, name, keep[-1])
    args = [b"goldrush_path"] + [a.encode() for a in sys.argv[1:]]
    arr = (C.c_char_p * (len(args) + 1))(*args, None)
    rc = host.load().gr_path_main_ext(len(args), arr, C.byref(eng.vt), C.byref(ext))
    sys.stdout.flush(); sys.stderr.flush()
    if os.environ.get("EXPECT_BAM_PARSE"):
        assert n_bam[0] > 0 and eng.n_parse == 0, (n_bam, eng.n_parse)
    os._exit(rc)
""")

COMMON = ["-k22", "-w16", "-t500", "-u5", "-a1", "-o0.1", "-h3", "-j2", "-d5", "-x10", "-s1011011110110111101101", "-g60000", "-b4", "-H600000", "--verbose"]
MODES = {"silver": ["-P0", "-r0.9", "--silver_path", "-M3", "-m1500"], "golden": ["-P12", "-m0"], "debug": ["-P12", "-m2500", "--debug"]}
KEEP = ("Expected entries", "Total expected entries", "\toccupancy", "Visited", "Saw:", "Assigned:", "Unassigned:", "Total queries", "Total hits", "Total misses", "Num reads", "m_filterSize",
        "\texpected hash space", "\tminimum average phred", "num_", "Total reads skipped", "name:", "num tiles:", "too short", "skipping:", "hairpin or quality", "phred avg:", "phred delta:",
        "Number of reads used", "Median array:")


def _tiny_records():
    """the reads of tests/golden/tiny.fq as BAM records, and among them what FASTQ has no trouble with and BAM might: a
    record without bases, one with other codes than A, C, G, T, names with a comment, CIGAR operations and tags"""
    lines = open(os.path.join(GOLD, "tiny.fq"), "rb").read().split(b"\n")
    recs = []
    for i in range(len(lines) // 4):
        name, seq, qual = lines[4 * i][1:], lines[4 * i + 1], lines[4 * i + 3]
        if i % 9 == 4:
            seq = seq[:700] + b"N" + seq[701:]
        if i % 9 == 7:
            seq = seq[:-1]
            qual = qual[:-1]
        recs.append(_rec(name + (b" zm:i:%d" % i if i % 4 == 1 else b""), seq, bytes(q - 33 for q in qual), cigar=(16,) * (i % 3), tags=b"rqf\0\0\x80\x3f" * (i % 5), pad=i % 16, flag=4 | (77 if i % 2 else 0)))
        if i == 10:
            recs.append(_rec(b"empty", b""))
    return recs


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("bam_cpu")
    recs = _tiny_records()
    bam, twin = BC.bam_file(recs, sizes=(1, 65280, 7, 30011, 2, 513), text=b"@HD\tVN:1.6\tSO:unknown\n" + b"@CO\t" + b"c" * 70000 + b"\n", refs=[(b"chr1", 1000)])
    paths = {"bam": str(d / "reads.bam"), "twin": str(d / "reads.fq")}
    open(paths["bam"], "wb").write(bam)
    open(paths["twin"], "wb").write(twin)
    raw, hb, _ = BC.stream(recs)
    paths["plain_bam"] = str(d / "not_compressed.bam")  # BAM\\1 at the file's first byte: the same format, whatever the name
    open(paths["plain_bam"], "wb").write(raw)
    (d / "runner.py").write_text(RUNNER.format(root=ROOT))
    return d, paths, recs


def _run(files, tag, mode, path, **env):
    d = files[0] / tag
    d.mkdir()
    e = dict(os.environ, OMP_NUM_THREADS="2", **env)
    for k in ("GRP_HOST_INGEST", "GRP_INGEST_CHUNK", "GRP_BATCH_RECORDS", "GRP_BGZF"):
        if k not in env:
            e.pop(k, None)
    rp = subprocess.run([sys.executable, str(files[0] / "runner.py")] + COMMON + MODES[mode] + ["-i", path, "-p", str(d / "out")], capture_output=True, text=True, timeout=900, env=e)
    return rp, {f: open(d / f, "rb").read() for f in sorted(os.listdir(d))}


def _pick(rp):
    return [l for l in rp.stderr.splitlines() if l.startswith(KEEP)]


@pytest.fixture(scope="module")
def twin_runs(oracle, native, files):
    out = {}
    for mode in MODES:
        rp, fo = _run(files, "twin_" + mode, mode, files[1]["twin"])
        assert rp.returncode == 0 and fo and any(fo.values()), rp.stderr[-3000:]
        out[mode] = (rp, fo)
    return out


@pytest.mark.parametrize("mode,env", [("silver", {}), ("golden", {}), ("silver", {"GRP_BATCH_RECORDS": "7", "GRP_INGEST_CHUNK": "3000"}), ("golden", {"GRP_BATCH_RECORDS": "1"}),
                                      ("debug", {"GRP_BATCH_RECORDS": "11"})])
def test_host_reader_on_a_bam_file_equals_its_twin(files, twin_runs, mode, env):
    """the oracle engine has no ingest entry points: the host reader hands FastqStream's consumers the twin's records"""
    rp, fo = _run(files, "host_%s_%d" % (mode, len(env)), mode, files[1]["bam"], **env)
    assert rp.returncode == 0, rp.stderr[-3000:]
    assert fo == twin_runs[mode][1]
    assert _pick(rp) == _pick(twin_runs[mode][0]) and len(_pick(rp)) > 5


def test_bam_that_is_not_compressed_is_bam_whatever_its_name(files, twin_runs):
    rp, fo = _run(files, "plain_bam", "golden", files[1]["plain_bam"])
    assert rp.returncode == 0, rp.stderr[-3000:]
    assert fo == twin_runs["golden"][1] and _pick(rp) == _pick(twin_runs["golden"][0])


@pytest.mark.parametrize("mode,env", [("silver", {}), ("golden", {"GRP_INGEST_CHUNK": "3000"}), ("silver", {"GRP_INGEST_CHUNK": "70001"}), ("golden", {"GRP_BGZF": "off", "GRP_INGEST_CHUNK": "20000"}),
                                      ("debug", {"GRP_INGEST_CHUNK": "9000"})])
def test_chunked_source_on_a_bam_file_equals_its_twin(files, twin_runs, mode, env):
    """the chunked source (reader thread, carried tails, a header that spans chunks, records longer than a chunk) with
    grp_bam_parse restated in Python where fastq_parse stands for text"""
    rp, fo = _run(files, "chunked_%s_%d" % (mode, len(env)), mode, files[1]["bam"], BAM_STAND_IN="1", EXPECT_BAM_PARSE="1", **env)
    assert rp.returncode == 0, rp.stderr[-3000:]
    assert fo == twin_runs[mode][1]
    assert _pick(rp) == _pick(twin_runs[mode][0])


def test_an_engine_without_bam_parse_takes_the_host_reader(files, twin_runs):
    """ingest entry points, but no bam_parse in the second table: a BAM file is read by the host, text still by the engine"""
    d, paths, _ = files
    script = d / "runner_old.py"
    script.write_text(RUNNER.format(root=ROOT).replace("ext.bam_parse = keep[0]", "pass"))
    for tag, path in (("old_bam", paths["bam"]), ("old_twin", paths["twin"])):
        o = d / tag
        o.mkdir()
        rp = subprocess.run([sys.executable, str(script)] + COMMON + MODES["golden"] + ["-i", path, "-p", str(o / "out")], capture_output=True, text=True, timeout=900,
                            env=dict(os.environ, OMP_NUM_THREADS="2", BAM_STAND_IN="1"))
        assert rp.returncode == 0, rp.stderr[-3000:]
        assert {f: open(o / f, "rb").read() for f in sorted(os.listdir(o))} == twin_runs["golden"][1]


def _damaged(recs, what):
    recs = [dict(r) for r in recs]
    if what == "flag 16":
        recs[20]["flag"] = 16
    elif what == "absent qualities":
        recs[20]["quals"] = b"\xff" * len(recs[20]["bases"])
    elif what == "quality 94":
        recs[20]["quals"] = recs[20]["quals"][:-1] + b"\x5e"
    elif what == "name without NUL":
        recs[20]["nul"] = False
    elif what == "block_size":
        recs[20]["block_size"] = 40
    return recs


@pytest.mark.parametrize("what", ["flag 16", "absent qualities", "quality 94", "name without NUL", "block_size", "cut inside a record", "cut inside the header"])
@pytest.mark.parametrize("stand_in", [False, True])
def test_refused_inputs_end_the_run_with_the_file_named(oracle, native, files, what, stand_in):
    d, _, recs = files
    text = b"@CO\t" + b"h" * 5000 + b"\n"
    if what.startswith("cut"):
        raw, hb, _ = BC.stream(recs, text=text)
        cut = hb // 2 if "header" in what else BC.walk(raw[hb:])[0][20]["off"] + hb + 50
        data = BC.B.bgzf_file(raw[:cut], [4000, 9000])  # every member is whole: BGZF is intact, BAM is not
    else:
        data, _ = BC.bam_file(_damaged(recs, what), sizes=(4000, 9000), text=text)
    path = str(d / ("bad_%s_%d.bam" % (what.replace(" ", "_"), stand_in)))
    open(path, "wb").write(data)
    env = {"BAM_STAND_IN": "1", "GRP_INGEST_CHUNK": "20000"} if stand_in else {}
    rp, _ = _run(files, "bad_%s_%d" % (what.replace(" ", "_"), stand_in), "golden", path, **env)
    assert rp.returncode != 0, "a damaged BAM file passed for a shorter input"
    assert "failed" in rp.stderr and os.path.basename(path) in rp.stderr and "byte" in rp.stderr, rp.stderr[-2000:]
    if what == "flag 16" and not stand_in:  # (the reason is the engine's to give: the stand-in has the oracle engine's fixed text)
        assert "samtools fastq" in rp.stderr
