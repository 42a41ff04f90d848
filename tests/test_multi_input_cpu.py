"""CPU: several input files in one run (repeated -i, ".fofn" lists).  The option parser and the expansion of lists; then the
product's whole host program over the oracle engine: a run on files f1 .. fn against the run on their FASTQ twin — one file
with the records of f1, then f2, and so on — through the host reader and through the chunked source (the oracle engine's
restated ingest, grp_bam_parse restated in Python beside it: tests/test_bam_cpu.py)."""
import gzip
import os
import resource
import subprocess
import sys

import pytest

import bam_cases as BC
import test_bam_cpu as TB

ROOT = TB.ROOT
COMMON, MODES = TB.COMMON, TB.MODES
ENV_KEYS = ("GRP_HOST_INGEST", "GRP_INGEST_CHUNK", "GRP_BATCH_RECORDS", "GRP_BGZF", "GRP_RESIDENT", "GRP_GZIP_INDEX", "BAM_STAND_IN", "EXPECT_BAM_PARSE")


# ---- the command line ------------------------------------------------------------------------------------------------------
BASE = ["-k22", "-w16", "-g1000"]


def _dump(native, argv):
    from goldrush_amd import host

    rc, rows = host.inputs_dump(BASE + argv)
    return rc, [v for k, v in rows if k == "input"], [v for k, v in rows if k == "inputs"], [v for k, v in rows if k == "file"], [v for k, v in rows if k == "error"]


def test_one_input_is_what_it_was(native):
    from goldrush_amd import host

    rc, last, inputs, files, err = _dump(native, ["-i", "a.fq"])
    assert (rc, last, inputs, files, err) == (-1, ["a.fq"], ["a.fq"], ["a.fq"], [])
    assert host.process_options_dump(BASE + ["-i", "a.fq"])[1]["input"] == "a.fq"
    rc, last, inputs, files, err = _dump(native, [])
    assert (rc, last, inputs, files) == (-1, [""], [], [])


def test_every_i_adds_an_input_in_order(native):
    from goldrush_amd import host

    rc, last, inputs, files, err = _dump(native, ["-i", "b.bam", "-t", "500", "-i", "a.fq", "-ic.fq.gz"])
    assert (rc, last, inputs, files, err) == (-1, ["c.fq.gz"], ["b.bam", "a.fq", "c.fq.gz"], ["b.bam", "a.fq", "c.fq.gz"], [])
    # the dump that is compared with the reference's own opt.cpp holds what the reference would: the last -i
    assert host.process_options_dump(BASE + ["-i", "b.bam", "-i", "a.fq"])[1]["input"] == "a.fq"


def test_a_fofn_stands_for_the_files_it_lists(native, tmp_path):
    sub = tmp_path / "lists"
    sub.mkdir()
    lst = sub / "cells.fofn"
    lst.write_text("# two cells\n\ncell1/hifi_reads.bam\r\n  \n/abs/cell2.bam\n   # indented comment\n../other dir/x.fq  \n")
    rc, last, inputs, files, err = _dump(native, ["-i", "first.fq", "-i", str(lst), "-i", "last.fq"])
    assert rc == -1 and err == [] and last == ["last.fq"] and inputs == ["first.fq", str(lst), "last.fq"]
    assert files == ["first.fq", str(sub) + "/cell1/hifi_reads.bam", "/abs/cell2.bam", str(sub) + "/../other dir/x.fq", "last.fq"]
    # a list named without a directory resolves against the working directory, as written
    cwd = os.getcwd()
    os.chdir(sub)
    try:
        assert _dump(native, ["-i", "cells.fofn"])[3] == ["cell1/hifi_reads.bam", "/abs/cell2.bam", "../other dir/x.fq"]
    finally:
        os.chdir(cwd)


@pytest.mark.parametrize("what", ["nested", "empty", "only comments", "unreadable"])
def test_a_bad_list_is_named(native, tmp_path, what):
    lst = tmp_path / ("%s.fofn" % what.replace(" ", "_"))
    if what == "nested":
        lst.write_text("a.fq\ninner.fofn\n")
    elif what == "empty":
        lst.write_text("")
    elif what == "only comments":
        lst.write_text("# nothing\n\n")
    rc, last, inputs, files, err = _dump(native, ["-i", "a.fq", "-i", str(lst)])
    assert rc == 1 and files == [] and len(err) == 1 and str(lst) in err[0]
    if what == "nested":
        assert "inner.fofn" in err[0]


# ---- the whole host program ------------------------------------------------------------------------------------------------
def _fastq(recs, nl=b"\n", final_newline=True):
    out = nl.join(nl.join((b"@" + n, s, b"+", q)) for n, s, q in recs)
    return out + (nl if final_newline and recs else b"")


def _tiny():
    lines = open(os.path.join(TB.GOLD, "tiny.fq"), "rb").read().split(b"\n")
    return [(lines[4 * i][1:], lines[4 * i + 1], lines[4 * i + 3]) for i in range(len(lines) // 4)]


@pytest.fixture(scope="module")
def work(tmp_path_factory, oracle, native):
    d = tmp_path_factory.mktemp("multi_cpu")
    (d / "runner.py").write_text(TB.RUNNER.format(root=ROOT))
    return d


def _run(work, tag, mode, inputs, extra=(), preexec_fn=None, **env):
    d = work / tag
    d.mkdir()
    e = dict(os.environ, OMP_NUM_THREADS="2", **env)
    for k in ENV_KEYS:
        if k not in env:
            e.pop(k, None)
    args = COMMON + MODES[mode] + list(extra)
    for i in inputs:
        args += ["-i", str(i)]
    rp = subprocess.run([sys.executable, str(work / "runner.py")] + args + ["-p", str(d / "out")], capture_output=True, text=True, timeout=900, env=e, preexec_fn=preexec_fn)
    return rp, {f: open(d / f, "rb").read() for f in sorted(os.listdir(d))}


# how a run reads: the host reader, or the chunked source with the reads kept between the passes, or parsed again
READERS = {"host": {}, "host_small_batches": {"GRP_BATCH_RECORDS": "5"}, "chunked": {"BAM_STAND_IN": "1"}, "chunked_small": {"BAM_STAND_IN": "1", "GRP_INGEST_CHUNK": "9000"},
           "chunked_two_pass": {"BAM_STAND_IN": "1", "GRP_RESIDENT": "off", "GRP_INGEST_CHUNK": "30000"}}


@pytest.fixture(scope="module")
def plain(work):
    """three plain files — CRLF line ends, not a byte, no final newline — and the twin; a -f list of reads of two files"""
    recs = _tiny()
    a, c = recs[:13], recs[13:]
    paths = [work / "crlf.fq", work / "empty.fq", work / "no_newline.fq"]
    paths[0].write_bytes(_fastq(a, nl=b"\r\n"))
    paths[1].write_bytes(b"")
    paths[2].write_bytes(_fastq(c, final_newline=False))
    twin = work / "plain_twin.fq"
    twin.write_bytes(_fastq(a + c))
    flt = work / "skip.txt"
    flt.write_bytes(b"\n".join([a[2][0].split()[0], a[12][0].split()[0], c[0][0].split()[0], c[-1][0].split()[0], b"not_a_read"]) + b"\n")
    cases = {"silver": ("silver", []), "golden": ("golden", []), "golden_f": ("golden", ["-f", str(flt)])}
    twins = {}
    for name, (mode, extra) in cases.items():
        rp, fo = _run(work, "plain_twin_" + name, mode, [twin], extra)
        assert rp.returncode == 0 and fo and any(fo.values()), rp.stderr[-3000:]
        twins[name] = (rp, fo)
    return paths, cases, twins


@pytest.mark.parametrize("reader", sorted(READERS))
@pytest.mark.parametrize("case", ["silver", "golden", "golden_f"])
def test_three_plain_files_equal_their_twin(work, plain, case, reader):
    paths, cases, twins = plain
    mode, extra = cases[case]
    rp, fo = _run(work, "plain_%s_%s" % (case, reader), mode, paths, extra, **READERS[reader])
    assert rp.returncode == 0, rp.stderr[-3000:]
    assert fo == twins[case][1]
    assert TB._pick(rp) == TB._pick(twins[case][0]) and len(TB._pick(rp)) > 5
    assert [l for l in rp.stderr.splitlines() if l.startswith("opening: ")] == ["opening: %s" % p for p in paths]


@pytest.mark.parametrize("reader", ["host", "chunked", "chunked_small"])
def test_a_file_that_ends_at_a_garbage_line_ends_there_and_the_next_one_is_read(work, reader):
    """each file yields the records it yields on its own: a line that is no FASTQ header ends ITS file, in whatever chunk of
    it the line stands, and the files behind it are read all the same"""
    recs = _tiny()
    first = work / ("garbage_%s.fq" % reader)
    first.write_bytes(_fastq(recs[:6]) + b"no header here\n" + _fastq(recs[6:20]))
    second = work / ("behind_garbage_%s.fq" % reader)
    second.write_bytes(_fastq(recs[20:]))
    twin = work / ("garbage_twin_%s.fq" % reader)
    twin.write_bytes(_fastq(recs[:6] + recs[20:]))
    rt, ft = _run(work, "garbage_twin_" + reader, "golden", [twin], **READERS[reader])
    rp, fo = _run(work, "garbage_" + reader, "golden", [first, second], **READERS[reader])
    assert rt.returncode == rp.returncode == 0, rp.stderr[-3000:]
    assert fo == ft and any(ft.values()) and TB._pick(rp) == TB._pick(rt)


@pytest.fixture(scope="module")
def mixed(work):
    """plain FASTQ, gzip, BGZF FASTQ and BAM in one run, the same name in two of the files"""
    recs = _tiny()
    parts = [recs[:7], recs[7:15], recs[15:24], recs[24:]]
    parts[2] = parts[2] + [(recs[3][0], recs[3][1], recs[3][2])]  # a read of the first file again, in the third
    paths = [work / "a.fq", work / "b.fastq.gz", work / "c.fq.bgz", work / "d.bam"]
    paths[0].write_bytes(_fastq(parts[0]))
    paths[1].write_bytes(gzip.compress(_fastq(parts[1], final_newline=False)))
    paths[2].write_bytes(BC.B.bgzf_file(_fastq(parts[2]), [3000, 65280, 11]))
    bam, bam_twin = BC.bam_file([TB._rec(n, s, bytes(q - 33 for q in ql)) for n, s, ql in parts[3]], sizes=(4000, 65280, 9), text=b"@HD\tVN:1.6\n", refs=[(b"chr1", 10)])
    paths[3].write_bytes(bam)
    twin = work / "mixed_twin.fq"
    twin.write_bytes(_fastq(parts[0]) + _fastq(parts[1]) + _fastq(parts[2]) + bam_twin)
    twins = {}
    for mode in ("silver", "golden"):
        rp, fo = _run(work, "mixed_twin_" + mode, mode, [twin])
        assert rp.returncode == 0 and fo and any(fo.values()), rp.stderr[-3000:]
        twins[mode] = (rp, fo)
    return paths, twins


@pytest.mark.parametrize("reader", ["host", "chunked", "chunked_small", "chunked_two_pass"])
@pytest.mark.parametrize("mode", ["silver", "golden"])
def test_fastq_gzip_bgzf_and_bam_in_one_run_equal_their_twin(work, mixed, mode, reader):
    paths, twins = mixed
    rp, fo = _run(work, "mixed_%s_%s" % (mode, reader), mode, paths, **READERS[reader])
    assert rp.returncode == 0, rp.stderr[-3000:]
    assert fo == twins[mode][1]
    assert TB._pick(rp) == TB._pick(twins[mode][0])


def test_the_same_inputs_through_a_fofn(work, mixed):
    paths, twins = mixed
    lst = work / "mixed.fofn"
    lst.write_text("# the four of them\n" + "\n".join([paths[1].name, str(paths[2]), "./" + paths[3].name]) + "\n")
    rp, fo = _run(work, "mixed_fofn", "golden", [paths[0], lst], BAM_STAND_IN="1")
    assert rp.returncode == 0, rp.stderr[-3000:]
    assert fo == twins["golden"][1] and TB._pick(rp) == TB._pick(twins["golden"][0])


@pytest.mark.parametrize("reader", ["host", "chunked_small"])
@pytest.mark.parametrize("what", ["truncated second", "third is not FASTQ", "missing"])
def test_a_failing_input_is_the_one_named(work, mixed, what, reader):
    paths, _ = mixed
    good = [paths[0], paths[2], paths[3]]
    if what == "truncated second":
        bad = work / ("cut_%s.fastq.gz" % reader)
        z = paths[1].read_bytes()
        bad.write_bytes(z[:len(z) // 2])
        inputs = [good[0], bad, good[1], good[2]]
    elif what == "third is not FASTQ":
        bad = work / ("notes_%s.txt" % reader)
        bad.write_bytes(b">contig\nACGT\n")
        inputs = [good[0], good[1], bad, good[2]]
    else:
        bad = work / ("not_there_%s.fq" % reader)
        inputs = [good[0], good[1], good[2], bad]
    rp, fo = _run(work, "bad_%s_%s" % (what.replace(" ", "_"), reader), "golden", inputs, **READERS[reader])
    assert rp.returncode == 1, rp.stderr[-3000:]
    named = [l for l in rp.stderr.splitlines() if bad.name in l and not l.startswith("opening: ")]
    assert named, rp.stderr[-3000:]
    for g in good:  # nothing named wrongly: the good files appear in no line that reports a failure
        assert not [l for l in rp.stderr.splitlines() if g.name in l and not l.startswith("opening: ")], rp.stderr[-3000:]
    if what == "truncated second":
        assert "failed" in "".join(named) and rp.stderr.rstrip().splitlines()[-1].startswith("ERROR: ")
    else:  # found before any pass: the reference's message behind the line that names the file
        lines = rp.stderr.splitlines()
        assert lines[-1] == "Gold Path requires fastq format" and bad.name in lines[-2]
        assert "inserting bit vector" not in rp.stderr and not fo


def test_more_files_than_descriptors(work):
    """200 one-record files through a list, the process limited to 128 descriptors: the reads kept between the passes are
    read back from files opened on demand"""
    recs = _tiny()
    many = [(b"r%d_" % i + recs[i % len(recs)][0], recs[i % len(recs)][1][:1800 + 7 * i], recs[i % len(recs)][2][:1800 + 7 * i]) for i in range(200)]
    d = work / "cells"
    d.mkdir()
    for i, r in enumerate(many):
        (d / ("c%03d.fq" % i)).write_bytes(_fastq([r], final_newline=i % 3 != 0))
    (d / "all.fofn").write_text("".join("c%03d.fq\n" % i for i in range(200)))
    twin = work / "cells_twin.fq"
    twin.write_bytes(_fastq(many))
    # a -f list with a read of every other file: each of these names is compared through its file, so records are read back
    # from 100 files at the least, more than are held open at once
    flt = work / "cells_skip.txt"
    flt.write_bytes(b"".join(many[i][0] + b"\n" for i in range(0, 200, 2)))
    limit = lambda: resource.setrlimit(resource.RLIMIT_NOFILE, (128, 128))  # noqa: E731
    rt, ft = _run(work, "cells_twin", "golden", [twin], ["-f", str(flt)], BAM_STAND_IN="1")
    assert rt.returncode == 0 and any(ft.values()), rt.stderr[-3000:]
    for reader in ("chunked", "host"):
        rp, fo = _run(work, "cells_" + reader, "golden", [d / "all.fofn"], ["-f", str(flt)], preexec_fn=limit, **READERS[reader])
        assert rp.returncode == 0, rp.stderr[-3000:]
        assert fo == ft and TB._pick(rp) == TB._pick(rt)
