"""GPU end-to-end: goldrush-path with GRP_RESIDENT=all on BGZF, plain gzip, BAM and mixed inputs.  The reads stay on the
device between the passes and the written records are fetched through grp_records_fetch (the trace line proves it: units
inflated, records fetched, formatted on the device); every output file and the log are those of the run on the plain twin.
The same cases run on the oracle engine in tests/test_resident_compressed_cpu.py."""
import gzip
import os
import re
import subprocess

import pytest

import bam_cases as BC
import bgzf_cases as B
from cli_runner import cli, log as _log  # noqa: F401 (cli: a fixture)
from test_gpu_cli import _mk_fastq

pytestmark = pytest.mark.gpu

BASE = ["-k22", "-w16", "-t500", "-u5", "-a1", "-o0.1", "-h3", "-j4", "-d5", "-x10", "-s1011011110110111101101", "-g150000", "-b4", "-H2500000", "-P0", "--verbose"]
MODES = {"silver": ["-r0.9", "--silver_path", "-M2", "-m3500"], "golden": ["-m3500"]}
FETCH = re.compile(r"GRP_TRACE_INGEST resident fetch: (\d+) flushes, units inflated (\d+), text bytes inflated (\d+), records fetched (\d+) \(trimmed (\d+), in two or more units (\d+)\), output bytes (\d+) \((.*)\)")
SIZES = [1, 65280, 7, 30011, 2, 64000, 513, 40000]
ENV_KEYS = ("GRP_GZIP_INDEX", "GRP_GZIP_SPAN", "GRP_GZIP_INDEX_MAX_GB", "GRP_INGEST_CHUNK", "GRP_RESIDENT", "GRP_RESIDENT_MAX_GB", "GRP_WORLD", "GRP_RANK")


def _records(text):
    lines = text.split(b"\n")
    return [(lines[4 * i][1:], lines[4 * i + 1], lines[4 * i + 3]) for i in range(len(lines) // 4)]


def _fastq(recs):
    return b"".join(b"@" + n + b"\n" + s + b"\n+\n" + q + b"\n" for n, s, q in recs)


def _bam(recs, sizes):
    return BC.bam_file([dict(name=n.split(b" ")[0], bases=s.upper(), quals=bytes(c - 33 for c in q)) for n, s, q in recs], sizes=sizes, text=b"@HD\tVN:1.6\n")


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("resident_cli")
    fq = str(d / "reads.fq")
    _mk_fastq(fq, 150_000, 260, 6000, 4000, seed=31, lower=True, with_n=13)
    text = open(fq, "rb").read()
    recs = _records(text)
    assert _fastq(recs) == text
    (d / "reads.bgzf.fq.gz").write_bytes(B.bgzf_file(text, SIZES))
    (d / "reads.fq.gz").write_bytes(gzip.compress(text, 6))
    bam, twin = _bam(recs, SIZES)
    (d / "reads.bam").write_bytes(bam)
    (d / "bam_twin.fq").write_bytes(twin)
    n = len(recs)
    cut = [0, n // 5, 2 * n // 5, 3 * n // 5, 4 * n // 5, n]
    part = [recs[cut[i]:cut[i + 1]] for i in range(5)]
    (d / "m0.fq").write_bytes(_fastq(part[0]))
    (d / "m1.fq.gz").write_bytes(gzip.compress(_fastq(part[1]), 6))
    (d / "m2.bgzf.fq.gz").write_bytes(B.bgzf_file(_fastq(part[2]), SIZES))
    mbam, mtwin = _bam(part[3], SIZES)
    (d / "m3.bam").write_bytes(mbam)
    (d / "m4.fq").write_bytes(_fastq(part[4])[:-1])
    (d / "mixed_twin.fq").write_bytes(_fastq(part[0]) + _fastq(part[1]) + _fastq(part[2]) + mtwin + _fastq(part[4]))
    return {"bgzf": ([d / "reads.bgzf.fq.gz"], fq), "gzip": ([d / "reads.fq.gz"], fq), "bam": ([d / "reads.bam"], str(d / "bam_twin.fq")),
            "mixed": ([d / "m0.fq", d / "m1.fq.gz", d / "m2.bgzf.fq.gz", d / "m3.bam", d / "m4.fq"], str(d / "mixed_twin.fq"))}


def _run(cli, tmp_path_factory, mode, paths, popen=False, **env):
    d = tmp_path_factory.mktemp("run")
    e = dict(os.environ, GRP_TRACE_INGEST="1", GRP_GZIP_SPAN="50000", **env)
    for k in ENV_KEYS:
        if k not in env and k != "GRP_GZIP_SPAN":
            e.pop(k, None)
    args = BASE + MODES[mode]
    for p in paths:
        args += ["-i", str(p)]
    cmd = [cli] + args + ["-p", str(d / "out")]
    if popen:
        return subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=e), d
    rp = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=e)
    return rp, {f: open(d / f, "rb").read() for f in sorted(os.listdir(d))}


def _counters(rp):
    keep = ("Visited", "Saw:", "Assigned:", "Unassigned:", "Total queries", "Total hits", "Total misses", "Num reads", "Average Phred", "m_filterSize", "num_", "Total reads skipped")
    return [l for l in rp.stderr.splitlines() if l.startswith(keep)]


@pytest.fixture(scope="module")
def twins(cli, inputs, tmp_path_factory):
    out = {}
    for twin in sorted({t for _, t in inputs.values()}):
        for mode in MODES:
            rp, files = _run(cli, tmp_path_factory, mode, [twin])
            assert rp.returncode == 0 and files and all(files.values()), rp.stderr[-2000:]
            out[twin, mode] = (rp, files)
    return out


@pytest.mark.parametrize("chunk", [None, "100000"], ids=["default_chunk", "small_chunk"])
@pytest.mark.parametrize("mode", ["silver", "golden"])
@pytest.mark.parametrize("fmt", ["bgzf", "gzip", "bam", "mixed"])
def test_resident_compressed_input_gives_the_twins_outputs(cli, inputs, twins, tmp_path_factory, fmt, mode, chunk):
    paths, twin = inputs[fmt]
    env = {"GRP_INGEST_CHUNK": chunk} if chunk else {}
    rp, files = _run(cli, tmp_path_factory, mode, paths, GRP_RESIDENT="all", **env)
    assert rp.returncode == 0, rp.stderr[-3000:]
    want_rp, want = twins[twin, mode]
    assert files == want
    assert _counters(rp) == _counters(want_rp) and len(_counters(rp)) > 5
    assert "GRP_RESIDENT=all: the reads are not kept" not in rp.stderr
    m = FETCH.search(rp.stderr)
    assert m, rp.stderr[-3000:]
    flushes, units, text_bytes, fetched, trimmed, straddling, out_bytes = (int(x) for x in m.groups()[:7])
    assert units > 0 and fetched > 0 and "formatted on the device" in m.group(8), m.group(0)
    if chunk:
        assert flushes >= 4, m.group(0)
    if fmt != "mixed":
        assert out_bytes == sum(len(v) for v in files.values())
    # one source fewer than the two-pass form: the Phred median and the fill
    assert len([l for l in rp.stderr.splitlines() if l.startswith("GRP_TRACE_INGEST source:")]) == 2


def test_unset_stays_in_two_passes(cli, inputs, twins, tmp_path_factory):
    paths, twin = inputs["bgzf"]
    rp, files = _run(cli, tmp_path_factory, "silver", paths)
    assert rp.returncode == 0 and files == twins[twin, "silver"][1]
    assert len([l for l in rp.stderr.splitlines() if l.startswith("GRP_TRACE_INGEST source:")]) == 3 and not FETCH.search(rp.stderr)


def test_two_ranks_on_one_device(cli, inputs, twins, tmp_path_factory):
    """GRP_WORLD=2 on the one device: rank 0 fetches and writes what the single run writes, rank 1 is silent and fetches nothing"""
    paths, twin = inputs["mixed"]
    key = "gpu_resident_%d" % os.getpid()
    procs = []
    for rank in range(2):
        procs.append(_run(cli, tmp_path_factory, "silver", paths, popen=True, GRP_RESIDENT="all", GRP_WORLD="2", GRP_RANK=str(rank), GRP_LOCAL_RANK="0", GRP_SHM_KEY=key,
                          GRP_STREAM_WGS_PER_CU="2", GRP_INGEST_CHUNK="400000"))
    outs = []
    try:
        for p, _ in procs:
            outs.append(p.communicate(timeout=300))
    finally:
        for p, _ in procs:
            if p.poll() is None:
                p.kill()
    assert [p.returncode for p, _ in procs] == [0, 0], [o[1][-2000:] for o in outs]
    d0 = procs[0][1]
    files = {f: open(d0 / f, "rb").read() for f in sorted(os.listdir(d0))}
    assert files == twins[twin, "silver"][1]
    m = FETCH.search(outs[0][1])
    assert m and int(m.group(4)) > 0 and "formatted on the device" in m.group(8)
    assert outs[1][0].strip() == "" and outs[1][1].strip() == ""
    assert not os.listdir(procs[1][1]) or all(os.path.getsize(procs[1][1] / f) == 0 for f in os.listdir(procs[1][1]))
