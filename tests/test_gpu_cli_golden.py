"""GPU end-to-end: --golden_path — the golden path behind the silver paths in ONE run of the goldrush-path binary.  On the
input and with the options of tests/test_gpu_cli.py::test_silver_then_golden_byte_identical, the fused run writes the silver
files and PREFIX.fa of the oracle CLI's two runs with `cat` between them (bin/goldrush:238-260), byte for byte, and both
stages' verbose counters are the oracle's — with the silver reads handed to the second stage on the device (the default), read
back from their files, with a two-pass first stage, a BGZF input kept on the device, and many parts.  A run of twelve paths
shows the order of `cat out_*.fq`: out_10.fq in front of out_2.fq."""
import os
import re
import subprocess

import pytest

import bgzf_cases as B
import test_gpu_cli as TC

pytestmark = pytest.mark.gpu

COMMON = ["-k22", "-w16", "-t500", "-u5", "-a1", "-o0.1", "-h3", "-j8", "-d5", "-x10", "-s1011011110110111101101", "-g300000", "-b4", "-H4000000"]
SILVER = {"three": ["-P0", "-r0.9", "--silver_path", "-M3", "-m3500"], "twelve": ["-P0", "-r0.04", "--silver_path", "-M12", "-m3500"]}
TRACE = re.compile(r"^GRP_TRACE_INGEST golden: route=(device|files) records=(\d+) parts=(\d+) batches=(\d+) bytes_read=(\d+)$", re.M)
FALLBACK = "--golden_path: the silver reads are read back from their files: "


@pytest.fixture(scope="module")
def host(native):
    from goldrush_amd import host as h

    assert os.path.exists(h.CLI_PATH), "goldrush-path binary missing: run __graft_entry__.build()"
    return h


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    d = tmp_path_factory.mktemp("golden_gpu")
    fq = str(d / "reads.fq")
    TC._mk_fastq(fq, 300_000, 900, 6000, 4000, seed=5, lower=True, with_n=50, short=40)
    text = open(fq, "rb").read()
    (d / "reads.bgzf.fq.gz").write_bytes(B.bgzf_file(text, [65280, 40000, 513, 65280]))
    return d, fq, str(d / "reads.bgzf.fq.gz")


@pytest.fixture(scope="module")
def pipeline(oracle, reads):
    """the oracle CLI's process #1, `cat`, process #2 — once per set of silver options"""
    d, fq, _ = reads
    out = {}
    for name, silver in SILVER.items():
        da = d / ("oracle_" + name)
        da.mkdir()
        ra = oracle.run_cli(COMMON + silver + ["-i", fq, "--verbose", "-p", str(da / "out")], timeout=900)
        assert ra.returncode == 0, ra.stderr[-2000:]
        files = {f: open(da / f, "rb").read() for f in sorted(os.listdir(da))}
        order = sorted((f for f in files if files[f]), key=lambda f: f.encode())  # cat out_*.fq
        allfq = d / ("oracle_%s_all.fq" % name)
        allfq.write_bytes(b"".join(files[f] for f in order))
        rb = oracle.run_cli(COMMON + ["-P0", "-m0", "-i", str(allfq), "--verbose", "-p", str(da / "gold")], timeout=900)
        assert rb.returncode == 0 and os.path.getsize(da / "gold.fa") > 0, rb.stderr[-2000:]
        files["gold.fa"] = open(da / "gold.fa", "rb").read()
        out[name] = (files, order, TC._verbose_counters(ra.stderr) + TC._verbose_counters(rb.stderr))
    return out


def _fused(host, reads, tag, silver, input_, **env):
    d = reads[0] / tag
    d.mkdir()
    e = dict(os.environ, GRP_TRACE_INGEST="1")
    for k in ("GRP_GOLDEN_RESIDENT", "GRP_RESIDENT", "GRP_INGEST_CHUNK", "GRP_HOST_INGEST", "GRP_RESIDENT_MAX_GB", "GRP_WORLD", "WORLD_SIZE"):
        e.pop(k, None)
    e.update(env)
    rp = subprocess.run([host.CLI_PATH] + COMMON + silver + ["-i", input_, "--verbose", "-p", "out", "--golden_path", "gold"], capture_output=True, text=True, timeout=900, env=e, cwd=d)
    return rp, {f: open(d / f, "rb").read() for f in sorted(os.listdir(d))}


def _check(rp, files, want, route):
    want_files, order, counters = want
    assert rp.returncode == 0, rp.stderr[-3000:]
    assert sorted(files) == sorted(want_files)
    for f in want_files:
        assert files[f] == want_files[f], f + " differs"
    assert TC._verbose_counters(rp.stderr) == counters
    t = TRACE.findall(rp.stderr)
    assert len(t) == 1 and t[0][0] == route, rp.stderr[-2000:]
    n_records = sum(want_files[f].count(b"\n+\n") for f in order)
    assert int(t[0][1]) == n_records
    said = [l for l in rp.stderr.splitlines() if l.startswith(FALLBACK)]
    if route == "device":
        assert int(t[0][4]) == 0 and int(t[0][2]) >= 1 and int(t[0][3]) >= len(order) and not said
    else:
        assert int(t[0][4]) == sum(len(want_files[f]) for f in order) and int(t[0][2]) == 0 and len(said) == 1
    opened = [l[len("opening: "):] for l in rp.stderr.splitlines() if l.startswith("opening: out_")]
    assert opened == order  # the second stage's inputs: the silver files that hold something, in the order of `cat out_*.fq`
    return t[0]


def test_default_route_hands_the_reads_over_on_the_device(host, reads, pipeline):
    rp, files = _fused(host, reads, "default", SILVER["three"], reads[1])
    assert sorted(pipeline["three"][0]) == ["gold.fa", "out_1.fq", "out_2.fq", "out_3.fq"]
    text = b"".join(pipeline["three"][0][f] for f in pipeline["three"][1])
    assert text.count(b"_untrimmed\n") > 20 and text.count(b"_trimmed\n") > 20  # both kinds of slices
    _check(rp, files, pipeline["three"], "device")
    assert "route=device" in rp.stderr and "bytes_read=0" in rp.stderr


def test_files_route(host, reads, pipeline):
    rp, files = _fused(host, reads, "files", SILVER["three"], reads[1], GRP_GOLDEN_RESIDENT="off")
    _check(rp, files, pipeline["three"], "files")
    assert FALLBACK + "GRP_GOLDEN_RESIDENT=off" in rp.stderr


def test_two_pass_first_stage(host, reads, pipeline):
    rp, files = _fused(host, reads, "two_pass", SILVER["three"], reads[1], GRP_RESIDENT="off")
    _check(rp, files, pipeline["three"], "device")


def test_bgzf_input_kept_on_the_device(host, reads, pipeline):
    rp, files = _fused(host, reads, "bgzf", SILVER["three"], reads[2], GRP_RESIDENT="all")
    _check(rp, files, pipeline["three"], "device")
    assert "GRP_TRACE_INGEST resident fetch:" in rp.stderr  # the first stage's records came through the deferred fetch


def test_many_parts_merged_by_the_second_gather(host, reads, pipeline):
    rp, files = _fused(host, reads, "chunks", SILVER["three"], reads[1], GRP_INGEST_CHUNK="300000")
    t = _check(rp, files, pipeline["three"], "device")
    assert int(t[2]) >= 8, t  # a part per chunk of the first stage that committed a read


def test_twelve_paths_in_the_order_of_cat(host, reads, pipeline):
    want_files, order, _ = pipeline["twelve"]
    silver = [f for f in want_files if f.startswith("out_")]
    assert len(silver) >= 11, silver  # (checked on the CPU: the oracle CLI alone writes twelve)
    assert order.index("out_10.fq") < order.index("out_2.fq")
    for route, env in (("device", {}), ("files", {"GRP_GOLDEN_RESIDENT": "off"})):
        rp, files = _fused(host, reads, "twelve_" + route, SILVER["twelve"], reads[1], **env)
        _check(rp, files, pipeline["twelve"], route)
