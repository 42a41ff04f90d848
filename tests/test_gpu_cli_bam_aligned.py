"""GPU end-to-end: goldrush-path on ALIGNED BAM with GRP_BAM_ALIGNED=on.  The input of tests/test_gpu_cli_bam.py made
aligned: a third of its records on the reverse strand (the read that is longer than a chunk among them), secondary and
supplementary copies in between.  Every output file and the log are those of the same run on the aligned twin — the FASTQ
that `samtools fastq -n` writes for the file with its default filters, written down from the SAM specification
(tests/bam_aligned_cases.py), not pinned against samtools' output — whatever routes the input; the log has one
GRP_BAM_ALIGNED: line more.  Without the switch the file is refused as before."""
import os

import numpy as np
import pytest

import bam_aligned_cases as BA
import bam_cases as BC
from cli_runner import cli, log as _log, run as _run  # noqa: F401 (cli: a fixture)
from test_gpu_cli import _mk_fastq
from test_gpu_cli_bgzf import SILVER, SIZES

pytestmark = pytest.mark.gpu

GOLDEN = [a for a in SILVER if a not in ("-r0.9", "--silver_path", "-M2")]
ON = {"GRP_BAM_ALIGNED": "on"}


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("bam_aligned_cli")
    reads = _mk_fastq(str(d / "source.fq"), 150_000, 260, 6000, 4000, seed=31, lower=False, with_n=13)
    rng = np.random.default_rng(5)
    reads.insert(100, (b"a_read_longer_than_a_chunk", np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=100_001)].tobytes(), bytes(rng.integers(35, 80, size=100_001).astype(np.uint8))))
    recs = []
    for i, (rid, seq, qual) in enumerate(reads):
        name, raw = rid.split(b" ")[0], bytes(q - 33 for q in qual)
        kw = dict(cigar=(16,) * (i % 3), tags=b"rqf\0\0\x80\x3f" * (i % 4), pad=i % 16)
        if i % 3 == 1:  # (100 % 3: the long read too) stored as the aligner stores a read of the reverse strand
            recs.append(dict(name=name, bases=seq.upper().translate(BA.COMPLEMENT)[::-1], quals=raw[::-1], flag=0x10 | (1 | 128 if i % 2 else 0), **kw))
        else:
            recs.append(dict(name=name, bases=seq, quals=raw, flag=(4 if i % 2 else 0) | (0x400 if i % 5 == 0 else 0), **kw))
        if i % 17 == 4:
            recs.append(dict(name=name, bases=seq, quals=raw, flag=0x100 | (0x10 if i % 2 else 0)))
        if i % 17 in (4, 9):
            recs.append(dict(name=name, bases=seq[:2000], quals=b"\xff" * 2000, flag=0x800, tags=b"SAZchr1,5,+,2000M,60,0;\0"))
    assert recs[[r["name"] for r in recs].index(b"a_read_longer_than_a_chunk")]["flag"] & 0x10
    n_skipped, n_reversed = BA.counts(recs)
    assert n_reversed == 87 and n_skipped >= 40
    text = b"@HD\tVN:1.6\tSO:coordinate\n" + b"@CO\t" + b"c" * 200_000 + b"\n"
    raw, hb, _ = BC.stream(recs, text=text, refs=[(b"chr1", 150_000)])
    paths = {"bam": str(d / "aligned.bam"), "twin": str(d / "aligned_twin.fq"), "other": str(d / "source.fq")}
    open(paths["bam"], "wb").write(BC.B.bgzf_file(raw, SIZES))
    open(paths["twin"], "wb").write(BA.aligned_twin(recs))
    return paths, (n_skipped, n_reversed)


def _without_said(rp, *paths):
    lines = _log(rp, paths[0])
    for k, p in enumerate(paths[1:]):
        lines = [l.replace(p, "INPUT%d" % (k + 2)) for l in lines]
    return [l for l in lines if not l.startswith("GRP_BAM_ALIGNED:")]


def _said_once(rp, inputs):
    paths, (n_skipped, n_reversed) = inputs
    said = [l for l in rp.stderr.splitlines() if l.startswith("GRP_BAM_ALIGNED:")]
    assert len(said) == 1, rp.stderr[-3000:]
    words = said[0].split()
    assert paths["bam"] in said[0] and str(n_skipped) in words and str(n_reversed) in words and words.index(str(n_skipped)) < words.index(str(n_reversed)), said


@pytest.fixture(scope="module")
def twins(cli, inputs, tmp_path_factory):
    """the runs on the aligned twin: silver (also with GRP_RESIDENT=all, which that run is compared with) and golden"""
    out = {}
    for key, args, env in (("silver", SILVER, {}), ("silver-all", SILVER, {"GRP_RESIDENT": "all"}), ("golden", GOLDEN, {})):
        rp, files = _run(cli, tmp_path_factory, args, inputs[0]["twin"], **ON, **env)
        assert rp.returncode == 0 and files and all(files.values()) and "GRP_BAM_ALIGNED:" not in rp.stderr, rp.stderr[-2000:]
        out[key] = (rp, files)
    assert out["silver"][1] == out["silver-all"][1]
    return out


@pytest.mark.parametrize("env", [{}, {"GRP_INGEST_CHUNK": "4096"}, {"GRP_BGZF": "off"}, {"GRP_HOST_INGEST": "1"}, {"GRP_RESIDENT": "all"}], ids=lambda e: "-".join(e) or "default")
def test_aligned_bam_input_gives_the_aligned_twins_outputs(cli, inputs, twins, tmp_path_factory, env):
    paths, _ = inputs
    rp, files = _run(cli, tmp_path_factory, SILVER, paths["bam"], **ON, **env)
    assert rp.returncode == 0, rp.stderr[-2000:]
    twin = twins["silver-all" if "GRP_RESIDENT" in env else "silver"]
    assert files == twin[1]
    assert _without_said(rp, paths["bam"]) == _without_said(twin[0], paths["twin"])
    _said_once(rp, inputs)
    if "GRP_RESIDENT" in env:  # the reads stayed, the written records came through the fetch
        assert "not kept on the device" not in rp.stderr and "GRP_TRACE_INGEST resident fetch" in rp.stderr and "formatted on the device" in rp.stderr, rp.stderr[-3000:]


def test_golden_run(cli, inputs, twins, tmp_path_factory):
    paths, _ = inputs
    rp, files = _run(cli, tmp_path_factory, GOLDEN, paths["bam"], **ON)
    assert rp.returncode == 0, rp.stderr[-2000:]
    assert files == twins["golden"][1]
    assert _without_said(rp, paths["bam"]) == _without_said(twins["golden"][0], paths["twin"])
    _said_once(rp, inputs)


def test_an_aligned_file_next_to_a_plain_fastq(cli, inputs, tmp_path_factory):
    paths, _ = inputs
    ro, fo = _run(cli, tmp_path_factory, SILVER + ["-i", paths["other"]], paths["twin"], **ON)
    rp, fp = _run(cli, tmp_path_factory, SILVER + ["-i", paths["other"]], paths["bam"], **ON)
    assert ro.returncode == rp.returncode == 0, rp.stderr[-2000:]
    assert fp == fo and fo and all(fo.values())
    assert _without_said(rp, paths["bam"], paths["other"]) == _without_said(ro, paths["twin"], paths["other"])
    _said_once(rp, inputs)


@pytest.mark.parametrize("env", [{}, {"GRP_BAM_ALIGNED": "off"}], ids=["unset", "off"])
def test_without_the_switch_the_file_is_refused_as_before(cli, inputs, tmp_path_factory, env):
    path = inputs[0]["bam"]
    rp, _ = _run(cli, tmp_path_factory, SILVER, path, **env)
    assert rp.returncode != 0 and "failed" in rp.stderr and os.path.basename(path) in rp.stderr and "samtools fastq" in rp.stderr, rp.stderr[-2000:]
    assert "GRP_BAM_ALIGNED:" not in rp.stderr
    if env:
        return
    rp, _ = _run(cli, tmp_path_factory, SILVER, path, GRP_BAM_ALIGNED="yes")  # no value of the switch: the run ends before its first pass
    assert rp.returncode == 1 and "GRP_BAM_ALIGNED" in rp.stderr and "inserting bit vector" not in rp.stderr, rp.stderr[-2000:]
