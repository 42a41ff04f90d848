"""GPU end-to-end at 9 to 16 spaced seeds per frame (-h 9 .. 16, the many-seed kernel form): the goldrush-path CLI must
write files byte-identical to the oracle CLI's — silver paths, then the golden path over them; a designed seed; --ntcard
— and refuse -h 17 loudly."""
import filecmp
import glob
import os
import subprocess

import pytest

from helpers import SEED22

pytestmark = pytest.mark.gpu


def _mk_fastq(path, genome_len, n_reads, seed):
    """reads with few errors (a frame of 16 seeds is lost to an error in any of its spans): the paths see hits"""
    from goldrush_amd import synth

    g = synth.random_genome(genome_len, seed)
    reads = synth.make_reads(g, n_reads, mean_len=7000, min_len=5000, seed=seed + 1, sub=0.004, ins=0.0005, dele=0.0005)
    out = []
    for i, (rid, seq, qual) in enumerate(reads):
        if i % 13 == 4:
            seq, qual = seq[:700], qual[:700]  # shorter than -m: skipped
        out.append((rid, seq, qual))
    synth.write_fastq(path, out)


def _run_both(oracle, host, tmp_path, args, tag):
    d_o = tmp_path / f"{tag}_o"
    d_p = tmp_path / f"{tag}_p"
    d_o.mkdir()
    d_p.mkdir()
    ro = oracle.run_cli(args + ["-p", str(d_o / "out")], timeout=900)
    rp = subprocess.run([host.CLI_PATH] + args + ["-p", str(d_p / "out")], capture_output=True, text=True, timeout=900)
    assert rp.returncode == ro.returncode == 0, (rp.returncode, ro.returncode, rp.stderr[-2000:], ro.stderr[-2000:])
    fo = sorted(os.path.basename(p) for p in glob.glob(str(d_o / "*")))
    fp = sorted(os.path.basename(p) for p in glob.glob(str(d_p / "*")))
    assert fo == fp, (fo, fp)
    for f in fo:
        assert filecmp.cmp(d_o / f, d_p / f, shallow=False), f"{f} differs"
    return ro, rp, d_p, fo


def _counters(stderr):
    keep = ("Visited", "Saw:", "Assigned:", "Unassigned:", "Total queries", "Total hits", "Total misses", "Num reads", "m_filterSize",
            "expected hash space", "Expected entries for seed pattern", "Total expected entries")
    return [l for l in stderr.splitlines() if l.strip().startswith(keep)]


@pytest.fixture(scope="module")
def host(native):
    from goldrush_amd import host as h

    assert os.path.exists(h.CLI_PATH), "goldrush-path binary missing: run __graft_entry__.build()"
    return h


@pytest.mark.parametrize("h", [9, 16])
def test_many_seeds_preset_silver_then_golden(oracle, host, tmp_path, h):
    """the default preset (-s, k = 22) at h seeds: spans 22 .. 21 + h; silver paths, then the golden path over them"""
    fq = str(tmp_path / "reads.fq")
    _mk_fastq(fq, 150_000, 140, seed=60 + h)
    common = ["-k22", "-w16", "-h%d" % h, "-s" + SEED22, "-t500", "-u5", "-a1", "-o0.1", "-j4", "-d5", "-x8", "-g150000", "-b4", "-H%d" % (700_000 * h), "-P10",
              "--verbose"]
    ro, rp, d_p, files = _run_both(oracle, host, tmp_path, common + ["-r0.9", "--silver_path", "-M3", "-m4000", "-i", fq], "silver%d" % h)
    assert len(files) >= 1 and all(os.path.getsize(d_p / f) > 0 for f in files), files
    assert _counters(rp.stderr) == _counters(ro.stderr)
    allfq = str(tmp_path / "all.fq")
    with open(allfq, "wb") as out:
        for f in files:
            out.write(open(d_p / f, "rb").read())
    ro, rp, d_p, files = _run_both(oracle, host, tmp_path, common + ["-m0", "-i", allfq], "golden%d" % h)
    assert files == ["out.fa"]
    assert open(d_p / "out.fa", "rb").read().count(b">") > 5
    assert _counters(rp.stderr) == _counters(ro.stderr)


@pytest.mark.parametrize("h", [9, 16])
def test_many_seeds_designed_seed(oracle, host, tmp_path, h):
    """a designed seed (no -s: make_seed_pattern's glibc-rand design) of span 24 at h seeds"""
    fq = str(tmp_path / "reads.fq")
    _mk_fastq(fq, 150_000, 140, seed=70 + h)
    args = ["-k24", "-w16", "-h%d" % h, "-t500", "-u5", "-a1", "-o0.1", "-j2", "-P10", "-d5", "-x8", "-g150000", "-b4", "-r0.9", "--silver_path", "-M3",
            "-m4000", "-i", fq, "--verbose"]
    ro, rp, d_p, files = _run_both(oracle, host, tmp_path, args, "designed%d" % h)
    assert len(files) >= 1 and all(os.path.getsize(d_p / f) > 0 for f in files), files
    assert _counters(rp.stderr) == _counters(ro.stderr)


@pytest.mark.parametrize("h", [9, 16])
def test_many_seeds_ntcard(oracle, host, tmp_path, h):
    """--ntcard at h seeds: the estimate sizes the filter, the golden path follows"""
    fq = str(tmp_path / "reads.fq")
    _mk_fastq(fq, 150_000, 120, seed=80 + h)
    with open(fq, "ab") as f:
        for i, seq in enumerate([b"ACGT" * 8, b"ACGT" * 8 + b"A", b"ACGTAC" * 30 + b"N" + b"TTGCA" * 40]):
            f.write(b"@extra%d\n%s\n+\n%s\n" % (i, seq, b"5" * len(seq)))
    args = ["-k22", "-w16", "-h%d" % h, "-s" + SEED22, "-t500", "-u5", "-a1", "-o0.1", "-j4", "-d5", "-x8", "-g150000", "-b4", "-P10", "-m0",
            "--ntcard", "-i", fq, "--verbose"]
    ro, rp, d_p, files = _run_both(oracle, host, tmp_path, args, "ntc%d" % h)
    assert files == ["out.fa"] and os.path.getsize(d_p / "out.fa") > 0
    assert "Calculating expected entries" in rp.stderr
    assert _counters(rp.stderr) == _counters(ro.stderr)


def test_seventeen_seeds_are_refused(host, tmp_path):
    fq = str(tmp_path / "reads.fq")
    _mk_fastq(fq, 20_000, 4, seed=3)
    args = ["-k22", "-w16", "-h17", "-s" + SEED22, "-t500", "-g20000", "-b4", "-H2000000", "-P10", "-i", fq, "-p", str(tmp_path / "out")]
    rp = subprocess.run([host.CLI_PATH] + args, capture_output=True, text=True, timeout=300)
    assert rp.returncode == 1, (rp.returncode, rp.stderr[-2000:])
    assert "h=17" in rp.stderr and "16" in rp.stderr, rp.stderr[-2000:]
