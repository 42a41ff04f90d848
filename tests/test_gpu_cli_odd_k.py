"""GPU end-to-end at odd -k (seeds one base shorter than k, a tile of tile + 1 frames): the goldrush-path CLI must write
files byte-identical to the oracle CLI's and print the same counters — designed seeds (silver paths, then the golden
path), a 23-character preset, --ntcard, a long odd preset, -h 9, and -m 0 with reads of k + h - 2 bases."""
import filecmp
import glob
import os
import subprocess

import pytest

from helpers import palindromic_preset

pytestmark = pytest.mark.gpu


def _verbose_counters(stderr):
    keep = ("Visited", "Saw:", "Assigned:", "Unassigned:", "Total queries", "Total hits", "Total misses", "Num reads", "Average Phred",
            "m_filterSize", "expected hash space", "minimum average phred", "num_", "Total reads skipped")
    return [l for l in stderr.splitlines() if l.strip().startswith(keep)]


def _mk_fastq(path, genome_len, n_reads, seed, short=(), sub=0.01):
    from goldrush_amd import synth

    g = synth.random_genome(genome_len, seed)
    reads = synth.make_reads(g, n_reads, mean_len=6000, min_len=4000, seed=seed + 1, max_len=9000, sub=sub, ins=sub / 10, dele=sub / 10)
    out = []
    for i, (rid, seq, qual) in enumerate(reads):
        if i % 13 == 4:
            seq, qual = seq[:700], qual[:700]
        out.append((rid, seq, qual))
    for j, n in enumerate(short):  # reads of n bases (cut from the genome)
        out.append((b"short%d" % j, g[1000 * j: 1000 * j + n].tobytes(), b"5" * n))
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
    assert _verbose_counters(rp.stderr) == _verbose_counters(ro.stderr)
    assert any(l.strip().startswith("Total queries") for l in _verbose_counters(rp.stderr)) or "-m0" in args
    return rp, d_p, fo


@pytest.fixture(scope="module")
def host(native):
    from goldrush_amd import host as h

    assert os.path.exists(h.CLI_PATH), "goldrush-path binary missing: run __graft_entry__.build()"
    return h


COMMON = ["-t500", "-u5", "-a1", "-o0.1", "-j4", "-d5", "-x8", "-g150000", "-b4", "-H2000000", "-P10", "--verbose"]


def test_designed_k23_silver_then_golden(oracle, host, tmp_path):
    fq = str(tmp_path / "reads.fq")
    _mk_fastq(fq, 150_000, 140, seed=23)
    seed = ["-k23", "-w16", "-h3"]
    rp, d_p, files = _run_both(oracle, host, tmp_path, seed + COMMON + ["-r0.9", "--silver_path", "-M3", "-m4000", "-i", fq], "silver")
    assert len(files) >= 2 and all(os.path.getsize(d_p / f) > 0 for f in files), files
    allfq = str(tmp_path / "all.fq")
    with open(allfq, "wb") as out:
        for f in files:
            out.write(open(d_p / f, "rb").read())
    rp, d_p, files = _run_both(oracle, host, tmp_path, seed + COMMON + ["-m0", "-i", allfq], "golden")
    assert files == ["out.fa"] and open(d_p / "out.fa", "rb").read().count(b">") > 5


@pytest.mark.parametrize("args,tag", [(["-k23", "-w17", "-h3", "-s10110111101101111011011"], "preset23"), (["-k23", "-w16", "-h9"], "h9"),
                                      (["-k129", "-w31", "-h2", "-s" + palindromic_preset(129, 30, 5)], "long129")])
def test_odd_k_silver_paths(oracle, host, tmp_path, args, tag):
    fq = str(tmp_path / "reads.fq")
    _mk_fastq(fq, 150_000, 140, seed=7, sub=0.004 if tag == "long129" else 0.01)
    rp, d_p, files = _run_both(oracle, host, tmp_path, args + COMMON + ["-r0.9", "--silver_path", "-M3", "-m4000", "-i", fq], tag)
    assert files and all(os.path.getsize(d_p / f) > 0 for f in files), files


def test_odd_k_ntcard(oracle, host, tmp_path):
    """--ntcard (no -H: the estimate sizes the filter) with windows of 22 - 24 bases, reads of 22 - 24 bases and a record
    with a non-ACGT character"""
    fq = str(tmp_path / "reads.fq")
    _mk_fastq(fq, 150_000, 120, seed=31, short=(22, 23, 24))
    with open(fq, "ab") as f:
        seq = b"ACGTAC" * 30 + b"N" + b"TTGCA" * 40
        f.write(b"@dirty\n%s\n+\n%s\n" % (seq, b"5" * len(seq)))
    rp, d_p, files = _run_both(oracle, host, tmp_path, ["-k23", "-w16", "-h3"] + [a for a in COMMON if not a.startswith("-H")] + ["-m0", "--ntcard", "-i", fq], "ntc")
    assert files == ["out.fa"] and "Calculating expected entries" in rp.stderr


def test_odd_k_reads_one_base_shorter_than_k_plus_h_minus_1(oracle, host, tmp_path):
    """-m 0: reads of k + h - 2 = 24 bases are as long as the longest seed and take part in the fill"""
    fq = str(tmp_path / "reads.fq")
    _mk_fastq(fq, 150_000, 60, seed=41, short=(24,) * 20 + (23,) * 5 + (25,) * 5)
    rp, d_p, files = _run_both(oracle, host, tmp_path, ["-k23", "-w16", "-h3"] + COMMON + ["-m0", "-i", fq], "short")
    assert files == ["out.fa"]
