"""GPU end-to-end: goldrush-path on several input files (repeated -i, a ".fofn" list).  A run on f1 .. fn writes what the
oracle CLI writes on the FASTQ twin — one file with the records of f1, then f2, and so on, built here from the records —
whatever the formats (plain, gzip, BGZF, BAM, mixed in one run) and whatever routes them: the reads kept between the passes
or parsed again, chunks smaller than a file, the host reader, two ranks."""
import filecmp
import glob
import gzip
import os
import re
import subprocess

import pytest

import bam_cases as BC
from test_gpu_cli import _mk_fastq, _verbose_counters

pytestmark = pytest.mark.gpu

BASE = ["-k22", "-w16", "-t500", "-u5", "-a1", "-o0.1", "-h3", "-j4", "-d5", "-x10", "-s1011011110110111101101", "-g200000", "-b4", "-m3500", "--verbose"]
SIZED = ["-H3000000"]
SILVER = ["-P0", "-r0.9", "--silver_path", "-M2"]
SOURCES = re.compile(r"^GRP_TRACE_INGEST source:", re.M)
GZIP_SEGS = re.compile(r"gzip segments inflated on the device (\d+)")
BGZF_BLOCKS = re.compile(r"BGZF blocks inflated on the device (\d+)")
CHUNK = 30000


@pytest.fixture(scope="module")
def host(native):
    from goldrush_amd import host as h

    assert os.path.exists(h.CLI_PATH), "goldrush-path binary missing: run __graft_entry__.build()"
    return h


def _fastq(recs, final_newline=True):
    out = b"\n".join(b"\n".join((b"@" + n, s, b"+", q)) for n, s, q in recs)
    return out + (b"\n" if final_newline and recs else b"")


def _inputs(paths):
    return [a for p in paths for a in ("-i", str(p))]


class Oracle:
    """the oracle CLI's run on a twin, once per argument list"""

    def __init__(self, oracle, d):
        self.oracle, self.d, self.done = oracle, d, {}

    def __call__(self, args, twin):
        key = (tuple(args), str(twin))
        if key not in self.done:
            d = self.d / ("o%d" % len(self.done))
            d.mkdir()
            ro = self.oracle.run_cli(list(args) + ["-i", str(twin), "-p", str(d / "out")], timeout=900)
            self.done[key] = (ro, d, sorted(os.listdir(d)))
        return self.done[key]


def _product(host, d, args, inputs, env=None):
    d.mkdir()
    e = dict(os.environ, GRP_TRACE_INGEST="1", **(env or {}))
    for k in ("GRP_RESIDENT", "GRP_INGEST_CHUNK", "GRP_HOST_INGEST", "GRP_BGZF", "GRP_GZIP_INDEX", "GRP_WORLD", "GRP_RANK"):
        if k not in (env or {}):
            e.pop(k, None)
    return subprocess.run([host.CLI_PATH] + list(args) + _inputs(inputs) + ["-p", str(d / "out")], capture_output=True, text=True, timeout=900, env=e)


def _same(rp, d_p, want):
    ro, d_o, fo = want
    assert rp.returncode == ro.returncode, (rp.returncode, ro.returncode, rp.stderr[-2000:])
    assert sorted(os.listdir(d_p)) == fo and fo, (sorted(os.listdir(d_p)), fo)
    for f in fo:
        assert filecmp.cmp(d_o / f, d_p / f, shallow=False), f"{f} differs"
    assert any(os.path.getsize(d_p / f) for f in fo)
    assert _verbose_counters(rp.stderr) == _verbose_counters(ro.stderr)


@pytest.fixture(scope="module")
def data(oracle, tmp_path_factory):
    d = tmp_path_factory.mktemp("multi")
    recs = _mk_fastq(str(d / "source.fq"), 200_000, 360, 6000, 4000, seed=61, lower=True, with_n=17, short=9)
    # three plain files of unequal size.  The second lacks its final newline and ends a little behind a multiple of CHUNK: a
    # chunk boundary lands inside its last record
    a = 37
    b = next(n for n in range(a + 150, len(recs) - 40) if 0 < (len(_fastq(recs[a:n], False)) % CHUNK) < len(_fastq(recs[n - 1:n], False)))
    plain = [d / "one.fq", d / "two.fq", d / "three.fq"]
    plain[0].write_bytes(_fastq(recs[:a]))
    plain[1].write_bytes(_fastq(recs[a:b], final_newline=False))
    plain[2].write_bytes(_fastq(recs[b:]))
    twin = d / "twin.fq"
    twin.write_bytes(_fastq(recs))
    names = [r[0].split()[0] for r in recs]
    flt = d / "skip.txt"
    flt.write_bytes(b"\n".join([names[2], names[a - 1], names[a], names[b - 1], names[b + 3], names[-1], b"not_a_read"]) + b"\n")
    return dict(dir=d, recs=recs, plain=plain, twin=twin, flt=flt, cut=(a, b), oracle=Oracle(oracle, d))


MODES = {"silver": lambda data: BASE + SIZED + SILVER, "golden_f": lambda data: BASE + SIZED + ["-P10", "-f", str(data["flt"])]}


@pytest.mark.parametrize("env", [{}, {"GRP_RESIDENT": "off"}, {"GRP_INGEST_CHUNK": str(CHUNK)}, {"GRP_HOST_INGEST": "1"}], ids=["default", "two_pass", "small_chunks", "host_reader"])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_three_plain_files_equal_the_oracle_on_their_twin(host, data, tmp_path, mode, env):
    args = MODES[mode](data)
    rp = _product(host, tmp_path / "p", args, data["plain"], env)
    _same(rp, tmp_path / "p", data["oracle"](args, data["twin"]))
    assert [l for l in rp.stderr.splitlines() if l.startswith("opening: ")] == ["opening: %s" % p for p in data["plain"]]
    if "GRP_HOST_INGEST" not in env:
        # one source per pass, not one per pass and file: the Phred median (-P0), the fill, and the classification where the
        # reads are not kept on the device
        passes = (1 if mode == "silver" else 0) + 1 + (1 if env.get("GRP_RESIDENT") == "off" else 0)
        assert len(SOURCES.findall(rp.stderr)) == passes, rp.stderr[-3000:]
        assert "files 3, begun 3" in rp.stderr


def test_ntcard_counts_every_file(host, data, tmp_path):
    args = BASE + ["-P10", "--ntcard"]
    rp = _product(host, tmp_path / "p", args, data["plain"])
    want = data["oracle"](args, data["twin"])
    _same(rp, tmp_path / "p", want)
    keep = ("Expected entries for seed pattern", "Total expected entries")
    assert [l for l in rp.stderr.splitlines() if l.startswith(keep)] == [l for l in want[0].stderr.splitlines() if l.startswith(keep)]


@pytest.fixture(scope="module")
def mixed(data):
    """plain + gzip + BGZF FASTQ + two BAM files with different headers (one with reference entries and a text longer than
    a BGZF member) holding the same records as the twin"""
    d, recs = data["dir"], data["recs"]
    cuts = [0, 50, 130, 200, 290, len(recs)]
    part = [recs[cuts[i]:cuts[i + 1]] for i in range(5)]

    def bam(rs, **kw):
        return BC.bam_file([dict(name=n.split(b" ")[0], bases=s.upper(), quals=bytes(c - 33 for c in q), cigar=(16,) * (i % 3), tags=b"rqf\0\0\x80\x3f" * (i % 4), pad=i % 16, flag=4 | (77 if i % 2 else 0))
                            for i, (n, s, q) in enumerate(rs)], sizes=(65280, 7, 30011), **kw)

    paths = [d / "m_plain.fq", d / "m_reads.fastq.gz", d / "m_bgzf.fq.gz", d / "m_cell1.bam", d / "m_cell2.bam"]
    paths[0].write_bytes(_fastq(part[0], final_newline=False))
    paths[1].write_bytes(gzip.compress(_fastq(part[1]), 6))
    paths[2].write_bytes(BC.B.bgzf_file(_fastq(part[2]), [65280, 1, 40000, 513]))
    bam1, twin1 = bam(part[3], text=b"@HD\tVN:1.6\tSO:unknown\n")
    bam2, twin2 = bam(part[4], text=b"@HD\tVN:1.6\n@CO\t" + b"c" * 150_000 + b"\n", refs=[(b"chr1", 1000), (b"chr2", 5)])
    paths[3].write_bytes(bam1)
    paths[4].write_bytes(bam2)
    twin = d / "m_twin.fq"
    # (a BAM record has no comment behind its name and no lower case: its twin is what the program reads in its place)
    twin.write_bytes(_fastq(part[0]) + _fastq(part[1]) + _fastq(part[2]) + twin1 + twin2)
    return paths, twin, part


@pytest.mark.parametrize("env", [{}, {"GRP_BGZF": "off"}, {"GRP_GZIP_INDEX": "off"}], ids=["default", "bgzf_off", "gzip_index_off"])
def test_mixed_formats_in_one_run(host, data, mixed, tmp_path, env):
    paths, twin, _ = mixed
    args = BASE + SIZED + SILVER
    rp = _product(host, tmp_path / "p", args, paths, env)
    _same(rp, tmp_path / "p", data["oracle"](args, twin))
    lines = [l for l in rp.stderr.splitlines() if l.startswith("GRP_TRACE_INGEST source:")]
    assert len(lines) == 3, rp.stderr[-3000:]  # the Phred median, the fill, the classification: one source each
    segs = [int(GZIP_SEGS.search(l).group(1)) for l in lines]
    blocks = [int(BGZF_BLOCKS.search(l).group(1)) for l in lines]
    if "GRP_GZIP_INDEX" in env:
        assert segs == [0, 0, 0]
    else:
        # the gzip file is the second input: the first pass that read it to its end left its index, the later ones have its
        # segments inflated on the device
        assert segs[0] == 0 and segs[1] > 0 and segs[2] > 0, segs
    if "GRP_BGZF" in env:
        assert blocks == [0, 0, 0]
    else:
        assert all(x > 0 for x in blocks), blocks


def test_a_fofn_gives_the_same_bytes(host, data, mixed, tmp_path):
    paths, twin, _ = mixed
    args = BASE + SIZED + SILVER
    lst = data["dir"] / "cells.fofn"
    lst.write_text("# the cells\n\n" + "\n".join([paths[1].name, str(paths[2]), "./" + paths[3].name]) + "\n")
    rp = _product(host, tmp_path / "p", args, [paths[0], lst, paths[4]])
    _same(rp, tmp_path / "p", data["oracle"](args, twin))


def test_two_ranks_with_two_input_files(host, data, tmp_path):
    """GRP_WORLD=2 on the one device: batch b belongs to rank b % 2 with b counted across the files; rank 0's files equal the
    oracle's, rank 1 is silent"""
    recs = data["recs"]
    files = [tmp_path / "a.fq", tmp_path / "b.fq"]
    files[0].write_bytes(_fastq(recs[:150], final_newline=False))
    files[1].write_bytes(_fastq(recs[150:]))
    for tag, extra in (("silver", SILVER), ("golden", ["-P10"])):
        args = BASE + SIZED + extra
        want = data["oracle"](args, data["twin"])
        d_p = tmp_path / (tag + "_p")
        d_p.mkdir()
        key = "gpu_multi_%d_%s" % (os.getpid(), tag)
        procs = []
        for rank in range(2):
            env = dict(os.environ, GRP_WORLD="2", GRP_RANK=str(rank), GRP_LOCAL_RANK="0", GRP_SHM_KEY=key, GRP_STREAM_WGS_PER_CU="2", GRP_INGEST_CHUNK="400000")
            procs.append(subprocess.Popen([host.CLI_PATH] + args + _inputs(files) + ["-p", str(d_p / "out")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env))
        outs = [p.communicate(timeout=900) for p in procs]
        ro, d_o, fo = want
        assert [p.returncode for p in procs] == [ro.returncode, ro.returncode], [o[1][-2000:] for o in outs]
        assert sorted(os.path.basename(p) for p in glob.glob(str(d_p / "*"))) == fo and fo
        for f in fo:
            assert filecmp.cmp(d_o / f, d_p / f, shallow=False), f"{f} differs"
        assert _verbose_counters(outs[0][1]) == _verbose_counters(ro.stderr)
        assert outs[1][0].strip() == "" and outs[1][1].strip() == ""


def test_a_refused_record_in_the_second_bam_names_it(host, data, mixed, tmp_path):
    paths, _, part = mixed
    recs = [dict(name=n.split(b" ")[0], bases=s.upper(), quals=bytes(c - 33 for c in q)) for n, s, q in part[4]]
    recs[40]["flag"] = 0x10
    text = b"@HD\tVN:1.6\n@CO\t" + b"c" * 150_000 + b"\n"
    raw, hb, _ = BC.stream(recs, text=text)
    at = hb + BC.walk(raw[hb:])[2]
    bad = tmp_path / "reverse_strand.bam"
    bad.write_bytes(BC.B.bgzf_file(raw, [65280, 7, 30011]))
    rp = _product(host, tmp_path / "p", BASE + SIZED + SILVER, [paths[0], paths[3], bad, paths[2]])
    assert rp.returncode != 0, "a refused record passed"
    msg = [l for l in rp.stderr.splitlines() if "failed" in l]
    assert msg and all(bad.name in l for l in msg) and "byte %d of the decompressed stream" % at in msg[-1] and "samtools fastq" in msg[-1], rp.stderr[-2000:]
    assert not any(p.name in l for l in msg for p in paths)


def test_a_bgzf_file_cut_inside_a_member_names_it(host, data, mixed, tmp_path):
    paths, _, part = mixed
    text = _fastq(part[2])
    members = [BC.B.bgzf_member(text[i:i + 50000], 1) for i in range(0, len(text), 50000)]
    assert len(members) > 6
    start = sum(len(m) for m in members[:5])
    bad = tmp_path / "cut_inside_a_member.fq.gz"
    bad.write_bytes(b"".join(members[:5]) + members[5][:len(members[5]) // 2])
    rp = _product(host, tmp_path / "p", BASE + SIZED + SILVER, [paths[0], paths[1], bad, paths[3]])
    assert rp.returncode != 0, "a truncated file passed for a shorter one"
    msg = [l for l in rp.stderr.splitlines() if "failed" in l]
    assert msg and all(bad.name in l for l in msg) and "BGZF member at byte %d" % start in msg[-1], rp.stderr[-2000:]
    assert not any(p.name in l for l in msg for p in paths)
