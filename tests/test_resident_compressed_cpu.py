"""CPU: GRP_RESIDENT=all — the reads of BGZF, plain gzip and BAM inputs kept between the passes, the written records fetched
through their inflatable units (csrc/host/gr_writer.cpp: Deferred; gr_units.hpp).  The product's whole host program runs over
the oracle engine (tests/resident_runner.py), once with zlib stand-ins for the two inflate entry points only — the host's own
fetch — and once with a Python restatement of grp_records_fetch.  Every run's files and verbose counters, "Average Phred"
included, are those of the run on the FASTQ twin and of the same input with GRP_RESIDENT=off."""
import gzip
import json
import os
import re
import subprocess
import sys

import pytest

import bam_cases as BC
import bgzf_cases as B
import resident_runner as RR
import test_bam_cpu as TB

ROOT = TB.ROOT
FETCH = re.compile(r"GRP_TRACE_INGEST resident fetch: (\d+) flushes, units inflated (\d+), text bytes inflated (\d+), records fetched (\d+) \(trimmed (\d+), in two or more units (\d+)\), output bytes (\d+) \((.*)\)")
# three silver paths of ~11 kb each and a golden path with a -f list
MODES = {"silver": ["-P0", "-r0.9", "--silver_path", "-M4", "-m1500", "-g12000"], "golden": ["-P12", "-m0"]}
ENV_KEYS = ("GRP_HOST_INGEST", "GRP_INGEST_CHUNK", "GRP_BATCH_RECORDS", "GRP_BGZF", "GRP_RESIDENT", "GRP_RESIDENT_MAX_GB", "GRP_GZIP_INDEX", "GRP_GZIP_SPAN", "GRP_GZIP_INDEX_MAX_GB", "FETCH_STAND_IN")
KEEP = TB.KEEP + ("Average Phred",)


def _fastq(recs):
    return b"".join(b"@" + n + b"\n" + s + b"\n+\n" + q + b"\n" for n, s, q in recs)


def _tiny():
    lines = open(os.path.join(TB.GOLD, "tiny.fq"), "rb").read().split(b"\n")
    return [(lines[4 * i][1:], lines[4 * i + 1], lines[4 * i + 3]) for i in range(len(lines) // 4)]


def _bgzf_with_an_empty_member(text):
    f = B.bgzf_file(text, [65280, 1, 40000, 513])
    blocks, _, why = B.walk_members(f)
    assert why == 1 and len(blocks) > 4
    at = blocks[2][0] - 18  # in front of the third member
    f = f[:at] + B.BGZF_EOF + f[at:]
    blocks, _, why = B.walk_members(f)
    assert why == 1 and blocks[2][2] == 0 and blocks[3][2] > 0
    return f


def _bam(recs, sizes=(65280, 1, 40000, 513)):
    return BC.bam_file([dict(name=n.split(b" ")[0], bases=s.upper(), quals=bytes(c - 33 for c in q)) for n, s, q in recs], sizes=sizes, text=b"@HD\tVN:1.6\n")[0]


@pytest.fixture(scope="module")
def work(tmp_path_factory, oracle, native):
    d = tmp_path_factory.mktemp("resident_cpu")
    (d / "runner.py").write_text(RR.RUNNER.format(root=ROOT))
    recs = _tiny()
    text = _fastq(recs)
    (d / "twin.fq").write_bytes(text)
    (d / "reads.bgzf.fq.gz").write_bytes(_bgzf_with_an_empty_member(text))
    (d / "reads.fq.gz").write_bytes(gzip.compress(text, 6))
    (d / "reads.bam").write_bytes(_bam(recs))
    # five files of four formats in one run (the reads of the twin, in its order)
    n = len(recs)
    cut = [0, n // 5, 2 * n // 5, 3 * n // 5, 4 * n // 5, n]
    part = [recs[cut[i]:cut[i + 1]] for i in range(5)]
    (d / "m0.fq").write_bytes(_fastq(part[0]))
    (d / "m1.fq.gz").write_bytes(gzip.compress(_fastq(part[1]), 6))
    (d / "m2.bgzf.fq.gz").write_bytes(B.bgzf_file(_fastq(part[2]), [30011, 7, 65280]))
    (d / "m3.bam").write_bytes(_bam(part[3], sizes=(20000, 3, 65280)))
    (d / "m4.fq").write_bytes(_fastq(part[4])[:-1])
    flt = d / "skip.txt"
    flt.write_bytes(b"\n".join([recs[2][0].split()[0], recs[n // 2][0].split()[0], recs[-1][0].split()[0], b"not_a_read"]) + b"\n")
    inputs = {"bgzf": [d / "reads.bgzf.fq.gz"], "gzip": [d / "reads.fq.gz"], "bam": [d / "reads.bam"], "mixed": [d / ("m0.fq"), d / "m1.fq.gz", d / "m2.bgzf.fq.gz", d / "m3.bam", d / "m4.fq"]}
    return d, inputs, {"silver": [], "golden": ["-f", str(flt)]}


def _run(work, tag, mode, inputs, **env):
    d = work[0] / tag
    d.mkdir()
    e = dict(os.environ, OMP_NUM_THREADS="2", GRP_TRACE_INGEST="1", BAM_STAND_IN="1", GRP_GZIP_SPAN=env.pop("GRP_GZIP_SPAN", "20000"), FETCH_OUT=str(work[0] / (tag + ".calls.json")), **env)
    for k in ENV_KEYS:
        if k not in env and k != "GRP_GZIP_SPAN":
            e.pop(k, None)
    args = TB.COMMON + MODES[mode] + work[2][mode]
    for i in inputs:
        args += ["-i", str(i)]
    rp = subprocess.run([sys.executable, str(work[0] / "runner.py")] + args + ["-p", str(d / "out")], capture_output=True, text=True, timeout=900, env=e)
    calls = json.load(open(e["FETCH_OUT"])) if os.path.exists(e["FETCH_OUT"]) else None
    return rp, {f: open(d / f, "rb").read() for f in sorted(os.listdir(d))}, calls


def _pick(rp):
    return [l for l in rp.stderr.splitlines() if l.startswith(KEEP)]


def _sources(rp):
    return len([l for l in rp.stderr.splitlines() if l.startswith("GRP_TRACE_INGEST source:")])


@pytest.fixture(scope="module")
def twins(work):
    out = {}
    for mode in MODES:
        rp, fo, _ = _run(work, "twin_" + mode, mode, [work[0] / "twin.fq"], GRP_RESIDENT="off")
        assert rp.returncode == 0 and fo and all(fo.values()), rp.stderr[-3000:]
        out[mode] = (rp, fo)
    assert sorted(out["silver"][1]) == ["out_1.fq", "out_2.fq", "out_3.fq", "out_4.fq"] or sorted(out["silver"][1]) == ["out_1.fq", "out_2.fq", "out_3.fq"], sorted(out["silver"][1])  # at least two rollovers
    assert sum(1 for l in out["silver"][0].stderr.splitlines() if l.startswith("Average Phred")) >= 3
    return out


@pytest.mark.parametrize("fetch", ["host", "stand_in"])
@pytest.mark.parametrize("mode", ["silver", "golden"])
@pytest.mark.parametrize("fmt", ["bgzf", "gzip", "bam", "mixed"])
def test_resident_compressed_run_equals_the_twin_and_the_two_pass_run(work, twins, fmt, mode, fetch):
    env = {"FETCH_STAND_IN": "1"} if fetch == "stand_in" else {}
    rp, fo, calls = _run(work, "%s_%s_%s" % (fmt, mode, fetch), mode, work[1][fmt], GRP_RESIDENT="all", **env)
    assert rp.returncode == 0, rp.stderr[-3000:]
    assert "GRP_RESIDENT=all: the reads are not kept" not in rp.stderr, rp.stderr[-3000:]
    assert fo == twins[mode][1]
    assert _pick(rp) == _pick(twins[mode][0]) and len(_pick(rp)) > 5
    m = FETCH.search(rp.stderr)
    assert m, rp.stderr[-3000:]
    flushes, units, text_bytes, fetched, trimmed, straddling, out_bytes = (int(x) for x in m.groups()[:7])
    assert flushes > 0 and units > 0 and fetched > 0 and trimmed > 0 and straddling > 0, m.group(0)
    assert ("on the device" in m.group(8)) == (fetch == "stand_in")
    if fetch == "stand_in":
        assert calls["fetch"] > 0 and calls["fetch_records"] == fetched
    else:
        assert calls["fetch"] == 0
    if fmt != "mixed":
        assert out_bytes == sum(len(v) for v in fo.values())  # every written record came through the fetch
    if mode == "silver" and fetch == "host":
        off, fo2, _ = _run(work, "%s_%s_off" % (fmt, mode), mode, work[1][fmt], GRP_RESIDENT="off")
        assert off.returncode == 0 and fo2 == fo and _pick(off) == _pick(rp)
        assert _sources(rp) == _sources(off) - 1 and not FETCH.search(off.stderr)


@pytest.mark.parametrize("fmt", ["bgzf", "gzip", "mixed"])
def test_a_small_chunk_gives_many_flushes(work, twins, fmt):
    rp, fo, _ = _run(work, "small_" + fmt, "silver", work[1][fmt], GRP_RESIDENT="all", GRP_INGEST_CHUNK="30000", FETCH_STAND_IN="1")
    assert rp.returncode == 0, rp.stderr[-3000:]
    assert fo == twins["silver"][1] and _pick(rp) == _pick(twins["silver"][0])
    assert int(FETCH.search(rp.stderr).group(1)) >= 4


def test_unset_and_off_leave_compressed_inputs_in_two_passes(work, twins):
    for env in ({}, {"GRP_RESIDENT": "off"}):
        rp, fo, calls = _run(work, "unset_%d" % len(env), "silver", work[1]["bgzf"], **env)
        assert rp.returncode == 0 and fo == twins["silver"][1]
        assert _sources(rp) == 3 and not FETCH.search(rp.stderr) and "GRP_RESIDENT" not in rp.stderr


@pytest.mark.parametrize("case", ["max_gb", "gzip_index_off", "gzip_member_appended"])
def test_dropped_residency_ends_in_the_two_pass_output_with_its_reason(work, twins, case):
    d = work[0]
    if case == "max_gb":
        inputs, env, why, name = work[1]["bgzf"], {"GRP_RESIDENT_MAX_GB": "0.00001"}, "GRP_RESIDENT_MAX_GB", "reads.bgzf.fq.gz"
    elif case == "gzip_index_off":
        inputs, env, why, name = work[1]["gzip"], {"GRP_GZIP_INDEX": "off"}, "gzip index", "reads.fq.gz"
    else:
        recs = _tiny()
        half = len(recs) // 2
        p = d / "bgzf_then_gzip.fq.gz"
        p.write_bytes(B.bgzf_file(_fastq(recs[:half]), [65280], eof=False) + gzip.compress(_fastq(recs[half:]), 6))
        inputs, env, why, name = [p], {}, "not BGZF", p.name
    rp, fo, _ = _run(work, "drop_" + case, "silver", inputs, GRP_RESIDENT="all", **env)
    assert rp.returncode == 0, rp.stderr[-3000:]
    assert fo == twins["silver"][1] and _pick(rp) == _pick(twins["silver"][0])
    line = [l for l in rp.stderr.splitlines() if l.startswith("GRP_RESIDENT=all: the reads are not kept on the device")]
    assert len(line) == 1 and why in line[0] and name in line[0], rp.stderr[-3000:]
    assert _sources(rp) == 3 and not FETCH.search(rp.stderr)
