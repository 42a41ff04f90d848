"""GPU end-to-end: goldrush-path with GRP_GZIP_WALK=on.  Five small .fastq.gz files behind a .fofn, one of them of two
members: in front of the first pass the restart points of all five are found on the device (csrc/host/gr_gzwalk.cpp over
grp_gzip_walk), so the first pass reads them through their segments too, where without the switch it reads them through
zlib.  The output files are those of the run without the switch and of the oracle CLI on the FASTQ twin."""
import re

import pytest

import gzip_cases as G
from test_gpu_cli_multi_input import BASE, SIZED, SILVER, GZIP_SEGS, Oracle, _fastq, _product, _same, host  # noqa: F401 (host: a fixture)
from test_gpu_cli import _mk_fastq

pytestmark = pytest.mark.gpu

WALK = re.compile(r"^GRP_TRACE_INGEST gzip walk: files=(\d+) walked=(\d+) left_to_zlib=(\d+) rounds=(\d+) text=(\d+) seconds=([0-9.e+-]+)$", re.M)
ARGS = BASE + SIZED + SILVER


@pytest.fixture(scope="module")
def data(oracle, tmp_path_factory):
    d = tmp_path_factory.mktemp("gzip_walk_cli")
    recs = _mk_fastq(str(d / "source.fq"), 200_000, 300, 6000, 4000, seed=73, lower=True, with_n=17, short=9)
    cuts = [0, 31, 90, 170, 171, len(recs)]
    parts = [_fastq(recs[cuts[i]:cuts[i + 1]]) for i in range(5)]
    files = []
    for i, text in enumerate(parts):
        p = d / ("cell%d.fastq.gz" % i)
        half = text.index(b"\n@", len(text) // 2) + 700 if i == 2 else 0  # two members that meet inside a record
        p.write_bytes(G.member(text[:half], 6) + G.member(text[half:], 1) if half else G.member(text, (1, 6, 9)[i % 3]))
        files.append(p)
    fofn = d / "cells.fofn"
    fofn.write_text("\n".join(str(p) for p in files) + "\n")
    twin = d / "twin.fq"
    twin.write_bytes(b"".join(parts))
    return dict(fofn=fofn, twin=twin, n_text=sum(len(t) for t in parts), oracle=Oracle(oracle, d))


@pytest.fixture(scope="module")
def unset(host, data, tmp_path_factory):
    d = tmp_path_factory.mktemp("unset") / "p"
    return _product(host, d, ARGS, [data["fofn"]]), d


def _no_switch(monkeypatch):
    for k in ("GRP_GZIP_WALK", "GRP_GZIP_WALK_ROOM", "GRP_GZIP_SPAN", "GRP_GZIP_INDEX_MAX_GB"):
        monkeypatch.delenv(k, raising=False)


def test_the_switch_unset_has_no_walk(unset, data):
    rp, d = unset
    _same(rp, d, data["oracle"](ARGS, data["twin"]))
    assert "gzip walk" not in rp.stderr
    lines = [l for l in rp.stderr.splitlines() if l.startswith("GRP_TRACE_INGEST source:")]
    assert int(GZIP_SEGS.search(lines[0]).group(1)) == 0 and int(GZIP_SEGS.search(lines[1]).group(1)) > 0, lines  # the first pass: zlib


def test_walk_on_gives_the_same_files(host, data, unset, tmp_path, monkeypatch):
    _no_switch(monkeypatch)
    rp = _product(host, tmp_path / "p", ARGS, [data["fofn"]], {"GRP_GZIP_WALK": "on"})
    _same(rp, tmp_path / "p", data["oracle"](ARGS, data["twin"]))
    for f in data["oracle"](ARGS, data["twin"])[2]:
        assert (tmp_path / "p" / f).read_bytes() == (unset[1] / f).read_bytes(), f
    walks = WALK.findall(rp.stderr)
    assert len(walks) == 1, rp.stderr[-3000:]  # once per run, not once per pass
    files, walked, left, rounds, text, seconds = walks[0]
    assert (int(files), int(walked), int(left)) == (5, 5, 0) and int(rounds) >= 2 and int(text) == data["n_text"], walks
    lines = [l for l in rp.stderr.splitlines() if l.startswith("GRP_TRACE_INGEST source:")]
    assert len(lines) == len([l for l in unset[0].stderr.splitlines() if l.startswith("GRP_TRACE_INGEST source:")])
    assert all(int(GZIP_SEGS.search(l).group(1)) > 0 for l in lines), lines  # the first full pass too reads through segments
    assert rp.stderr.index("gzip walk:") < rp.stderr.index("GRP_TRACE_INGEST source:")
    # the log of the run proper is that of the run without the switch
    keep = lambda s: [l for l in s.splitlines() if not (l.startswith("in ") or "(sec)" in l or l.startswith("GRP_TRACE_INGEST"))]
    assert keep(rp.stderr) == keep(unset[0].stderr)


def test_off_is_unset(host, data, unset, tmp_path, monkeypatch):
    _no_switch(monkeypatch)
    rp = _product(host, tmp_path / "p", ARGS, [data["fofn"]], {"GRP_GZIP_WALK": "off"})
    assert rp.returncode == 0 and "gzip walk" not in rp.stderr
    for f in data["oracle"](ARGS, data["twin"])[2]:
        assert (tmp_path / "p" / f).read_bytes() == (unset[1] / f).read_bytes(), f


def test_a_bad_value_ends_the_run_before_the_first_pass(host, data, tmp_path, monkeypatch):
    _no_switch(monkeypatch)
    rp = _product(host, tmp_path / "p", ARGS, [data["fofn"]], {"GRP_GZIP_WALK": "maybe"})
    assert rp.returncode == 1, rp.stderr[-2000:]
    assert "GRP_GZIP_WALK=maybe" in rp.stderr and "on or off" in rp.stderr
    assert "opening: " not in rp.stderr and "GRP_TRACE_INGEST" not in rp.stderr and not list((tmp_path / "p").iterdir())
