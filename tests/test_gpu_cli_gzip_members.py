"""GPU end-to-end: goldrush-path with GRP_GZIP_WALK=on and GRP_GZIP_WALK_MEMBERS=on on ONE .fastq.gz of six members — what
`cat cell*.fastq.gz > reads.fq.gz` makes — whose members meet inside records, not only between them.  In front of the
first pass the members are walked side by side on the device (csrc/host/gr_gzwalk.cpp: GzWalkMembers): the chain from
byte 0 adopts the five streams begun behind it.  The output files are those of the run with the walk alone, of the run
with neither switch and of the oracle CLI on the FASTQ twin."""
import re

import pytest

import gzip_cases as G
from test_gpu_cli_multi_input import BASE, SIZED, SILVER, GZIP_SEGS, Oracle, _fastq, _product, _same, host  # noqa: F401 (host: a fixture)
from test_gpu_cli import _mk_fastq

pytestmark = pytest.mark.gpu

WALK = re.compile(r"^GRP_TRACE_INGEST gzip walk: files=(\d+) walked=(\d+) left_to_zlib=(\d+) rounds=(\d+) text=(\d+) seconds=([0-9.e+-]+)$", re.M)
MEMBERS = re.compile(r"^GRP_TRACE_INGEST gzip walk members: candidates=(\d+) streams=(\d+) adopted=(\d+) dropped=(\d+) max_in_flight=(\d+) wasted_text=(\d+) scan_seconds=([0-9.e+-]+)$", re.M)
ARGS = BASE + SIZED + SILVER
BOTH = {"GRP_GZIP_WALK": "on", "GRP_GZIP_WALK_MEMBERS": "on"}


@pytest.fixture(scope="module")
def data(oracle, tmp_path_factory):
    d = tmp_path_factory.mktemp("gzip_members_cli")
    recs = _mk_fastq(str(d / "source.fq"), 200_000, 300, 6000, 4000, seed=79, lower=True, with_n=17, short=9)
    text = _fastq(recs)
    # five cuts: inside a sequence line, inside a quality line, inside a name, between two records, one byte behind a record's first
    marks = [text.index(b"\n@", len(text) * i // 6) + 1 for i in range(1, 6)]
    cuts = [0, marks[0] + 700, marks[1] - 300, marks[2] + 5, marks[3], marks[4] + 1, len(text)]
    assert cuts == sorted(cuts) and sum(text[c - 1:c] == b"\n" for c in cuts[1:-1]) == 1
    parts = [text[cuts[i]:cuts[i + 1]] for i in range(6)]
    one = d / "reads.fq.gz"
    one.write_bytes(b"".join(G.member(p, (6, 1, 9, 0, 6, 1)[i]) for i, p in enumerate(parts)))
    twin = d / "twin.fq"
    twin.write_bytes(text)
    return dict(gz=one, twin=twin, n_text=len(text), oracle=Oracle(oracle, d))


@pytest.fixture(scope="module")
def neither(host, data, tmp_path_factory):
    d = tmp_path_factory.mktemp("neither") / "p"
    return _product(host, d, ARGS, [data["gz"]]), d


def _no_switch(monkeypatch):
    for k in ("GRP_GZIP_WALK", "GRP_GZIP_WALK_MEMBERS", "GRP_GZIP_WALK_STREAMS", "GRP_GZIP_WALK_ROOM", "GRP_GZIP_SPAN", "GRP_GZIP_INDEX_MAX_GB"):
        monkeypatch.delenv(k, raising=False)


def _walk_line(rp, data):
    walks = WALK.findall(rp.stderr)
    assert len(walks) == 1, rp.stderr[-3000:]
    files, walked, left, rounds, text, seconds = walks[0]
    assert (int(files), int(walked), int(left)) == (1, 1, 0) and int(text) == data["n_text"], walks
    return int(rounds)


def test_neither_switch(neither, data):
    rp, d = neither
    _same(rp, d, data["oracle"](ARGS, data["twin"]))
    assert "gzip walk" not in rp.stderr


def test_both_switches_give_the_same_files(host, data, neither, tmp_path, monkeypatch):
    _no_switch(monkeypatch)
    rp = _product(host, tmp_path / "p", ARGS, [data["gz"]], BOTH)
    _same(rp, tmp_path / "p", data["oracle"](ARGS, data["twin"]))
    for f in data["oracle"](ARGS, data["twin"])[2]:
        assert (tmp_path / "p" / f).read_bytes() == (neither[1] / f).read_bytes(), f
    rounds = _walk_line(rp, data)
    members = MEMBERS.findall(rp.stderr)
    assert len(members) == 1, rp.stderr[-3000:]
    candidates, streams, adopted, dropped, in_flight, wasted, scan = members[0]
    assert int(adopted) == 5 and int(candidates) >= 5 and int(in_flight) >= 6, members
    assert rp.stderr.index("gzip walk:") < rp.stderr.index("gzip walk members:") < rp.stderr.index("GRP_TRACE_INGEST source:")
    lines = [l for l in rp.stderr.splitlines() if l.startswith("GRP_TRACE_INGEST source:")]
    assert all(int(GZIP_SEGS.search(l).group(1)) > 0 for l in lines), lines  # the first pass too reads through segments
    # the walk alone: the same files, no second line, and the rounds of six members one after the other
    ro = _product(host, tmp_path / "w", ARGS, [data["gz"]], {"GRP_GZIP_WALK": "on"})
    assert ro.returncode == 0 and "gzip walk members" not in ro.stderr
    for f in data["oracle"](ARGS, data["twin"])[2]:
        assert (tmp_path / "w" / f).read_bytes() == (neither[1] / f).read_bytes(), f
    assert _walk_line(ro, data) > rounds
    keep = lambda s: [l for l in s.splitlines() if not (l.startswith("in ") or "(sec)" in l or l.startswith("GRP_TRACE_INGEST"))]
    assert keep(rp.stderr) == keep(ro.stderr) == keep(neither[0].stderr)


def test_members_without_the_walk_has_no_effect(host, data, neither, tmp_path, monkeypatch):
    _no_switch(monkeypatch)
    rp = _product(host, tmp_path / "p", ARGS, [data["gz"]], {"GRP_GZIP_WALK_MEMBERS": "on"})
    assert rp.returncode == 0 and "gzip walk" not in rp.stderr
    for f in data["oracle"](ARGS, data["twin"])[2]:
        assert (tmp_path / "p" / f).read_bytes() == (neither[1] / f).read_bytes(), f


def test_resident_all(host, data, neither, tmp_path, monkeypatch):
    _no_switch(monkeypatch)
    rp = _product(host, tmp_path / "p", ARGS, [data["gz"]], dict(BOTH, GRP_RESIDENT="all"))
    _same(rp, tmp_path / "p", data["oracle"](ARGS, data["twin"]))
    for f in data["oracle"](ARGS, data["twin"])[2]:
        assert (tmp_path / "p" / f).read_bytes() == (neither[1] / f).read_bytes(), f
    _walk_line(rp, data)
    assert [m[2] for m in MEMBERS.findall(rp.stderr)] == ["5"], rp.stderr[-3000:]
    assert "GRP_RESIDENT=all: the reads are not kept" not in rp.stderr


def test_a_bad_value_ends_the_run_before_the_first_pass(host, data, tmp_path, monkeypatch):
    _no_switch(monkeypatch)
    rp = _product(host, tmp_path / "p", ARGS, [data["gz"]], {"GRP_GZIP_WALK": "on", "GRP_GZIP_WALK_MEMBERS": "maybe"})
    assert rp.returncode == 1, rp.stderr[-2000:]
    assert "GRP_GZIP_WALK_MEMBERS=maybe" in rp.stderr and "on or off" in rp.stderr
    assert "opening: " not in rp.stderr and "GRP_TRACE_INGEST" not in rp.stderr and not list((tmp_path / "p").iterdir())
