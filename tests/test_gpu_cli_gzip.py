"""GPU end-to-end: goldrush-path on plain gzip FASTQ.  The first pass that reads the file to its end goes through zlib and
writes down the restart points (csrc/host/gr_gzidx.cpp); every pass behind it has the device inflate the segments
(grp_gzip_inflate) in front of the ingest.  Every output file and the log are those of the run on the plain file, at a
point on every block (GRP_GZIP_SPAN=1) and every 200 000 bytes, with slots (GRP_INGEST_CHUNK) of 100 000 and 400 000 bytes
and of the default size.  zlib puts 130 to 180 KB of this file's text into one block, so no segment fits a slot of 100 000
bytes: that index is unusable and every pass stays with zlib (the index itself says so: its longest segment); slots of
400 000 bytes hold one or two segments each."""
import os
import re

import pytest

import gzip_cases as G
from cli_runner import cli, traced, log as _log, run as _run  # noqa: F401 (cli: a fixture)
from test_gpu_cli import _mk_fastq

pytestmark = pytest.mark.gpu

SILVER = ["-k22", "-w16", "-t500", "-u5", "-a1", "-o0.1", "-h3", "-j4", "-d5", "-x10", "-s1011011110110111101101", "-g150000", "-b4", "-H2500000", "-P0", "-r0.9",
          "--silver_path", "-M2", "-m3500", "--verbose"]
NTCARD = ["-k22", "-w16", "-t500", "-u5", "-a1", "-o0.1", "-h3", "-j4", "-d5", "-x10", "-s1011011110110111101101", "-g150000", "-b4", "-P0", "-m0", "--ntcard", "--verbose"]
TRACE = re.compile(r"gzip segments inflated on the device (\d+)")


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("gzip_cli")
    fq = str(d / "reads.fq")
    _mk_fastq(fq, 150_000, 260, 6000, 4000, seed=31, lower=True, with_n=13)  # (the 3 MB file of test_gpu_cli_bgzf.py)
    text = open(fq, "rb").read()
    cut = text.index(b"\n@", len(text) // 3) + 1000  # the members meet inside a record
    files = {"level1": G.member(text, 1), "level6": G.member(text, 6), "two_members": G.member(text[:cut], 6) + G.member(text[cut:], 1)}
    paths = {"plain": fq}
    for name, data in files.items():
        paths[name] = str(d / (name + ".fq.gz"))
        open(paths[name], "wb").write(data)
    return paths


def _traced(rp):
    return traced(rp, TRACE)


@pytest.fixture(scope="module")
def plain(cli, inputs, tmp_path_factory):
    out = {}
    for form, args in (("silver", SILVER), ("ntcard", NTCARD)):
        rp, files = _run(cli, tmp_path_factory, args, inputs["plain"])
        assert rp.returncode == 0 and files and all(files.values()), rp.stderr[-2000:]
        assert set(_traced(rp)) == {0}
        out[form] = (rp, files)
    return out


def _fits(path, span, chunk):
    """the index's longest segment fits a slot: the passes behind the first use it"""
    from goldrush_amd import host

    return not chunk or host.gzip_index(path, span)["max_text"] <= chunk


def _check(rp, files, plain, path, used):
    assert rp.returncode == 0, rp.stderr[-2000:]
    assert files == plain[1]
    assert _log(rp, path) == _log(plain[0], path.rsplit("/", 1)[0] + "/reads.fq")
    n = _traced(rp)
    if used:  # nothing in the pass that builds the index, segments in every pass behind it
        assert len(n) >= 2 and n[0] == 0 and all(x > 0 for x in n[1:]), n
    else:
        assert set(n) == {0}, n


@pytest.mark.parametrize("name", ["level1", "level6", "two_members"])
@pytest.mark.parametrize("span,chunk", [(1, 100000), (200000, 100000), (1, 400000), (200000, 400000), (200000, 0)])
def test_gzip_input_gives_the_plain_files_outputs(cli, inputs, plain, tmp_path_factory, name, span, chunk):
    env = {"GRP_GZIP_SPAN": str(span)}
    if chunk:
        env["GRP_INGEST_CHUNK"] = str(chunk)
    rp, files = _run(cli, tmp_path_factory, SILVER, inputs[name], **env)
    used = _fits(inputs[name], span, chunk)
    assert used == (chunk != 100000)
    _check(rp, files, plain["silver"], inputs[name], used)


@pytest.mark.parametrize("name,span,chunk", [("level1", 200000, 400000), ("level6", 1, 100000), ("two_members", 1, 0)])
def test_ntcard_form(cli, inputs, plain, tmp_path_factory, name, span, chunk):
    env = {"GRP_GZIP_SPAN": str(span)}
    if chunk:
        env["GRP_INGEST_CHUNK"] = str(chunk)
    rp, files = _run(cli, tmp_path_factory, NTCARD, inputs[name], **env)
    _check(rp, files, plain["ntcard"], inputs[name], _fits(inputs[name], span, chunk))
    assert len(_traced(rp)) >= 3  # the --ntcard pass, the fill and the classification


def test_switch_selects_the_zlib_path(cli, inputs, plain, tmp_path_factory):
    rp, files = _run(cli, tmp_path_factory, SILVER, inputs["level6"], GRP_GZIP_INDEX="off", GRP_GZIP_SPAN="1")
    _check(rp, files, plain["silver"], inputs["level6"], used=False)


def test_a_truncated_file_is_an_error(cli, inputs, tmp_path_factory):
    path = inputs["level6"][:-6] + "_cut.fq.gz"
    data = open(inputs["level6"], "rb").read()
    open(path, "wb").write(data[:len(data) // 2])
    rp, _ = _run(cli, tmp_path_factory, SILVER, path, GRP_GZIP_SPAN="1")
    assert rp.returncode != 0, "a truncated gzip file passed for a shorter input"
    assert "failed" in rp.stderr and os.path.basename(path) in rp.stderr, rp.stderr[-2000:]
