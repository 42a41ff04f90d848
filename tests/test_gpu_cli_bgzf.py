"""GPU end-to-end: goldrush-path on BGZF-compressed FASTQ.  The members are inflated on the device (grp_bgzf_inflate) in
front of the ingest; every output file and the log are those of the run on the plain file, whatever the chunking, and a
damaged file ends the run with an error."""
import gzip
import os
import re

import pytest

import bgzf_cases as B
from cli_runner import cli, traced, log as _log, run as _run  # noqa: F401 (cli: a fixture)
from test_gpu_cli import _mk_fastq

pytestmark = pytest.mark.gpu

SILVER = ["-k22", "-w16", "-t500", "-u5", "-a1", "-o0.1", "-h3", "-j4", "-d5", "-x10", "-s1011011110110111101101", "-g150000", "-b4", "-H2500000", "-P0", "-r0.9",
          "--silver_path", "-M2", "-m3500", "--verbose"]
NTCARD = ["-k22", "-w16", "-t500", "-u5", "-a1", "-o0.1", "-h3", "-j4", "-d5", "-x10", "-s1011011110110111101101", "-g150000", "-b4", "-P0", "-m0", "--ntcard", "--verbose"]
TRACE = re.compile(r"BGZF blocks inflated on the device (\d+)")
SIZES = [1, 65280, 7, 30011, 2, 64000, 513, 40000]  # text bytes per member: records straddle the members


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("bgzf_cli")
    fq = str(d / "reads.fq")
    _mk_fastq(fq, 150_000, 260, 6000, 4000, seed=31, lower=True, with_n=13)
    text = open(fq, "rb").read()
    cut = text.index(b"\n@", len(text) * 3 // 4) + 1
    whole = B.bgzf_file(text, SIZES)
    files = {"bgzf": whole, "bgzf_then_gzip": B.bgzf_file(text[:cut], SIZES) + gzip.compress(text[cut:], 1)}
    blocks = B.walk_members(whole)[0]
    off, ln = blocks[len(blocks) // 2][:2]
    files["cut"] = whole[:off + ln // 2]  # the file ends inside a member
    flipped = bytearray(whole)
    flipped[off + ln // 2] ^= 0x04
    files["flipped"] = bytes(flipped)
    paths = {"plain": fq}
    for name, data in files.items():
        paths[name] = str(d / (name + ".fq.gz"))
        open(paths[name], "wb").write(data)
    return paths, len(blocks)


def _traced(rp):
    return traced(rp, TRACE)


@pytest.fixture(scope="module")
def plain(cli, inputs, tmp_path_factory):
    rp, files = _run(cli, tmp_path_factory, SILVER, inputs[0]["plain"])
    assert rp.returncode == 0 and files and all(files.values()), rp.stderr[-2000:]
    assert set(_traced(rp)) == {0}
    return rp, files


@pytest.mark.parametrize("name,env", [("bgzf", {}), ("bgzf_then_gzip", {}), ("bgzf", {"GRP_INGEST_CHUNK": "4096"}), ("bgzf", {"GRP_INGEST_CHUNK": "100000"}),
                                      ("bgzf_then_gzip", {"GRP_INGEST_CHUNK": "100000"})])
def test_bgzf_input_gives_the_plain_files_outputs(cli, inputs, plain, tmp_path_factory, name, env):
    paths, n_members = inputs
    rp, files = _run(cli, tmp_path_factory, SILVER, paths[name], **env)
    assert rp.returncode == 0, rp.stderr[-2000:]
    assert files == plain[1]
    assert _log(rp, paths[name]) == _log(plain[0], paths["plain"])
    n = _traced(rp)
    assert all(x > 0 for x in n), n  # every pass had the device inflate its members ...
    if name == "bgzf":            # ... all of them, but for the classification, which ends with its last silver path
        assert max(n) == n_members and all(x <= n_members for x in n), n


def test_a_file_written_by_libdeflate_gives_the_plain_files_outputs(cli, tmp_path_factory):
    """tests/golden/tiny_libdeflate.fq.gz: tiny.fq as bgzip writes it (htslib's encoder is libdeflate, not zlib)"""
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    fq, gz = os.path.join(gold, "tiny.fq"), os.path.join(gold, "tiny_libdeflate.fq.gz")
    n_members = len(B.walk_members(open(gz, "rb").read())[0])
    ro, fo = _run(cli, tmp_path_factory, SILVER, fq)
    rp, fp = _run(cli, tmp_path_factory, SILVER, gz)
    assert ro.returncode == rp.returncode == 0, rp.stderr[-2000:]
    assert fp == fo and fo
    assert _log(rp, gz) == _log(ro, fq)
    assert set(_traced(ro)) == {0}
    n = _traced(rp)
    assert max(n) == n_members == 4 and all(0 < x <= n_members for x in n), n


def test_switch_selects_the_zlib_path(cli, inputs, plain, tmp_path_factory):
    rp, files = _run(cli, tmp_path_factory, SILVER, inputs[0]["bgzf"], GRP_BGZF="off")
    assert rp.returncode == 0, rp.stderr[-2000:]
    assert files == plain[1] and set(_traced(rp)) == {0}
    assert _log(rp, inputs[0]["bgzf"]) == _log(plain[0], inputs[0]["plain"])


@pytest.mark.parametrize("name", ["cut", "flipped"])
def test_a_damaged_bgzf_file_is_an_error(cli, inputs, tmp_path_factory, name):
    path = inputs[0][name]
    rp, _ = _run(cli, tmp_path_factory, SILVER, path, GRP_INGEST_CHUNK="200000")
    assert rp.returncode != 0, "a damaged BGZF file passed for a shorter input"
    assert "failed" in rp.stderr and os.path.basename(path) in rp.stderr, rp.stderr[-2000:]


def test_ntcard_form(cli, inputs, tmp_path_factory):
    paths, n_members = inputs
    ro, fo = _run(cli, tmp_path_factory, NTCARD, paths["plain"])
    rp, fp = _run(cli, tmp_path_factory, NTCARD, paths["bgzf"])
    assert ro.returncode == rp.returncode == 0, rp.stderr[-2000:]
    assert fp == fo and fo and all(fo.values())
    assert _log(rp, paths["bgzf"]) == _log(ro, paths["plain"])
    n = _traced(rp)
    assert len(n) >= 3 and max(n) == n_members and all(0 < x <= n_members for x in n), n  # the --ntcard pass, the fill and the classification
