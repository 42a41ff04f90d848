"""GPU end-to-end: goldrush-path on unaligned BAM.  The members are inflated on the device, the records parsed and packed
there (grp_bam_parse); every output file and the log are those of the run on the FASTQ twin, whatever routes the input —
the chunk size, zlib in place of the device's inflate, the host reader — and a damaged file ends the run with an error."""
import os

import numpy as np
import pytest

import bam_cases as BC
from cli_runner import cli, traced, log as _log, run as _run  # noqa: F401 (cli: a fixture)
from test_gpu_cli import _mk_fastq
from test_gpu_cli_bgzf import NTCARD, SILVER, SIZES, TRACE

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("bam_cli")
    reads = _mk_fastq(str(d / "source.fq"), 150_000, 260, 6000, 4000, seed=31, lower=False, with_n=13)
    recs = [dict(name=rid.split(b" ")[0], bases=seq, quals=bytes(q - 33 for q in qual), cigar=(16,) * (i % 3), tags=b"rqf\0\0\x80\x3f" * (i % 4), pad=i % 16, flag=4 | (77 if i % 2 else 0))
            for i, (rid, seq, qual) in enumerate(reads)]
    rng = np.random.default_rng(5)
    long_read = dict(name=b"a_read_longer_than_a_chunk", bases=np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=100_001)].tobytes(), quals=bytes([40]) * 100_001, pad=9)
    recs.insert(100, long_read)
    text = b"@HD\tVN:1.6\tSO:unknown\n" + b"@CO\t" + b"c" * 200_000 + b"\n"
    raw, hb, twin = BC.stream(recs, text=text, refs=[(b"chr1", 1000)])
    whole = BC.B.bgzf_file(raw, SIZES)
    files = {"bam": whole}
    at = BC.walk(raw[hb:])[0]
    files["cut"] = BC.B.bgzf_file(raw[:hb + at[150]["off"] + 1000], SIZES)  # cut at a member boundary inside a record: BGZF is intact, BAM is not
    for name, change in (("flag16", dict(flag=16)), ("noqual", dict(quals=b"\xff" * len(recs[150]["bases"])))):
        bad = [dict(r) for r in recs]
        bad[150].update(change)
        files[name] = BC.B.bgzf_file(BC.stream(bad, text=text)[0], SIZES)
    paths = {"twin": str(d / "twin.fq")}
    open(paths["twin"], "wb").write(twin)
    for name, data in files.items():
        paths[name] = str(d / (name + ".bam"))
        open(paths[name], "wb").write(data)
    return paths, len(BC.B.walk_members(whole)[0])


@pytest.fixture(scope="module")
def twin(cli, inputs, tmp_path_factory):
    rp, files = _run(cli, tmp_path_factory, SILVER, inputs[0]["twin"])
    assert rp.returncode == 0 and files and all(files.values()), rp.stderr[-2000:]
    return rp, files


@pytest.mark.parametrize("env", [{}, {"GRP_INGEST_CHUNK": "4096"}, {"GRP_INGEST_CHUNK": "100000"}, {"GRP_BGZF": "off"}, {"GRP_HOST_INGEST": "1"}])
def test_bam_input_gives_the_twins_outputs(cli, inputs, twin, tmp_path_factory, env):
    paths, n_members = inputs
    rp, files = _run(cli, tmp_path_factory, SILVER, paths["bam"], **env)
    assert rp.returncode == 0, rp.stderr[-2000:]
    assert files == twin[1]
    assert _log(rp, paths["bam"]) == _log(twin[0], paths["twin"])
    if "GRP_HOST_INGEST" in env:
        return
    n = traced(rp, TRACE)
    if "GRP_BGZF" in env:
        assert set(n) == {0}, n  # the bytes came through zlib; the parse is still the device's
    else:
        assert all(x > 0 for x in n), n  # every pass had the device inflate its members ...
    if not env:                          # ... all of them, but for the classification, which ends with its last silver path
        assert max(n) == n_members and all(x <= n_members for x in n), n


def test_ntcard_form(cli, inputs, tmp_path_factory):
    paths, n_members = inputs
    ro, fo = _run(cli, tmp_path_factory, NTCARD, paths["twin"])
    rp, fp = _run(cli, tmp_path_factory, NTCARD, paths["bam"])
    assert ro.returncode == rp.returncode == 0, rp.stderr[-2000:]
    assert fp == fo and fo and all(fo.values())
    assert _log(rp, paths["bam"]) == _log(ro, paths["twin"])
    n = traced(rp, TRACE)
    assert len(n) >= 3 and max(n) == n_members and all(0 < x <= n_members for x in n), n  # the --ntcard pass, the fill and the classification


@pytest.mark.parametrize("name", ["cut", "flag16", "noqual"])
def test_a_damaged_bam_file_is_an_error(cli, inputs, tmp_path_factory, name):
    path = inputs[0][name]
    rp, _ = _run(cli, tmp_path_factory, SILVER, path, GRP_INGEST_CHUNK="200000")
    assert rp.returncode != 0, "a damaged BAM file passed for a shorter input"
    assert "failed" in rp.stderr and os.path.basename(path) in rp.stderr, rp.stderr[-2000:]
    if name == "flag16":
        assert "samtools fastq" in rp.stderr
