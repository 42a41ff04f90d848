"""The oracle's whole path against the MINI REFERENCE: calc_num_assigned_tiles, the body of process_read,
silver_path_check, insertMIBF (unique ranks, count, reservoir test) / setData / atRank / getData ... compiled from
the reference's own text (oracle/ref_mini_main.cpp says what is the reference's and what is ours: the hashes, the
bit vector + rank, the set, the record type).  Same reads, same flags:
  * live, wherever oracle/_ref/ref_mini exists (the build container; the binary travels to the GPU box): the files
    the mini reference writes, its counters and the IDs / counts of every rank equal the oracle's — elsewhere what
    tests/golden/reference_mini.json stored of them (files, counters, sha256 of the IDs / counts) does;
  * everywhere: the oracle CLI's files equal the sha256 the mini reference's files had when
    tests/golden/reference_mini.json was made (tests/golden/make_reference_fixtures.py);
  * -m gpu: so do the files of the product's goldrush-path on the HIP engine.
Rows a8-a10 (what feeds the vote), a13 (decision glue, ID allocation, output), a14 (reservoir rule, setData, the
vec_size indexing of insertMIBF) and a15 (rollover) of SURVEY.md 8 are pinned by this down to the hash values,
the positional semantics of bit vector + rank and the uniqueness of a set."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import ref_mini

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "reference_mini.json")


@pytest.mark.parametrize("case", [c[0] for c in ref_mini.CASES])
def test_oracle_path_equals_the_mini_reference(oracle, tmp_path, case):
    """Live where oracle/_ref/ref_mini is built; elsewhere against what it wrote when tests/golden/reference_mini.json was
    made: its files, its end-state counters and the sha256 of its ID / count arrays (its --verbose log is live only)."""
    live = os.path.exists(ref_mini.BIN)
    name, spec, flags = next(c for c in ref_mini.CASES if c[0] == case)
    fq = ref_mini.make_fastq(spec, str(tmp_path / "reads.fq"))
    args = flags + ["-i", fq]
    pre_r, pre_o = str(tmp_path / "ref"), str(tmp_path / "orc")
    p, seeds = ref_mini.write_scenario(oracle, args, str(tmp_path / "scenario.bin"), pre_r)
    p.close()
    rr = ref_mini.run_mini(str(tmp_path / "scenario.bin")) if live else None
    # the oracle: its CLI for the files and the log, the library for the end state
    ro = oracle.run_cli(args + ["-p", pre_o], timeout=600)
    assert ro.returncode == 0, ro.stderr[-2000:]
    if live:
        assert ref_mini.outputs(pre_r) == ref_mini.outputs(pre_o) and ref_mini.outputs(pre_r)
        st, ids, counts = ref_mini.mini_state(pre_r)
    else:
        exp = _fixture()["cases"][case]
        assert ref_mini.sha(fq) == exp["input_sha256"]
        assert ref_mini.outputs(pre_o) == exp["files"] and exp["files"]
        st = exp["state"]
    q = oracle.Path(args + ["-p", str(tmp_path / "orc2")])
    decs = q.run_all()
    li = q.log_info()
    o = q.opts
    mf = q.mibf(o.tile_length, o.kmer_size, seeds)
    if live:
        assert np.array_equal(mf.ids(), ids) and np.array_equal(mf.counts(), counts)
        assert int(counts.max()) >= 1
    else:
        assert hashlib.sha256(mf.ids().tobytes()).hexdigest() == exp["ids_sha256"]
        assert hashlib.sha256(mf.counts().tobytes()).hexdigest() == exp["counts_sha256"]
        assert int(mf.counts().max()) == exp["max_count"] >= 1
    for mine, theirs in ref_mini.LOG_KEYS.items():
        assert st[mine] == li[theirs], (mine, st[mine], li[theirs])
    assert st["phred_sum_in_path_bits"] == int(np.float64(li["phred_sum_in_path"]).view(np.uint64))
    q.close()
    # the per-path log of --verbose (log_path_stat is the reference's own function there)
    keep = ("Visited", "Saw:", "Assigned:", "Unassigned:", "Total queries", "Total hits", "Total misses", "Num reads", "Average Phred")
    pick = lambda text: [l for l in text.splitlines() if l.startswith(keep)]  # noqa: E731
    if live:
        assert pick(rr.stderr) == pick(ro.stderr)
    kinds = {d[0] for d in decs}
    if case.startswith("cover5_b"):
        assert {2, 4} <= kinds  # whole and trimmed inserts
    if case == "cover5_silver_h5":  # the paths roll over and the run ends by the reference's exit(0) inside silver_path_check
        assert st["exit_in_silver_path_check"] and st["curr_path"] == o.max_paths + 1


def _fixture():
    return json.load(open(FIX))


@pytest.mark.parametrize("case", [c[0] for c in ref_mini.CASES])
def test_oracle_cli_writes_the_mini_references_files(oracle, tmp_path, case):
    name, spec, flags = next(c for c in ref_mini.CASES if c[0] == case)
    exp = _fixture()["cases"][case]
    fq = ref_mini.make_fastq(spec, str(tmp_path / "reads.fq"))
    assert ref_mini.sha(fq) == exp["input_sha256"]  # the same reads as when the fixture was made
    pre = str(tmp_path / "orc")
    ro = oracle.run_cli(flags + ["-i", fq, "-p", pre], timeout=600)
    assert ro.returncode == 0, ro.stderr[-2000:]
    assert ref_mini.outputs(pre) == exp["files"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c[0] for c in ref_mini.CASES])
def test_product_cli_writes_the_mini_references_files(native, tmp_path, case):
    from goldrush_amd import host

    name, spec, flags = next(c for c in ref_mini.CASES if c[0] == case)
    exp = _fixture()["cases"][case]
    fq = ref_mini.make_fastq(spec, str(tmp_path / "reads.fq"))
    assert ref_mini.sha(fq) == exp["input_sha256"]
    pre = str(tmp_path / "hip")
    rp = subprocess.run([host.CLI_PATH] + flags + ["-i", fq, "-p", pre], capture_output=True, text=True, timeout=900)
    assert rp.returncode == 0, rp.stderr[-2000:]
    assert ref_mini.outputs(pre) == exp["files"]
