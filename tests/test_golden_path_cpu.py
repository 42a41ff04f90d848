"""CPU: --golden_path — the golden path behind the silver paths in one run (csrc/host/gr_path.cpp, gr_golden.cpp).  The
product's whole host program runs over the oracle engine (tests/golden_runner.py: grp_reads_gather and grp_rewind restated
over its batches).  The fused run on either route — the silver reads handed over on the device, or read back from their
files — writes the files and the log of the pipeline's two runs: process #1, then process #2 over the silver files that hold
something, in the byte order of their names (what `cat PREFIX_*.fq` gives)."""
import json
import os
import subprocess
import sys

import pytest

import golden_runner as GR
import test_bam_cpu as TB

ROOT = TB.ROOT
SILVER = ["-P0", "-r0.9", "--silver_path", "-M4", "-m1500", "-g12000"]
# a path per inserted read (90 bases fill one): more than ten silver files, and an empty one behind the last read
MANY = ["-P0", "-r0.9", "--silver_path", "-M100", "-m1500", "-g100"]
ENV_KEYS = ("GRP_HOST_INGEST", "GRP_INGEST_CHUNK", "GRP_BATCH_RECORDS", "GRP_BGZF", "GRP_RESIDENT", "GRP_RESIDENT_MAX_GB", "GRP_GZIP_INDEX", "GRP_GOLDEN_RESIDENT", "GRP_WORLD", "GRP_RANK", "WORLD_SIZE", "RANK",
            "BAM_STAND_IN", "FETCH_STAND_IN", "GOLDEN_NO_ENTRIES", "GOLDEN_GATHER_NOMEM")
FALLBACK = "--golden_path: the silver reads are read back from their files: "
TRACE = "GRP_TRACE_INGEST golden: "


def _tiny():
    lines = open(os.path.join(TB.GOLD, "tiny.fq"), "rb").read().split(b"\n")
    return [(lines[4 * i][1:], lines[4 * i + 1], lines[4 * i + 3]) for i in range(len(lines) // 4)]


def _fastq(recs):
    return b"".join(b"@" + n + b"\n" + s + b"\n+\n" + q + b"\n" for n, s, q in recs)


@pytest.fixture(scope="module")
def work(tmp_path_factory, oracle, native):
    d = tmp_path_factory.mktemp("golden_cpu")
    (d / "runner.py").write_text(GR.RUNNER.format(root=ROOT))
    recs = _tiny()
    (d / "tiny.fq").write_bytes(_fastq(recs))
    # the same reads with qualities that change from tile to tile: a written slice's average is not its read's, so the
    # second stage's median and its Phred filters have something to decide
    varied = [(n, s, bytes(33 + 8 + ((5 * i + 11 * (j // 500)) % 31) for j in range(len(s)))) for i, (n, s, q) in enumerate(recs)]
    (d / "varied.fq").write_bytes(_fastq(varied))
    return d


def _run(work, tag, args, **env):
    d = work / tag
    d.mkdir()
    e = dict(os.environ, OMP_NUM_THREADS="2", GRP_TRACE_INGEST="1", GOLDEN_OUT=str(work / (tag + ".calls.json")))
    for k in ENV_KEYS:
        e.pop(k, None)
    e.update(env)
    rp = subprocess.run([sys.executable, str(work / "runner.py")] + TB.COMMON + args, capture_output=True, text=True, timeout=900, env=e, cwd=d)
    calls = json.load(open(e["GOLDEN_OUT"])) if os.path.exists(e["GOLDEN_OUT"]) else None
    return rp, {f: open(d / f, "rb").read() for f in sorted(os.listdir(d))}, calls


def _log(rp, strip=()):
    """stderr without the timing and trace lines, the line that says why the files are read back, and the run's own directories"""
    out = []
    for l in rp.stderr.splitlines():
        if l.startswith("in ") or "(sec)" in l or l.startswith("GRP_TRACE_INGEST") or l.startswith(FALLBACK):
            continue
        for s in strip:
            l = l.replace(s, "")
        out.append(l)
    return out


def _pipeline(work, tag, input_, stage_a, extra=(), **env):
    """process #1, then process #2 on its silver files (-i each, in the byte order of their names, the empty ones left out)
    and on their concatenation: the two must agree (several inputs are their concatenation); -> the runs and the order"""
    a, fa, _ = _run(work, tag + "_a", stage_a + list(extra) + ["-i", str(input_), "-p", "out"], **env)
    assert a.returncode == 0 and fa, a.stderr[-3000:]
    order = sorted((f for f in fa if fa[f]), key=lambda f: f.encode())
    assert order, "the first stage wrote nothing"
    common_b = ["-P0", "-m0"] + list(extra) + ["-p", "gold"]
    args = []
    for f in order:
        args += ["-i", str(work / (tag + "_a") / f)]
    b, fb, _ = _run(work, tag + "_b", common_b + args, **env)
    (work / (tag + "_all.fq")).write_bytes(b"".join(fa[f] for f in order))
    c, fc, _ = _run(work, tag + "_c", common_b + ["-i", str(work / (tag + "_all.fq"))], **env)
    assert b.returncode == c.returncode == 0 and fb == fc and fb["gold.fa"], (b.stderr[-2000:], c.stderr[-2000:])
    return a, fa, b, fb, order


def _fused(work, tag, input_, stage_a, extra=(), **env):
    return _run(work, tag, stage_a + list(extra) + ["-i", str(input_), "-p", "out", "--golden_path", "gold"], **env)


def _same(work, tag, pipe, fused):
    a, fa, b, fb, order = pipe
    f, ff, calls = fused
    assert f.returncode == 0, f.stderr[-3000:]
    assert ff == dict(fa, **fb), (sorted(ff), sorted(fa), sorted(fb))
    strip_pipe = [str(work / d) + "/" for d in os.listdir(work) if (work / d).is_dir()]
    assert _log(f, strip_pipe) == _log(a, strip_pipe) + _log(b, strip_pipe)
    trace = [l for l in f.stderr.splitlines() if l.startswith(TRACE)]
    assert len(trace) == 1
    return trace[0], [l for l in f.stderr.splitlines() if l.startswith(FALLBACK)], calls


@pytest.fixture(scope="module")
def pipe(work):
    return _pipeline(work, "pipe", work / "tiny.fq", SILVER)


@pytest.mark.parametrize("env", [{}, {"GRP_BATCH_RECORDS": "7"}, {"BAM_STAND_IN": "1"}, {"BAM_STAND_IN": "1", "GRP_RESIDENT": "off", "GRP_INGEST_CHUNK": "40000"}], ids=["plain", "small_batches", "ingest", "ingest_two_pass"])
def test_device_route_is_the_two_runs(work, pipe, env):
    tag = "dev_" + "_".join(sorted(env)).lower()
    trace, said, calls = _same(work, tag, pipe, _fused(work, tag, work / "tiny.fq", SILVER, **env))
    n = sum(pipe[1][f].count(b"\n+\n") for f in pipe[1])
    assert said == [] and "route=device" in trace and "records=%d " % n in trace and trace.endswith("bytes_read=0")
    parts, batches = (int(trace.split(k + "=")[1].split()[0]) for k in ("parts", "batches"))
    # one engine for both stages, rewound once; a gather per part and per batch of the second stage's fill
    assert calls["creates"] == 1 and calls["rewind"] == 1 and calls["gather"] == parts + batches and batches == len(pipe[4])
    assert parts >= (2 if "GRP_BATCH_RECORDS" in env or "GRP_INGEST_CHUNK" in env else 1)


@pytest.mark.parametrize("why,env,extra", [
    ("GRP_GOLDEN_RESIDENT=off", {"GRP_GOLDEN_RESIDENT": "off"}, []),
    ("--ntcard", {}, ["--ntcard"]),
    ("the engine has no grp_reads_gather / grp_rewind", {"GOLDEN_NO_ENTRIES": "1"}, []),
    ("no device memory for the silver reads", {"GOLDEN_GATHER_NOMEM": "2", "GRP_BATCH_RECORDS": "7"}, []),
    ("GRP_RESIDENT_MAX_GB", {"GRP_RESIDENT_MAX_GB": "0.00001"}, []),
], ids=["switch", "ntcard", "no_entries", "nomem", "cap"])
def test_file_route_is_the_two_runs_and_says_why(work, pipe, why, env, extra):
    tag = "file_" + "".join(c for c in why if c.isalnum())[:24]
    p = pipe if not extra else _pipeline(work, tag + "_pipe", work / "tiny.fq", SILVER, extra)
    trace, said, calls = _same(work, tag, p, _fused(work, tag, work / "tiny.fq", SILVER, extra, **env))
    assert len(said) == 1 and why in said[0], said
    assert "route=files" in trace and "parts=0" in trace and not trace.endswith("bytes_read=0")
    assert calls["creates"] == 2 and calls["rewind"] == 0  # (the second stage has its own engine)
    if "NOMEM" in "".join(env):
        assert calls["gather"] >= 2  # the parts cut before the refusal were freed; nothing of them is used


def test_debug_takes_the_file_route(work):
    p = _pipeline(work, "dbg_pipe", work / "tiny.fq", SILVER, ["--debug"])
    trace, said, calls = _same(work, "dbg", p, _fused(work, "dbg", work / "tiny.fq", SILVER, ["--debug"]))
    assert len(said) == 1 and "--debug" in said[0] and "route=files" in trace and calls["rewind"] == 0


@pytest.mark.parametrize("route", ["device", "files"])
def test_more_than_ten_paths_and_an_empty_last_file(work, route):
    env = {} if route == "device" else {"GRP_GOLDEN_RESIDENT": "off"}
    p = _pipeline(work, "many_pipe_" + route, work / "tiny.fq", MANY)
    a, fa, b, fb, order = p
    names = sorted(fa, key=lambda f: int(f[4:-3]))
    assert len(names) >= 12 and fa[names[-1]] == b"" and all(fa[f] for f in names[:-1])  # a path per inserted read, and the file opened behind the last
    assert order.index("out_10.fq") < order.index("out_2.fq") and names[-1] not in order
    fu = _fused(work, "many_" + route, work / "tiny.fq", MANY, **env)
    trace, said, calls = _same(work, "many_" + route, p, fu)
    f = fu[0]
    opened = [l[len("opening: "):].split("/")[-1] for l in f.stderr.splitlines() if l.startswith("opening: ") and "out_" in l]
    assert opened == order
    assert ("route=" + route) in trace


@pytest.mark.parametrize("route", ["device", "files"])
def test_ids_that_end_in_trimmed_already(work, pipe, route):
    """the silver reads of one run as the input of the next: ids "<id>_trimmed_trimmed", "<id>_untrimmed_trimmed", ..."""
    env = {} if route == "device" else {"GRP_GOLDEN_RESIDENT": "off"}
    src = work / "pipe_all.fq"
    stage_a = ["-P0", "-r0.9", "--silver_path", "-M3", "-m0", "-g9000"]
    p = _pipeline(work, "again_pipe_" + route, src, stage_a)
    text = b"".join(p[1].values())
    assert b"_trimmed_trimmed\n" in text or b"_trimmed_untrimmed\n" in text or b"_untrimmed_trimmed\n" in text
    trace, said, calls = _same(work, "again_" + route, p, _fused(work, "again_" + route, src, stage_a, **env))
    assert ("route=" + route) in trace


def test_median_from_the_stored_sums(work):
    """-P 0 in the second stage: its median and its Phred filters come from the sums kept with the records, and decide as the
    file run's decide from the text — on qualities that differ between a read and its written slice"""
    p = _pipeline(work, "var_pipe", work / "varied.fq", SILVER)
    b_log = p[2].stderr
    skipped = [int(l.split(":")[1]) for l in b_log.splitlines() if l.startswith(("num_reads_skipped_by_phred", "num_reads_skipped_by_delta"))]
    assert len(skipped) == 2 and sum(skipped) > 0, b_log[-2000:]  # the second stage's filters drop something
    assert "Minimum phred score calculated with median" in b_log
    trace, said, calls = _same(work, "var", p, _fused(work, "var", work / "varied.fq", SILVER))
    assert "route=device" in trace and said == []


@pytest.mark.parametrize("what,args,env,must", [
    ("no --silver_path", ["-P0", "-m0", "--golden_path", "gold"], {}, "--silver_path"),
    ("empty prefix", SILVER + ["--golden_path", ""], {}, "empty"),
    ("several ranks", SILVER + ["--golden_path", "gold"], {"GRP_WORLD": "2", "GRP_RANK": "0"}, "out of scope"),
])
def test_refused_before_the_first_pass(work, what, args, env, must):
    rp, files, calls = _run(work, "refused_" + what.replace(" ", "_").replace("-", ""), args + ["-i", str(work / "tiny.fq"), "-p", "out"], **env)
    lines = [l for l in rp.stderr.splitlines() if l.strip()]
    assert rp.returncode == 1 and len(lines) == 1 and "--golden_path" in lines[0] and must in lines[0], rp.stderr
    assert files == {} and calls["creates"] == 0  # nothing was opened, no engine made


def test_a_failing_first_stage_ends_the_run(work):
    rp, files, calls = _run(work, "nofile", SILVER + ["-i", str(work / "missing.fq"), "-p", "out", "--golden_path", "gold"])
    assert rp.returncode != 0 and "gold.fa" not in files and "Calculating the golden path" not in rp.stderr


def test_option_dump_and_usage_stay(native):
    from goldrush_amd import host

    rc, dump = host.process_options_dump(["-k22", "-w16", "-g100", "--silver_path", "--golden_path", "x"])
    rc0, dump0 = host.process_options_dump(["-k22", "-w16", "-g100", "--silver_path"])
    assert rc == rc0 == -1 and dump == dump0 and not any("golden" in k for k in dump)
