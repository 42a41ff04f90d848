"""What the end-to-end GPU tests of compressed input share (tests/test_gpu_cli_bgzf.py, tests/test_gpu_cli_gzip.py): the
goldrush-path binary, a run of it with the ingest's trace on, its log without what differs between two runs, and the
counts of its GRP_TRACE_INGEST lines."""
import os
import subprocess

import pytest


@pytest.fixture(scope="module")
def cli(native):
    from goldrush_amd import host as h

    assert os.path.exists(h.CLI_PATH), "goldrush-path binary missing: run __graft_entry__.build()"
    return h.CLI_PATH


def run(cli, tmp_path_factory, args, path, **env):
    d = tmp_path_factory.mktemp("run")
    e = dict(os.environ, GRP_TRACE_INGEST="1", **env)
    for k in ("GRP_GZIP_INDEX", "GRP_GZIP_SPAN", "GRP_GZIP_INDEX_MAX_GB", "GRP_INGEST_CHUNK"):
        if k not in env:
            e.pop(k, None)
    rp = subprocess.run([cli] + args + ["-i", path, "-p", str(d / "out")], capture_output=True, text=True, timeout=900, env=e)
    files = {f: open(d / f, "rb").read() for f in sorted(os.listdir(d))}
    return rp, files


def log(rp, path):
    """stderr without the timing lines (and the input's name)"""
    return [l.replace(path, "INPUT") for l in rp.stderr.splitlines() if not (l.startswith("in ") or "(sec)" in l or l.startswith("GRP_TRACE_INGEST"))]


def traced(rp, trace):
    n = [int(x) for x in trace.findall(rp.stderr)]
    assert n, "no GRP_TRACE_INGEST line"
    return n
