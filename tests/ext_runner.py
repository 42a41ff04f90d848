"""The product's whole host program (gr_path_main_ext) in a process of its own, over the oracle engine with zlib-backed
stand-ins for grp_bgzf_inflate / grp_gzip_inflate in the second engine table (tests/test_bgzf_cpu.py,
tests/test_gzip_index_cpu.py).  run() fills the entries the caller names; every call a stand-in accepts is recorded as the
[crc32, text_len] of its members / segments."""
import json
import os
import re
import subprocess
import sys
import textwrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RUNNER = textwrap.dedent("""
    import ctypes as C, json, os, sys, zlib
    import numpy as np
    sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests")); sys.path.insert(0, os.path.join({root!r}, "oracle"))
    import orc
    import gzip_cases as G
    from goldrush_amd import host, native
    from oracle_engine import OracleCliEngine
    eng = OracleCliEngine(orc, ingest=True)
    calls = {{"bgzf": [], "gzip": []}}

    def bgzf_inflate(ctx, comp_p, n_comp, blocks_p, n, text_p, cap, bad_p):  # grp_bgzf_inflate through zlib
        comp = C.string_at(comp_p, n_comp)
        blocks = np.frombuffer(C.string_at(blocks_p, n * native.bgzf_block_dtype.itemsize), dtype=native.bgzf_block_dtype)
        assert int(blocks["text_len"].sum()) <= cap
        out, seen = [], []
        for i, b in enumerate(blocks):
            off, ln = int(b["comp_off"]), int(b["comp_len"])
            assert off + ln <= n_comp
            try:
                t = zlib.decompress(comp[off:off + ln], -15)
            except zlib.error:
                t = None
            if t is None or len(t) != int(b["text_len"]) or zlib.crc32(t) != int(b["crc32"]):
                bad_p[0] = i
                return -1
            out.append(t)
            seen.append([int(b["crc32"]), len(t)])
        text = b"".join(out)
        C.memmove(text_p, text, len(text))
        calls["bgzf"].append(seen)
        return 0

    def gzip_inflate(ctx, comp_p, n_comp, dict_p, n_dict, segs_p, n, text_p, cap, bad_p):  # grp_gzip_inflate through zlib
        comp, hist = C.string_at(comp_p, n_comp), C.string_at(dict_p, n_dict)
        segs = np.frombuffer(C.string_at(segs_p, n * native.gzip_segment_dtype.itemsize), dtype=native.gzip_segment_dtype)
        assert int(segs["text_len"].sum()) <= cap
        out, seen = [], []
        for i, g in enumerate(segs):
            bit, nb, do, dl = int(g["comp_bit"]), int(g["n_bits"]), int(g["dict_off"]), int(g["dict_len"])
            assert bit + nb <= 8 * n_comp and do + dl <= n_dict and dl <= 32768
            try:
                t, eof = G.inflate_segment(comp, bit, nb, hist[do:do + dl])
            except zlib.error:
                t = None
            if t is None or len(t) != int(g["text_len"]) or zlib.crc32(t) != int(g["crc32"]) or eof != bool(int(g["flags"]) & 1):
                bad_p[0] = i
                return -1
            out.append(t)
            seen.append([int(g["crc32"]), len(t)])
        text = b"".join(out)
        C.memmove(text_p, text, len(text))
        calls["gzip"].append(seen)
        return 0

    ext = host.grp_engine_ext()
    ext.struct_size = C.sizeof(host.grp_engine_ext)
    cbs = {{"bgzf": host.BGZF_INFLATE_FN(bgzf_inflate), "gzip": host.GZIP_INFLATE_FN(gzip_inflate)}}
    if os.environ.get("OLD_EXT"):  # a caller from before grp_gzip_inflate: its table ends in front of it
        ext.struct_size = host.grp_engine_ext.gzip_inflate.offset
    elif not os.environ.get("NO_EXT_INFLATE"):
        for name in os.environ["EXT_ENTRIES"].split(","):
            setattr(ext, name + "_inflate", cbs[name])
    args = [b"goldrush_path"] + [a.encode() for a in sys.argv[1:]]
    arr = (C.c_char_p * (len(args) + 1))(*args, None)
    rc = host.load().gr_path_main_ext(len(args), arr, C.byref(eng.vt), C.byref(ext))
    sys.stdout.flush(); sys.stderr.flush()
    json.dump(calls, open(os.environ["CALLS_OUT"], "w"))
    os._exit(rc)
""")

ARGS = ["-k22", "-w16", "-t500", "-u5", "-a1", "-o0.1", "-h3", "-j2", "-d5", "-x10", "-s1011011110110111101101", "-g60000", "-b4", "-H600000", "--verbose",
        "-P0", "-r0.9", "--silver_path", "-M3", "-m1500"]
BGZF_TRACE = re.compile(r"BGZF blocks inflated on the device (\d+)")
GZIP_TRACE = re.compile(r"gzip segments inflated on the device (\d+)")


def run(tmp_path, tag, path, entries, **env):
    """-> the finished process, {file name: bytes} of its outputs, {"bgzf": calls, "gzip": calls} (None: it did not get that far)"""
    d = tmp_path / tag
    d.mkdir()
    script = tmp_path / "runner.py"
    script.write_text(RUNNER.format(root=ROOT))
    calls = str(d / "calls.json")
    e = dict(os.environ, OMP_NUM_THREADS="2", GRP_TRACE_INGEST="1", CALLS_OUT=calls, EXT_ENTRIES=",".join(entries), **env)
    for k in ("GRP_HOST_INGEST", "GRP_GZIP_INDEX", "GRP_GZIP_SPAN", "GRP_GZIP_INDEX_MAX_GB"):
        if k not in env:
            e.pop(k, None)
    rp = subprocess.run([sys.executable, str(script)] + ARGS + ["-i", str(path), "-p", str(d / "out")], capture_output=True, text=True, timeout=900, env=e)
    files = {f: open(d / f, "rb").read() for f in sorted(os.listdir(d)) if f != "calls.json"}
    return rp, files, json.load(open(calls)) if os.path.exists(calls) else None


def pick(stderr):
    keep = ("Visited", "Saw:", "Assigned:", "Unassigned:", "Total queries", "Total hits", "Total misses", "Num reads", "m_filterSize", "num_", "Total reads skipped")
    return [l for l in stderr.splitlines() if l.startswith(keep)]
