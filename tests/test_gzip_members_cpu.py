"""CPU: the members switch of the gzip walk without a device (csrc/host/gr_gzwalk.cpp: GzWalkMembers; GRP_GZIP_WALK_MEMBERS).
tools/dev/inflate_host_check.cpp --members, built by the plain host compiler without sanitizer flags, runs the rounds over the
decoder compiled for the host on the files of tests/gzip_member_cases.py: with the switch and without it, against the index
GzIndexReader writes, at spans 1, 50 000 and 10^9.  The program compares the indexes (and, for a file left to zlib, the
reason and the status); the tests here read its statistics: how many streams the chain adopted and dropped, how many took
steps at a time, how many rounds the walk took.  Then the two switches, and the entry from before the switch, which reads
neither variable."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

import gzip_member_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = re.compile(r"^members: ((?:\w+=\d+ ?)+)$", re.M)
RANDOM = re.compile(r"^random: (\d+) steps ended at a boundary, (\d+) ran out of input, (\d+) out of room, (\d+) were refused; (\d+) bad$", re.M)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    out = str(tmp_path_factory.mktemp("members_exe") / "inflate_host_check")
    src = [os.path.join(ROOT, p) for p in ("tools/dev/inflate_host_check.cpp", "goldrush_amd/csrc/host/gr_gzidx.cpp", "goldrush_amd/csrc/host/gr_fastq.cpp")]
    subprocess.run([cxx, "-std=c++17", "-O2", "-w"] + src + ["-lz", "-o", out], check=True, capture_output=True, text=True)
    return out


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    d = tmp_path_factory.mktemp("members_cases")
    out = M.all_cases()
    for name, case in out.items():
        (d / (name + ".gz")).write_bytes(case.data)
    return out, d


def _run(exe, cases, names, **env):
    """the program over the named cases in one walk: {span: its statistics}, every file as the reader has it (bad == 0)"""
    all_cases, d = cases
    e = {k: v for k, v in os.environ.items() if not k.startswith("GRP_GZIP_WALK")}
    e.update({k: str(v) for k, v in env.items()})
    rp = subprocess.run([exe, "--members"] + [str(d / (n + ".gz")) for n in names], capture_output=True, text=True, timeout=600, env=e)
    lines = [dict((k, int(v)) for k, v in (kv.split("=") for kv in m.split())) for m in LINE.findall(rp.stdout)]
    r = RANDOM.search(rp.stdout)
    assert rp.returncode == 0 and len(lines) == 3 and r, (rp.stdout[-3000:], rp.stderr[-1000:])
    assert [l["span"] for l in lines] == list(M.SPANS) and all(l["bad"] == 0 for l in lines) and int(r.group(5)) == 0, rp.stdout[-3000:]
    good = [all_cases[n] for n in names if all_cases[n].text is not None]
    for l in lines:
        assert (l["files"], l["walked"], l["left_to_zlib"]) == (len(names), len(good), len(names) - len(good)), l
        if len(good) == len(names):
            assert l["text"] == l["serial_text"] == sum(len(c.text) for c in good), l
    return {l["span"]: l for l in lines}, [int(x) for x in r.groups()]


def test_m1_ragged_members(exe, cases):
    got, random = _run(exe, cases, ["m1_ragged"])
    for span, l in got.items():
        assert l["adopted"] == 11 and l["candidates"] >= 11 and l["rounds"] < l["serial_rounds"], l
    # the open form from 10 000 pseudo-random bits: nearly all refused, some end at a boundary, none outside its buffers
    assert sum(random[:4]) == 10000 and random[3] > 5000 and random[0] > 0, random


def test_m2_the_members_take_the_rounds_of_one(exe, cases):
    one, _ = _run(exe, cases, ["m2_one"], GRP_GZIP_WALK_ROOM="65536,32768")
    got, _ = _run(exe, cases, ["m2_equal"], GRP_GZIP_WALK_ROOM="65536,32768")
    for span in M.SPANS:
        r1 = one[span]["serial_rounds"]
        assert one[span]["rounds"] == r1 and one[span]["adopted"] == 0, one[span]
        l = got[span]
        assert r1 >= 3 and l["rounds"] <= r1 + 1 and l["adopted"] == 7 and l["serial_rounds"] >= 8 * r1 - 8, (r1, l)


@pytest.mark.parametrize("name", sorted(M.m3_false_candidates()))
def test_m3_false_candidates(exe, cases, name):
    case = cases[0]["m3_" + name]
    env = dict(GRP_GZIP_WALK_STREAMS=64) if name.startswith("d_") else {}
    got, _ = _run(exe, cases, ["m3_" + name], **env)
    for span, l in got.items():
        assert l["adopted"] == case.members - 1 and l["candidates"] > l["adopted"] and l["dropped"] == l["streams"] - l["adopted"], l
        if name.startswith("c_"):
            assert l["dropped"] >= 3 and l["wasted_text"] > 0, l
        if name.startswith("d_"):
            assert l["candidates"] >= 2000 and l["max_in_flight"] <= 64, l


@pytest.mark.parametrize("budget", (1, 3, 1024))
def test_m4_budget(exe, cases, budget):
    got, _ = _run(exe, cases, ["m1_ragged"], GRP_GZIP_WALK_STREAMS=budget)
    for span, l in got.items():
        assert 1 <= l["max_in_flight"] <= budget, l
        if budget == 1:
            assert l["rounds"] == l["serial_rounds"] and l["streams"] == l["adopted"] == 0, l


def test_m5_several_files(exe, cases):
    names = sorted(n for n in cases[0] if n.startswith("m5_"))
    got, _ = _run(exe, cases, names)
    for span, l in got.items():
        assert len(names) == 10 and l["max_in_flight"] > 10 and l["adopted"] == sum(cases[0][n].members - 1 for n in names), l


def test_m6_left_to_zlib_as_before(exe, cases):
    """(the program compares `left` and `status` of every such file with those of the walk without the switch)"""
    faults = sorted(n for n in cases[0] if n.startswith("m6_"))
    assert len(faults) == 5
    got, _ = _run(exe, cases, ["m5_several3"] + faults + ["m5_several8"])
    for span, l in got.items():
        assert (l["walked"], l["left_to_zlib"]) == (2, 5) and l["streams"] >= 5, l


def test_the_switches(native, monkeypatch):
    from goldrush_amd import host

    lib = host.load()
    monkeypatch.delenv("GRP_GZIP_WALK_MEMBERS", raising=False)
    monkeypatch.delenv("GRP_GZIP_WALK", raising=False)
    assert lib.gr_gzip_walk_members_switch() == 0
    for value, want in (("on", 1), ("off", 0), ("maybe", -1), ("", -1), ("ON", -1), ("1", -1), ("on ", -1)):
        monkeypatch.setenv("GRP_GZIP_WALK_MEMBERS", value)
        assert lib.gr_gzip_walk_members_switch() == want, value
        assert lib.gr_gzip_walk_switch() == 0  # (the two are read apart)


def test_the_old_entry_reads_neither_variable(native, monkeypatch, tmp_path):
    """gr_gzidx_build_device_many with GRP_GZIP_WALK_MEMBERS=on set: one step in the first launch of a three-member file, as
    before; gr_gzidx_build_device_many_ex with its flag: three, and with GRP_GZIP_WALK_STREAMS=2 two.  (The table's walk is a
    function of this test that notes the launch and fails it: no decoder is needed to see what a round holds.)"""
    from goldrush_amd import host

    case = M.m3_false_candidates()["a_member_in_fextra"]
    p = tmp_path / "three.gz"
    p.write_bytes(case.data)
    seen = []

    def walk(ctx, comp, n_comp, hist, n_hist, steps, n_steps, res, hist_out, text, cap, bad):
        seen.append(n_steps)
        return 1

    ext = host.grp_engine_ext()
    ext.struct_size = ctypes.sizeof(host.grp_engine_ext)
    ext.gzip_walk = host.GZIP_WALK_FN(walk)
    for value in ("on", "maybe"):
        monkeypatch.setenv("GRP_GZIP_WALK_MEMBERS", value)
        got, stats = host.gzip_index_device(None, [p], 4096, ext=ext)
        assert seen == [1] and got[0]["left"] == "a launch of the walk failed" and stats["left_to_zlib"] == 1 and "adopted" not in stats, (seen, got, stats)
        del seen[:]
    monkeypatch.setenv("GRP_GZIP_WALK_MEMBERS", "off")  # (the flag of the new entry is its argument, not the variable)
    got, stats = host.gzip_index_device(None, [p], 4096, members=True, ext=ext)
    assert seen == [4] and got[0]["left"] == "a launch of the walk failed", (seen, got)  # the head, two members, the member inside the FEXTRA field
    assert (stats["candidates"], stats["streams"], stats["max_in_flight"], stats["adopted"]) == (3, 3, 4, 0), stats
    del seen[:]
    monkeypatch.setenv("GRP_GZIP_WALK_STREAMS", "2")
    got, stats = host.gzip_index_device(None, [p], 4096, members=True, ext=ext)
    assert seen == [2] and stats["max_in_flight"] == 2, (seen, stats)
