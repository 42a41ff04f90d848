"""CPU: the host side of BGZF input.  gr_bgzf_scan against a Python walk of the same bytes, and the product's whole host
program (gr_path_main_ext) over the oracle engine with a zlib-backed stand-in for grp_bgzf_inflate in the second engine
table: a BGZF file, and a BGZF file followed by a plain gzip member, give the plain file's outputs, and the stand-in is
handed every member exactly once per pass.  (tests/test_gpu_cli_bgzf.py does the same with the HIP engine.)"""
import gzip
import os
import struct

import pytest

import bgzf_cases as B
import ext_runner as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def host(native):
    from goldrush_amd import host as h

    h.load()
    return h


def _check_scan(host, buf, cap=1 << 12):
    got = host.bgzf_scan(buf, cap)
    exp = B.walk_members(buf)
    assert got == exp, (got[1:], exp[1:])
    return got


def test_scan_finds_the_members_of_a_file(host):
    text = open(os.path.join(GOLD, "tiny.fq"), "rb").read()
    f = B.bgzf_file(text, [1, 65280, 7, 300, 40000])
    blocks, consumed, why = _check_scan(host, f)
    assert consumed == len(f) and why == 1 and sum(b[2] for b in blocks) == len(text)
    assert blocks[-1][2] == 0 and blocks[-1][1] == 2  # the empty end-of-file member is a block like any other
    import zlib

    assert b"".join(zlib.decompress(f[o:o + n], -15) for o, n, _, _ in blocks) == text
    assert _check_scan(host, b"") == ([], 0, 1)


def test_scan_skips_extra_subfields_in_front_of_bc(host):
    extra = b"XY" + struct.pack("<H", 5) + b"hello" + b"BX" + struct.pack("<H", 2) + b"\1\2" + b"AB" + struct.pack("<H", 0)
    f = B.bgzf_member(b"first member", extra=extra) + B.bgzf_member(b"second") + B.BGZF_EOF
    blocks, consumed, why = _check_scan(host, f)
    assert [b[2] for b in blocks] == [12, 6, 0] and consumed == len(f) and why == 1
    assert blocks[0][0] == 12 + len(extra) + 6


def test_scan_asks_for_more_data_at_every_cut_of_a_member(host):
    extra = b"ZZ" + struct.pack("<H", 3) + b"abc"
    first = B.bgzf_member(b"ACGT" * 50)
    second = B.bgzf_member(b"TTGCA" * 40, extra=extra)
    for cut in range(len(second)):
        blocks, consumed, why = _check_scan(host, first + second[:cut])
        assert len(blocks) == 1 and consumed == len(first)
        assert why == (1 if cut == 0 else 0), cut
    # ... and of the first member's header alone
    for cut in range(1, 18):
        assert _check_scan(host, first[:cut]) == ([], 0, 0)


def test_scan_stops_at_a_member_that_is_not_bgzf(host):
    first = B.bgzf_member(b"ACGT" * 50)
    plain = gzip.compress(b"plain gzip member")
    named = b"\x1f\x8b\x08\x0c" + first[4:]            # FEXTRA and FNAME: the payload is not where a BGZF member has it
    no_bc = B.bgzf_member(b"x").replace(b"BC", b"BD")  # FEXTRA without the BC subfield
    big = bytearray(first)
    big[-4:] = struct.pack("<I", 65537)                # an ISIZE no BGZF member has
    for other in (plain, named, no_bc, bytes(big), b"garbage", b"\x1f", b"\x1f\x8b\x09"):
        blocks, consumed, why = _check_scan(host, first + other + first)
        assert len(blocks) == 1 and consumed == len(first), other[:8]
        assert why == 2, other[:8]
    assert _check_scan(host, first + plain)[2] == 2 and _check_scan(host, first + b"garbage")[2] == 2
    assert _check_scan(host, plain)[2] == 2


def test_scan_respects_the_table_capacity(host):
    f = b"".join(B.bgzf_member(b"%d" % i) for i in range(10))
    sizes = [len(B.bgzf_member(b"%d" % i)) for i in range(10)]
    for cap in (0, 1, 3, 10, 11):
        blocks, consumed, why = host.bgzf_scan(f, cap)
        assert len(blocks) == min(cap, 10) and consumed == sum(sizes[:cap]) and why == 1
        assert blocks == B.walk_members(f)[0][:cap]


TRACE = X.BGZF_TRACE
_pick = X.pick


def _run(tmp_path, tag, path, **env):
    rp, files, calls = X.run(tmp_path, tag, path, ("bgzf",), **env)
    return rp, files, calls and calls["bgzf"]


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("bgzf_inputs")
    text = open(os.path.join(GOLD, "tiny.fq"), "rb").read()
    sizes = [1, 65280, 7, 3000, 40000, 2, 12345]  # records straddle the members
    cut = text.index(b"\n@read", len(text) * 2 // 3) + 1
    files = {"plain": text, "bgzf": B.bgzf_file(text, sizes), "no_eof_member": B.bgzf_file(text, sizes, eof=False),
             "bgzf_then_gzip": B.bgzf_file(text[:cut], sizes) + gzip.compress(text[cut:])}
    paths = {}
    for name, data in files.items():
        paths[name] = d / (name + (".fq" if name == "plain" else ".fq.gz"))
        paths[name].write_bytes(data)
    return paths, files


@pytest.fixture(scope="module")
def plain_run(oracle, native, inputs, tmp_path_factory):
    rp, files, calls = _run(tmp_path_factory.mktemp("plain"), "plain", inputs[0]["plain"])
    assert rp.returncode == 0 and files and any(files.values()), rp.stderr[-2000:]
    assert calls == [] and [int(n) for n in TRACE.findall(rp.stderr)] == [0] * len(TRACE.findall(rp.stderr)) and TRACE.findall(rp.stderr)
    return rp, files


@pytest.mark.parametrize("name,chunk", [("bgzf", 0), ("bgzf", 4096), ("bgzf", 100000), ("no_eof_member", 70000), ("bgzf_then_gzip", 0), ("bgzf_then_gzip", 66000)])
def test_host_program_inflates_bgzf_through_the_ext_table(oracle, native, tmp_path, inputs, plain_run, name, chunk):
    paths, data = inputs
    rp, files, calls = _run(tmp_path, name, paths[name], **({"GRP_INGEST_CHUNK": str(chunk)} if chunk else {}))
    assert rp.returncode == 0, rp.stderr[-3000:]
    assert files == plain_run[1]
    assert _pick(rp.stderr) == _pick(plain_run[0].stderr)
    # every member was handed over exactly once per pass, in file order
    members = [[crc, isize] for _, _, isize, crc in B.walk_members(data[name])[0]]
    assert len(members) > 5
    traced = [int(n) for n in TRACE.findall(rp.stderr)]
    passes = len(traced)
    assert passes >= 2 and traced == [len(members)] * passes, traced
    assert [b for call in calls for b in call] == members * passes
    if chunk:  # a slot takes whole members up to its text capacity, max(chunk, 64 KiB)
        assert max(sum(b[1] for b in call) for call in calls) <= max(chunk, 65536)
        assert len(calls) > passes


@pytest.mark.parametrize("name,chunk", [("bgzf_then_gzip", 66000), ("bgzf", 0)])
def test_bgzf_comes_first_where_the_table_has_both_entries(oracle, native, tmp_path, inputs, plain_run, name, chunk):
    """both stand-ins in the table: a BGZF file is still taken by the BGZF form, what follows its members by zlib, and the
    gzip segments' entry is not called in any pass"""
    paths, data = inputs
    rp, files, calls = X.run(tmp_path, name, paths[name], ("bgzf", "gzip"), **({"GRP_INGEST_CHUNK": str(chunk)} if chunk else {}))
    assert rp.returncode == 0, rp.stderr[-3000:]
    assert files == plain_run[1]
    assert _pick(rp.stderr) == _pick(plain_run[0].stderr)
    members = [[crc, isize] for _, _, isize, crc in B.walk_members(data[name])[0]]
    assert len(members) > 5
    traced = [int(n) for n in TRACE.findall(rp.stderr)]
    passes = len(traced)
    assert passes >= 2 and traced == [len(members)] * passes, traced
    assert [b for call in calls["bgzf"] for b in call] == members * passes
    assert [int(n) for n in X.GZIP_TRACE.findall(rp.stderr)] == [0] * passes
    assert calls["gzip"] == []


def test_switch_and_missing_entry_point_take_the_zlib_path(oracle, native, tmp_path, inputs, plain_run):
    for tag, env in (("off", {"GRP_BGZF": "off"}), ("no_ext", {"NO_EXT_INFLATE": "1"})):
        rp, files, calls = _run(tmp_path, tag, inputs[0]["bgzf"], **env)
        assert rp.returncode == 0, rp.stderr[-3000:]
        assert files == plain_run[1] and calls == []
        traced = [int(n) for n in TRACE.findall(rp.stderr)]
        assert traced and set(traced) == {0}


def test_damaged_bgzf_files_end_the_run_with_an_error(oracle, native, tmp_path, inputs):
    whole = inputs[1]["bgzf"]
    blocks = B.walk_members(whole)[0]
    off, ln = blocks[3][0], blocks[3][1]
    cut = tmp_path / "cut.fq.gz"
    cut.write_bytes(whole[:off + ln // 2])  # the file ends inside a member
    flipped = tmp_path / "flipped.fq.gz"
    b = bytearray(whole)
    b[off + ln // 2] ^= 0x20
    flipped.write_bytes(bytes(b))
    for path in (cut, flipped):
        rp, files, calls = _run(tmp_path, path.name.split(".")[0], path, GRP_INGEST_CHUNK="70000")
        assert rp.returncode != 0, "a damaged BGZF file passed for a shorter input"
        assert "failed" in rp.stderr and path.name in rp.stderr, rp.stderr[-2000:]
    assert "BGZF member at byte" in rp.stderr
