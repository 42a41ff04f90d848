"""CPU: the gzip walk without a device.  tools/dev/inflate_host_check.cpp --walk, built by the plain host compiler without
sanitizer flags: the open form of the decoder (csrc/grp_inflate.inc under GRP_INFLATE_HOST, the 64 lanes one after the other)
under the rounds of csrc/host/gr_gzwalk.cpp, against the index GzIndexReader writes — every stream of tests/gzip_cases.py at
spans 1, 4096 and 262144, with the default sizes of a step and with tiny ones, then damaged copies of every file and damaged
steps.  And the two pieces of the walk that need no decoder: the header parser, on hand-made headers with every optional
field, and the switch."""
import os
import re
import shutil
import struct
import subprocess
import zlib

import pytest

import gzip_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = re.compile(r"^steps: (\d+) open steps over the reader's segments, (\d+) damaged forms: (\d+) refused, (\d+) gave the segment's text$")
LAST = re.compile(r"^walk: (\d+) indexes equal the reader's; (\d+) steps, (\d+) repeated; (\d+) damaged files: (\d+) left to zlib, (\d+) indexed as the reader does; (\d+) bad$")


def test_the_walk_on_the_host_gives_the_readers_index(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "inflate_host_check")
    src = [os.path.join(ROOT, p) for p in ("tools/dev/inflate_host_check.cpp", "goldrush_amd/csrc/host/gr_gzidx.cpp", "goldrush_amd/csrc/host/gr_fastq.cpp")]
    subprocess.run([cxx, "-std=c++17", "-O2", "-w"] + src + ["-lz", "-o", exe], check=True, capture_output=True, text=True)
    streams = G.streams()
    files = []
    for name, (f, text) in streams.items():
        files.append(str(tmp_path / (name + ".gz")))
        open(files[-1], "wb").write(f)
    rp = subprocess.run([exe, "--walk"] + files, capture_output=True, text=True, timeout=600)
    m = LAST.match(rp.stdout.splitlines()[-1]) if rp.stdout else None
    assert rp.returncode == 0 and m, (rp.stdout[-3000:], rp.stderr[-1000:])
    same, steps, repeats, damaged, left, dmg_same, bad = (int(x) for x in m.groups())
    # three spans, two sizes of a step
    assert same == len(streams) * 3 * 2 and bad == 0
    # one open step per segment of the reader's index at span 4096 (a sample where there are many) and its damaged forms
    s = STEPS.match(rp.stdout.splitlines()[-2])
    assert s, rp.stdout[-3000:]
    n_steps, forms, refused, gave_text = (int(x) for x in s.groups())
    assert n_steps > 400 and forms > 300 and refused + gave_text == forms and refused > forms // 2 and gave_text > 0
    assert repeats > 100 and steps > 2000  # the tiny sizes: every step repeated until its block fits
    assert damaged == 40 * len(streams) and left + dmg_same == damaged and left > damaged // 2


def _header(flg, extra=b"", name=b"", comment=b"", hcrc=None, cm=8):
    """a gzip header with the given FLG and its optional fields in RFC 1952's order; hcrc None: the right CRC16"""
    h = bytes([0x1f, 0x8b, cm, flg]) + struct.pack("<IBB", 1234567, 2, 3)
    if flg & 4:
        h += struct.pack("<H", len(extra)) + extra
    if flg & 8:
        h += name + b"\0"
    if flg & 16:
        h += comment + b"\0"
    if flg & 2:
        h += struct.pack("<H", (zlib.crc32(h) & 0xffff) if hcrc is None else hcrc)
    return h


HEADERS = {"plain": dict(flg=0), "fextra": dict(flg=4, extra=b"AB\x03\0xyz"), "fextra_empty": dict(flg=4), "fname": dict(flg=8, name=b"reads.fastq"), "fname_empty": dict(flg=8),
           "fcomment": dict(flg=16, comment=b"a comment"), "fhcrc": dict(flg=2), "ftext": dict(flg=1),
           "all": dict(flg=31, extra=bytes(range(1, 200)) + b"\0\0", name=b"n", comment=b"c" * 300),
           "extra_holds_a_nul_and_the_magic": dict(flg=12, extra=b"\0\x1f\x8b\x08\0", name=b"x")}


def test_the_header_parser_on_every_optional_field(native):
    """gzip_header_bytes (csrc/host/gr_gzwalk.cpp) on hand-made headers with each of FEXTRA, FNAME, FCOMMENT and FHCRC, alone and
    together: the length is the header's, zlib reads the member behind it, and every proper prefix asks for more bytes"""
    from goldrush_amd import host

    lib = host.load()
    text = b"@r\nACGT\n+\n!!!!\n"
    raw = zlib.compress(text, 6)[2:-4]
    for name, kw in HEADERS.items():
        h = _header(**kw)
        f = h + raw + struct.pack("<II", zlib.crc32(text), len(text))
        assert zlib.decompress(f, 31) == text, name
        assert lib.gr_gzip_header_bytes(f, len(f)) == len(h) == G.payload_bit(f) // 8, name
        assert lib.gr_gzip_header_bytes(h, len(h)) == len(h), name
        for n in range(len(h)):
            assert lib.gr_gzip_header_bytes(h[:n], n) == 0, (name, n)
    # what zlib does not take is not taken: the FHCRC that does not match, a reserved flag, another method, another magic
    good = _header(flg=2)
    bad = {"hcrc": _header(flg=2, hcrc=(zlib.crc32(good[:-2]) & 0xffff) ^ 1), "hcrc_all": _header(**dict(HEADERS["all"], hcrc=0x1234)), "reserved_flag": _header(flg=32),
           "method_7": _header(flg=0, cm=7), "magic": b"\x1f\x8c" + _header(flg=0)[2:], "magic_first": b"\x1e\x8b" + _header(flg=0)[2:]}
    assert zlib.crc32(_header(**dict(HEADERS["all"]))[:-2]) & 0xffff != 0x1234
    for name, h in bad.items():
        f = h + raw + struct.pack("<II", zlib.crc32(text), len(text))
        with pytest.raises(zlib.error):
            zlib.decompress(f, 31)
        assert lib.gr_gzip_header_bytes(f, len(f)) == -1, name


def test_the_switch(native, monkeypatch):
    from goldrush_amd import host

    lib = host.load()
    monkeypatch.delenv("GRP_GZIP_WALK", raising=False)
    assert lib.gr_gzip_walk_switch() == 0
    for value, want in (("on", 1), ("off", 0), ("maybe", -1), ("", -1), ("ON", -1), ("1", -1), ("on ", -1)):
        monkeypatch.setenv("GRP_GZIP_WALK", value)
        assert lib.gr_gzip_walk_switch() == want, value


def test_a_table_without_the_walk_is_refused(native):
    """gr_gzidx_build_device with a table that ends in front of gzip_walk, the last member: no handle, nothing called"""
    import ctypes

    from goldrush_amd import host

    lib = host.load()
    ext = host.grp_engine_ext()
    ext.struct_size = host.grp_engine_ext.gzip_walk.offset
    assert not lib.gr_gzidx_build_device(ext, None, b"/nonexistent", 4096, 1 << 30)
    assert host.grp_engine_ext.gzip_walk.offset + ctypes.sizeof(ctypes.c_void_p) == ctypes.sizeof(host.grp_engine_ext)
