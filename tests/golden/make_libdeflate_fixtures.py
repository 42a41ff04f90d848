#!/usr/bin/env python3
"""Generates tests/golden/tiny_libdeflate.fq.gz and libdeflate_members.bgzf: BGZF as htslib writes it (bgzip, samtools,
dorado, pbbam), whose DEFLATE encoder is libdeflate — other block splits, code length distributions and header trimming
than zlib's compressor, which writes every other good stream of tests/bgzf_cases.py and tests/gzip_cases.py.

The library is loaded with ctypes (libdeflate.so.0); the files are committed, so no test needs it: the expected text of
a member is always what zlib inflates from its payload.  tests/test_deflate_gen_cpu.py rebuilds both files in memory where
the library loads and compares them byte for byte with the committed ones.  Re-run after a change of tiny.fq or of
bgzf_cases.texts():  python tests/golden/make_libdeflate_fixtures.py
"""
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import bgzf_cases as B  # noqa: E402

TINY = os.path.join(HERE, "tiny_libdeflate.fq.gz")
MEMBERS = os.path.join(HERE, "libdeflate_members.bgzf")
MEMBER_TEXT = 65280  # what bgzip puts into a member
TINY_LEVELS = (0, 1, 2, 9, 12)
TEXT_NAMES = ("bytes", "run_of_A", "period258", "longest_distance", "len0", "len1", "len258")
TEXT_LEVELS = (1, 12)


def load():
    """the library, or None where it is absent"""
    try:
        lib = ctypes.CDLL("libdeflate.so.0")
    except OSError:
        return None
    lib.libdeflate_alloc_compressor.restype = ctypes.c_void_p
    lib.libdeflate_alloc_compressor.argtypes = [ctypes.c_int]
    lib.libdeflate_deflate_compress_bound.restype = ctypes.c_size_t
    lib.libdeflate_deflate_compress_bound.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    lib.libdeflate_deflate_compress.restype = ctypes.c_size_t
    lib.libdeflate_deflate_compress.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]
    lib.libdeflate_free_compressor.restype = None
    lib.libdeflate_free_compressor.argtypes = [ctypes.c_void_p]
    return lib


def deflate(lib, text, level):
    """raw DEFLATE of `text` by libdeflate"""
    c = lib.libdeflate_alloc_compressor(level)
    assert c, "libdeflate_alloc_compressor(%d)" % level
    try:
        cap = lib.libdeflate_deflate_compress_bound(c, len(text))
        out = ctypes.create_string_buffer(max(cap, 1))
        n = lib.libdeflate_deflate_compress(c, text, len(text), out, cap)
        assert n, "libdeflate_deflate_compress"
        return out.raw[:n]
    finally:
        lib.libdeflate_free_compressor(c)


def tiny():
    return open(os.path.join(HERE, "tiny.fq"), "rb").read()


def member(lib, text, level):
    payload = deflate(lib, text, level)
    assert B.confirm_good(payload)[0] == text
    return B.bgzf_member(text, payload=payload)


def build_tiny(lib):
    t = tiny()
    return b"".join(member(lib, t[a:a + MEMBER_TEXT], 6) for a in range(0, len(t), MEMBER_TEXT)) + B.BGZF_EOF


def member_list():
    """[(name, text, level)] of libdeflate_members.bgzf, in file order"""
    t, texts = tiny()[:MEMBER_TEXT], B.texts()
    return [("tiny", t, lv) for lv in TINY_LEVELS] + [(n, texts[n], lv) for n in TEXT_NAMES for lv in TEXT_LEVELS]


def build_members(lib):
    return b"".join(member(lib, text, lv) for _, text, lv in member_list())


def main():
    lib = load()
    if lib is None:
        sys.exit("libdeflate.so.0 does not load")
    for path, data in ((TINY, build_tiny(lib)), (MEMBERS, build_members(lib))):
        open(path, "wb").write(data)
        print(os.path.basename(path), len(data), "bytes")


if __name__ == "__main__":
    main()
