"""CPU: the generated DEFLATE corpus (tests/deflate_gen.py) and the libdeflate fixtures (tests/golden) before they reach
the device (tests/test_gpu_inflate_generated.py): the generator's invariants, what the corpus covers — asserted here, so
that a change of seed cannot hollow it out —, zlib's word on every stream, good and refused, and the decoder's own text
(csrc/grp_inflate.inc) compiled as plain C++ (tools/dev/inflate_host_check.cpp), where the 64 lanes run one after the
other, on the whole corpus."""
import importlib.util
import os
import re
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import bgzf_cases as B
import deflate_gen as D
import gzip_cases as G
from test_gpu_inflate_generated import MEMBER_REASONS, SEGMENT_REASONS, STATUS_TEXT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- the generator ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_len,n", [(15, 2), (15, 16), (15, 17), (15, 286), (7, 2), (7, 8), (7, 19)])
def test_random_codes_are_complete_prefix_codes(max_len, n):
    for bias in D.BIASES + (1.0,):
        for seed in range(5):
            depths = D.random_depths(np.random.default_rng((seed, n)), n, max_len, bias)
            assert len(depths) == n and 1 <= min(depths) and max(depths) <= max_len
            assert sum(2 ** (max_len - d) for d in depths) == 2 ** max_len  # Kraft: complete
            codes = B.canonical(depths)
            words = sorted(format(c, "0%db" % l) for c, l in codes.values())
            assert len(words) == n and not any(b.startswith(a) for a, b in zip(words, words[1:]))  # prefix-free
    if n <= max_len + 1:  # (the last bias, 1) always the deepest leaf: 1, 2, ..., n - 1, n - 1
        assert sorted(depths) == list(range(1, n)) + [n - 1]
    assert sorted(D.random_depths(np.random.default_rng(0), 16, 15, 1.0)) == list(range(1, 16)) + [15]


def test_code_length_symbols_stand_for_the_lengths():
    rng = np.random.default_rng(4)
    for _ in range(200):
        lens = [int(x) for x in rng.choice([0, 0, 0, 3, 3, 7, 15], int(rng.integers(1, 320)))]
        for r in (None, rng):
            seq = B.rle_lengths(lens, r)
            assert B.expand_lengths(seq) == lens
            assert all((s < 16 and (ev, eb) == (0, 0)) or (s, eb) in ((16, 2), (17, 3), (18, 7)) and 0 <= ev < 1 << eb for s, ev, eb in seq)


def test_the_corpus_is_a_function_of_its_seeds():
    a = D.members()[37]
    rng = np.random.default_rng(a.seed)
    max_text = D.SMALL_TEXT if rng.random() < 0.3 else int(rng.integers(1, D.SMALL_TEXT + 1))
    payload, text, _ = D.random_stream(rng, max_text, D.BIASES[37 % 3])
    assert (payload, text) == (a.payload, a.text) and a.seed == (D.SEED, 1, 37)


def test_corpus_sizes():
    members, streams = D.members(), D.gzip_streams()
    assert len(members) == 400 and len(streams) == 40
    big = [i for i, s in enumerate(members) if len(s.text) > 3000]
    assert big and all(i % 20 == 19 for i in big) and max(len(s.text) for s in members) <= 65536
    assert max(len(members[i].text) for i in big) > 49152  # (beyond the second flush behind the ring's wrap)
    assert all(1 <= s.info["blocks"] <= 11 for s in members + streams) and {s.info["blocks"] for s in members} == set(range(1, 12))
    assert max(len(s.text) for s in streams) > 4 * 65536


def test_corpus_coverage():
    info = D.merge_info([s.info for s in D.members() + D.gzip_streams()])
    assert max(info["lit_bits"]) == 15 and max(info["dist_bits"]) == 15  # codes USED by a token
    assert max(info["cl_bits"]) == 7
    assert {10, 11} <= info["lit_bits"] and {8, 9} <= info["dist_bits"]  # the two sides of the direct tables
    assert {257, 286} <= info["hlit"] and {1, 30} <= info["hdist"]
    assert 19 in info["n_cl"]
    for sym, top in ((16, 3), (17, 7), (18, 127)):
        assert {(sym, 0), (sym, top)} <= info["repeats"]
    assert info["crossing"] > 0  # a repeat from the literal/length lengths into the distance lengths
    assert {s if isinstance(s, int) else s[0] for s in info["len_syms"]} == set(range(29)) and info["dist_syms"] == set(range(30))
    assert {(27, 31), (28, 0)} <= info["len_syms"]  # both spellings of 258
    assert info["kinds"] == info["empty"] == {"stored", "fixed", "dynamic"}
    assert info["stored"] == set(D.STORED_LENGTHS)


def test_fewest_code_length_code_lengths():
    """HCLEN + 4 = 4 is out of a good block's reach: symbol 256 needs a length of 1 .. 15, and those come from the fifth code
    length code length on.  So 5 is a hand-written good block's, and 4 a refused one's (no code at all)"""
    def n_cl(p):
        return ((int.from_bytes(p[:3], "little") >> 13) & 15) + 4

    assert n_cl(B.hand_written()["five_code_length_lengths"]) == 5
    assert n_cl(B.refused()["no_code_at_all"][0]) == 4 == n_cl(B.refused()["oversubscribed_code_lengths"][0])
    assert all(B.CL_ORDER.index(s) >= 4 for s in range(1, 16))


def test_match_sweep_and_thresholds():
    sweep, pairs = D.match_sweep()
    assert pairs == {(d, n) for d in D.SWEEP_DISTANCES for n in D.SWEEP_LENGTHS} and len(pairs) == 141 * 81
    assert all(len(s.text) <= 65536 for s in sweep) and 700000 < sum(len(s.text) for s in sweep) < 1100000
    th = D.threshold_members()
    assert len(th) == 48 and all(len(s.text) <= 65536 for s, _ in th)
    # what reads back across the threshold p: the source of a match on both sides of it (distance 1: the byte in front)
    at = {(p, step, k): across for (p, step, k), (_, across) in zip(((p, step, k) for p in D.THRESHOLDS for step in D.STEPS for k in D.BELOW), th)}
    for p in D.THRESHOLDS:
        assert all({1, 64} <= at[p, "literal", k] for k in D.BELOW)
        assert 1 in at[p, "match258", 2] and 200 in at[p, "match258", 1] and 64 in at[p, "match258", 257]
        for key, across in at.items():
            if key[0] == p:
                assert (16384 in across) == (p <= 32768) and (32768 in across) == (p == 16384), key
    for s in sweep + [m for m, _ in th]:
        assert B.confirm_good(s.payload)[0] == s.text


def test_every_good_stream_is_zlibs():
    for s in D.members():
        assert zlib.decompress(s.payload, -15) == s.text, (s.name, s.seed)
    for s in D.gzip_streams():
        d = zlib.decompressobj(31)
        assert d.decompress(s.payload) == s.text and d.eof and not d.unused_data, (s.name, s.seed)
    for name, p in B.hand_written().items():
        assert B.confirm_good(p)[0], name


def test_hand_made_segments():
    segs = D.hand_segments()
    assert len(segs) == 56 and {(len(g["dict"]), g["comp_bit"] % 8) for _, _, g, _ in segs} == {(n, ph) for n in D.HISTORY_LENGTHS for ph in range(8)}
    for name, f, g, text in segs:
        assert G.inflate_segment(f, g["comp_bit"], g["n_bits"], g["dict"]) == (text, bool(g["flags"])), name
        if g["dict"]:  # the first token reaches exactly the first byte of the history — one byte less of it is not enough
            with pytest.raises(zlib.error, match="too far back"):
                G.inflate_segment(f, g["comp_bit"], g["n_bits"], g["dict"][1:])
    assert {g["flags"] for _, _, g, _ in segs} == {0, 1}


def test_every_refused_stream_is_refused_by_zlib_for_the_reason_in_the_table():
    refused, reasons = B.refused(), B.refused_reasons()
    assert set(refused) == set(reasons) == set(MEMBER_REASONS)
    for name, (p, text_len, crc) in refused.items():
        d = zlib.decompressobj(-15)
        try:
            text = d.decompress(p)
            assert reasons[name] is None
            assert not d.eof or len(text) != text_len or d.unused_data or zlib.crc32(text) != crc, name
        except zlib.error as e:
            assert str(e).endswith(": " + reasons[name]) and MEMBER_REASONS[name] == reasons[name], name
    for name, (f, g, reason) in D.refused_segments().items():
        assert SEGMENT_REASONS[name] == reason == "invalid distance too far back"
    # the tables name every status of the decoder, and in zlib's words where it has them
    assert set(MEMBER_REASONS.values()) | set(SEGMENT_REASONS.values()) == set(STATUS_TEXT)
    src = open(os.path.join(ROOT, "goldrush_amd", "csrc", "grp_inflate.inc")).read()
    table = src[src.index("INF_STATUS_TEXT[INF_STATUS_COUNT] = {"):]
    assert re.findall(r'^\s*"(.*)",$', table[:table.index("};")], re.M) == ["ok"] + STATUS_TEXT


# ---- the libdeflate fixtures -----------------------------------------------------------------------------------------
def _fixture(name):
    return open(os.path.join(GOLD, name), "rb").read()


def test_fixtures_inflate_with_zlib_and_walk():
    tiny = G.tiny()
    buf = _fixture("tiny_libdeflate.fq.gz")
    blocks, consumed, why = B.walk_members(buf)
    assert consumed == len(buf) and why == 1 and buf.endswith(B.BGZF_EOF)
    assert [b[2] for b in blocks] == [65280, 65280, len(tiny) - 2 * 65280, 0]
    assert b"".join(zlib.decompress(buf[o:o + n], -15) for o, n, _, _ in blocks) == tiny
    mk = _load(os.path.join(GOLD, "make_libdeflate_fixtures.py"), "make_libdeflate_fixtures")
    buf = _fixture("libdeflate_members.bgzf")
    blocks, consumed, why = B.walk_members(buf)
    want = mk.member_list()
    assert consumed == len(buf) and why == 1 and len(blocks) == len(want) == 5 + 2 * 7
    for (o, n, isize, crc), (name, text, level) in zip(blocks, want):
        got = zlib.decompress(buf[o:o + n], -15)
        assert got == text and (len(got), zlib.crc32(got)) == (isize, crc), (name, level)
    assert want[0][1] == tiny[:65280]
    # The members that make_libdeflate_fixtures.py lists hold 231 KB of bytes no encoder can shrink (level 0 of 65 280 bytes, the
    # random texts at two levels each), so the two files are 453 KB; they must not grow beyond that unnoticed
    assert len(_fixture("tiny_libdeflate.fq.gz")) + len(buf) < 460000
    # not zlib's streams: no form of bgzf_cases.FORMS writes these payloads
    o, n = blocks[1][:2]
    assert all(B.deflate(tiny[:65280], **kw) != buf[o:o + n] for kw in B.FORMS.values())


def test_fixtures_are_what_libdeflate_writes_today():
    mk = _load(os.path.join(GOLD, "make_libdeflate_fixtures.py"), "make_libdeflate_fixtures")
    lib = mk.load()
    if lib is None:
        pytest.skip("libdeflate.so.0 does not load: the committed fixtures are checked by zlib alone")
    assert mk.build_tiny(lib) == _fixture("tiny_libdeflate.fq.gz")
    assert mk.build_members(lib) == _fixture("libdeflate_members.bgzf")


# ---- the decoder on the host -----------------------------------------------------------------------------------------
def test_the_decoders_text_on_the_host(tmp_path):
    """tools/dev/inflate_host_check.cpp, built by the plain host compiler without sanitizer flags, on the whole corpus:
    members, hand-made segments and the gzip files through the index at spans 1, 50 000 and 10^9"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "inflate_host_check")
    src = [os.path.join(ROOT, p) for p in ("tools/dev/inflate_host_check.cpp", "goldrush_amd/csrc/host/gr_gzidx.cpp", "goldrush_amd/csrc/host/gr_fastq.cpp")]
    subprocess.run([cxx, "-std=c++17", "-O2", "-w"] + src + ["-lz", "-o", exe], check=True, capture_output=True, text=True)
    cases = _load(os.path.join(ROOT, "tools", "dev", "inflate_host_cases.py"), "inflate_host_cases")
    members, segments, files = cases.write_generated(str(tmp_path / "corpus"))
    generated = cases.generated_cases()
    rp = subprocess.run([exe, members], capture_output=True, text=True, timeout=600)
    assert rp.returncode == 0 and rp.stdout.splitlines()[-1] == "%d cases, 0 bad" % len(generated), rp.stdout[-2000:]
    # ... and the reasons of the refused members are those the device must give
    said = dict(re.findall(r"^case (\d+) refused: (.*)$", rp.stdout, re.M))
    for i, (name, _, bad) in enumerate(generated):
        if bad is not None:
            assert said.get(str(i), "CRC32 of the text differs from the member's") == MEMBER_REASONS[name], name
    rp = subprocess.run([exe, "--segments", segments], capture_output=True, text=True, timeout=600)
    n = len(D.hand_segments()) + len(D.refused_segments())
    assert rp.returncode == 0 and rp.stdout.splitlines()[-1] == "%d segments, 0 bad" % n, rp.stdout[-2000:]
    assert re.findall(r"^segment \d+ refused: (.*)$", rp.stdout, re.M) == [SEGMENT_REASONS[k] for k in D.refused_segments()]
    rp = subprocess.run([exe, "--gzip"] + files, capture_output=True, text=True, timeout=600)
    assert rp.returncode == 0 and rp.stdout.splitlines()[-1].endswith("; 0 bad") and len(files) == 41, rp.stdout[-2000:]
