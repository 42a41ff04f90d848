"""GPU: grp_gzip_inflate (csrc/grp_inflate.inc, k_inflate<grp_gzip_segment>) — the segments of a serial DEFLATE stream inflated one wave
per segment: a start at any bit, a preset history, an end at a block boundary, any amount of text.  The streams are those of
tests/gzip_cases.py, the segments the index's (csrc/host/gr_gzidx.cpp; tests/test_gzip_index_cpu.py checks every one of them
with zlib), the expectation is the text zlib inflates; every refused input is one zlib refuses too, or holds another text.
The launcher, the buffer pool and the CRC32 tables are those of grp_bgzf_inflate (tests/test_gpu_bgzf.py): the last test
mixes the two on one engine."""
import zlib

import numpy as np
import pytest

import bgzf_cases as B
import gzip_cases as G
from helpers import default_seeds
from test_gpu_bgzf import _pack as _pack_members

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(native):
    e = native.Engine(22, 3, 1000, 1 << 20, default_seeds())
    yield e
    e.close()


@pytest.fixture(scope="module")
def host(native):
    from goldrush_amd import host as h

    h.load()
    return h


@pytest.fixture(scope="module")
def cases(tmp_path_factory, host):
    """name -> (file bytes, text, {span: segments})"""
    d = tmp_path_factory.mktemp("gzip_gpu")
    streams = dict(G.streams())
    t = G.tiny()
    streams["long"] = (G.member(t + t[::-1] + t, 6), t + t[::-1] + t)  # 564 KB: at span 10^9 one segment of all of it
    out = {}
    for name, (f, text) in streams.items():
        p = d / (name + ".gz")
        p.write_bytes(f)
        out[name] = (f, text, {span: host.gzip_index(p, span)["segments"] for span in G.SPANS})
        assert all(sum(g["text_len"] for g in segs) == len(text) for segs in out[name][2].values())
    return out


def _pack(items, gap=0):
    """[(file, segment)] -> (comp, dict, table): the files one after the other (each once), the histories with `gap` + i % 4
    bytes of other data between them (every alignment)"""
    comp, hist, table, at = bytearray(), bytearray(), [], {}
    for i, (f, g) in enumerate(items):
        if id(f) not in at:
            at[id(f)] = len(comp)
            comp += f
        hist += b"\xa5" * ((gap + i) % 4 if gap else 0)
        table.append((8 * at[id(f)] + g["comp_bit"], g["n_bits"], len(hist), len(g["dict"]), g["text_len"], g["crc32"], g["flags"]))
        hist += g["dict"]
    return bytes(comp), bytes(hist), table


@pytest.mark.parametrize("span", G.SPANS)
def test_every_case_inflates_to_its_text(eng, cases, span):
    for gap in (0, 1):  # histories 4-byte aligned (where their length allows), and at every alignment
        for name, (f, text, segs) in cases.items():
            comp, hist, table = _pack([(f, g) for g in segs[span]], gap)
            assert eng.gzip_inflate(comp, hist, table) == text, (name, gap)
    assert {g["comp_bit"] % 8 for g in cases["flushed"][2][1]} == set(range(8))
    assert max(g["text_len"] for g in cases["long"][2][10 ** 9]) == len(cases["long"][1]) > 500000


def test_one_call_with_all_segments_of_all_cases(eng, cases):
    items, expect = [], []
    for name, (f, text, segs) in cases.items():
        for span in G.SPANS:
            items += [(f, g) for g in segs[span]]
            expect.append(text)
    assert len(items) > 100
    comp, hist, table = _pack(items, gap=3)
    before = eng.gzip_stats()
    text = eng.gzip_inflate(comp, hist, table)
    assert text == b"".join(expect)
    after = eng.gzip_stats()
    assert after["segments"] - before["segments"] == len(items)
    assert after["comp_bytes"] - before["comp_bytes"] == len(comp)
    assert after["text_bytes"] - before["text_bytes"] == len(text)
    assert after["kernel_us"] > before["kernel_us"]
    # ... and in another order than the file's: the segments are independent of each other
    order = np.random.default_rng(3).permutation(len(items))
    comp, hist, table = _pack([items[i] for i in order], gap=2)
    got = eng.gzip_inflate(comp, hist, table)
    at = 0
    for i in order:
        f, g = items[i]
        assert zlib.crc32(got[at:at + g["text_len"]]) == g["crc32"]
        at += g["text_len"]
    assert at == len(got)


def _zlib_refuses(f, g, text):
    """zlib turns the segment down, or inflates it to something else than `text`"""
    try:
        got, eof = G.inflate_segment(f, g["comp_bit"], g["n_bits"], g["dict"])
    except (zlib.error, AssertionError):
        return True
    return got != text or len(got) != g["text_len"] or eof != bool(g["flags"] & 1)


def _bad_forms(cases):
    """name -> (file, damaged segment): each is confirmed to be bad without the device"""
    f, text, segs = cases["tiny_level6"]
    g = dict(segs[50000][1])  # (two blocks of tiny.fq, 32 KiB of history)
    off = segs[50000][0]["text_len"]
    own = text[off:off + g["text_len"]]
    assert not _zlib_refuses(f, g, own) and len(g["dict"]) == 32768
    out = {}
    flipped = bytearray(f)
    bit = g["comp_bit"] + g["n_bits"] // 2
    flipped[bit >> 3] ^= 1 << (bit & 7)
    out["flipped_payload_bit"] = (bytes(flipped), g)
    out["wrong_crc"] = (f, dict(g, crc32=g["crc32"] ^ 0x10))
    out["text_len_plus_1"] = (f, dict(g, text_len=g["text_len"] + 1))
    out["text_len_minus_1"] = (f, dict(g, text_len=g["text_len"] - 1))
    blocks = [b for b in G.walk_blocks(f, G.payload_bit(f)) if g["comp_bit"] <= b[0] < g["comp_bit"] + g["n_bits"]]
    assert len(blocks) >= 2 and blocks[-1][3] > blocks[-1][2]
    out["n_bits_short_by_a_block"] = (f, dict(g, n_bits=blocks[-1][0] - g["comp_bit"]))
    out["n_bits_inside_a_block"] = (f, dict(g, n_bits=g["n_bits"] - 9))
    last = dict(segs[50000][-1])
    assert last["flags"] == 1
    out["final_block_in_a_segment_that_is_not_the_last"] = (f, dict(last, flags=0))
    out["no_final_block_where_the_member_ends"] = (f, dict(g, flags=1))
    fd, td, sd = cases["distance_32768"]
    h = dict(sd[1][1])
    assert len(h["dict"]) == 32768 and not _zlib_refuses(fd, h, td[32768:])
    out["history_one_byte_short"] = (fd, dict(h, dict=h["dict"][1:]))
    for name, (ff, gg) in out.items():
        if name not in ("wrong_crc", "final_block_in_a_segment_that_is_not_the_last", "no_final_block_where_the_member_ends"):
            assert _zlib_refuses(ff, gg, own if ff is not fd else td[32768:]), name
    return out


BAD = ["flipped_payload_bit", "wrong_crc", "text_len_plus_1", "text_len_minus_1", "n_bits_short_by_a_block", "n_bits_inside_a_block", "final_block_in_a_segment_that_is_not_the_last",
       "no_final_block_where_the_member_ends", "history_one_byte_short"]


@pytest.mark.parametrize("name", BAD)
def test_refused_segments_are_named(eng, native, cases, name):
    fb, gb = _bad_forms(cases)[name]
    f, text, segs = cases["tiny_level1"]
    ok = [(f, g) for g in segs[50000][:3]]
    comp, hist, table = _pack([ok[0], ok[1], (fb, gb), ok[2]], gap=2)
    with pytest.raises(native.GrpError) as e:
        eng.gzip_inflate(comp, hist, table)
    assert e.value.code == native.GRP_ERR_INVALID and e.value.bad_seg == 2, str(e.value)
    assert "segment 2" in str(e.value)
    # the engine goes on: the good segments alone
    comp, hist, table = _pack(ok, gap=2)
    assert eng.gzip_inflate(comp, hist, table) == text[:sum(g["text_len"] for _, g in ok)]


def test_argument_errors_launch_nothing(eng, native, cases):
    f, text, segs = cases["tiny_level6"]
    g0, g1 = segs[50000][0], segs[50000][1]
    comp, hist, table = _pack([(f, g0), (f, g1)])
    good = table[1]
    before = eng.gzip_stats()
    forms = [((good[0], 8 * len(comp) - good[0] + 1) + good[2:], None),  # a segment outside comp
             ((8 * len(comp) + 1,) + good[1:], None),
             (good[:2] + (len(hist) - good[3] + 1,) + good[3:], None),    # a history outside dict
             (good[:3] + (32769,) + good[4:], None),                      # dict_len > 32768
             (good[:6] + (2,), None),                                     # an unknown flag
             (good, good[4] + table[0][4] - 1)]                           # the sum of the texts > text_cap
    for bad, cap in forms:
        with pytest.raises(native.GrpError) as e:
            eng.gzip_inflate(comp, hist, [table[0], bad], text_cap=cap)
        assert e.value.code == native.GRP_ERR_INVALID and (cap is not None or e.value.bad_seg == 1), str(e.value)
    assert eng.gzip_stats() == before
    assert eng.gzip_inflate(comp, hist, table) == text[:g0["text_len"] + g1["text_len"]]
    assert eng.gzip_inflate(b"", b"", []) == b""


def test_segments_and_members_on_one_engine(native, cases):
    """the two formats share the launcher and the CRC32 tables and have a pool each: calls of both on one engine, the
    segments first, give zlib's texts, name the refused block and count their own work only"""
    f, text, segs = cases["tiny_level1"]
    ok = [(f, g) for g in segs[50000][:3]]
    seg_text = text[:sum(g["text_len"] for _, g in ok)]
    members = [B.confirm_good(p) + (p,) for p in (B.deflate(B.texts()[t], **B.FORMS[form]) for t, form in (("fastq", "level6"), ("bytes", "level1"), ("len257", "fixed")))]
    items = [(p, len(t), crc) for t, crc, p in members]
    e = native.Engine(22, 3, 1000, 1 << 20, default_seeds())
    try:
        comp, hist, table = _pack(ok, gap=2)
        assert e.gzip_inflate(comp, hist, table) == seg_text
        mcomp, blocks = _pack_members(items, gap=2)
        assert e.bgzf_inflate(mcomp, blocks) == b"".join(t for t, _, _ in members)
        assert e.gzip_inflate(comp, hist, table) == seg_text
        bcomp, bblocks = _pack_members([items[0], B.refused()["wrong_crc"], items[2]], gap=2)
        with pytest.raises(native.GrpError) as err:
            e.bgzf_inflate(bcomp, bblocks)
        assert err.value.code == native.GRP_ERR_INVALID and err.value.bad_block == 1 and "block 1" in str(err.value), str(err.value)
        gs, bs = e.gzip_stats(), e.bgzf_stats()
        assert (gs["segments"], gs["comp_bytes"], gs["text_bytes"]) == (6, 2 * len(comp), 2 * len(seg_text))
        # (a call whose table passes the checks is counted, whatever its kernels find)
        assert (bs["blocks"], bs["comp_bytes"], bs["text_bytes"]) == (6, len(mcomp) + len(bcomp), sum(b[2] for b in blocks + bblocks))
        assert gs["kernel_us"] > 0 and bs["kernel_us"] > 0
    finally:
        e.close()
