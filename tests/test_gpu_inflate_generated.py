"""GPU: the device inflate (csrc/grp_inflate.inc: k_inflate<grp_bgzf_block>, k_inflate<grp_gzip_segment>, k_inflate_crc) on the
streams no compressor of the suite writes (tests/deflate_gen.py: random codes up to 15 bits, every (distance, length)
pair of the match copy, members across the flush thresholds, hand-made histories at every bit phase and alignment), on
what htslib's encoder writes (the libdeflate fixtures of tests/golden), and on every refused input with its REASON: the
message must name zlib's own reason where zlib names one, and all 18 statuses of the decoder are provoked.

The expectation is zlib's everywhere.  tests/test_deflate_gen_cpu.py runs the same corpus through the decoder's text
compiled as plain C++, where the 64 lanes run one after the other; here they share the tables, the match copy, the flush
and the history through LDS."""
import gzip
import os
import zlib

import numpy as np
import pytest

import bgzf_cases as B
import deflate_gen as D
import gzip_cases as G
from helpers import default_seeds
from test_gpu_bgzf import _pack as _pack_members
from test_gpu_gzip import BAD as OLD_BAD_SEGMENTS, _bad_forms, _pack as _pack_segments, cases, host  # noqa: F401 (cases, host: fixtures)

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# INF_STATUS_TEXT[1:] of csrc/grp_inflate.inc (tests/test_deflate_gen_cpu.py compares the two)
STATUS_TEXT = [
    "invalid block type",
    "invalid stored block lengths",
    "the compressed data ends inside the stream",
    "the stream holds more text than the member's ISIZE",
    "invalid distance too far back",
    "too many length or distance symbols",
    "invalid code lengths set",
    "invalid bit length repeat",
    "invalid code -- missing end-of-block",
    "invalid literal/lengths set",
    "invalid distances set",
    "invalid literal/length code",
    "invalid distance code",
    "the stream holds less text than the member's ISIZE",
    "compressed bytes behind the end of the stream",
    "CRC32 of the text differs from the member's",
    "a final block inside a segment that does not end its member",
    "the segment ends its member, its bits end in front of a final block",
]
ENDS, MORE, LESS, BEHIND, CRC, FINAL_INSIDE, NO_FINAL = (STATUS_TEXT[i] for i in (2, 3, 13, 14, 15, 16, 17))

# The reason the device must give for every refused input.  Where zlib names a reason (bgzf_cases.refused_reasons,
# deflate_gen.refused_segments, zlib.error on the segment) the entry IS zlib's wording, and the tests check that it is;
# the other entries are the statuses zlib has no word for.
MEMBER_REASONS = {
    "wrong_crc": CRC, "text_len_plus_1": LESS, "text_len_minus_1": MORE, "cut_by_5": ENDS,
    "block_type_3": "invalid block type", "stored_len_mismatch": "invalid stored block lengths", "oversubscribed_code_lengths": "invalid code lengths set",
    "incomplete_literal_set": "invalid literal/lengths set", "match_at_position_0": "invalid distance too far back", "distance_symbol_30": "invalid distance code",
    "hlit_287": "too many length or distance symbols", "hdist_31": "too many length or distance symbols", "hdist_32": "too many length or distance symbols",
    "repeat16_first": "invalid bit length repeat", "repeat16_past_the_end": "invalid bit length repeat", "repeat17_past_the_end": "invalid bit length repeat",
    "repeat18_past_the_end": "invalid bit length repeat",
    "no_end_of_block_code": "invalid code -- missing end-of-block", "no_code_at_all": "invalid code -- missing end-of-block",
    "oversubscribed_distance_set": "invalid distances set", "incomplete_distance_set": "invalid distances set",
    # zlib looks for symbol 256 before it looks at the code: "missing end-of-block", not "invalid literal/lengths set"
    "single_literal_code": "invalid code -- missing end-of-block",
    "fixed_symbol_286": "invalid literal/length code", "fixed_symbol_287": "invalid literal/length code", "single_distance_code_other_bit": "invalid distance code",
    "trailing_1_byte": BEHIND, "trailing_4_bytes": BEHIND, "stored_block_beyond_text_len": MORE, "match_beyond_text_len": MORE,
}
SEGMENT_REASONS = {
    # (zlib inflates the flipped stream to as many bytes of another text; the bits that are cut hold the end-of-block code)
    "flipped_payload_bit": CRC, "wrong_crc": CRC, "text_len_plus_1": LESS, "text_len_minus_1": MORE, "n_bits_short_by_a_block": LESS, "n_bits_inside_a_block": ENDS,
    "final_block_in_a_segment_that_is_not_the_last": FINAL_INSIDE, "no_final_block_where_the_member_ends": NO_FINAL,
    "history_one_byte_short": "invalid distance too far back",
    "first_match_in_front_of_a_history_of_5": "invalid distance too far back", "first_match_in_front_of_a_history_of_32767": "invalid distance too far back",
}
REFUSED = [("member", n) for n in MEMBER_REASONS] + [("segment", n) for n in SEGMENT_REASONS]


@pytest.fixture(scope="module")
def eng(native):
    e = native.Engine(22, 3, 1000, 1 << 20, default_seeds())
    yield e
    e.close()


def _items(streams):
    """[(payload, text length, CRC32)] and the texts, both by zlib"""
    texts = [B.confirm_good(s.payload)[0] for s in streams]
    return [(s.payload, len(t), zlib.crc32(t)) for s, t in zip(streams, texts)], texts


def _inflate_and_compare(eng, streams, gap, order=None):
    items, texts = _items(streams)
    order = range(len(items)) if order is None else order
    comp, blocks = _pack_members([items[i] for i in order], gap=gap)
    got = eng.bgzf_inflate(comp, blocks)
    at = 0
    for i in order:
        s, exp = streams[i], texts[i]
        assert got[at:at + len(exp)] == exp, "member %d (%s, seed %s): %d bytes of text differ from zlib's" % (i, s.name, s.seed, len(exp))
        at += len(exp)
    assert at == len(got)
    return blocks, [len(texts[i]) for i in order]


def test_generated_members_inflate_to_zlibs_text(eng):
    members = D.members()
    assert len(members) == D.N_MEMBERS
    blocks, lens = _inflate_and_compare(eng, members, gap=1)
    # payloads and texts start at every alignment
    assert {b[0] % 4 for b in blocks} == {0, 1, 2, 3}
    assert {int(x) % 4 for x in np.cumsum([0] + lens[:-1])} == {0, 1, 2, 3}
    # ... and in another order: the members are independent of each other
    _inflate_and_compare(eng, members, gap=3, order=[int(i) for i in np.random.default_rng(11).permutation(len(members))])


def test_every_distance_and_length_of_the_match_copy(eng):
    sweep, pairs = D.match_sweep()
    assert pairs == {(d, n) for d in D.SWEEP_DISTANCES for n in D.SWEEP_LENGTHS} and len(pairs) > 11000
    _inflate_and_compare(eng, sweep, gap=1)


def test_text_carried_across_the_flush_thresholds(eng):
    members = [m for m, _ in D.threshold_members()]
    assert len(members) == len(D.THRESHOLDS) * len(D.STEPS) * len(D.BELOW)
    _inflate_and_compare(eng, members, gap=1)
    _inflate_and_compare(eng, members, gap=0)


@pytest.mark.parametrize("name", ["libdeflate_members.bgzf", "tiny_libdeflate.fq.gz"])
def test_libdeflate_written_members(eng, name):
    buf = open(os.path.join(GOLD, name), "rb").read()
    blocks, consumed, why = B.walk_members(buf)
    assert consumed == len(buf) and why == 1 and len(blocks) >= 4
    texts = [zlib.decompress(buf[o:o + n], -15) for o, n, _, _ in blocks]  # zlib's word, never a stored copy
    assert all((len(t), zlib.crc32(t)) == (isize, crc) for t, (_, _, isize, crc) in zip(texts, blocks))
    got = eng.bgzf_inflate(buf, blocks)
    at = 0
    for i, t in enumerate(texts):
        assert got[at:at + len(t)] == t, "%s: member %d" % (name, i)
        at += len(t)
    assert at == len(got)
    if name.startswith("tiny"):
        assert got == G.tiny()


@pytest.fixture(scope="module")
def gen_streams(tmp_path_factory, host):
    """name -> (file bytes, text by zlib, {span: segments}) of the generated gzip streams and tiny_libdeflate.fq.gz"""
    d = tmp_path_factory.mktemp("gzip_generated")
    files = {s.name + " (seed %s)" % (s.seed,): s.payload for s in D.gzip_streams()}
    files["tiny_libdeflate.fq.gz"] = open(os.path.join(GOLD, "tiny_libdeflate.fq.gz"), "rb").read()
    out = {}
    for k, (name, f) in enumerate(files.items()):
        p = d / ("%d.gz" % k)
        p.write_bytes(f)
        text = gzip.decompress(f)
        out[name] = (f, text, {span: host.gzip_index(p, span)["segments"] for span in G.SPANS})
        assert all(sum(g["text_len"] for g in segs) == len(text) for segs in out[name][2].values()), name
    return out


@pytest.mark.parametrize("span", G.SPANS)
def test_generated_streams_inflate_segment_by_segment(eng, gen_streams, span):
    assert len(gen_streams) == D.N_STREAMS + 1
    for gap in (0, 1):
        for name, (f, text, segs) in gen_streams.items():
            comp, hist, table = _pack_segments([(f, g) for g in segs[span]], gap)
            assert eng.gzip_inflate(comp, hist, table) == text, (name, span, gap)
    if span == 1:  # (every block that holds text is a segment: they start on every bit)
        assert {g["comp_bit"] % 8 for _, _, segs in gen_streams.values() for g in segs[1]} == set(range(8))


def test_hand_made_segments(eng):
    segs = D.hand_segments()
    assert len(segs) == 8 * len(D.HISTORY_LENGTHS)
    for gap in (1, 2, 3, 0):
        comp, hist, table = _pack_segments([(f, g) for _, f, g, _ in segs], gap)
        assert {t[0] % 8 for t in table} == set(range(8))
        assert {t[3] % 4 for t in table} == {0, 1, 2, 3}
        if gap:  # the histories start at every address, those of a multiple of 4 bytes too (the dword loop and the byte loop)
            assert {t[2] % 4 for t in table if t[3]} == {0, 1, 2, 3} == {t[2] % 4 for t in table if t[3] == 32768}
        got = eng.gzip_inflate(comp, hist, table)
        at = 0
        for name, f, g, text in segs:  # (text: zlib's, deflate_gen.hand_segments)
            assert got[at:at + len(text)] == text, (name, gap)
            at += len(text)
        assert at == len(got)


# ---- refusals ----------------------------------------------------------------------------------------------------------
_SEEN = {}


def _device_reason(err):
    hits = [t for t in STATUS_TEXT if str(err).endswith(t)]
    assert len(hits) == 1, str(err)
    return hits[0]


def _refuse(eng, native, cases, kind, name):
    """the refused input between good entries -> the reason the device gives; the good entries alone inflate afterwards"""
    if (kind, name) in _SEEN:
        return _SEEN[kind, name]
    if kind == "member":
        bad = B.refused()[name]  # (zlib has turned it down: bgzf_cases.refused)
        assert B.refused_reasons()[name] in (None, MEMBER_REASONS[name]), "zlib names another reason: %s" % B.refused_reasons()[name]
        good, texts = _items([s for s in D.members()[:60] if len(s.text) > 100][:3])
        comp, blocks = _pack_members([good[0], good[1], bad, good[2]], gap=2)
        with pytest.raises(native.GrpError) as e:
            eng.bgzf_inflate(comp, blocks)
        assert e.value.code == native.GRP_ERR_INVALID and e.value.bad_block == 2 and "block 2" in str(e.value), str(e.value)
        comp, blocks = _pack_members(good, gap=2)
        assert eng.bgzf_inflate(comp, blocks) == b"".join(texts)
    else:
        if name in OLD_BAD_SEGMENTS:
            fb, gb = _bad_forms(cases)[name]
            try:
                G.inflate_segment(fb, gb["comp_bit"], gb["n_bits"], gb["dict"])
                named = None
            except zlib.error as z:
                named = str(z).split(": ", 1)[1]
            except AssertionError:
                named = None
        else:
            fb, gb, named = D.refused_segments()[name]
        assert named in (None, SEGMENT_REASONS[name]), "zlib names another reason: %s" % named
        f, text, segs = cases["tiny_level1"]
        ok = [(f, g) for g in segs[50000][:3]]
        comp, hist, table = _pack_segments([ok[0], ok[1], (fb, gb), ok[2]], gap=2)
        with pytest.raises(native.GrpError) as e:
            eng.gzip_inflate(comp, hist, table)
        assert e.value.code == native.GRP_ERR_INVALID and e.value.bad_seg == 2 and "segment 2" in str(e.value), str(e.value)
        comp, hist, table = _pack_segments(ok, gap=2)
        assert eng.gzip_inflate(comp, hist, table) == text[:sum(g["text_len"] for _, g in ok)]
    _SEEN[kind, name] = _device_reason(e.value)
    return _SEEN[kind, name]


@pytest.mark.parametrize("kind,name", REFUSED)
def test_refused_inputs_name_the_reason(eng, native, cases, kind, name):
    want = (MEMBER_REASONS if kind == "member" else SEGMENT_REASONS)[name]
    assert _refuse(eng, native, cases, kind, name) == want


def test_every_status_of_the_decoder_is_provoked(eng, native, cases):
    assert set(MEMBER_REASONS) == set(B.refused()) and set(SEGMENT_REASONS) == set(OLD_BAD_SEGMENTS) | set(D.refused_segments())
    seen = {_refuse(eng, native, cases, kind, name) for kind, name in REFUSED}
    assert seen == set(STATUS_TEXT) and len(STATUS_TEXT) == 18
