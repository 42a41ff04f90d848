"""GPU: grp_gzip_walk (csrc/grp_inflate.inc, k_inflate<InfWalkEntry>: the open form of the decoder) and the rounds that
drive it (csrc/host/gr_gzwalk.cpp) through gr_gzidx_build_device: the restart index of plain gzip files built on the device,
the files side by side.  The expectation is the index the zlib reader writes (gr_gzidx_build; tests/test_gzip_index_cpu.py
checks that one against a walk in Python and zlib): the two must agree field by field, whatever the span, the sizes of a
step or the number of rounds, and every file the walk does not complete is left to the reader untouched."""
import os
import zlib

import numpy as np
import pytest

import bgzf_cases as B
import deflate_gen as D
import gzip_cases as G
from helpers import default_seeds

pytestmark = pytest.mark.gpu

SPANS = (1, 4096, 262144)
INFO = ("complete", "n_text", "index_bytes", "max_text", "file_size", "matches", "dropped", "failed")


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


@pytest.fixture()
def sizes(monkeypatch):
    """GRP_GZIP_WALK_ROOM for one test: sizes(room, window, cap)"""
    monkeypatch.delenv("GRP_GZIP_WALK_ROOM", raising=False)
    return lambda *v: monkeypatch.setenv("GRP_GZIP_WALK_ROOM", ",".join(str(x) for x in v))


def _write(d, files):
    paths = []
    for name, data in files.items():
        p = d / (name + ".gz")
        p.write_bytes(data)
        paths.append(p)
    return paths


def _same(dev, ref, what):
    """the device-built index is the reader's, field by field"""
    assert dev is not None and dev["left"] is None, (what, dev and dev["left"], dev and dev["status"])
    assert len(dev["segments"]) == len(ref["segments"]), (what, len(dev["segments"]), len(ref["segments"]))
    for i, (a, b) in enumerate(zip(dev["segments"], ref["segments"])):
        for k in ("comp_bit", "n_bits", "text_len", "crc32", "flags"):
            assert a[k] == b[k], (what, i, k, a[k], b[k])
        assert a["dict"] == b["dict"], (what, i, "history", len(a["dict"]), len(b["dict"]))
    for k in INFO:
        assert dev[k] == ref[k], (what, k, dev[k], ref[k])


def _inflate(eng, f, segs):
    hist, table = bytearray(), []
    for g in segs:
        hist += b"\0" * (-len(hist) % 4)
        table.append((g["comp_bit"], g["n_bits"], len(hist), len(g["dict"]), g["text_len"], g["crc32"], g["flags"]))
        hist += g["dict"]
    return eng.gzip_inflate(f, bytes(hist), table)


# ---- 1. the index is the reader's index ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    streams = G.streams()
    return streams, _write(tmp_path_factory.mktemp("gzip_walk"), {name: f for name, (f, _) in streams.items()})


@pytest.mark.parametrize("span", SPANS)
def test_the_index_is_the_readers_index(eng, host, cases, sizes, span):
    streams, paths = cases
    got, stats = host.gzip_index_device(eng, paths, span)
    assert stats["files"] == stats["walked"] == len(paths) and stats["left_to_zlib"] == 0, stats
    for (name, (f, text)), p, dev in zip(streams.items(), paths, got):
        ref = host.gzip_index(p, span)
        assert ref["complete"] and sum(g["text_len"] for g in ref["segments"]) == len(text)
        _same(dev, ref, (name, span))
        assert _inflate(eng, f, dev["segments"]) == text, (name, span)
    # one file alone (gr_gzidx_build_device's case): the same rounds with one step each
    one, _ = host.gzip_index_device(eng, paths[:1], span)
    _same(one[0], host.gzip_index(paths[0], span), "alone")


# ---- 2. the history from step to step ---------------------------------------------------------------------------------------
CARRY = (0, 1, 32767, 32768, 32769, 3 * 32768 + 5)


def _carry_stream(n):
    """three members over the first n bytes of tiny.fq: blocks of 5000 bytes of text, of 11 000, and zlib's own"""
    t = G.tiny()[:n]
    assert len(t) == n
    return G.member(t, 6, flush_every=5000) + G.member(t, 1, flush_every=11000) + G.member(t, 9), t * 3


@pytest.mark.parametrize("span", (4096, 40000))
def test_history_carry(eng, host, tmp_path, sizes, span):
    """span 4096: every round of the first member yields 5000 bytes, less than 32 KiB: the history is the old tail and the
    text; span 40 000: a round yields 40 000 and more: the history is the tail of the text alone"""
    streams = {"carry%d" % n: _carry_stream(n) for n in CARRY}
    paths = _write(tmp_path, {k: f for k, (f, _) in streams.items()})
    got, stats = host.gzip_index_device(eng, paths, span)
    assert stats["walked"] == len(paths) and stats["rounds"] >= 3 * (CARRY[-1] // max(span, 11000)), stats
    for (name, (f, text)), p, dev in zip(streams.items(), paths, got):
        ref = host.gzip_index(p, span)
        _same(dev, ref, (name, span))
        assert _inflate(eng, f, dev["segments"]) == text, name
    sizes_seen = {len(g["dict"]) for dev in got for g in dev["segments"]}
    assert 32768 in sizes_seen and 0 in sizes_seen and (span != 4096 or any(0 < s < 32768 for s in sizes_seen)), sorted(sizes_seen)


def test_steps_at_the_engine_entry(eng, native):
    """grp_gzip_walk itself, a stream walked step by step from Python: bits, text, CRC32, the final flag and the history of
    every step against the blocks a walk in Python finds and zlib's text"""
    text = G.tiny()[:3 * 32768 + 5]
    f = G.member(text, 6, flush_every=5000)
    blocks = G.walk_blocks(f, G.payload_bit(f))
    ends = {b1: (t1, final) for (_, b1, _, t1, final) in blocks}
    for min_text in (1, 7000, 50000):
        bit, hist, out, n_steps = G.payload_bit(f), b"", b"", 0
        while True:
            res, hists, texts = eng.gzip_walk(f, hist, [(bit, 8 * len(f) - bit, 0, len(hist), min_text, 1 << 18)], want_text=True)
            r = res[0]
            assert r["status"] == 0, (min_text, n_steps, native.load().grp_gzip_status_text(int(r["status"])))
            assert r["text_len"] >= min_text or r["final"]
            bit += int(r["bits"])
            out += texts[0]
            assert ends[bit] == (len(out), bool(r["final"])), (min_text, n_steps)
            assert r["crc32"] == zlib.crc32(texts[0]) and len(texts[0]) == r["text_len"]
            assert hists[0] == (hist + texts[0])[-32768:] == out[-32768:], (min_text, n_steps)
            hist = hists[0]
            n_steps += 1
            if r["final"]:
                break
        assert out == text and n_steps >= (3 if min_text < 50000 else 2)


# ---- 3. ragged rounds --------------------------------------------------------------------------------------------------------
def test_ragged_rounds(eng, host, tmp_path, sizes):
    t = G.tiny() * 2
    lengths = [int(len(t) * (i / 67.0) ** 2.5) for i in range(68)]
    assert lengths[0] == 0 and lengths[1] < 20 and lengths[-1] > 300000
    files = {"r%02d" % i: G.member(t[:n], (1, 6, 9)[i % 3]) for i, n in enumerate(lengths)}
    whole = G.member(t[:70000], 6)
    files["tail"] = whole + b"\0\0\0"            # bytes behind the last member that are no member
    files["cut"] = whole[:len(whole) * 2 // 3]   # the file ends inside a block
    paths = _write(tmp_path, files)
    assert len(paths) == 70
    refs = [host.gzip_index(p, 100000) for p in paths]
    got, stats = host.gzip_index_device(eng, paths, 100000)
    assert (stats["files"], stats["walked"], stats["left_to_zlib"]) == (70, 68, 2) and stats["launches"] == stats["rounds"] >= 4, stats
    for name, p, dev, ref in zip(files, paths, got, refs):
        if name in ("tail", "cut"):
            assert not dev["complete"] and dev["left"] and not dev["segments"], (name, dev["left"])
            assert not ref["complete"] and ref["failed"] == (name == "cut")
        else:
            _same(dev, ref, name)
    assert got[-1]["status"] == native_status("INPUT_ENDS") and "end of the file" in got[-1]["left"]
    assert "no member" in got[-2]["left"]
    # the reader's answer for the truncated file is what it was: the walk has touched nothing of it
    again = host.gzip_index(paths[-1], 100000)
    assert (again["failed"], again["n_text"], again["complete"]) == (True, refs[-1]["n_text"], False)


def native_status(name):
    from goldrush_amd import native

    return {"INPUT_ENDS": native.GZIP_WALK_INPUT_ENDS, "NO_ROOM": native.GZIP_WALK_NO_ROOM}[name]


# ---- 4. growth ----------------------------------------------------------------------------------------------------------------
def _run_block(n):
    """one fixed block: a literal and matches of distance 1 up to n bytes — a block whose text is far larger than its bits"""
    w = B.BitWriter()
    left, syms = n - 1, [ord("A")]
    while left:
        k = min(left, 258) if left - min(left, 258) == 0 or left - min(left, 258) >= 3 else left - 3
        syms.append(("m", k, 1))
        left -= k
    B.fixed_block(w, True, syms)
    raw, text = w.done(), b"A" * n
    assert zlib.decompress(raw, -15) == text
    return D.gzip_wrap(raw, text), text


def test_growth(eng, host, tmp_path, sizes):
    run, run_text = _run_block(100000)
    stored = G.member(G.tiny()[:150000], 0)  # stored blocks of 65 535 bytes
    other = G.member(G.tiny()[:30000], 6, flush_every=900)
    paths = _write(tmp_path, {"run": run, "stored": stored, "other": other})
    refs = [host.gzip_index(p, 4096) for p in paths]
    sizes(512, 256, 1 << 20)  # the first room and window; both far below a block of either file
    got, stats = host.gzip_index_device(eng, paths, 4096)
    assert stats["walked"] == 3 and stats["repeats"] >= 8, stats  # 512 -> 131 072 for the run: eight doublings
    for p, dev, ref in zip(paths, got, refs):
        _same(dev, ref, p.name)
    assert _inflate(eng, run, got[0]["segments"]) == run_text
    # the cap below the block: that file is left to zlib, the others are what they were
    sizes(512, 256, 32768)
    got, stats = host.gzip_index_device(eng, paths, 4096)
    assert (stats["walked"], stats["left_to_zlib"]) == (1, 2), stats
    assert got[0]["left"] and got[0]["status"] == native_status("NO_ROOM") and not got[0]["complete"]
    assert got[1]["left"] and got[1]["status"] in (native_status("NO_ROOM"), native_status("INPUT_ENDS"))
    _same(got[2], refs[2], "other")
    assert host.gzip_index(paths[0], 4096) == refs[0]


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------
def _member_of(write):
    w = B.BitWriter()
    write(w)
    return b"\x1f\x8b\x08\0\0\0\0\0\0\x03" + w.done() + b"\0" * 8


def _damaged():
    """status -> a gzip file whose first block the open form refuses with it: every status inf_stream<INF_OPEN> can return but
    3 (the input ends: test_ragged_rounds, test_growth) and 19 (no room: test_growth).  The statuses that judge a given end
    — 4, 14, 15, 17, 18: text_len, n_bits, the flag — cannot occur, an open step has no such end; 16 is the CRC kernel's
    comparison, which a step does not make."""
    out = {}
    out[1] = _member_of(lambda w: (w.bits(1, 1), w.bits(3, 2), w.bits(0, 32)))                                   # block type 3
    out[2] = _member_of(lambda w: (w.bits(1, 1), w.bits(0, 2), w.align(), w.bits(5, 16), w.bits(5, 16)))         # LEN / NLEN
    out[5] = _member_of(lambda w: B.fixed_block(w, True, [65, 66, 67, ("m", 3, 4)]))                             # a distance in front of the member
    out[6] = _member_of(lambda w: (w.bits(1, 1), w.bits(2, 2), w.bits(30, 5), w.bits(0, 5), w.bits(0, 4), w.bits(0, 32)))  # 287 literal/length codes
    out[7] = _member_of(lambda w: (w.bits(1, 1), w.bits(2, 2), w.bits(0, 5), w.bits(0, 5), w.bits(0, 4), [w.bits(1, 3) for _ in range(4)], w.bits(0, 32)))  # an over-subscribed code length code
    # the faults of a dynamic block's header: the payloads tests/bgzf_cases.py builds for the member form, one defect each
    refused = B.refused()
    for status, name in ((8, "repeat16_first"), (9, "no_end_of_block_code"), (10, "incomplete_literal_set"), (11, "oversubscribed_distance_set")):
        out[status] = b"\x1f\x8b\x08\0\0\0\0\0\0\x03" + refused[name][0] + b"\0" * 8
    out[12] = _member_of(lambda w: (w.bits(1, 1), w.bits(1, 2), w.code(0xC0 + 6, 8), w.bits(0, 32)))             # length symbol 286
    out[13] = _member_of(lambda w: (w.bits(1, 1), w.bits(1, 2), B.fixed_code(w, 65), B.fixed_code(w, 257), w.code(30, 5), w.bits(0, 32)))  # distance symbol 30
    return out


def test_refusals(eng, host, native, tmp_path, sizes):
    bad = _damaged()
    assert sorted(bad) == [1, 2, 5, 6, 7, 8, 9, 10, 11, 12, 13]
    good_f, good_t = G.member(G.tiny()[:50000], 6), G.tiny()[:50000]
    for status, f in bad.items():
        with pytest.raises(zlib.error):
            zlib.decompress(f, 31)
    # the steps themselves, good ones between them: every damaged one answers with its status, the good ones with their text
    comp, steps, at = bytearray(), [], {}
    for name, f in [("good0", good_f)] + [(s, f) for s, f in bad.items()] + [("good1", good_f)]:
        comp += b"\0" * (-len(comp) % 8)
        at[name] = len(comp)
        steps.append((8 * len(comp) + G.payload_bit(f), 8 * len(f) - G.payload_bit(f), 0, 0, 1 << 20, 1 << 16))
        comp += f
    res, hists, texts = eng.gzip_walk(bytes(comp), b"", steps, want_text=True)
    assert [int(r["status"]) for r in res] == [0] + list(bad) + [0], [native.load().grp_gzip_status_text(int(r["status"])) for r in res]
    for r in res[1:-1]:
        assert (r["bits"], r["text_len"], r["crc32"], r["final"], r["hist_len"]) == (0, 0, 0, 0, 0)
    for k in (0, -1):
        assert texts[k] == good_t and res[k]["final"] == 1 and res[k]["crc32"] == zlib.crc32(good_t) and hists[k] == good_t[-32768:]
    # ... and the files: each is left to zlib with that status, the good ones beside them get the reader's index
    files = {"good0": good_f}
    files.update({"bad%d" % s: f for s, f in bad.items()})
    files["good1"] = good_f
    paths = _write(tmp_path, files)
    got, stats = host.gzip_index_device(eng, paths, 4096)
    assert (stats["walked"], stats["left_to_zlib"]) == (2, len(bad)), stats
    for (status, _), dev, p in zip(bad.items(), got[1:-1], paths[1:-1]):
        assert dev["left"] and dev["status"] == status and not dev["complete"], (status, dev["left"], dev["status"])
        assert host.gzip_index(p, 4096)["failed"]
    for k in (0, -1):
        _same(got[k], host.gzip_index(paths[k], 4096), "good")


# ---- 6. table checks ------------------------------------------------------------------------------------------------------------
def test_bad_table_entries_are_refused_and_named(eng, native):
    """(the checks stand in front of the first allocation and launch in grp_gzip_walk; what a test can see of that is the
    entry named, no answer, and an engine that goes on)"""
    f = G.member(G.tiny()[:20000], 6)
    bit = G.payload_bit(f)
    hist = b"h" * 40000
    good = (bit, 8 * len(f) - bit, 0, 0, 1 << 20, 1 << 16)
    forms = [((bit, 8 * len(f) - bit + 1) + good[2:], None),      # the bits leave comp
             ((8 * len(f) + 1,) + good[1:], None),
             (good[:2] + (len(hist) - 99, 100) + good[4:], None),  # the history leaves dict
             (good[:3] + (32769,) + good[4:], None),               # dict_len > 32768
             (good + (1,), None),                                  # a reserved field
             (good, 2 * (1 << 16) - 1)]                            # the sum of the rooms > text_cap
    for bad, cap in forms:
        with pytest.raises(native.GrpError) as e:
            eng.gzip_walk(f, hist, [good, bad], want_text=True, text_cap=cap)
        assert e.value.code == native.GRP_ERR_INVALID and e.value.bad_step == 1 and "step 1" in str(e.value), str(e.value)
    with pytest.raises(native.GrpError) as e:  # the rooms of all steps together, without a text buffer: 2^34
        eng.gzip_walk(f, hist, [good[:5] + (1 << 31,)] * 9)
    assert e.value.code == native.GRP_ERR_INVALID and e.value.bad_step == 8
    res, hists, texts = eng.gzip_walk(f, hist, [good, good], want_text=True)
    assert [int(r["status"]) for r in res] == [0, 0] and texts[0] == texts[1] == G.tiny()[:20000]
    res, _, _ = eng.gzip_walk(b"", b"", [])
    assert len(res) == 0
