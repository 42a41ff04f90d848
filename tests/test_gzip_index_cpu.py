"""CPU: the index of a plain gzip file (csrc/host/gr_gzidx.cpp) and the host program's use of it.  Every segment of every
stream of tests/gzip_cases.py is checked without the code under test — its bits inflated by Python's zlib with its history
as the preset dictionary — and, for the one-member streams, against a walk over the blocks in Python.  Then the product's
whole host program (gr_path_main_ext) over the oracle engine with a zlib-backed stand-in for grp_gzip_inflate in the second
engine table: the outputs are the plain file's, the stand-in is handed every segment exactly once, in order, in each pass
behind the one that built the index.  (tests/test_gpu_gzip.py and test_gpu_cli_gzip.py do the same with the HIP engine.)"""
import gzip
import os
import zlib

import pytest

import ext_runner as X
import gzip_cases as G

NAMES = ["tiny_level1", "tiny_level6", "tiny_level9", "fixed", "stored", "flushed", "acgt", "distance_32768", "two_members_and_an_empty_one", "bgzf"]
ONE_MEMBER = ("flushed", "stored", "acgt", "distance_32768", "fixed")


@pytest.fixture(scope="module")
def host(native):
    from goldrush_amd import host as h

    h.load()
    return h


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """name -> (path, file bytes, text)"""
    d = tmp_path_factory.mktemp("gzip_cases")
    out = {}
    for name, (f, text) in G.streams().items():
        assert gzip.decompress(f) == text  # (zlib's word)
        p = d / (name + ".fq.gz")
        p.write_bytes(f)
        out[name] = (p, f, text)
    return out


@pytest.fixture(scope="module")
def walks(cases):
    return {n: G.walk_blocks(cases[n][1], G.payload_bit(cases[n][1])) for n in ONE_MEMBER}


def check_index(ix, f, text, span):
    """every segment by zlib; the segments tile the text and, inside a member, the bit stream"""
    assert ix["complete"] and not ix["dropped"] and not ix["failed"] and ix["matches"]
    assert ix["n_text"] == len(text) and ix["text"] == text and ix["file_size"] == len(f)
    off = member_start = 0
    prev = None
    for i, g in enumerate(ix["segments"]):
        assert g["text_len"] > 0 and g["n_bits"] > 0 and g["flags"] in (0, 1), (i, g["text_len"], g["flags"])
        assert g["comp_bit"] + g["n_bits"] <= 8 * len(f)
        if prev is not None and not prev["flags"] & 1:
            assert g["comp_bit"] == prev["comp_bit"] + prev["n_bits"], i  # no gap, no overlap
        elif prev is not None:
            assert g["comp_bit"] >= prev["comp_bit"] + prev["n_bits"] + 8 * (8 + 10) and g["comp_bit"] % 8 == 0, i  # a trailer and a header between
        if prev is None or prev["flags"] & 1:
            assert g["dict"] == b"" and g["comp_bit"] % 8 == 0, i  # behind a member's header
            member_start = off
        else:
            assert g["dict"] == text[max(member_start, off - 32768):off], i
        if not g["flags"] & 1:
            assert g["text_len"] >= span, i
        got, eof = G.inflate_segment(f, g["comp_bit"], g["n_bits"], g["dict"])
        assert eof == bool(g["flags"] & 1), i
        assert len(got) == g["text_len"] and got == text[off:off + g["text_len"]], i
        assert zlib.crc32(got) == g["crc32"], i
        off += g["text_len"]
        prev = g
    assert off == len(text) and (prev is None or prev["flags"] & 1)
    assert ix["max_text"] == max([g["text_len"] for g in ix["segments"]] + [0])


@pytest.mark.parametrize("span", G.SPANS)
@pytest.mark.parametrize("name", NAMES)
def test_every_segment_inflates_on_its_own_with_zlib(host, cases, walks, name, span):
    p, f, text = cases[name]
    ix = host.gzip_index(p, span, text_cap=len(text) + 1)
    check_index(ix, f, text, span)
    if name in ONE_MEMBER:  # ... and the points are where a walk over the blocks puts them
        assert [(g["comp_bit"], g["n_bits"], g["text_len"], g["flags"]) for g in ix["segments"]] == [(a, b, d, e) for a, b, _, d, e in G.expected_segments(f, span, walks[name])]
    if span == 10 ** 9:  # one segment per member that has text
        members = sum(1 for b in G.B.walk_members(f)[0] if b[2]) if name == "bgzf" else 2 if name == "two_members_and_an_empty_one" else 1
        assert len(ix["segments"]) == members


def test_the_cases_cover_what_they_are_meant_to(host, cases, walks):
    assert set(cases) == set(NAMES)
    # segments start on all eight bit phases, with empty stored blocks inside them
    ix = host.gzip_index(cases["flushed"][0], 1)
    assert {g["comp_bit"] % 8 for g in ix["segments"]} == set(range(8))
    assert sum(1 for b in walks["flushed"] if b[2] == b[3]) >= 20 and len(ix["segments"]) >= 20
    # all stored blocks; segments longer than 64 KiB; a distance of exactly 32768 onto the first byte of the history
    assert all((cases["stored"][1][b[0] >> 3] >> (b[0] & 7)) & 6 == 0 for b in walks["stored"])
    assert max(g["text_len"] for g in host.gzip_index(cases["tiny_level6"][0], 10 ** 9)["segments"]) > 65536
    f, text = cases["distance_32768"][1:]
    g = host.gzip_index(cases["distance_32768"][0], 1)["segments"][1]
    assert g["dict"] == text[:32768] and G.inflate_segment(f, g["comp_bit"], g["n_bits"], g["dict"])[0] == text[32768:]
    with pytest.raises(zlib.error):
        G.inflate_segment(f, g["comp_bit"], g["n_bits"], g["dict"][1:])
    assert len(host.gzip_index(cases["tiny_level6"][0], 1)["segments"]) >= 5


def test_an_early_ended_build_is_incomplete(host, cases):
    p, f, text = cases["tiny_level6"]
    ix = host.gzip_index(p, 1, stop_after=100000)
    assert not ix["complete"] and not ix["dropped"] and 100000 <= ix["n_text"] < len(text)
    assert 1 <= len(ix["segments"]) < len(host.gzip_index(p, 1)["segments"])


def test_the_cap_drops_the_index_and_the_text_still_comes(host, cases):
    p, f, text = cases["tiny_level6"]
    ix = host.gzip_index(p, 1, max_bytes=1 << 19, text_cap=len(text))
    assert ix["dropped"] and not ix["complete"] and ix["segments"] == [] and not ix["failed"]
    assert ix["text"] == text


def test_a_file_written_since_no_longer_matches(host, cases, tmp_path):
    p = tmp_path / "a.fq.gz"
    p.write_bytes(cases["tiny_level6"][1])
    lib = host.load()
    h = lib.gr_gzidx_build(os.fsencode(str(p)), 50000, 1 << 30, 0, None, 0)
    try:
        assert lib.gr_gzidx_matches(h, os.fsencode(str(p))) == 1
        p.write_bytes(cases["tiny_level1"][1])
        assert lib.gr_gzidx_matches(h, os.fsencode(str(p))) == 0
        p.write_bytes(cases["tiny_level6"][1])
        os.utime(p, ns=(1, 1))  # the same size at another time
        assert lib.gr_gzidx_matches(h, os.fsencode(str(p))) == 0
    finally:
        lib.gr_gzidx_free(h)


def test_reader_hands_out_what_gzread_hands_out(host, cases, tmp_path):
    """concatenated members, bytes behind the last member (ignored by gzread: the index is dropped), a truncated stream"""
    import numpy as np
    f, text = cases["two_members_and_an_empty_one"][1:]

    def gzread(path):
        buf = np.zeros(len(text) + 10, dtype=np.uint8)
        n = host.load().gr_input_read(os.fsencode(str(path)), 1 << 16, buf.ctypes.data, buf.size)
        return buf[:n].tobytes()

    for tag, data, dropped, failed in (("whole", f, False, False), ("garbage", f + b"not a member", True, False), ("one_byte", f + b"\x1f", True, False),
                                       ("zeros", f + bytes(100), True, False), ("cut_in_trailer", f[:-3], True, True), ("cut_in_payload", f[:len(f) // 2], True, True),
                                       ("cut_in_second_header", f[:f.index(b"\x1f\x8b", 100) + 5], True, True)):
        p = tmp_path / (tag + ".gz")
        p.write_bytes(data)
        ix = host.gzip_index(p, 50000, text_cap=len(text) + 10)
        assert ix["text"] == gzread(p), tag
        assert (ix["dropped"], ix["failed"], ix["complete"]) == (dropped, failed, not dropped), tag
        assert not failed or len(ix["text"]) < len(text) or tag == "cut_in_trailer"


ARGS = X.ARGS  # (the same list: run() sees what a test appends)
TRACE = X.GZIP_TRACE
BGZF_TRACE = X.BGZF_TRACE
_pick = X.pick


def _run(tmp_path, tag, path, **env):
    rp, files, calls = X.run(tmp_path, tag, path, ("gzip",), **env)
    return rp, files, calls and calls["gzip"]


@pytest.fixture(scope="module")
def plain_run(oracle, native, cases, tmp_path_factory):
    d = tmp_path_factory.mktemp("plain")
    p = d / "plain.fq"
    p.write_bytes(cases["tiny_level6"][2])
    rp, files, calls = _run(d, "plain", p)
    assert rp.returncode == 0 and files and any(files.values()), rp.stderr[-2000:]
    assert calls == [] and TRACE.findall(rp.stderr) and {int(n) for n in TRACE.findall(rp.stderr)} == {0}
    return rp, files


@pytest.mark.parametrize("name,span,chunk,ntcard", [("tiny_level6", 1, 0, False), ("tiny_level6", 50000, 100000, False), ("tiny_level1", 50000, 100000, True), ("two_members_and_an_empty_one", 1, 100000, False),
                                                    ("flushed_whole", 1, 70000, False), ("stored", 1, 100000, False), ("bgzf_off", 50000, 70000, False)])
def test_host_program_inflates_the_segments_through_the_ext_table(oracle, native, host, tmp_path, cases, plain_run, name, span, chunk, ntcard):
    env = {"GRP_GZIP_SPAN": str(span)}
    if chunk:
        env["GRP_INGEST_CHUNK"] = str(chunk)
    if name == "flushed_whole":  # tiny.fq whole with a flush every 997 bytes
        path = tmp_path / "flushed_whole.fq.gz"
        path.write_bytes(G.member(cases["tiny_level6"][2], 6, flush_every=997))
    elif name == "bgzf_off":  # a BGZF file is plain gzip to zlib: with the BGZF form switched off it takes this road
        path, env["GRP_BGZF"] = cases["bgzf"][0], "off"
    else:
        path = cases[name][0]
    plain = plain_run
    if ntcard:
        ARGS.append("--ntcard")
        try:
            pp = tmp_path / "plain.fq"
            pp.write_bytes(cases["tiny_level6"][2])
            plain = _run(tmp_path, "plain_ntcard", pp)[:2]
            rp, files, calls = _run(tmp_path, name, path, **env)
        finally:
            ARGS.remove("--ntcard")
    else:
        rp, files, calls = _run(tmp_path, name, path, **env)
    assert rp.returncode == 0, rp.stderr[-3000:]
    assert files == plain[1]
    assert _pick(rp.stderr) == _pick(plain[0].stderr)
    segs = [[g["crc32"], g["text_len"]] for g in host.gzip_index(path, span)["segments"]]
    assert len(segs) >= (4 if span == 1 else 1)
    traced = [int(n) for n in TRACE.findall(rp.stderr)]
    later = [n for n in traced if n]
    # nothing in the passes up to the first that reads the file to its end, every segment once in each pass behind it
    assert traced[0] == 0 and len(later) >= 1 and traced == [0] * (len(traced) - len(later)) + [len(segs)] * len(later), traced
    assert len(traced) - len(later) <= 2  # (a pass that ends early, the Phred median's, leaves no index)
    assert [g for call in calls for g in call] == segs * len(later)
    assert {int(n) for n in BGZF_TRACE.findall(rp.stderr)} == {0}
    if chunk:  # a slot takes whole segments up to its text capacity
        assert max(sum(g[1] for g in call) for call in calls) <= chunk
        assert len(calls) > len(later)


@pytest.mark.parametrize("tag,env", [("off", {"GRP_GZIP_INDEX": "off"}), ("no_ext", {"NO_EXT_INFLATE": "1"}), ("old_ext", {"OLD_EXT": "1"}), ("cap", {"GRP_GZIP_INDEX_MAX_GB": "0.0001", "GRP_GZIP_SPAN": "1"}),
                                     ("segment_larger_than_a_slot", {"GRP_GZIP_SPAN": "150000"})])
def test_switch_old_caller_and_missing_entry_point_take_the_zlib_path(oracle, native, tmp_path, cases, plain_run, tag, env):
    rp, files, calls = _run(tmp_path, tag, cases["tiny_level6"][0], GRP_INGEST_CHUNK="100000", **env)
    assert rp.returncode == 0, rp.stderr[-3000:]
    assert files == plain_run[1] and calls == []
    traced = [int(n) for n in TRACE.findall(rp.stderr)]
    assert traced and set(traced) == {0}


def test_damaged_files_end_the_run_with_an_error(oracle, native, tmp_path, cases):
    f = cases["tiny_level6"][1]
    cut = tmp_path / "cut.fq.gz"
    cut.write_bytes(f[:len(f) // 2])
    rp, files, calls = _run(tmp_path, "cut", cut, GRP_GZIP_SPAN="1")
    assert rp.returncode != 0 and "failed" in rp.stderr and "cut.fq.gz" in rp.stderr and "truncated" in rp.stderr, rp.stderr[-2000:]
    assert calls == []
