"""GPU: the members of a concatenated gzip file walked side by side (csrc/host/gr_gzwalk.cpp: GzWalkMembers) through
gr_gzidx_build_device_many_ex over grp_gzip_walk: streams begun at every gzip header found behind byte 0 of a file, adopted
by the chain of members from byte 0 where it arrives at them and dropped where it does not.  The expectation is the index
the zlib reader writes (gr_gzidx_build), field by field with the histories, whatever the span, the budget of streams or
what stands in the file where `1f 8b 08` does; the text grp_gzip_inflate gives over the index; and, for a file the walk
leaves to zlib, the reason and status of the walk without the switch.  The files are those of tests/gzip_member_cases.py."""
import pytest

import gzip_member_cases as M
from test_gpu_gzip_walk import _inflate, _same, _write, eng, host, sizes  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu


@pytest.fixture()
def budget(monkeypatch):
    """GRP_GZIP_WALK_STREAMS for one test"""
    monkeypatch.delenv("GRP_GZIP_WALK_STREAMS", raising=False)
    return lambda n: monkeypatch.setenv("GRP_GZIP_WALK_STREAMS", str(n))


@pytest.fixture(scope="module")
def refs(host):
    """the reader's index of a file at a span, computed once"""
    memo = {}

    def ref(path, span):
        if (str(path), span) not in memo:
            memo[(str(path), span)] = host.gzip_index(path, span)
        return memo[(str(path), span)]

    return ref


def _good(eng, host, refs, cases, paths, span):
    """the acceptance of every good case: the reader's index, the text over it, nothing left to zlib"""
    got, stats = host.gzip_index_device(eng, paths, span, members=True)
    assert stats["files"] == stats["walked"] == len(paths) and stats["left_to_zlib"] == 0, stats
    for case, p, dev in zip(cases, paths, got):
        ref = refs(p, span)
        assert ref["complete"] and ref["n_text"] == len(case.text)
        _same(dev, ref, (p.name, span))
        assert _inflate(eng, case.data, dev["segments"]) == case.text, (p.name, span)
    assert stats["text_bytes"] == sum(len(c.text) for c in cases), stats
    return got, stats


# ---- M1, M4 -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ragged(tmp_path_factory):
    case = M.m1_ragged()
    return case, _write(tmp_path_factory.mktemp("members_m1"), {"m1_ragged": case.data})


@pytest.mark.parametrize("span", M.SPANS)
def test_m1_ragged_members(eng, host, refs, ragged, sizes, budget, span):
    case, paths = ragged
    _, stats = _good(eng, host, refs, [case], paths, span)
    serial, serial_stats = host.gzip_index_device(eng, paths, span)
    _same(serial[0], refs(paths[0], span), "serial")
    assert stats["adopted"] == 11 and stats["candidates"] >= 11 and stats["rounds"] < serial_stats["rounds"], (stats, serial_stats)


@pytest.mark.parametrize("n", (1, 3, 1024))
def test_m4_budget(eng, host, refs, ragged, sizes, budget, n):
    case, paths = ragged
    budget(n)
    for span in M.SPANS:
        _, stats = _good(eng, host, refs, [case], paths, span)
        assert 1 <= stats["max_in_flight"] <= n, stats
        if n == 1:
            _, serial_stats = host.gzip_index_device(eng, paths, span)
            assert stats["rounds"] == serial_stats["rounds"] and stats["streams"] == stats["adopted"] == 0, (stats, serial_stats)


# ---- M2: the test that fails without the switch ------------------------------------------------------------------------------------
def test_m2_eight_members_take_the_rounds_of_one(eng, host, refs, tmp_path, sizes, budget):
    eight, one = M.m2_equal()
    paths = _write(tmp_path, {"m2_equal": eight.data, "m2_one": one.data})
    sizes(65536, 32768)
    span = 50000
    _, alone = host.gzip_index_device(eng, paths[1:], span)
    r1 = alone["rounds"]
    assert r1 >= 3, alone
    got, stats = _good(eng, host, refs, [eight], paths[:1], span)
    assert stats["rounds"] <= r1 + 1 and stats["adopted"] == 7, (r1, stats)
    serial, serial_stats = host.gzip_index_device(eng, paths[:1], span)
    assert serial_stats["rounds"] >= 8 * r1 - 8, (r1, serial_stats)
    _same(serial[0], refs(paths[0], span), "serial")
    assert serial[0]["segments"] == got[0]["segments"]


# ---- M3 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(M.m3_false_candidates()))
def test_m3_false_candidates(eng, host, refs, tmp_path, sizes, budget, name):
    case = M.m3_false_candidates()[name]
    paths = _write(tmp_path, {name: case.data})
    if name.startswith("d_"):
        budget(64)
    for span in M.SPANS:
        _, stats = _good(eng, host, refs, [case], paths, span)
        assert stats["adopted"] == case.members - 1 and stats["candidates"] > stats["adopted"] and stats["dropped"] == stats["streams"] - stats["adopted"], (span, stats)
        if name.startswith("c_"):  # the three inner members decode, their trailers match, and they do not appear
            assert stats["dropped"] >= 3 and stats["wasted_text"] > 0, (span, stats)
        if name.startswith("d_"):
            assert stats["candidates"] >= 2000 and stats["max_in_flight"] <= 64, (span, stats)


# ---- M5 -------------------------------------------------------------------------------------------------------------------------
def test_m5_several_files(eng, host, refs, tmp_path, sizes, budget):
    cases = M.m5_several_files()
    paths = _write(tmp_path, {k: c.data for k, c in cases.items()})
    for span in M.SPANS:
        _, stats = _good(eng, host, refs, list(cases.values()), paths, span)
        assert len(paths) == 10 and stats["max_in_flight"] > 10 and stats["adopted"] == sum(c.members - 1 for c in cases.values()), (span, stats)


# ---- M6 -------------------------------------------------------------------------------------------------------------------------
def test_m6_left_to_zlib_as_before(eng, host, refs, tmp_path, sizes, budget):
    faults, good = M.m6_left_to_zlib(), M.m5_several_files()
    files = {"good0": good["several3"].data}
    files.update({k: c.data for k, c in faults.items()})
    files["good1"] = good["several8"].data
    paths = _write(tmp_path, files)
    for span in M.SPANS:
        serial, serial_stats = host.gzip_index_device(eng, paths, span)
        got, stats = host.gzip_index_device(eng, paths, span, members=True)
        assert (stats["walked"], stats["left_to_zlib"]) == (serial_stats["walked"], serial_stats["left_to_zlib"]) == (2, 5), (stats, serial_stats)
        for name, p, dev, ser in zip(files, paths, got, serial):
            if name.startswith("good"):
                _same(dev, refs(p, span), (name, span))
            else:
                assert ser["left"] and not ser["complete"] and not dev["complete"] and not dev["segments"], (name, span)
                assert (dev["left"], dev["status"]) == (ser["left"], ser["status"]), (name, span, dev["left"], ser["left"])
        reasons = {name: dev["left"] for name, dev in zip(files, got) if not name.startswith("good")}
        assert "no member" in reasons["trailing_bytes"] and "header" in reasons["method_9"] and "trailer" in reasons["crc"] and "trailer" in reasons["isize"] and "end of the file" in reasons["truncated"], reasons
