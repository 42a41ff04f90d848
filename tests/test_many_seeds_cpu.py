"""CPU: the host side of 9 to 16 spaced seeds — the seed design (make_seed_pattern, spaced_seeds.cpp:58-66) against the
oracle and, where the reference parts were built (oracle/_ref), against the reference's own compiled code; the filter
sizing, which grows linearly with h."""
import ctypes as C
import os

import pytest

from helpers import SEED22

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libref_parts.so")


@pytest.fixture(scope="module")
def host(native):
    from goldrush_amd import host as h

    h.load()
    return h


def _ref_seeds():
    if not os.path.exists(REF_LIB):
        return None
    lib = C.CDLL(REF_LIB)
    lib.ref_make_seed_pattern.restype = C.c_int
    lib.ref_make_seed_pattern.argtypes = [C.c_char_p, C.c_uint, C.c_uint, C.c_uint, C.c_char_p, C.c_size_t]

    def ref(preset, k, w, h):
        buf = C.create_string_buffer(512 * h)
        n = lib.ref_make_seed_pattern(preset.encode(), k, w, h, buf, 512)
        return [buf.raw[i * 512:(i + 1) * 512].split(b"\0", 1)[0].decode() for i in range(n)]

    return ref


CASES = [(SEED22, 22, 16, h) for h in range(9, 17)] + [("", 22, 16, h) for h in range(9, 17)] + [("", 24, 12, 16), ("", 40, 20, 12), ("", 80, 30, 16),
                                                                                              ("1101" * 8, 32, 24, 16)]


def test_many_seed_patterns(oracle, host):
    ref = _ref_seeds()
    for preset, k, w, h in CASES:
        got = host.make_seed_pattern(preset, k, w, h)
        assert len(got) == h and [len(s) for s in got] == [k + i for i in range(h)], (preset, k, w, h)
        assert got == oracle.make_seed_pattern(preset, k, w, h), (preset, k, w, h)
        if ref is not None:
            assert got == ref(preset, k, w, h), (preset, k, w, h)
        # left || 0^i || right: the family the query kernels' shared halves are written for (i up to 15)
        cut = k // 2
        assert all(s == got[0][:cut] + "0" * i + got[0][cut:] for i, s in enumerate(got)), (preset, k, w, h)


def test_filter_size_grows_with_h(oracle, host):
    hl, ol = host.load(), oracle.load()
    for h in range(1, 17):
        u = hl.gr_hash_universe(16, 3_000_000_000, h)
        assert u == ol.orc_hash_universe(16, 3_000_000_000, h)
        assert hl.gr_calc_optimal_size(u, 1, 0.1) == ol.orc_calc_optimal_size(u, 1, 0.1)
    assert hl.gr_hash_universe(16, 3_000_000_000, 16) > 5 * hl.gr_hash_universe(16, 3_000_000_000, 3)

