"""CPU: the host side of odd -k — the seed design (make_seed_pattern, spaced_seeds.cpp:27-66: halves of k/2 positions, so
seed i spans k - 1 + i) against the oracle and, where the reference parts were built (oracle/_ref), against the
reference's own compiled code; the --ntcard split of a record into ACGT runs with the seeds' own spans."""
import ctypes as C
import os

import numpy as np
import pytest

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


CASES = [("", 23, 16, 3), ("", 21, 16, 1), ("", 33, 16, 3), ("", 65, 16, 3), ("", 23, 16, 9), ("", 23, 16, 16), ("", 31, 20, 5),
         ("10110111101101111011011", 23, 16, 3), ("1" + "01" * 64, 129, 65, 2), ("11011" * 51, 255, 200, 2)]


def test_odd_k_seed_patterns(oracle, host):
    ref = _ref_seeds()
    for preset, k, w, h in CASES:
        got = host.make_seed_pattern(preset, k, w, h)
        assert [len(s) for s in got] == [k - 1 + i for i in range(h)], (preset, k, w, h)
        assert got == oracle.make_seed_pattern(preset, k, w, h), (preset, k, w, h)
        if ref is not None:
            assert got == ref(preset, k, w, h), (preset, k, w, h)
        if preset:
            assert got[0] == preset[: k - 1]  # the last character of an odd preset is dropped
        # left || 0^i || right with the cut at span0 / 2 = k / 2: the family the query kernels' shared halves serve
        cut = (k - 1) // 2
        assert cut == k // 2 and all(s == got[0][:cut] + "0" * i + got[0][cut:] for i, s in enumerate(got)), (preset, k, w, h)


def _windows(seq, span):
    """the oracle's per-seed window count (orc_ntcard.c: a running count of clean characters)"""
    n = clean = 0
    for c in seq:
        clean = clean + 1 if c in b"ACGTacgt" else 0
        n += clean >= span
    return n


@pytest.mark.parametrize("k,h", [(23, 3), (23, 16), (129, 2)])
def test_ntcard_split_with_odd_k_spans(host, k, h):
    """runs of at least span0 = k - 1 bases; with each run's windows of seed s (span k - 1 + s) and the stale repeats on its
    last run, every seed is counted F = the windows of seed 0 times, as orc_ntcard_add_read counts it"""
    rng = np.random.default_rng(k + h)
    span0 = k - 1
    spans = [span0 + s for s in range(h)]
    for trial in range(40):
        n = int(rng.integers(span0 - 2, 6 * k))
        seq = bytearray(b"ACGT"[i] for i in rng.integers(0, 4, size=n))
        for p in rng.integers(0, max(n, 1), size=int(rng.integers(0, 5))):
            seq[p] = ord("N")
        if trial == 0:  # runs of exactly span0 and span0 + 1 bases
            seq = bytearray(b"A" * span0 + b"N" + b"C" * (span0 + 1) + b"N" + b"G" * (span0 - 1))
        seq = bytes(seq)
        runs, extra = host.ntcard_split(seq, span0, h)
        assert all(ln >= span0 for _, ln in runs)
        assert sum(1 for o, ln in runs) == sum(1 for r in seq.replace(b"N", b" ").split() if len(r) >= span0)
        V = [_windows(seq, sp) for sp in spans]
        F = V[0]
        for s in range(h):
            got = sum(max(ln - spans[s] + 1, 0) for _, ln in runs)
            assert got == V[s], (trial, s)
            assert (int(extra[:, s].sum()) if len(runs) else 0) == (F - V[s] if V[s] else 0), (trial, s)
