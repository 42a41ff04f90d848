"""GPU: grp_reads_gather — slices of packed reads cut into a new batch on the device (csrc/grp_gather.inc).  The sources
are one uploaded batch and one grp_reads_wrap_device batch over a device buffer of exactly its words; the slices cover every
shift against every length residue, slices that end at the end of a batch's last read (whose last word is partial), whole
reads, a read taken twice, single bases and a slice of more words than a workgroup has lanes, alternating between the
sources.  The result is read back word for word (grp_reads_download) and must be the packing of the sliced strings; its
tile prefix and the bit vector it fills are those of an uploaded twin.  Integers throughout: no tolerance."""
import numpy as np
import pytest

from helpers import default_seeds, random_reads

pytestmark = pytest.mark.gpu

K, H, TILE, M = 22, 3, 500, 1 << 20
WG_BASES = 256 * 16  # bases one round of a workgroup packs


def _sources():
    lens_a = [1, 2, 3, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 70, 3000, 5120, 8999]
    lens_b = [5, 16, 30, 33, 34, 40, 50, 60, 64, 66, 69, 70, 1, 4001, 6543, 9000, 3003]
    ra = [random_reads(1, n, n, 100 + i)[0] for i, n in enumerate(lens_a)]
    rb = [random_reads(1, n, n, 200 + i)[0] for i, n in enumerate(lens_b)]
    assert len(ra[-1]) % 16 and len(rb[-1]) % 16  # the last read of either batch ends inside a word
    return ra, rb


def _slices(ra, rb):
    src = [ra, rb]
    long_of = [lens.index(max(lens)) for lens in ([len(r) for r in ra], [len(r) for r in rb])]
    last = [len(ra) - 1, len(rb) - 1]
    out = []
    # every first_base & 15 against every n_bases & 15, alternating between the two sources
    for fb in range(16):
        for nb in range(16):
            s = (fb + nb) & 1
            out.append((s, long_of[s], 16 * (3 + nb) + fb, 16 * (2 + fb % 3) + nb))
    # ending exactly at the end of the batch's last read, from every shift
    for s in (0, 1):
        n = len(src[s][last[s]])
        for fb in range(16):
            first = n - 100 - fb
            out.append((s, last[s], first, n - first))
    for s in (0, 1):
        for r in range(len(src[s])):  # whole reads, the single-base one among them
            out.append((s, r, 0, len(src[s][r])))
    out.append((0, 16, 0, len(ra[16])))  # the same read twice
    out.append((0, 16, 0, len(ra[16])))
    for s in (0, 1):  # single bases: first, last, in the middle of a word and at its ends
        n = len(src[s][last[s]])
        for first in (0, 15, 16, 17, 31, n // 2, n - 2, n - 1):
            out.append((s, last[s], first, 1))
    # more words than a workgroup has lanes: several rounds, from an odd shift
    assert len(ra[-1]) - 7 > WG_BASES and len(rb[15]) - 13 > 2 * WG_BASES
    out.append((0, last[0], 7, len(ra[-1]) - 7))
    out.append((1, 15, 13, 2 * WG_BASES + 5))
    return out


@pytest.fixture(scope="module")
def gathered(native):
    import torch

    ra, rb = _sources()
    eng = native.Engine(K, H, TILE, M, default_seeds(H))
    a = eng.upload(ra)
    packed, word_off, lens = native.pack_reads(rb)
    assert packed.size == int(word_off[-1])
    dev = torch.from_numpy(packed.view(np.int32).copy()).to("cuda")  # exactly the reads' words
    torch.cuda.synchronize()
    b = eng.wrap_device(dev.data_ptr(), word_off, lens, keep=dev)
    sl = _slices(ra, rb)
    g = eng.reads_gather([a, b], sl)
    strings = [[ra, rb][s][r][f:f + n] for s, r, f, n in sl]
    yield eng, a, b, g, sl, strings
    eng.close()


def test_words_are_the_packing_of_the_sliced_strings(native, gathered):
    eng, a, b, g, sl, strings = gathered
    want_packed, want_off, want_len = native.pack_reads(strings)
    packed, word_off, lens = eng.reads_download(g)
    assert g.n_reads == len(sl) and np.array_equal(lens, want_len) and np.array_equal(word_off, want_off)
    bad = np.nonzero(packed != want_packed)[0]
    assert bad.size == 0, "first differing word %d (slice %d)" % (bad[0], np.searchsorted(want_off, bad[0], side="right") - 1)
    # (the unused bits of every read's last word are zero: part of the comparison, said once more on its own)
    for i, n in enumerate(want_len):
        if n % 16:
            assert int(packed[int(word_off[i + 1]) - 1]) >> (2 * (int(n) % 16)) == 0, i
    # the sources read back as they went up
    for batch, reads in ((a, _sources()[0]), (b, _sources()[1])):
        p, wo, ln = eng.reads_download(batch)
        wp, wwo, wln = native.pack_reads(reads)
        assert np.array_equal(p, wp) and np.array_equal(wo, wwo) and np.array_equal(ln, wln)


def test_tile_prefix_and_fill_are_the_uploaded_twins(native, gathered):
    eng, a, b, g, sl, strings = gathered
    twin = eng.upload(strings)
    assert np.array_equal(g.tile0, twin.tile0)
    assert int(g.tile0[-1]) == sum(len(s) // TILE for s in strings) > 40
    eng.bv_insert(g)
    eng.finalize()
    got = eng.export_bits()
    other = native.Engine(K, H, TILE, M, default_seeds(H))
    try:
        other.bv_insert(other.upload(strings))
        other.finalize()
        want = other.export_bits()
    finally:
        other.close()
    assert got.any() and np.array_equal(got, want)


def test_every_bad_slice_is_refused(native, gathered):
    eng, a, b, g, sl, strings = gathered
    other = native.Engine(K, H, TILE, M, default_seeds(H))
    try:
        foreign = other.upload(strings[:3])
        n_last = int(a.lens[-1])
        cases = {
            "src >= n_srcs": ([a, b], [(0, 0, 0, 1), (2, 0, 0, 1)]),
            "read >= n_reads": ([a, b], [(1, b.n_reads, 0, 1)]),
            "n_bases 0": ([a, b], [(0, a.n_reads - 1, 5, 0)]),
            "one base behind the read": ([a, b], [(0, a.n_reads - 1, 1, n_last)]),
            "first_base behind the read": ([a, b], [(0, a.n_reads - 1, n_last, 1)]),
            "first_base + n_bases wraps": ([a, b], [(0, a.n_reads - 1, 0xFFFFFFFF, 2)]),
            "a source of another context": ([a, foreign], [(0, 0, 0, 1)]),
        }
        for what, (srcs, slices) in cases.items():
            with pytest.raises(native.GrpError) as e:
                eng.reads_gather(srcs, slices)
            assert e.value.code == native.GRP_ERR_INVALID, what
        # ... and a good call still works behind them; no slice at all is an empty batch
        again = eng.reads_gather([a, b], sl[:5])
        assert np.array_equal(eng.reads_download(again)[0], native.pack_reads(strings[:5])[0])
        empty = eng.reads_gather([a, b], [])
        assert empty.n_reads == 0 and eng.reads_download(empty)[0].size == 0
    finally:
        other.close()
