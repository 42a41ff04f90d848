"""GPU: grp_rewind — an engine that has been filled with reads A (and finalized, and given IDs) is rewound and filled with
reads B; everything it then answers equals what a fresh engine filled with B answers: the bit vector, rank samples, the ID
and count arrays behind the same inserts, a query pass.  With and without the occupancy hint (one that fits, one far too
low: the prepared tables are dropped for tables of the measured size), and with the rewind in front of the first finalize.
The batches uploaded before the rewind stay usable behind it.  Integers throughout: no tolerance."""
import time

import numpy as np
import pytest

from helpers import default_seeds, low_error_reads

pytestmark = pytest.mark.gpu

K, H, TILE, M, BLOCK = 22, 3, 1000, 1 << 22, 4
MODES = ["no_hint", "hint_fits", "hint_far_too_low", "rewind_before_finalize"]


@pytest.fixture(scope="module")
def reads():
    _, a = low_error_reads(120_000, 70, 21, mean_len=4500)
    _, b = low_error_reads(90_000, 50, 33, mean_len=5000)
    return a, b


def _insert_ids(eng, batch, reads):
    for i in range(0, len(reads), 7):
        eng.insert_read(batch, i, 0, len(reads[i]) // TILE, BLOCK, 1 + 3 * i, 0)
    eng.insert_tiles(batch, 1, 1, 3, 4000)


def _observe(eng, batch, reads):
    """finalize, the same inserts, then everything the engine can be asked"""
    pop = eng.finalize()
    _insert_ids(eng, batch, reads)
    ids, counts = eng.export_ids()
    pos = (np.arange(20000, dtype=np.uint64) * 7919) % M
    bit, rank = eng.rank(pos)
    tiles, lists, stats = eng.query_tiles(batch, 0, len(reads))
    # (a tile's list lies where its workgroup reserved room in the arena: list_off depends on the order they came in)
    q = [(int(t["top_id"]), int(t["top_count"]), int(t["hits"]), int(t["misses"]), lists[t["list_off"]: t["list_off"] + t["list_n"]].tobytes()) for t in tiles]
    return {"pop": pop, "bits": eng.export_bits().tobytes(), "ids": ids.tobytes(), "counts": counts.tobytes(), "bit": bit.tobytes(), "rank": rank.tobytes(), "query": q, "stats": dict(stats)}


@pytest.fixture(scope="module")
def fresh(native, reads):
    eng = native.Engine(K, H, TILE, M, default_seeds(H))
    b = eng.upload(reads[1])
    eng.bv_insert(b)
    want = _observe(eng, b, reads[1])
    eng.close()
    assert 0.05 < want["pop"] / M < 0.6 and np.frombuffer(want["ids"], dtype=np.uint32).any()
    return want


@pytest.mark.parametrize("mode", MODES)
def test_rewound_engine_equals_a_fresh_one(native, reads, fresh, mode):
    ra, rb = reads
    hint = {"hint_fits": fresh["pop"] / M, "hint_far_too_low": 0.001}.get(mode)
    eng = native.Engine(K, H, TILE, M, default_seeds(H))
    try:
        a, b = eng.upload(ra), eng.upload(rb)  # (b is uploaded in front of the rewind and used behind it)
        if hint:
            eng.set_occupancy_hint(hint)
        eng.bv_insert(a)
        if mode != "rewind_before_finalize":
            pop_a = eng.finalize()
            assert pop_a != fresh["pop"]
            _insert_ids(eng, a, ra)
            assert eng.export_ids()[0].any()
            eng.classify_reads(a, 0, 20)  # (leaves first decisions kept for a batch)
        eng.rewind()
        with pytest.raises(native.GrpError) as e:  # back in the fill state: nothing to query
            eng.query_tiles(b, 0, 1)
        assert e.value.code == native.GRP_ERR_STATE
        if hint:
            eng.set_occupancy_hint(hint)
        eng.bv_insert(b)
        got = _observe(eng, b, rb)
        print(mode, "prepared tables used:", eng.finalize_times()["prepared_tables_used"])  # (a hint is a hint: they are taken where the device had the room)
        if mode in ("no_hint", "hint_far_too_low"):
            assert not eng.finalize_times()["prepared_tables_used"]
        for name in fresh:
            assert got[name] == fresh[name], name
        # a second rewind, straight behind a finalize with IDs, and the same answers once more
        eng.rewind()
        eng.bv_insert(b)
        again = _observe(eng, b, rb)
        for name in fresh:
            assert again[name] == fresh[name], name
    finally:
        eng.close()


def test_rewind_is_refused_while_a_window_is_outstanding(native, reads, fresh):
    rb = reads[1]
    eng = native.Engine(K, H, TILE, M, default_seeds(H))
    try:
        b = eng.upload(rb)
        eng.bv_insert(b)
        eng.finalize()
        eng.stream_begin(b, 0, 8, 0)
        t0 = time.time()
        while not eng.stream_poll(0):  # (the launch ends where it parks; the window stays open until stream_end)
            assert time.time() - t0 < 60, "the launch does not end"
        with pytest.raises(native.GrpError) as e:
            eng.rewind()
        assert e.value.code == native.GRP_ERR_STATE
        eng.stream_end(0)
        eng.classify_begin(b, 0, 8, 1)
        with pytest.raises(native.GrpError) as e:
            eng.rewind()
        assert e.value.code == native.GRP_ERR_STATE
        eng.classify_end(1)
        eng.rewind()
        eng.bv_insert(b)
        got = _observe(eng, b, rb)
        for name in fresh:
            assert got[name] == fresh[name], name
    finally:
        eng.close()
