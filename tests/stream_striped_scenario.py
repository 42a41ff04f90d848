"""Test helper (GPU): ONE rank's launch of a striped resumable window (grp_classify_stream_begin_striped_resumable), driven
the way the ranks of a multi-GPU run drive theirs — but one rank at a time, scripted by the oracle's serial loop.  A rank's
replica of the miBF is independent of the others': what the ranks' record exchange tells a rank (every read in front of an
insert has been decided by its owner; the insert's tiles and IDs) is taken from oracle_engine.serial_reference's commit
tuples instead, so a test needs neither several processes nor several live windows (two resumable windows of two contexts in
one process would wait for each other: a striped window does not leave by itself).

run_owner: fill, finalize, the window, its records, the engine's ID / count arrays and what the in-launch inserts kept.
Every wait has a time limit and looks at stream_poll; whatever fails, the window is aborted and ended before the failure
propagates: no launch is left waiting for its idle limit."""
import time
from collections import namedtuple

import numpy as np

import stream_keep_scenario as sc

Geometry = namedtuple("Geometry", "k h tile block")
KEEP_GEOMETRY = Geometry(sc.K, sc.H, sc.TILE, sc.BLOCK)

NO_TILE_READS = ((30, 1), (100, 120), (329, 499))  # (position in the stream, bases): shorter than a tile, decided by the host


def make_stream():
    """stream_keep_scenario's stream; three reads without a tile in different ranks' stripes of every geometry the tests
    use; one more read of an island nobody has covered at the very end: it inserts behind the last own read of every rank
    but its owner — their launches have decided everything they own and must still be there"""
    from goldrush_amd import synth

    reads = sc.make_stream()
    rng = np.random.default_rng(105)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    for at, length in NO_TILE_READS:
        reads.insert(at, acgt[rng.integers(0, 4, size=length)].tobytes())
    reads.append(synth.random_genome(6_000, 300).tobytes())
    return reads


def owner_of(j, stripe, n_owners):
    return (j // stripe) % n_owners


def insert_args(e, n_bases, g):
    """(tile_start, tile_end, id_offset, IDs allocated behind first_id) of the commit tuple of a read that inserts: what
    the serial loop does with it (goldrush_path.cpp:988-990 whole read, :1048-1049 trimmed)"""
    if e[1] == 2:
        return 0, e[2], 0, n_bases // (g.tile * g.block)
    return e[4], e[5] + 1, 1, (e[5] - e[4]) // g.block


def stream_properties(exp, n_tiles, stripe, n_owners):
    """what the tests need the stream to be, from the oracle's commit tuples alone (no GPU): per owner the inserts it owns,
    the ones it does not, the ones of the latter with an own read with tiles behind them (`late` has a stale record to wait
    for) and the ones behind its last own read with tiles"""
    n = len(exp)
    inserts = [j for j in range(n) if exp[j][1] in (2, 4)]
    out = {"inserts": len(inserts), "owners": []}
    for o in range(n_owners):
        own = [j for j in range(n) if owner_of(j, stripe, n_owners) == o and n_tiles[j]]
        last = own[-1] if own else -1
        mine = [j for j in inserts if owner_of(j, stripe, n_owners) == o]
        others = [j for j in inserts if owner_of(j, stripe, n_owners) != o]
        out["owners"].append({"own": len(mine), "not_own": len(others), "not_own_with_own_read_behind": sum(1 for j in others if j < last),
                              "behind_last_own_read": sum(1 for j in inserts if j > last)})
    return out


def _window(eng, b, reads, exp, g, stripe, n_owners, owner, when, limit):
    assert when in ("eager", "late")
    n = len(reads)
    n_tiles = [int(b.tile0[j + 1] - b.tile0[j]) for j in range(n)]
    no_tile = [j for j in range(n) if n_tiles[j] == 0]
    mine = [n_owners == 1 or owner_of(j, stripe, n_owners) == owner for j in range(n)]
    next_own = [None] * n  # the owner's next read with tiles behind j
    nxt = None
    for j in range(n - 1, -1, -1):
        next_own[j] = nxt
        if mine[j] and n_tiles[j]:
            nxt = j

    def wait_record(j, gen, what):
        t0 = time.time()
        while int(v["pad"][j]) != gen:
            assert time.time() - t0 < limit, "owner %d: %s %d of generation %d never came (it shows generation %d)" % (owner, what, j, gen, int(v["pad"][j]))
            assert not eng.stream_poll(0) or int(v["pad"][j]) == gen, "owner %d: the launch ended without %s %d of generation %d" % (owner, what, j, gen)

    v = eng.stream_begin(b, 0, n, 0, stripe=stripe, n_owners=n_owners, owner=owner, resumable=True)
    ended = False
    try:
        assert eng.stream_resumable(0), "the window does not take inserts (the cooperative launch was refused?)"
        gen, ids_inserted = 1, 0
        own, host, stale = {}, {}, []
        for j in range(n):
            e = exp[j]
            if n_tiles[j] == 0:  # the host's record, with every owner: stream_insert has moved it to the generation of the day
                d = v[j].copy()
                assert int(d["pad"]) == gen, "owner %d: the host's record %d shows generation %d, not %d" % (owner, j, int(d["pad"]), gen)
                host[j] = (j, int(d["kind"]), int(d["num_tiles"]), int(d["num_assigned"]), 0, 0, 0, 1)
                assert host[j] == e, (owner, host[j], e)
            elif mine[j]:  # what the ranks' record exchange waits for before anything behind j is posted
                wait_record(j, gen, "record")
                d = v[j].copy()
                kind = int(d["kind"])
                assert int(d["pad"]) == gen and kind != 0, (owner, j, d)
                rec = (j, kind, int(d["num_tiles"]), int(d["num_assigned"]), int(d["trim_start"]) if kind == 4 else 0, int(d["trim_end"]) if kind == 4 else 0,
                       ids_inserted + 1 if kind in (2, 4) else 0, 1, int(d["hits"]), int(d["misses"]), gen)
                own[j] = rec
                assert rec[:8] == e, "owner %d (%s): record %s, the serial loop says %s" % (owner, when, rec, e)
            if e[1] in (2, 4):  # every rank posts every insert of the window, whoever owns the read
                j2 = next_own[j]
                if when == "late" and not mine[j] and j2 is not None:
                    # there is no own read between j and j2 at which the launch could have parked: it publishes j2 under the
                    # state in front of the insert — and has to replace that record under the new generation
                    wait_record(j2, gen, "stale record")
                    stale.append((j2, gen))
                ts, te, off, more = insert_args(e, len(reads[j]), g)
                assert e[6] == ids_inserted + 1
                ids_inserted = e[6] + more
                new_gen = eng.stream_insert(0, j, ts, te, g.block, e[6], off)
                assert new_gen == gen + 1
                gen = new_gen
                for z in no_tile:
                    assert z <= j or int(v["pad"][z]) == gen, "owner %d: the host's record %d stayed behind insert %d" % (owner, z, j)
                t0 = time.time()
                while True:
                    st = eng.stream_insert_done(0)
                    if st == 1:
                        break
                    assert st == 0, "owner %d: the launch ended without the insert of read %d (its own: %s)" % (owner, j, mine[j])
                    assert time.time() - t0 < limit, "owner %d: the insert of read %d was never applied (its own: %s)" % (owner, j, mine[j])
        for j2, g_old in stale:
            assert own[j2][10] > g_old, (owner, j2, g_old, own[j2])
        eng.stream_abort(0)
        t0 = time.time()
        while not eng.stream_poll(0):
            assert time.time() - t0 < limit, "owner %d: the aborted launch did not end" % owner
        ended = True
        decided = eng.stream_end(0)  # raises where the launch ended without the insert posted last (1 / 2)
    finally:
        if not ended:
            try:
                eng.stream_abort(0)
                eng.stream_end(0)
            except Exception:  # the failure that brought us here is the one to report
                pass
    return {"own": own, "host": host, "stale": stale, "generation": gen, "decided": decided}


def run_owner(native, g, seeds, m, reads, exp, stripe, n_owners, owner, when="eager", limit=20.0):
    """One rank of `n_owners` on a fresh engine -> its own records {read: commit tuple + (hits, misses, generation)}, the
    host's records, the stale records `late` waited for, pop, the final ID / count arrays and grp_debug_stream_stats"""
    eng = native.Engine(g.k, g.h, g.tile, m, seeds)
    try:
        b = eng.upload(reads)
        eng.bv_insert(b)
        pop = eng.finalize()
        t0 = time.time()
        r = _window(eng, b, reads, exp, g, stripe, n_owners, owner, when, limit)
        r["window_s"] = time.time() - t0
        r["pop"] = int(pop)
        r["ids"], r["counts"] = eng.export_ids()
        r["stats"] = eng.stream_stats()
        return r
    finally:
        eng.close()
