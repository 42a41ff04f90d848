"""GPU: every buffer group of ONE engine grows twice while it holds live state — the engine's paths are run with windows
of 2, then 40, then 300 reads — and every result of the 300-read calls equals what a FRESH engine returns that is given the
same filter state and only the 300-read calls (its buffers are allocated once, at their final size).  Integers throughout:
no tolerance.  A normal sequence of calls; it ends with both engines closed (batches freed before and behind the engine) and a
third engine that finalizes and classifies the 2-read window."""
import time

import numpy as np
import pytest

from helpers import default_seeds, low_error_reads

from goldrush_amd import native as native_mod

pytestmark = pytest.mark.gpu

K, H, TILE, M, BLOCK = 22, 3, 1000, 1 << 20, 10
N_READS, WINDOWS = 320, (2, 40, 300)
# A filter of 2^20 bits is half full with these reads: a tile counts for an ID from 200 of its 3000 probes on (chance hits
# give every ID some tens), and reads of 3 tiles can be new ones.  Five reads are in the ID array: chance hits put every ID
# on every tile's list, and a resumable window's list arena has room for 8 entries per tile.  Reads 0 and 1 and 223 of the
# first 300 are new ones then (the oracle's count).
DP = dict(threshold=200, unassigned_min=2)
BATCH_INSERTS = {2: 1, 40: 3, 300: 10}  # inserts of a window's batch: its record tables grow from each window to the next
FIELDS = ["kind", "num_tiles", "num_assigned", "trim_start", "trim_end", "hits", "misses"]


def _reads():
    # reads of 3 - 6 tiles over a genome they cover about ten times; in an order in which the first two are new reads that do not overlap
    _, reads = low_error_reads(150_000, N_READS, 11, mean_len=4500)
    reads = [r[: min(len(r), 6 * TILE + 999)] for r in reads]
    return reads[7:] + reads[:7]


def _engine(reads):
    eng = native_mod.Engine(K, H, TILE, M, default_seeds(H))
    b = eng.upload(reads)
    eng.bv_insert(b)
    eng.pop = eng.finalize()
    return eng, b


def _plan(d, reads, ids_inserted):
    """the inserts the decisions ask for with the IDs the serial loop would allocate, and the floors (tests/test_gpu_batch.py)"""
    ins, floors, shared = [], [], False
    for j, r in enumerate(d):
        floors.append((ids_inserted + 1) | (0x80000000 if shared else 0))
        kind = int(r["kind"])
        if kind == 2:
            ins.append((j, 0, int(r["num_tiles"]), ids_inserted + 1, 0))
            ids_inserted += 1 + len(reads[j]) // (TILE * BLOCK)
            shared = False
        elif kind == 4:
            ts, te = int(r["trim_start"]), int(r["trim_end"])
            ins.append((j, ts, te + 1, ids_inserted + 1, 1))
            ids_inserted += 1 + (te - ts) // BLOCK
            shared = (te - ts + 1) % BLOCK == 0
    return ins, floors


def _wait_record(eng, v, j, gen, slot=0):
    t0 = time.time()
    while int(v["pad"][j]) != gen:
        assert time.time() - t0 < 60, "record %d of generation %d never came" % (j, gen)
        assert not eng.stream_poll(slot) or int(v["pad"][j]) == gen, "the launch ended without record %d" % j


def _wait_end(eng, slot=0):
    t0 = time.time()
    while not eng.stream_poll(slot):
        assert time.time() - t0 < 60, "the launch does not end"


def _records(v, idx):
    return [tuple(int(v[f][j]) for f in FIELDS) for j in idx]


def _stream_plain(eng, b, n):
    """a window that ends where it parks: the records up to the first insert / hand-back one"""
    v = eng.stream_begin(b, 0, n, 0, **DP)
    _wait_end(eng)
    stop = next((j for j in range(n) if int(v["pad"][j]) != 1 or int(v["kind"][j]) in (0, 2, 4)), n - 1)
    assert np.all(v["pad"][: stop + 1] == 1)
    out = _records(v, range(stop + 1))
    eng.stream_end(0)
    return out


def _stream_resumable(eng, b, reads, n, next_id):
    """a resumable window in slot 1: ONE stream_insert at its first insert record, then the records of the next generation
    up to the next record it parks at"""
    v = eng.stream_begin(b, 0, n, 1, resumable=True, **DP)
    resumable = eng.stream_resumable(1)
    out, gen, inserted, j = [], 1, None, 0
    while j < n:
        _wait_record(eng, v, j, gen, slot=1)
        out.append(_records(v, [j])[0])
        kind = int(v["kind"][j])
        j += 1
        if kind not in (0, 2, 4):
            continue
        if kind == 0 or inserted is not None:
            break
        d = v[j - 1].copy()
        if kind == 2:
            inserted = (j - 1, 0, int(d["num_tiles"]), BLOCK, next_id, 0)
        else:
            inserted = (j - 1, int(d["trim_start"]), int(d["trim_end"]) + 1, BLOCK, next_id, 1)
        if not resumable:  # (the device could not keep the window resident: it ends where it parks, the host applies the insert)
            break
        gen = eng.stream_insert(1, *inserted)
        t0 = time.time()
        while eng.stream_insert_done(1) == 0:
            assert time.time() - t0 < 60, "the insert is never applied"
    if not eng.stream_poll(1):
        eng.stream_abort(1)
    _wait_end(eng, slot=1)
    eng.stream_end(1)
    if inserted is not None and not resumable:
        eng.insert_read(b, *inserted)
    return out, inserted, resumable


def _fastq(eng, reads, n):
    text = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, reads[i], b"I" * len(reads[i])) for i in range(n))
    fq, rec, used, stopped = eng.fastq_parse(text)
    assert len(rec) == n and used == len(text) and not stopped
    pb = eng.fastq_pack(fq, np.arange(n), rec["seq_len"])
    d = eng.classify_reads(pb, **DP)
    eng.fastq_free(fq)
    pb.free()
    return rec.tobytes(), d.tobytes()


def _run(eng, b, reads, n):
    """every path that grows buffers, over the first n reads; -> results by name"""
    res = {}
    res["ids_before"] = [a.tobytes() for a in eng.export_ids()]
    res["classify"] = eng.classify_reads(b, 0, n, **DP).tobytes()
    half = n // 2
    eng.classify_begin(b, 0, half, 0, **DP)
    eng.classify_begin(b, half, n - half, 1, **DP)
    res["pipelined"] = eng.classify_end(0).tobytes() + eng.classify_end(1).tobytes()
    tiles, lists, stats = eng.query_tiles(b, 0, n)
    # (a tile's list lies where its workgroup reserved room in the arena: list_off depends on the order they came in)
    res["query"] = ([(int(t["top_id"]), int(t["top_count"]), int(t["hits"]), int(t["misses"]), lists[t["list_off"]: t["list_off"] + t["list_n"]].tobytes()) for t in tiles], dict(stats))
    res["stream"] = _stream_plain(eng, b, n)
    next_id = int(max(1, np.frombuffer(res["ids_before"][0], dtype=np.uint32).max() + 1))
    # a resumable window with one in-launch insert (it takes the window's first new read; the batch takes the next ones)
    res["stream_resumable"] = out, inserted, resumable = _stream_resumable(eng, b, reads, n, next_id)
    print("window of %d reads: resumable %s, in-launch insert %s, %d records" % (n, resumable, inserted, len(out)))
    assert resumable and inserted is not None, (n, resumable, inserted)
    # a batch: insert -> classify -> verify -> undo (the small windows) / end (the last one)
    d0 = eng.classify_reads(b, 0, n, **DP)
    ins, floors = _plan(d0, reads, next_id + 100)
    ins = ins[: BATCH_INSERTS[n]]
    extra = min(max(1, n // 2), N_READS - n)
    assert len(ins) == BATCH_INSERTS[n], (n, len(ins))
    if ins:
        eng.batch_insert_reads(b, ins, BLOCK, 0)
        d1 = eng.batch_classify(b, 0, n, floors, **DP)
        dv = eng.batch_verify(b, 0, n, extra, floors + [0x7FFFFFFF] * extra, **DP)
        assert len(d1) == n and len(dv) == n + extra
        res["batch"] = (d1.tobytes(), dv.tobytes())
        if n == WINDOWS[-1]:
            eng.batch_end()
        else:
            eng.batch_undo(0, floors[0] & 0x7FFFFFFF)
    res["overlap"] = eng.window_overlap(b, 0, n).tobytes()
    eng.ntcard_begin()
    eng.ntcard_add(b, 0, n)
    res["ntcard"] = eng.ntcard_finish().tobytes()
    ids, counts = eng.export_ids()
    res["ids_after"] = (ids.tobytes(), counts.tobytes())
    eng.import_ids(0, ids, counts)
    res["ids_reimported"] = [a.tobytes() for a in eng.export_ids()]
    pos = (np.arange(n * 10, dtype=np.uint64) * 7919) % M
    res["rank"] = [a.tobytes() for a in eng.rank(pos)]
    res["bits"] = eng.export_bits().tobytes()
    res["fastq"] = _fastq(eng, reads, n)
    return res


def test_buffers_regrow_with_live_state():
    reads = _reads()
    assert all(3 * TILE <= len(r) < 7 * TILE for r in reads)
    eng, b = _engine(reads)
    fresh, fb = _engine(reads)
    assert eng.pop == fresh.pop
    empty = eng.classify_reads(b, 0, WINDOWS[0], **DP).tobytes()  # (against the empty ID array)
    for i in range(60, N_READS, 60):  # some reads are in the filter's ID array already
        eng.insert_read(b, i, 0, len(reads[i]) // TILE, BLOCK, 1 + i, 0)
    for n in WINDOWS[:-1]:
        _run(eng, b, reads, n)
    # the fresh engine is given the same state ...
    ids, counts = eng.export_ids()
    fresh.import_ids(0, ids, counts)
    # ... and only the 300-read calls
    want = _run(fresh, fb, reads, WINDOWS[-1])
    got = _run(eng, b, reads, WINDOWS[-1])
    assert got.keys() == want.keys()
    for name in want:
        assert got[name] == want[name], name
    assert got["ids_after"] == tuple(got["ids_reimported"])
    # batches freed before their engine, and behind it
    b.free()
    eng.close()
    fresh.close()
    fb.free()
    third, tb = _engine(reads)
    assert third.pop == eng.pop
    assert third.classify_reads(tb, 0, WINDOWS[0], **DP).tobytes() == empty
    third.close()
