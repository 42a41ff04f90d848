"""Shared helpers for the parity tests."""
import numpy as np

SEED22 = "1011011110110111101101"  # bin/goldrush:70


def default_seeds(h=3, preset=SEED22):
    half = len(preset) // 2
    return [preset[:half] + "0" * i + preset[half:] for i in range(h)]


def random_reads(n, lo, hi, seed, genome=None):
    """n random ACGT reads (bytes), lengths uniform in [lo, hi]; if genome is
    given the reads are error-free substrings (so they share k-mers)."""
    rng = np.random.default_rng(seed)
    out = []
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    for _ in range(n):
        L = int(rng.integers(lo, hi + 1))
        if genome is None:
            out.append(acgt[rng.integers(0, 4, size=L)].tobytes())
        else:
            s = int(rng.integers(0, len(genome) - L + 1))
            out.append(bytes(genome[s:s + L]))
    return out


def canon_list(lst):
    """[(id,count)] sorted count desc, id asc."""
    return sorted(((int(a), int(b)) for a, b in lst), key=lambda t: (-t[1], t[0]))


def palindromic_preset(k, weight, seed):
    """A palindromic care pattern of span k whose ends are care positions (the last one at base k - 1), ~weight ones, like
    the reference's designed seeds.  Odd k: the middle is a care position too — make_seed_pattern drops the last
    character (substr(k/2, k/2)), so seed 0 spans k - 1 and still ends in a care position."""
    rng = np.random.default_rng(seed)
    half = k // 2
    left = np.zeros(half, dtype=bool)
    left[0] = True
    left[rng.choice(np.arange(1, half), size=max(weight // 2 - 1, 0), replace=False)] = True
    s = "".join("1" if b else "0" for b in left)
    return s + ("1" if k % 2 else "") + s[::-1]


def compare_queries(eng, omf, batch, reads, first=0, count=None):
    """grp_query_tiles over reads [first, first + count) against the oracle, tile by tile: top ID and count, the count>2
    list, the query / hit / miss counters.  Returns (queries, hits, misses)."""
    if count is None:
        count = len(reads) - first
    tiles, lists, stats = eng.query_tiles(batch, first, count)
    ti = q = hh = ms = 0
    for seq in reads[first:first + count]:
        for top_id, top_count, lst, ctr in omf.query_read(seq):
            t = tiles[ti]
            assert (int(t["top_id"]), int(t["top_count"])) == (top_id, top_count), ti
            got = [(int(a), int(c)) for a, c in lists[t["list_off"]: t["list_off"] + t["list_n"]]]
            assert got == canon_list(lst), ti
            q += ctr[0]
            hh += ctr[1]
            ms += ctr[2]
            ti += 1
    assert ti == len(tiles)
    assert (stats["queries"], stats["hits"], stats["misses"]) == (q, hh, ms)
    return q, hh, ms


def thicken_engine(eng):
    """Between grp_bv_insert and grp_finalize: every 64-bit word of the engine's bit vector that holds a bit becomes all ones
    (the tail masked to m), on the device — filter_cases.thicken is the oracle's side.  Returns the thickened words."""
    import torch

    t = torch.zeros((eng.m + 63) // 64, dtype=torch.int64, device="cuda")  # (whole 64-bit words: at least grp_bv_words 32-bit ones)
    torch.cuda.synchronize()
    assert t.numel() * 8 >= eng.bv_words() * 4
    eng.bv_export_device(t.data_ptr())
    t = torch.where(t != 0, torch.full_like(t, -1), t)
    if eng.m & 63:
        t[-1] &= (1 << (eng.m & 63)) - 1
    torch.cuda.synchronize()
    eng.bv_import_device(t.data_ptr())
    return t.cpu().numpy().view(np.uint64)


# ---- streams of reads with few errors, and ONE resumable window over them ----
LOW_ERRORS = dict(sub=0.004, ins=0.0005, dele=0.0005)


def low_error_reads(genome_len, n, seed, mean_len=5000):
    from goldrush_amd import synth

    g = synth.random_genome(genome_len, seed)
    return g, [r[1] for r in synth.make_reads(g, n, mean_len=mean_len, min_len=3500, seed=seed + 1, max_len=9000, **LOW_ERRORS)]


def keep_stream():
    """tests/stream_keep_scenario.py's stream with few errors"""
    from stream_keep_scenario import make_stream

    return make_stream(**LOW_ERRORS)


def stream_resumable(eng, b, reads, tile, block, u=5, limit=120.0):
    """ONE resumable window over all reads; every insert record answered with stream_insert (the IDs the serial loop
    allocates) -> the commit tuples of oracle_engine.serial_reference"""
    import time

    n = len(reads)
    v = eng.stream_begin(b, 0, n, 0, unassigned_min=u, resumable=True)
    gen, ids_inserted = 1, 0
    got = []
    for j in range(n):
        t0 = time.time()
        while int(v["pad"][j]) != gen:
            assert time.time() - t0 < limit, "record %d of generation %d never came" % (j, gen)
            assert not eng.stream_poll(0) or int(v["pad"][j]) == gen, "the launch ended without record %d" % j
        d = v[j].copy()
        kind = int(d["kind"])
        assert kind != 0
        first_id = 0
        if kind in (2, 4):
            ids_inserted += 1
            first_id = ids_inserted
            if kind == 2:
                ts, te, off = 0, int(d["num_tiles"]), 0
                ids_inserted += len(reads[j]) // (tile * block)
            else:
                ts, te, off = int(d["trim_start"]), int(d["trim_end"]) + 1, 1
                ids_inserted += (int(d["trim_end"]) - int(d["trim_start"])) // block
            gen = eng.stream_insert(0, j, ts, te, block, first_id, off)
        got.append((j, kind, int(d["num_tiles"]), int(d["num_assigned"]), int(d["trim_start"]) if kind == 4 else 0, int(d["trim_end"]) if kind == 4 else 0, first_id, 1))
    t0 = time.time()
    while not eng.stream_poll(0):
        assert time.time() - t0 < 60
    eng.stream_end(0)
    return got


# ---- the btllib pin (tools/make_btllib_kat.py): a fixture anyone with a real btllib install can drop in ----
import hashlib  # noqa: E402
import json  # noqa: E402
import os  # noqa: E402

BTLLIB_KAT_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "btllib_seed_kat.json")


def load_btllib_kat(path=BTLLIB_KAT_FILE):
    """the known answers of a real btllib, or None (absent in this image: the tests skip)"""
    if not os.path.exists(path):
        return None
    with open(path) as f:
        return json.load(f)


def tiny_reads_by_id():
    fq = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiny.fq")
    lines = open(fq, "rb").read().split(b"\n")
    return {lines[i][1:].decode(): lines[i + 1] for i in range(0, len(lines) - 3, 4)}


def check_against_btllib_kat(kat, hashes_of):
    """`hashes_of(seeds, seq) -> [per seed: uint64 values of every position]` (the oracle's, or the device's) against the
    file's records: count, sha256 of the stream, first / last / strided values.  Returns the number of streams checked."""
    stride = int(kat["stride"])
    reads = tiny_reads_by_id()
    checked = 0
    for name, fam in kat["families"].items():
        seeds = fam["seeds"]
        for rid, recs in fam["reads"].items():
            mine = hashes_of(seeds, reads[rid])
            assert len(mine) == len(seeds) == len(recs)
            for s, (vals, rec) in enumerate(zip(mine, recs)):
                vals = [int(v) for v in vals]
                where = (name, rid, "seed %d" % s)
                assert len(vals) == rec["n"], where
                assert vals[:8] == rec["first"], where
                assert vals[-4:] == rec["last"], where
                assert vals[::stride] == rec["every_%d" % stride], where
                assert hashlib.sha256(b"".join(v.to_bytes(8, "little") for v in vals)).hexdigest() == rec["sha256"], where
                checked += 1
    return checked
