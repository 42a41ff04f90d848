"""Developer tool: raw kernel throughput (fill / query) on synthetic reads.
Not the judged benchmark (see bench.py); used to iterate on kernels."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from goldrush_amd import native  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=200000)
    ap.add_argument("--genome", type=float, default=100e6)
    ap.add_argument("--h", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--populate", type=int, default=4000, help="reads inserted as IDs before querying")
    ap.add_argument("--qbatches", type=int, default=8)
    ap.add_argument("--k", type=int, default=22, help="span of the base seed (k + h - 1 up to 256)")
    ap.add_argument("--w", type=int, default=16, help="weight of the seed (with --k other than 22 and no --preset: a preset is drawn)")
    ap.add_argument("--preset", default=None, help="seed preset of span k (default: the pipeline's 22-base preset at k = 22)")
    a = ap.parse_args()
    G = int(a.genome)
    k, w, tile = a.k, a.w, 1000
    preset = a.preset
    if preset is None:
        if k == 22 and w == 16:
            preset = "1011011110110111101101"
        else:  # care positions at both ends, the rest drawn
            last = k - 1 - k % 2  # (odd k: the last position is dropped from the seeds, below)
            care = np.zeros(k, dtype=bool)
            care[0] = care[last] = True
            care[np.random.default_rng(k).choice(np.arange(1, last), size=w - 2, replace=False)] = True
            preset = "".join("1" if c else "0" for c in care)
    assert len(preset) == k and preset.count("1") == w
    # make_seed_pattern's family (spaced_seeds.cpp:27-66): halves of k/2 positions, so at odd k the preset's last
    # position is dropped and seed 0 spans k - 1 (a tile of tile + 1 frames)
    seeds = [preset[:k // 2] + "0" * i + preset[k // 2: 2 * (k // 2)] for i in range(a.h)]
    U = int(np.float32(min(4 ** w, 2 * G)) * np.float32(0.5) * np.float32(a.h))
    n = int(-float(U) / np.log(1.0 - 0.1))
    m = n + (64 - n % 64)
    t = time.time()
    dr = native.synth_reads(a.reads, G)
    print(f"synth {a.reads} reads, {int(dr.lens.sum())/1e9:.2f} Gbases: {time.time()-t:.2f}s", flush=True)
    eng = native.Engine(k, a.h, tile, m, seeds)
    rb = eng.wrap_device(dr.d_ptr, dr.word_off, dr.lens)
    t = time.time()
    eng.bv_insert(rb)
    eng.sync()
    t_fill = time.time() - t
    ks_fill = eng.kernel_stats()["fill"]
    t = time.time()
    pop = eng.finalize()
    t_fin = time.time() - t
    print(f"m={m} pop={pop} occ={pop/m:.3f} fill {t_fill:.3f}s finalize {t_fin:.3f}s", flush=True)
    t = time.time()
    idn = 0
    for r in range(min(a.populate, a.reads)):
        nt = int(dr.lens[r]) // tile
        idn += 1
        for bs in range(0, nt, 10):
            eng.insert_tiles(rb, r, bs, min(bs + 10, nt), idn + bs // 10)
        idn += nt // 10
    eng.sync()
    print(f"populate {a.populate} reads: {time.time()-t:.3f}s", flush=True)
    eng.reset_kernel_stats()
    t = time.time()
    nq = 0
    hits = 0
    for b in range(a.qbatches):
        first = (a.populate + b * a.batch) % max(a.reads - a.batch, 1)
        tiles, lists, st = eng.query_tiles(rb, first, a.batch)
        nq += a.batch
        hits += st["hits"]
    wall = time.time() - t
    ks = eng.kernel_stats()
    q = ks["query"]
    gbps = q["units"] * 128 / (q["ms"] * 1e-3) / 1e9
    out = {"reads_per_s_wall": nq / wall, "reads_per_s_kernel": nq / (q["ms"] * 1e-3), "query_ms_per_launch": q["ms"] / q["launches"],
           "probes_per_launch": q["units"] / q["launches"], "GBps_128B_per_probe": gbps, "frac_of_8TBps": gbps / 8000,
           "hit_frac": hits / max(q["units"], 1), "fill_s": t_fill, "fill_Gprobes_per_s": ks_fill["units"] / max(t_fill, 1e-9) / 1e9 if ks_fill["units"] else None,
           "fill_Gprobes_per_s_kernel": ks_fill["units"] / (ks_fill["ms"] * 1e-3) / 1e9 if ks_fill["units"] and ks_fill["ms"] else None,
           "query_Gprobes_per_s_kernel": q["units"] / (q["ms"] * 1e-3) / 1e9, "k": k, "w": w, "h": a.h, "span": k + a.h - 1}
    ks_all = eng.kernel_stats()
    print(json.dumps(out))
    print(json.dumps(ks_all))


if __name__ == "__main__":
    main()
