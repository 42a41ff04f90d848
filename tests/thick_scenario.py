"""Test infrastructure: the reads, filter sizes and conditions of the thickened-filter tests (tests/test_gpu_thick_filter.py).

A filter is THICKENED (filter_cases.thicken) between the fill and finalize: every 64-bit word that holds a bit becomes all
ones.  The reads' own probes then land on the far ends of their buckets' rank ranges — IDs in the overflow table (in-bucket
index >= 13), count words in the far table (index >= 8) — where the hash fill puts under 1 % and about 5 % of them.

24 reads of 2 600 - 5 750 bases with few errors off a genome of 38 000 bases (coverage ~2.7: whole inserts, trimmed inserts
and reads assigned outright), tile 500, block 4.  Two geometries, by the filter size:

    m = 100 000 007   occupancy 0.077   W = 64: buckets are the full words themselves
    m =  40 000 003   occupancy 0.18    W = 33: full words straddle the buckets

The shares of the reads' probed ranks in the side tables, computed with the oracle and the model on the CPU
(tests/test_thick_scenario_cpu.py), and the least every GPU test asserts before it runs its protocol:

    geometry      index >= 13 (overflow ID)    index >= 8 (far count word)
    w64           0.796, asserted >= 0.70      0.876, asserted >= 0.80
    w33           0.504, asserted >= 0.40      0.680, asserted >= 0.60
    many_seeds    0.404, asserted >= 0.30      0.613, asserted >= 0.50     (h = 16, the first 8 reads, W = 25)
    long_span     0.798, asserted >= 0.70      0.876, asserted >= 0.80     (k = 128, h = 2, W = 64)
"""
import numpy as np

import filter_cases as fc
import filter_model as fm
from helpers import SEED22, default_seeds, palindromic_preset

K, H, TILE, BLOCK = 22, 3, 500, 4
GEOMETRIES = {
    # name: (m, W, least share at index >= 13, least share at index >= 8)
    "w64": (100_000_007, 64, 0.70, 0.80),
    "w33": (40_000_003, 33, 0.40, 0.60),
}
# the other query / insert forms: (k, h, reads used, m, W, least shares) — conditions computed as above, same margins
FORMS = {
    "many_seeds": dict(k=22, h=16, n_reads=8, m=100_000_007, W=25, least13=0.30, least8=0.50),
    "long_span": dict(k=128, h=2, n_reads=24, m=100_000_007, W=64, least13=0.70, least8=0.80),
}
SILVER = dict(silver=True, target_bases=20_000, max_paths=3)  # the path rolls over (grp_reset_ids) twice; the third path is full at read 17


def make_reads():
    from goldrush_amd import synth

    g = synth.random_genome(38_000, 41)
    return [r[1] for r in synth.make_reads(g, 24, mean_len=4200, min_len=2500, seed=42, max_len=6000, sub=0.004, ins=0.0005, dele=0.0005)]


def form_seeds(name):
    f = FORMS[name]
    if name == "many_seeds":
        return default_seeds(f["h"], SEED22)
    return default_seeds(f["h"], palindromic_preset(f["k"], 30, 7 + f["k"]))


def plant_thickened(mf):
    """serial_reference's plant=: the oracle's filter thickened between its fill and finalize"""
    mf.plant_bits(fc.thicken(mf.bits(), mf.m))


def side_table_shares(model, hashes):
    """of the probes (hash values, any order) that hit a set bit: the share whose rank lies at in-bucket index >= 13 and
    >= 8, and the number of such probes"""
    pos = np.asarray(hashes, dtype=np.uint64) % np.uint64(model.m)
    hit = model.bit(pos).astype(bool)
    idx = model.in_bucket_index_at(pos[hit])
    return float((idx >= fm.BUCKET_IDS).mean()), float((idx >= fm.NEAR_CW).mean()), int(hit.sum())
