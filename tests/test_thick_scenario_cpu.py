"""CPU: the conditions of the thickened-filter tests (tests/thick_scenario.py), computed with the oracle and the model:
on a thickened filter most of the reads' own probes land in the side tables, and the serial loop still takes every kind of
decision.  The GPU tests assert the same shares on what the engine built before they run their protocols."""
import numpy as np
import pytest

import filter_cases as fc
import filter_model as fm
import thick_scenario as ts
from helpers import default_seeds
from oracle_engine import cached_serial_reference


def _shares(oracle, reads, seeds, m, k):
    oseeds = oracle.Seeds(seeds)
    mf = oracle.MiBF(m, oseeds, ts.TILE, k)
    for s in reads:
        mf.bv_insert_read(s)
    plain_pop = fm.FilterModel(mf.bits(), m, keep_bits=False).pop
    ts.plant_thickened(mf)
    words = mf.bits()
    assert np.array_equal(words, fc.thicken(words, m)) and mf.finalize() > 10 * plain_pop
    mod = fm.FilterModel(words, m, keep_bits=False)
    assert mod.pop == mf.pop
    hashes = np.concatenate([oseeds.tile_hashes(s, ts.TILE, k, t) for s in reads for t in range(len(s) // ts.TILE)])
    s13, s8, n = ts.side_table_shares(mod, hashes)
    # the oracle's rank at a sample of the probes equals the model's
    pos = np.unique(hashes[::97] % np.uint64(m))
    bit, rank = mf.bits_ranks(pos)
    assert np.array_equal(bit, mod.bit(pos)) and np.array_equal(rank, mod.rank(pos))
    mf.close()
    return mod, s13, s8, n


@pytest.mark.parametrize("geometry", list(ts.GEOMETRIES))
def test_thickened_filter_puts_the_probes_into_the_side_tables(oracle, geometry):
    m, W, least13, least8 = ts.GEOMETRIES[geometry]
    reads = ts.make_reads()
    assert len(reads) == 24 and 100_000 < sum(map(len, reads)) < 115_000
    mod, s13, s8, n = _shares(oracle, reads, default_seeds(ts.H), m, ts.K)
    print("%s: W %d occupancy %.4f, %d probed ranks: %.3f at index >= 13, %.3f at index >= 8" % (geometry, mod.W, mod.pop / m, n, s13, s8))
    assert mod.W == W and s13 >= least13 + 0.09 and s8 >= least8 + 0.07  # the margins the GPU tests keep


@pytest.mark.parametrize("form", list(ts.FORMS))
def test_thickened_filter_forms(oracle, form):
    f = ts.FORMS[form]
    mod, s13, s8, n = _shares(oracle, ts.make_reads()[: f["n_reads"]], ts.form_seeds(form), f["m"], f["k"])
    print("%s: W %d occupancy %.4f, %d probed ranks: %.3f at index >= 13, %.3f at index >= 8" % (form, mod.W, mod.pop / f["m"], n, s13, s8))
    assert mod.W == f["W"] and s13 >= f["least13"] + 0.09 and s8 >= f["least8"] + 0.07


@pytest.mark.parametrize("geometry", list(ts.GEOMETRIES))
def test_serial_loop_on_a_thickened_filter_takes_every_decision(oracle, geometry):
    m = ts.GEOMETRIES[geometry][0]
    reads = ts.make_reads()
    exp, ids, counts, pop = cached_serial_reference(("thick", geometry), oracle, m, default_seeds(ts.H), ts.TILE, ts.K, reads, block=ts.BLOCK, plant=ts.plant_thickened)
    kinds = [e[1] for e in exp]
    assert len(exp) == 24 and {2, 3, 4} <= set(kinds) and kinds.count(2) >= 5 and kinds.count(4) >= 3 and ids.any() and counts.max() > 1
    exp, ids, counts, pop = cached_serial_reference(("thick_silver", geometry), oracle, m, default_seeds(ts.H), ts.TILE, ts.K, reads, block=ts.BLOCK, plant=ts.plant_thickened, **ts.SILVER)
    assert [e[7] for e in exp][0] == 1 and {e[7] for e in exp} == {1, 2, 3}  # grp_reset_ids twice, mid-run
