"""CPU: the host model of the read generator (tests/synth_model.py) against what include/grpath_synth.h states, each
statement checked from outside the model's own code — so that tests/test_gpu_synth.py compares k_synth with a reference
and not with a copy of itself.  Statistical bounds are 4.5 binomial standard deviations of the trial count at hand
(two-sided tail 7e-6 per check); the measured values stand next to them in comments."""
import ctypes as C
import math

import numpy as np
import pytest

import synth_model as sm
from synth_model import SynthParams

SIGMAS = 4.5


def _sigma_distance(hits, trials, p):
    return (hits - trials * p) / math.sqrt(trials * p * (1.0 - p))


def _revcomp(codes):
    return (3 - np.asarray(codes, dtype=np.uint8))[::-1]


def _apply_script(rd):
    """the edit script walked base by base, in plain Python"""
    out = []
    for i in range(rd.consumed):
        if rd.deleted[i]:
            assert not rd.substituted[i] and not rd.inserted[i]
            continue
        out.append(int(rd.sub_code[i]) if rd.substituted[i] else int(rd.source[i]))
        if rd.inserted[i]:
            out.append(int(rd.ins_code[i]))
    return np.array(out, dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------------------------
# no errors: a read is the genome's substring, or the reverse complement of the stretch below its start
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("genome_len,repeat_frac", [(1, 0.0), (2, 0.0), (7, 0.0), (1000, 0.0), (6144 * 4 + 5, 0.9)])
def test_error_free_read_is_the_genome_substring(genome_len, repeat_frac):
    G = genome_len
    p = SynthParams(G, genome_seed=11, p_sub=0.0, p_ins=0.0, p_del=0.0, repeat_frac=repeat_frac)
    genome = sm.genome_base(p, np.arange(G, dtype=np.uint64))
    assert genome.shape == (G,) and genome.max() <= 3
    for start in (0, G - 1, G, 2 * G + 3, G // 2):
        for length in (0, 1, 2, G, G + 1, 3 * G + 5, 700):
            fwd = sm.read(p, 5, start, length, 0)
            assert np.array_equal(fwd.codes, genome[(start % G + np.arange(length)) % G]), (start, length)
            # the stretch of `length` bases that ends at start, read upwards, then reverse-complemented as a whole
            stretch = genome[(start % G - (length - 1) + np.arange(length)) % G]
            rev = sm.read(p, 5, start, length, 1)
            assert np.array_equal(rev.codes, _revcomp(stretch)), (start, length)
            for rd in (fwd, rev):
                assert rd.consumed == length and not rd.deleted.any() and not rd.substituted.any() and not rd.inserted.any()


def test_error_free_read_does_not_depend_on_the_call_index_and_an_erroneous_one_does():
    clean = SynthParams(5000, p_sub=0.0, p_ins=0.0, p_del=0.0)
    assert np.array_equal(sm.read(clean, 0, 17, 900, 1).codes, sm.read(clean, 9, 17, 900, 1).codes)
    noisy = SynthParams(5000)
    assert not np.array_equal(sm.read(noisy, 0, 17, 900, 1).codes, sm.read(noisy, 9, 17, 900, 1).codes)
    assert np.array_equal(sm.read(noisy, 9, 17, 900, 1).codes, sm.read(noisy, 9, 17, 900, 1).codes)


# ---------------------------------------------------------------------------------------------------------------------
# the edit script
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p_sub,p_ins,p_del", [(0.03, 0.01, 0.01), (0.0, 0.5, 0.0), (0.0, 0.999, 0.0), (0.0, 0.0, 0.9), (1.0, 0.0, 0.0), (0.3, 0.3, 0.3)])
def test_edit_script_applied_to_the_source_gives_the_read(p_sub, p_ins, p_del):
    p = SynthParams(3001, genome_seed=4, error_seed=8, p_sub=p_sub, p_ins=p_ins, p_del=p_del)
    clean = SynthParams(3001, genome_seed=4, p_sub=0.0, p_ins=0.0, p_del=0.0)
    for call_index, (length, strand) in enumerate([(0, 0), (1, 1), (2, 0), (16, 1), (255, 0), (256, 1), (1000, 0), (4097, 1)]):
        rd = sm.read(p, call_index, 2990, length, strand)
        assert rd.codes.shape == (length,)
        for a in (rd.source, rd.deleted, rd.substituted, rd.sub_code, rd.inserted, rd.ins_code):
            assert a.shape == (rd.consumed,)
        # the source is the error-free read of as many bases as were consumed
        assert np.array_equal(rd.source, sm.read(clean, call_index, 2990, rd.consumed, strand).codes)
        assert np.array_equal(_apply_script(rd), rd.codes)
        if length:
            assert not rd.deleted[-1]  # the walk stops at the base that completes the read
        assert (rd.sub_code[rd.substituted] != rd.source[rd.substituted]).all()


def _rate_case():
    """genome 100 000, seeds 1 / 3, the default 0.03 / 0.01 / 0.01, call indices 0 .. 63, lengths 1 .. 6 000 (square-root
    spaced: about 256 k source bases)"""
    p = SynthParams(100000, genome_seed=1, error_seed=3, p_sub=0.03, p_ins=0.01, p_del=0.01)
    lens = [1 + round(5999 * math.sqrt(j / 63.0)) for j in range(64)]
    assert lens[0] == 1 and lens[-1] == 6000
    rng = np.random.default_rng(7)
    return p, [sm.read(p, j, int(rng.integers(0, 100000)), lens[j], j & 1) for j in range(64)]


def test_realised_error_rates_match_the_thresholds():
    p, reads = _rate_case()
    e_sub, e_ins, e_del = sm.effective_probabilities(p)
    assert abs(e_sub - 0.03) < 2 ** -20 and abs(e_ins - 0.01) < 2 ** -20 and abs(e_del - 0.01) < 2 ** -20
    n_src = sum(r.consumed for r in reads)
    assert n_src >= 200000
    n_del = sum(int(r.deleted.sum()) for r in reads)
    kept = n_src - n_del
    n_sub = sum(int(r.substituted.sum()) for r in reads)
    # an insertion behind a read's last source base may be cut off by the read's end: that base is no trial
    ins_trials = sum(int((~r.deleted[:-1]).sum()) for r in reads)
    n_ins = sum(int(r.inserted[:-1].sum()) for r in reads)
    d_del, d_sub, d_ins = _sigma_distance(n_del, n_src, e_del), _sigma_distance(n_sub, kept, e_sub), _sigma_distance(n_ins, ins_trials, e_ins)
    print(f"source bases {n_src}: deletions {d_del:+.2f} sigma, substitutions {d_sub:+.2f} sigma, insertions {d_ins:+.2f} sigma")
    # measured: 254 922 source bases; deletions +0.10, substitutions -0.03, insertions -0.52 sigma
    assert abs(d_del) <= SIGMAS and abs(d_sub) <= SIGMAS and abs(d_ins) <= SIGMAS


def test_substituted_and_inserted_bases():
    _, reads = _rate_case()
    sub_off = np.concatenate([(r.sub_code[r.substituted].astype(np.int64) - r.source[r.substituted]) % 4 for r in reads])
    assert sub_off.size > 1000 and set(sub_off.tolist()) == {1, 2, 3}  # never the source base, every other one
    ins = np.concatenate([r.ins_code[r.inserted] for r in reads])
    assert ins.size > 1000 and set(ins.tolist()) == {0, 1, 2, 3}
    for code in range(4):  # "one random inserted base": uniform
        assert abs(_sigma_distance(int((ins == code).sum()), ins.size, 0.25)) <= SIGMAS


def test_base_composition_of_the_unique_genome():
    n = 1 << 20
    for seed, first in ((1, 0), (99, (1 << 32) - n // 2), (5, (1 << 40) + 12345)):
        codes = sm.genome_base(SynthParams(1 << 62, genome_seed=seed), first + np.arange(n, dtype=np.uint64))
        d = [_sigma_distance(int((codes == c).sum()), n, 0.25) for c in range(4)]
        print(f"seed {seed} from {first}: A C G T at " + " ".join(f"{x:+.2f}" for x in d) + " sigma")
        assert max(abs(x) for x in d) <= SIGMAS
    # neighbours are independent: every dinucleotide near 1/16
    di = codes[:-1].astype(np.int64) * 4 + codes[1:]
    assert max(abs(_sigma_distance(int((di == c).sum()), di.size, 1 / 16)) for c in range(16)) <= SIGMAS


# ---------------------------------------------------------------------------------------------------------------------
# the repeat-rich genome, looked at slot by slot
# ---------------------------------------------------------------------------------------------------------------------
_SLOTS = {}


def _slot_survey(genome_len, repeat_frac):
    """every slot of the genome: its bases, where they differ from the unique sequence, and what the model says of it"""
    key = (genome_len, repeat_frac)
    if key not in _SLOTS:
        p = SynthParams(genome_len, genome_seed=1, repeat_frac=repeat_frac)
        n_slots = genome_len // sm.REP_SLOT
        bases = np.empty((n_slots, sm.REP_SLOT), dtype=np.uint8)
        differs = np.empty((n_slots, sm.REP_SLOT), dtype=bool)
        for s0 in range(0, n_slots, 250):
            s1 = min(s0 + 250, n_slots)
            coords = np.arange(s0 * sm.REP_SLOT, s1 * sm.REP_SLOT, dtype=np.uint64)
            bases[s0:s1] = sm.genome_base(p, coords).reshape(s1 - s0, sm.REP_SLOT)
            differs[s0:s1] = bases[s0:s1] != sm.unique_base(p.genome_seed, coords).reshape(s1 - s0, sm.REP_SLOT)
        _SLOTS[key] = (p, bases, differs, sm.slot_info(p, np.arange(n_slots)))
    return _SLOTS[key]


REPEAT_CASES = [(6144 * 3000, 0.3), (6144 * 3000 + 17, 0.1)]


@pytest.mark.parametrize("genome_len,repeat_frac", REPEAT_CASES)
def test_repeat_slots_share_and_unit_lengths(genome_len, repeat_frac):
    p, bases, differs, info = _slot_survey(genome_len, repeat_frac)
    n_slots = bases.shape[0]
    # seen from the sequence alone: a repeat slot differs from the unique genome at about 3/4 of its first 2048 bases,
    # any other slot nowhere
    head = differs[:, :2048].mean(axis=1)
    is_rep = head > 0.5
    assert (head[is_rep] > 0.75 - SIGMAS * math.sqrt(0.75 * 0.25 / 2048)).all()
    assert not differs[~is_rep].any()
    assert np.array_equal(is_rep, info.is_repeat)
    # share of repeat slots: binomial in the slot count at 1.5 f
    d = _sigma_distance(int(is_rep.sum()), n_slots, 1.5 * repeat_frac)
    # unit: up to the last base that differs from the unique sequence (a unit's last bases match it by chance with
    # probability 1/4 each: 4^-16 that sixteen do)
    seen_unit = sm.REP_SLOT - np.argmax(differs[is_rep, ::-1], axis=1)
    unit = info.unit[is_rep]
    share = seen_unit.sum() / genome_len
    print(f"G={genome_len} f={repeat_frac}: repeat slots {is_rep.mean():.4f} ({d:+.2f} sigma of {1.5 * repeat_frac:.3f}), units {seen_unit.min()} .. {seen_unit.max()}, "
          f"mean {seen_unit.mean():.0f}, repeat share of the genome {share:.4f}")
    # measured: f = 0.3: 0.4593 of the slots (+1.03 sigma), units 2108 .. 5779, 0.2994 of the genome;
    #           f = 0.1: 0.1513 (+0.20 sigma), units 2109 .. 5536, 0.0927
    assert abs(d) <= SIGMAS
    assert unit.min() >= 2048 and unit.max() <= 6144  # "2 to 6 kb long"
    assert (seen_unit <= unit).all() and (seen_unit >= unit - 16).all()  # beyond its unit a repeat slot is unique sequence
    # the units' mean is the 4096 that makes 1.5 f of the slots f of the genome: uniform on 2048 .. 6144 over the families
    fam_units = {int(f): int(u) for f, u in zip(info.family[is_rep], unit)}
    n_fam = len(fam_units)
    assert abs(np.mean(list(fam_units.values())) - 4096) <= SIGMAS * (4096 / math.sqrt(12)) / math.sqrt(n_fam)


@pytest.mark.parametrize("genome_len,repeat_frac", REPEAT_CASES)
def test_repeat_copies_diverge_as_stated(genome_len, repeat_frac):
    p, bases, differs, info = _slot_survey(genome_len, repeat_frac)
    rep = np.flatnonzero(info.is_repeat)
    families = {}
    for s in rep:
        families.setdefault(int(info.family[s]), []).append(int(s))
    # copies of one family: one unit length, and each copy 1 .. 5 % away from the family's consensus (majority over the
    # copies, families of nine or more), so two copies at most ~10 % apart and nowhere near 3/4
    per_copy, pairwise = [], []
    for fam, slots in families.items():
        unit = int(info.unit[slots[0]])
        assert all(int(info.unit[s]) == unit for s in slots)
        sd_pair = math.sqrt(0.0975 * 0.9025 / unit)
        for a, b in zip(slots[:-1], slots[1:]):
            frac = float((bases[a, :unit] != bases[b, :unit]).mean())
            pairwise.append(frac)
            assert 0.0 < frac <= 0.0975 + SIGMAS * sd_pair, (fam, a, b, frac)  # 1 - 0.95^2 = 0.0975
        if len(slots) >= 9:
            counts = np.stack([(bases[slots, :unit] == c).sum(axis=0) for c in range(4)])
            consensus = counts.argmax(axis=0)
            stated = int(info.div_percent[slots[0]]) / 100.0
            assert 0.01 <= stated <= 0.05
            for s in slots[:40]:
                frac = float((bases[s, :unit] != consensus).mean())
                per_copy.append(frac)
                assert abs(frac - stated) <= SIGMAS * math.sqrt(stated * (1 - stated) / unit), (fam, s, frac, stated)
    assert len(per_copy) >= 100 and len(pairwise) >= 100
    # copies of different families are unrelated: 3/4 of the positions differ
    firsts = [slots[0] for slots in families.values()]
    unrelated = [float((bases[a, :2048] != bases[b, :2048]).mean()) for a, b in zip(firsts[:-1], firsts[1:])]
    assert len(unrelated) >= 5
    print(f"G={genome_len} f={repeat_frac}: per copy {min(per_copy):.4f} .. {max(per_copy):.4f}, pairwise within a family {min(pairwise):.4f} .. {max(pairwise):.4f}, "
          f"across families {min(unrelated):.4f} .. {max(unrelated):.4f}")
    # measured: f = 0.3: per copy 0.0058 .. 0.0569, pairwise 0.0137 .. 0.1084, across families 0.7275 .. 0.7676
    #           f = 0.1: per copy 0.0052 .. 0.0576, pairwise 0.0137 .. 0.1078, across families 0.7251 .. 0.7666
    assert all(abs(f - 0.75) <= SIGMAS * math.sqrt(0.75 * 0.25 / 2048) for f in unrelated)


@pytest.mark.parametrize("genome_len,repeat_frac", REPEAT_CASES)
def test_repeat_tiers_and_copies_per_family(genome_len, repeat_frac):
    p, bases, differs, info = _slot_survey(genome_len, repeat_frac)
    rep = info.is_repeat
    n_rep = int(rep.sum())
    # "a third of the repeat slots each"
    for tier in range(3):
        assert abs(_sigma_distance(int((info.tier[rep] == tier).sum()), n_rep, 1 / 3)) <= SIGMAS
    # families of distinct tiers never share an id
    assert len({(int(t), int(f)) for t, f in zip(info.tier[rep], info.family[rep])}) == len(set(info.family[rep].tolist()))
    # the ~30-copy tier: tier_slots / 30 families, each copy choosing its family uniformly — copies per family are
    # Poisson-like around 30, and the median of n such counts has a standard deviation near 1.2533 sqrt(30 / n)
    fam30, copies = np.unique(info.family[rep & (info.tier == 2)], return_counts=True)
    tier_slots = int((genome_len // sm.REP_SLOT) * sm.p_slot(p) / 3.0)
    assert len(fam30) == tier_slots // 30
    median = float(np.median(copies))
    bound = SIGMAS * 1.2533 * math.sqrt(30.0 / len(fam30)) + 1.0  # + 1: a Poisson median lies up to 1 off its mean
    print(f"G={genome_len} f={repeat_frac}: {len(fam30)} families in the ~30 tier, median copies {median} (bound 30 +- {bound:.1f})")
    # measured: f = 0.3: 15 families, median 29 (30 +- 9.0); f = 0.1: 5 families, median 29 (30 +- 14.8)
    assert abs(median - 30.0) <= bound
    # the genome is too small for 10 000 copies: that tier is one family
    assert len(set(info.family[rep & (info.tier == 0)].tolist())) == 1


def test_p_slot_clamps_to_one():
    p = SynthParams(6144 * 50, repeat_frac=0.7)
    assert sm.p_slot(p) == 1.0 and sm.slot_info(p, np.arange(50)).is_repeat.all()
    assert sm.p_slot(SynthParams(6144 * 50, repeat_frac=0.3)) == float(np.float32(0.3) * np.float32(1.5))


# ---------------------------------------------------------------------------------------------------------------------
# the plan, and the refusals that need no device
# ---------------------------------------------------------------------------------------------------------------------
def test_synth_read_plan():
    from goldrush_amd import native

    for kw in (dict(), dict(mean_len=600, min_len=300, max_len=900), dict(mean_len=10, min_len=1, max_len=20, seed=5)):
        start, lens, strand, word_off = native.synth_read_plan(5000, 12345, **kw)
        assert start.dtype == np.uint64 and lens.dtype == np.uint32 and strand.dtype == np.uint8 and word_off.dtype == np.uint64
        assert lens.min() >= kw.get("min_len", 20000)
        if "max_len" in kw:
            assert lens.max() <= kw["max_len"]
        assert word_off[0] == 0 and np.array_equal(word_off[1:], np.cumsum((lens.astype(np.uint64) + 15) // 16))
        assert start.max() < 12345 and set(strand.tolist()) == {0, 1}
        again = native.synth_read_plan(5000, 12345, **kw)
        assert all(np.array_equal(a, b) for a, b in zip((start, lens, strand, word_off), again))
    other = native.synth_read_plan(5000, 12345, seed=3)
    assert not np.array_equal(other[0], native.synth_read_plan(5000, 12345, seed=2)[0])


def test_reads_ascii_uses_the_index_inside_the_call():
    from goldrush_amd import native

    plan = native.synth_read_plan(6, 5000, mean_len=300, min_len=100, max_len=500)
    p = SynthParams(5000)
    whole = sm.reads_ascii(p, plan, 0, 6)
    part = sm.reads_ascii(p, plan, 2, 5)
    assert [len(s) for s in part] == plan[1][2:5].tolist() and set(b"".join(whole)) <= set(b"ACGT")
    assert part[0] == sm.ACGT[sm.read(p, 0, int(plan[0][2]), int(plan[1][2]), int(plan[2][2])).codes].tobytes()
    assert all(a != b for a, b in zip(part, whole[2:5]))


BAD_PARAMS = [
    dict(p_sub=float("nan")), dict(p_ins=float("nan")), dict(p_del=float("nan")),
    dict(p_sub=float("inf")), dict(p_ins=float("inf")), dict(p_del=float("inf")), dict(p_del=float("-inf")),
    dict(p_sub=-0.01), dict(p_ins=-0.01), dict(p_del=-0.01),
    dict(p_sub=1.5), dict(p_ins=1.0000002), dict(p_del=1.0), dict(p_del=2.0), dict(p_del=0.99999999), dict(p_del=1e30),
    dict(repeat_frac=float("nan")), dict(repeat_frac=float("inf")), dict(repeat_frac=-0.1),
]


def call_synth(native, params_kw, d_out_ptr, n=1):
    """grp_synth_reads on one read of 40 bases with the given parameter overrides; (rc, message)"""
    lib = native.load()
    kw = dict(genome_len=1000, genome_seed=1, error_seed=3, p_sub=0.03, p_ins=0.01, p_del=0.01, repeat_frac=0.0)
    kw.update(params_kw)
    p = native.grp_synth_params(kw["genome_len"], kw["genome_seed"], kw["error_seed"], kw["p_sub"], kw["p_ins"], kw["p_del"], kw["repeat_frac"])
    start, lens, strand = np.array([5], dtype=np.uint64), np.array([40], dtype=np.uint32), np.array([0], dtype=np.uint8)
    word_off = np.array([0, 3], dtype=np.uint64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = lib.grp_synth_reads(C.byref(p), vp(start), vp(lens), vp(strand), vp(word_off), n, C.c_void_p(d_out_ptr), None)
    return rc, lib.grp_synth_last_error().decode()


@pytest.mark.parametrize("bad", BAD_PARAMS, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_parameters_outside_the_accepted_ranges_are_refused_before_any_device_call(native, bad):
    """-1 with a message, with or without a device: the validation comes before the first HIP call (a HIP failure is
    -3), so the output — here host memory no device call could write anyway — stays as it was."""
    out = np.full(8, 0xA5A5A5A5, dtype=np.uint32)
    rc, msg = call_synth(native, bad, out.ctypes.data)
    assert rc == -1 and msg.startswith("grp_synth_reads: ") and len(msg) > 25, (rc, msg)
    assert (out == 0xA5A5A5A5).all()
    rc, _ = call_synth(native, bad, out.ctypes.data, n=0)  # refused even where there is nothing to generate
    assert rc == -1
