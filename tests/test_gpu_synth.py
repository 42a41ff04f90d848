"""GPU: the read generator k_synth (csrc/grp_synth.hip) against the host model of include/grpath_synth.h
(tests/synth_model.py, itself held to the header by tests/test_synth_model_cpu.py), bit for bit.

Every case generates into a torch device tensor the test owns, prefilled with a sentinel, with a word_off built by hand
that leaves spare words between the reads and behind the last one.  The whole buffer is then compared with the one the
model predicts: each read's (len + 15) // 16 words equal native.pack_reads of the model's sequence — zero bits behind the
last base included — and every other word still holds the sentinel."""
import ctypes as C
import time

import numpy as np
import pytest

import synth_model as sm
from synth_model import SynthParams
from test_synth_model_cpu import BAD_PARAMS, call_synth

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5A5A5A5
T = 256  # source bases per chunk of k_synth
LENGTHS = [0, 1, 2, 15, 16, 17, 31, 32, 33, 255, 256, 257, 271, 272, 511, 512, 513, 527, 528, 4097]


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _word_off(lens, gaps):
    """read r at word_off[r], gaps[r] spare words behind it; word_off[n] is the end of the last gap"""
    lens = np.asarray(lens, dtype=np.uint64)
    off = np.zeros(lens.size + 1, dtype=np.uint64)
    np.cumsum((lens + np.uint64(15)) // np.uint64(16) + np.asarray(gaps, dtype=np.uint64), out=off[1:])
    return off


def generate(native, p: SynthParams, starts, lens, strands, word_off, stream=None, tail=8, n_reads=None):
    """grp_synth_reads into a sentinel-filled torch tensor; returns the tensor's content as uint32"""
    import torch

    lib = native.load()
    n_words = int(word_off[-1]) + tail
    buf = torch.full((n_words,), SENTINEL - (1 << 32), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    st, ln, sd = np.ascontiguousarray(starts, dtype=np.uint64), np.ascontiguousarray(lens, dtype=np.uint32), np.ascontiguousarray(strands, dtype=np.uint8)
    wo = np.ascontiguousarray(word_off, dtype=np.uint64)
    cp = native.grp_synth_params(p.genome_len, p.genome_seed, p.error_seed, p.p_sub, p.p_ins, p.p_del, p.repeat_frac)
    rc = lib.grp_synth_reads(C.byref(cp), _vp(st), _vp(ln), _vp(sd), _vp(wo), len(lens) if n_reads is None else n_reads, C.c_void_p(buf.data_ptr()), C.c_void_p(stream) if stream else None)
    assert rc == 0, lib.grp_synth_last_error().decode()
    torch.cuda.synchronize()
    return buf.cpu().numpy().view(np.uint32)


def expected_buffer(native, p, starts, lens, strands, word_off, n_words, call_index0=0):
    exp = np.full(n_words, SENTINEL, dtype=np.uint32)
    reads = []
    for r in range(len(lens)):
        rd = sm.read(p, call_index0 + r, int(starts[r]), int(lens[r]), int(strands[r]))
        reads.append(rd)
        words, _, _ = native.pack_reads([sm.ACGT[rd.codes].tobytes()])
        assert words.size == (int(lens[r]) + 15) // 16
        exp[int(word_off[r]): int(word_off[r]) + words.size] = words
    return exp, reads


def check_against_model(native, p, starts, lens, strands, stream=None):
    """runs the kernel and the model on one call's reads; returns the model's reads"""
    gaps = 1 + np.arange(len(lens)) % 3
    word_off = _word_off(lens, gaps)
    got = generate(native, p, starts, lens, strands, word_off, stream=stream)
    exp, reads = expected_buffer(native, p, starts, lens, strands, word_off, got.size)
    if not np.array_equal(got, exp):
        w = int(np.flatnonzero(got != exp)[0])
        r = int(np.searchsorted(word_off, w, side="right")) - 1
        r = min(r, len(lens) - 1)
        pytest.fail(f"word {w} is {got[w]:#010x}, the model says {exp[w]:#010x}: read {r} (len {int(lens[r])}, start {int(starts[r])}, strand {int(strands[r])}) "
                    f"begins at word {int(word_off[r])} and owns {(int(lens[r]) + 15) // 16}; {int((got != exp).sum())} words differ ({p})")
    return reads


def chunk_arithmetic(rd):
    """(codes waiting from the chunks before, codes this chunk emits) for every chunk of 256 source bases that the read's
    edit script spans — the quantities the kernel's scan, flush and carry work on, derived here from the model to assert
    that a case reaches the state it is meant to reach"""
    n_emit = (~rd.deleted).astype(np.int64) + rd.inserted
    out, waiting = [], 0
    for c0 in range(0, rd.consumed, T):
        total = int(n_emit[c0:c0 + T].sum())
        out.append((waiting, total))
        waiting = (waiting + total) % 16
    return out


def _seam_reads(genome_len, long_reads=0, seed=0):
    rng = np.random.default_rng(seed)
    lens = LENGTHS * 2
    strands = [0] * len(LENGTHS) + [1] * len(LENGTHS)
    if long_reads:
        from goldrush_amd import native

        _, real, _, _ = native.synth_read_plan(long_reads, genome_len, seed=seed + 1)  # the real distribution: ~25 kb
        lens = lens + real.tolist()
        strands = strands + [i & 1 for i in range(long_reads)]
    starts = rng.integers(0, genome_len, size=len(lens), dtype=np.uint64)
    return starts, np.array(lens, dtype=np.uint32), np.array(strands, dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------------------------
# lengths at the seams x error settings that change the chunk arithmetic
# ---------------------------------------------------------------------------------------------------------------------
def test_no_errors_every_chunk_holds_256_codes(native):
    p = SynthParams(1_000_003, p_sub=0.0, p_ins=0.0, p_del=0.0)
    reads = check_against_model(native, p, *_seam_reads(p.genome_len, long_reads=4))
    for rd in reads:
        assert all(total == min(T, rd.consumed - i * T) and waiting == 0 for i, (waiting, total) in enumerate(chunk_arithmetic(rd)))
    assert max(len(chunk_arithmetic(rd)) for rd in reads) >= 78


def test_default_errors(native):
    p = SynthParams(1_000_003)
    reads = check_against_model(native, p, *_seam_reads(p.genome_len, long_reads=4))
    assert {w for rd in reads for w, _ in chunk_arithmetic(rd)} == set(range(16))


def test_insertions_nearly_everywhere_fill_the_staging_buffer(native):
    """p_ins = 0.999: 510 .. 512 codes per chunk; with 15 waiting and 512 new the staging buffer is full to its top"""
    p = SynthParams(1_000_003, p_sub=0.0, p_ins=0.999, p_del=0.0)
    reads = check_against_model(native, p, *_seam_reads(p.genome_len, long_reads=4))
    arith = [wt for rd in reads for wt in chunk_arithmetic(rd)]
    assert max(w + t for w, t in arith) == 15 + 2 * T and (15, 2 * T) in arith


def test_insertions_always(native):
    """p_ins = 1: threshold 2^20, every base followed by an insertion — 512 codes per chunk, never a carry"""
    p = SynthParams(1_000_003, p_sub=0.0, p_ins=1.0, p_del=0.0)
    assert sm.thresholds(p)[1] == 1 << 20
    reads = check_against_model(native, p, *_seam_reads(p.genome_len, long_reads=1))
    assert all(rd.inserted[:-1].all() for rd in reads if rd.consumed)


def test_insertions_at_every_other_base_leave_every_carry(native):
    p = SynthParams(1_000_003, p_sub=0.0, p_ins=0.5, p_del=0.0)
    reads = check_against_model(native, p, *_seam_reads(p.genome_len, long_reads=2))
    assert {w for rd in reads for w, _ in chunk_arithmetic(rd)} == set(range(16))


@pytest.mark.parametrize("p_del,long_reads", [(0.9, 2), (0.99, 0)])
def test_deletions_nearly_everywhere(native, p_del, long_reads):
    """p_del = 0.9: ~26 codes per chunk, chunks that flush one word and chunks that flush two; p_del = 0.99: ~2.6 codes per
    chunk, several chunks per flushed word and most chunks flush nothing"""
    p = SynthParams(1_000_003, p_sub=0.03, p_ins=0.01, p_del=p_del)
    reads = check_against_model(native, p, *_seam_reads(p.genome_len, long_reads=long_reads))
    arith = [wt for rd in reads for wt in chunk_arithmetic(rd)[:-1]]
    flushed_words = {(w + t) // 16 for w, t in arith}
    assert {w for w, _ in arith} == set(range(16))
    if p_del == 0.9:
        assert {1, 2} <= flushed_words
    else:
        assert 0 in flushed_words and sum((w + t) < 16 for w, t in arith) > len(arith) // 2
        assert any(t == 0 for _, t in arith)  # a chunk of 256 deleted bases


def test_substitutions_nearly_everywhere(native):
    for p_sub in (0.999, 1.0):
        p = SynthParams(1_000_003, p_sub=p_sub, p_ins=0.01, p_del=0.01)
        reads = check_against_model(native, p, *_seam_reads(p.genome_len, long_reads=1))
        kept = np.concatenate([~rd.deleted for rd in reads])
        assert np.concatenate([rd.substituted for rd in reads])[kept].mean() > 0.99


# ---------------------------------------------------------------------------------------------------------------------
# coordinates
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("genome_len", [1, 2, 7, 255, 257, 1000])
def test_starts_at_the_genome_ends_and_genomes_shorter_than_the_read(native, genome_len):
    G = genome_len
    starts, lens, strands = [], [], []
    for s in (0, G - 1, G, 2 * G + 3):
        for length in (1, 17, 300, 777):
            for strand in (0, 1):
                starts.append(s), lens.append(length), strands.append(strand)
    for p in (SynthParams(G, p_sub=0.0, p_ins=0.0, p_del=0.0), SynthParams(G)):
        check_against_model(native, p, starts, lens, strands)


def test_genome_beyond_2_pow_33_bases(native):
    """coordinates on both sides of 2^32 and at the far end of a genome of 2^33 + 12345 bases: a 32-bit truncation of the
    coordinate, of start % genome_len or of the downward walk shows as another sequence"""
    G = (1 << 33) + 12345
    starts, lens, strands = [], [], []
    for s in ((1 << 32) - 300, (1 << 32) - 1, 1 << 32, (1 << 32) + 5, (1 << 32) + 300, G - 300, G - 1, 0, 5, G + (1 << 32) + 7, 3 * G + 2):
        for strand in (0, 1):
            starts.append(s), lens.append(600), strands.append(strand)
    for p in (SynthParams(G, p_sub=0.0, p_ins=0.0, p_del=0.0), SynthParams(G), SynthParams(G, repeat_frac=0.3)):
        check_against_model(native, p, starts, lens, strands)
    # the case is one a truncation changes: the bases at x and at x mod 2^32 are different sequences
    x = (1 << 32) + np.arange(600, dtype=np.uint64)
    assert not np.array_equal(sm.genome_base(SynthParams(G), x), sm.genome_base(SynthParams(G), x - np.uint64(1 << 32)))


# ---------------------------------------------------------------------------------------------------------------------
# the repeat-rich genome
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("genome_len,repeat_frac", [(6144 * 3000, 0.3), (6144 * 3000, 0.1), (6144 * 3000 + 17, 0.3), (6144 * 3000 + 17, 0.1),
                                                    (6144 * 3000 + 17, 0.67), (6144 * 3000, 1.0), (6144 * 2 + 100, 0.9), (5000, 0.9)])
def test_repeat_rich_genome(native, genome_len, repeat_frac):
    G = genome_len
    p0 = SynthParams(G, genome_seed=1, repeat_frac=repeat_frac)
    n_slots = -(-G // sm.REP_SLOT)
    info = sm.slot_info(p0, np.arange(n_slots))
    rep = np.flatnonzero(info.is_repeat)
    assert rep.size
    if repeat_frac >= 2 / 3:
        assert sm.p_slot(p0) == 1.0 and rep.size == n_slots
    starts = [0, 5, G - 10, G - 1]  # over the genome's end, which with G % 6144 != 0 lies in a short last slot
    # the first and last repeat slots, one of each tier, and a repeat slot that follows a repeat slot
    chosen = {int(rep[0]), int(rep[-1])} | {int(rep[info.tier[rep] == t][0]) for t in range(3) if (info.tier[rep] == t).any()}
    chosen |= {int(s) for s in rep[1:][np.diff(rep) == 1][:2]}
    for s in sorted(chosen):
        base, unit = s * sm.REP_SLOT, int(info.unit[s])
        # inside the unit; across the unit's end upwards and downwards; across the slot's two boundaries
        starts += [base + 100, base + unit - 300, base + unit + 300, base + sm.REP_SLOT - 300, base + 300, base, base + unit - 1, base + unit]
    starts = [s % G for s in starts]
    n = len(starts)
    starts, lens, strands = starts * 2, [700] * (2 * n), [0] * n + [1] * n
    for p in (SynthParams(G, p_sub=0.0, p_ins=0.0, p_del=0.0, repeat_frac=repeat_frac), p0):
        reads = check_against_model(native, p, starts, lens, strands)
    # the reads do lie in repeats: they are not what the unique genome gives
    uniq = SynthParams(G, genome_seed=1, repeat_frac=0.0)
    assert sum(not np.array_equal(rd.codes, sm.read(uniq, r, starts[r], 700, strands[r]).codes) for r, rd in enumerate(reads)) > n


# ---------------------------------------------------------------------------------------------------------------------
# more reads than one launch takes
# ---------------------------------------------------------------------------------------------------------------------
def test_more_than_2_pow_22_reads_in_one_call(native):
    """2^22 + 5 reads of 1 .. 20 bases: the second launch takes its reads, lengths, offsets and error seeds from index 2^22 on"""
    n = (1 << 22) + 5
    G = 1_000_003
    p = SynthParams(G)
    rng = np.random.default_rng(22)
    lens = rng.integers(1, 21, size=n).astype(np.uint32)
    starts = rng.integers(0, G, size=n, dtype=np.uint64)
    strands = (rng.random(n) < 0.5).astype(np.uint8)
    gaps = (np.arange(n) % 3 == 0).astype(np.uint64)
    gaps[-1] = 2
    word_off = _word_off(lens, gaps)
    t0 = time.perf_counter()
    got = generate(native, p, starts, lens, strands, word_off)
    wall = time.perf_counter() - t0
    print(f"{n} reads of 1 .. 20 bases: {wall:.3f} s for the prefill, the call and the download")
    # nothing outside the reads' own words, behind the last read included
    n_words = ((lens + 15) // 16).astype(np.int64)
    owned = np.zeros(got.size, dtype=bool)
    owned[word_off[:-1].astype(np.int64)] = True
    two = n_words == 2
    owned[word_off[:-1].astype(np.int64)[two] + 1] = True
    assert owned.sum() == n_words.sum()
    assert (got[~owned] == SENTINEL).all() and (got[int(word_off[n - 1]) + int(n_words[-1]):] == SENTINEL).all()
    # every read: zero bits behind its last base
    last = got[word_off[:-1].astype(np.int64) + n_words - 1]
    used = (lens - 1) % 16 + 1
    assert ((last.astype(np.uint64) >> (2 * used).astype(np.uint64)) == 0).all()
    # sampled reads against the model
    sample = sorted({0, 1, (1 << 22) - 2, (1 << 22) - 1, 1 << 22, (1 << 22) + 1, n - 2, n - 1} | set(rng.integers(0, n, size=300).tolist()))
    for r in sample:
        rd = sm.read(p, r, int(starts[r]), int(lens[r]), int(strands[r]))
        words, _, _ = native.pack_reads([sm.ACGT[rd.codes].tobytes()])
        a = int(word_off[r])
        assert np.array_equal(got[a:a + words.size], words), r
    # the slice index matters to the case: read 2^22 + j is not what read j's error seed would have given everywhere
    assert any(not np.array_equal(sm.read(p, r, int(starts[r]), int(lens[r]), int(strands[r])).codes,
                                  sm.read(p, r - (1 << 22), int(starts[r]), int(lens[r]), int(strands[r])).codes) for r in range(1 << 22, n))


# ---------------------------------------------------------------------------------------------------------------------
# the index inside the call, the download, streams, empty calls
# ---------------------------------------------------------------------------------------------------------------------
def test_error_pattern_follows_the_index_inside_the_call(native):
    G, lo, hi = 100_000, 5, 9
    kw = dict(mean_len=600, min_len=300, max_len=900)
    plan = native.synth_read_plan(12, G, **kw)
    p = SynthParams(G)
    part = native.synth_reads_range(plan, lo, hi, G)
    sub_plan = (plan[0][lo:hi].copy(), plan[1][lo:hi].copy(), plan[2][lo:hi].copy(), (plan[3][lo:hi + 1] - plan[3][lo]).copy())
    fresh = native.synth_reads_range(sub_plan, 0, hi - lo, G)
    whole = native.synth_reads(12, G, **kw)
    try:
        got_part, got_fresh, got_whole = part.download(0, hi - lo), fresh.download(0, hi - lo), whole.download(0, 12)
    finally:
        part.free(), fresh.free(), whole.free()
    assert got_part == sm.reads_ascii(p, plan, lo, hi)  # call indices 0 .. hi - lo - 1
    assert got_fresh == got_part
    assert got_whole == sm.reads_ascii(p, plan, 0, 12)
    assert all(a != b for a, b in zip(got_part, got_whole[lo:hi]))  # "the passes of one run must use the same batches"


def test_download_of_a_sub_range(native):
    G = 50_000
    kw = dict(mean_len=100, min_len=1, max_len=40, seed=9)
    plan = native.synth_read_plan(40, G, **kw)
    dr = native.synth_reads(40, G, repeat_frac=0.0, **kw)
    try:
        got = dr.download(7, 20)
    finally:
        dr.free()
    assert got == sm.reads_ascii(SynthParams(G), plan, 0, 40)[7:27]


def test_non_default_stream_gives_the_same_words(native):
    import torch

    p = SynthParams(1_000_003)
    starts, lens, strands = _seam_reads(p.genome_len, long_reads=1)
    side = torch.cuda.Stream(device=0)
    assert side.cuda_stream != 0
    check_against_model(native, p, starts, lens, strands, stream=side.cuda_stream)


def test_empty_calls_write_nothing(native):
    p = SynthParams(1000)
    got = generate(native, p, [5], [40], [0], np.array([0, 3], dtype=np.uint64), n_reads=0)
    assert (got == SENTINEL).all()
    n = 600  # more reads than a few, every length 0
    word_off = _word_off(np.zeros(n), np.arange(n) % 2)
    got = generate(native, p, np.arange(n), np.zeros(n), np.arange(n) % 2, word_off)
    assert (got == SENTINEL).all()


# ---------------------------------------------------------------------------------------------------------------------
# refusals (written after the validation: a p_del of 1 or more never returned before it)
# ---------------------------------------------------------------------------------------------------------------------
def test_refused_parameters_leave_the_buffer_untouched(native):
    import torch

    buf = torch.full((64,), SENTINEL - (1 << 32), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    for bad in BAD_PARAMS:
        rc, msg = call_synth(native, bad, buf.data_ptr())
        assert rc == -1 and msg.startswith("grp_synth_reads: "), (bad, rc, msg)
    torch.cuda.synchronize()
    assert (buf.cpu().numpy().view(np.uint32) == SENTINEL).all()
    with pytest.raises(native.GrpError) as ei:
        native.synth_reads(4, 1000, p_del=1.0, mean_len=40, min_len=20, max_len=60)
    assert ei.value.code == -1 and "p_del" in str(ei.value)
    with pytest.raises(native.GrpError):
        native.synth_reads_range(native.synth_read_plan(4, 1000, mean_len=40, min_len=20, max_len=60), 1, 3, 1000, p_sub=float("nan"))
    # the limits themselves are accepted
    rc, msg = call_synth(native, dict(p_sub=1.0, p_ins=1.0, p_del=0.0, repeat_frac=5.0), buf.data_ptr())
    assert rc == 0, msg
