"""The read generator of include/grpath_synth.h, restated on the host in numpy (test infrastructure).

The specification is the model text of the header: a counter-based genome, a read as the substring from its start
(coordinates wrap), reverse-complemented on the other strand, passed base by base through deletion, substitution and
insertion, cut after exactly `len` bases.  csrc/grp_synth.hip supplies only the constants: the mixer, the multipliers,
the bit fields of the per-base word, the 2^20 thresholds and the repeat-slot arithmetic.  Nothing of the kernel's
structure is here — no chunks of 256 source bases, no scan, no carry, no flush of 16-base words: a read is one
cumulative sum over its source bases.  tests/test_synth_model_cpu.py holds this model to the header's statements from
outside; tests/test_gpu_synth.py holds k_synth to this model bit for bit.

Arithmetic: uint64 arrays that wrap; float32 where the kernel's host code uses float (thresholds, p_slot), double for
tier_slots.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

U = np.uint64
REP_SLOT = 6144  # bases per slot of a repeat-rich genome
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)

K_GENOME = 0xD1342543DE82EF95  # unique genome: base i
K_READ = 0xA24BAED4963EE407  # per-read error seed: index of the read inside the call; also the copy's substitutions
K_BASE = 0x9FB21C651E98DF25  # per-base error word: index of the source base inside the read
K_SLOT, X_SLOT = 0xC2B2AE3D27D4EB4F, 0x5EEDC0DE5EEDC0DE
K_FAM, X_FAM = 0x9E3779B97F4A7C15, 0xFA111E5FA111E5
K_CONS = 0xD6E8FEB86659FD93
X_COPY = 0xD17E26E7CE
TIER_COPIES = (10000, 1000, 30)


@dataclass(frozen=True)
class SynthParams:
    genome_len: int
    genome_seed: int = 1
    error_seed: int = 3
    p_sub: float = 0.03
    p_ins: float = 0.01
    p_del: float = 0.01
    repeat_frac: float = 0.0


def _arr(x):
    return np.atleast_1d(np.asarray(x, dtype=np.uint64))


def mix64(x):
    """splitmix64's finaliser over a uint64 array"""
    with np.errstate(over="ignore"):
        x = _arr(x) + U(0x9E3779B97F4A7C15)
        x = (x ^ (x >> U(30))) * U(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> U(27))) * U(0x94D049BB133111EB)
        return x ^ (x >> U(31))


def _mul(a, k):
    with np.errstate(over="ignore"):
        return _arr(a) * U(k)


def thresholds(p: SynthParams):
    """(th_sub, th_ins, th_del): a 20-bit draw below the threshold triggers the event; (uint32)(float p * 2^20)"""
    return tuple(int(np.float32(v) * np.float32(1048576.0)) for v in (p.p_sub, p.p_ins, p.p_del))


def effective_probabilities(p: SynthParams):
    return tuple(t / 1048576.0 for t in thresholds(p))


def unique_base(genome_seed: int, coords):
    return (mix64(U(genome_seed) ^ _mul(coords, K_GENOME)) >> U(62)).astype(np.uint8)


def p_slot(p: SynthParams) -> float:
    """probability that a slot is a repeat copy: 1.5 f in float32, clamped to 1 (mean unit 4096 of 6144 bases)"""
    ps = np.float32(p.repeat_frac) * np.float32(1.5)
    return float(ps) if ps < np.float32(1.0) else 1.0


@dataclass
class Slots:
    is_repeat: np.ndarray  # bool
    tier: np.ndarray  # 0, 1, 2: ~10 000, ~1 000, ~30 copies per family (meaningful where is_repeat)
    family: np.ndarray  # uint64 id, unique over the tiers
    unit: np.ndarray  # length of the family's unit, 2048 .. 6144
    div_percent: np.ndarray  # 1 .. 5: share of the unit's positions a copy substitutes
    fh: np.ndarray  # the family's hash (consensus seed)


def slot_info(p: SynthParams, slots) -> Slots:
    slots = _arr(slots)
    h = mix64(U(p.genome_seed) ^ U(X_SLOT) ^ _mul(slots, K_SLOT))
    is_rep = (h & U(0xFFFFFF)).astype(np.float64) < p_slot(p) * 16777216.0
    tier = (h >> U(24)) % U(3)
    tier_slots = int(float(p.genome_len // REP_SLOT) * p_slot(p) / 3.0)
    n_fam = np.array([max(tier_slots // c, 1) for c in TIER_COPIES], dtype=np.uint64)[tier.astype(np.int64)]
    fam = (tier << U(48)) | ((h >> U(28)) % n_fam)
    fh = mix64(U(p.genome_seed) ^ U(X_FAM) ^ _mul(fam, K_FAM))
    unit = U(2048) + fh % U(4097)
    div = U(1) + (fh >> U(13)) % U(5)
    return Slots(is_rep, tier.astype(np.int64), fam, unit.astype(np.int64), div.astype(np.int64), fh)


def genome_base(p: SynthParams, coords):
    """2-bit codes of the genome at `coords` (each < genome_len): the unique genome, or with repeat_frac > 0 the
    repeat-rich one — inside the unit of a repeat slot the family's consensus with this copy's substitutions"""
    coords = _arr(coords)
    out = unique_base(p.genome_seed, coords)
    if not np.float32(p.repeat_frac) > 0:
        return out
    slot = coords // U(REP_SLOT)
    off = coords - slot * U(REP_SLOT)
    uniq_slots, inv = np.unique(slot, return_inverse=True)
    si = slot_info(p, uniq_slots)
    inside = si.is_repeat[inv] & (off < si.unit[inv].astype(np.uint64))
    if not inside.any():
        return out
    c, o = coords[inside], off[inside]
    fh, div = si.fh[inv][inside], si.div_percent[inv][inside].astype(np.uint64)
    b = mix64(fh ^ _mul(o, K_CONS)) >> U(62)
    m = mix64(U(p.genome_seed) ^ U(X_COPY) ^ _mul(c, K_READ))
    changed = (m % U(100)) < div
    b = np.where(changed, (b + U(1) + (m >> U(32)) % U(3)) & U(3), b)
    out[inside] = b.astype(np.uint8)
    return out


@dataclass
class Read:
    codes: np.ndarray  # uint8[len]: what the generator emits
    source: np.ndarray  # uint8[consumed]: the error-free source bases in read orientation
    deleted: np.ndarray  # bool[consumed]
    substituted: np.ndarray  # bool[consumed]
    sub_code: np.ndarray  # uint8[consumed]: the base emitted in place of source[i] where substituted[i]
    inserted: np.ndarray  # bool[consumed]: one base follows source base i (false where the read's end cut it off)
    ins_code: np.ndarray  # uint8[consumed]
    consumed: int  # source bases walked


def source_coords(p: SynthParams, start: int, idx, strand: int):
    """genome coordinate of source base idx of a read: upwards from start % genome_len, downwards on the other strand,
    both wrapping"""
    G = U(p.genome_len)
    s0 = U(int(start) % p.genome_len)
    k = _arr(idx) % G
    with np.errstate(over="ignore"):
        if strand:
            return np.where(k <= s0, s0 - k, s0 + (G - k))
        room = G - s0  # 1 .. G
        return np.where(k < room, s0 + k, k - room)


def _events(p: SynthParams, call_index: int, start: int, strand: int, i0: int, n: int):
    th_sub, th_ins, th_del = thresholds(p)
    idx = np.arange(i0, i0 + n, dtype=np.uint64)
    rseed = mix64(U(p.error_seed) ^ _mul(U(call_index), K_READ))[0]
    e = mix64(rseed ^ _mul(idx, K_BASE))
    F = U(0xFFFFF)
    deleted = (e & F) < U(th_del)
    sub = ~deleted & (((e >> U(20)) & F) < U(th_sub))
    ins = ~deleted & (((e >> U(40)) & F) < U(th_ins))
    src = genome_base(p, source_coords(p, start, idx, strand))
    if strand:
        src = (3 - src).astype(np.uint8)
    sub_code = ((src.astype(np.uint64) + U(1) + (e >> U(60)) % U(3)) & U(3)).astype(np.uint8)
    ins_code = (e >> U(62)).astype(np.uint8)
    return src, deleted, sub, sub_code, ins, ins_code


def read(p: SynthParams, call_index: int, start: int, length: int, strand: int) -> Read:
    """Read `call_index` of a call: `length` bases and the edit script that made them."""
    length = int(length)
    parts, have, i0, block = [], 0, 0, max(1024, length + length // 8)
    while have < length:
        ev = _events(p, call_index, start, strand, i0, block)
        parts.append(ev)
        have += int((~ev[1]).sum() + ev[4].sum())
        i0 += block
        block *= 2
    if not parts:
        z8, zb = np.zeros(0, np.uint8), np.zeros(0, bool)
        return Read(z8, z8, zb, zb, z8, zb, z8, 0)
    src, deleted, sub, sub_code, ins, ins_code = (np.concatenate(x) for x in zip(*parts))
    n_emit = (~deleted).astype(np.int64) + ins
    cum = np.cumsum(n_emit)
    consumed = int(np.searchsorted(cum, length, side="left")) + 1
    src, deleted, sub, sub_code, ins, ins_code, n_emit, cum = (a[:consumed] for a in (src, deleted, sub, sub_code, ins, ins_code, n_emit, cum))
    ins = ins.copy()
    if cum[-1] > length:  # the last source base wanted two places and one was left
        ins[-1] = False
    codes = np.zeros(int(cum[-1]), dtype=np.uint8)
    at = cum - n_emit
    kept = ~deleted
    codes[at[kept]] = np.where(sub, sub_code, src)[kept]
    codes[at[ins] + 1] = ins_code[ins]
    return Read(codes[:length], src, deleted, sub, sub_code, ins, ins_code, consumed)


def reads_ascii(p: SynthParams, plan, lo: int, hi: int):
    """What DeviceReads.download returns for native.synth_reads_range(plan, lo, hi, ...): the per-read error seed is the
    index inside the call, 0 .. hi - lo - 1"""
    start, lens, strand, _ = plan
    return [ACGT[read(p, j, int(start[lo + j]), int(lens[lo + j]), int(strand[lo + j])).codes].tobytes() for j in range(hi - lo)]
