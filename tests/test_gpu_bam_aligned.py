"""GPU: grp_bam_parse_ex (csrc/grp_ingest.inc: k_bam_records with the accepted flags, the backward chain of k_fq_phred, the
reversed form of k_bam_pack) against grp_fastq_parse of the ALIGNED twin on the same engine — the record table, the ACGT
flag, bit-identical Phred sums, the packed bases — then each bit of the mask, chunk cuts around skipped records and a body
uploaded ahead of its parse.  The aligned twin is written down from the SAM specification and samtools' documented
behaviour (tests/bam_aligned_cases.py); it is not pinned against samtools' output."""
import struct

import numpy as np
import pytest

import bam_aligned_cases as BA
import bam_cases as BC
from helpers import default_seeds
from test_gpu_bam import LENGTHS as UNALIGNED_LENGTHS

pytestmark = pytest.mark.gpu

K, H = 22, 4
TILE = K + H - 1
# the lengths of test_gpu_bam.py, and those around the 64-byte steps of the backward chain (one, two, three and four lines)
LENGTHS = UNALIGNED_LENGTHS + [191, 192, 193, 255, 256, 257]
REVERSED = 2  # GRP_FQ_REVERSED


def _records(seed=5, n=96):
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    recs = []
    for i in range(n):
        L = LENGTHS[i % len(LENGTHS)]
        bases = bytearray(acgt[rng.integers(0, 4, size=L)].tobytes())
        quals = bytes(rng.integers(0, 61, size=L).astype(np.uint8))
        if i % 9 == 1 and L:
            quals = quals[:L // 3] + b"\x5d" * (L - L // 3)
        # (the name's length moves the bases and the qualities through every residue of 16)
        name = bytes(rng.integers(ord("a"), ord("z") + 1, size=1 + (i * 3 + i // 32) % 37).astype(np.uint8))
        if i % 6 == 2 and len(name) > 4:
            name = name[:3] + b" " + name[4:]
        rev = 0x10 if (i // len(LENGTHS) + i) % 2 else 0  # every length on either strand
        recs.append(dict(name=name, bases=bases, quals=quals, cigar=(16 * (i + 1),) * (0, 1, 3)[i % 3], tags=(b"", b"NMC\x07z", b"t" * 300)[(i // 3) % 3], pad=(0, 5, 15, 8)[i % 4],
                         flag=rev | (4, 1 | 64, 1 | 128 | 0x200 | 0x400)[i % 3]))
    # other codes than A, C, G, T at the first and at the last base of reversed records (odd and even lengths), and in the middle
    marked = 0
    for i, r in enumerate(recs):
        if r["flag"] & 0x10 and len(r["bases"]) > 40 and marked < 6:
            at, ch = ((0, b"N"), (-1, b"N"), (-1, b"R"), (0, b"="), (17, b"Y"), (-1, b"K"))[marked]
            r["bases"][at] = ch[0]
            marked += 1
    assert marked == 6
    for r in recs:
        r["bases"] = bytes(r["bases"])
    # secondary and supplementary records in between: first, two in a row, last; without bases, with absent qualities
    sec = dict(name=b"sec", bases=b"ACGTTGCA" * 9, quals=b"\xff" * 72, flag=0x100 | 0x10, cigar=(72 << 4,))
    sup = dict(name=b"sup one", bases=b"ACGT" * 5, quals=bytes(range(20)), flag=0x800, tags=b"SAZchr1\0")
    none = dict(name=b"e", bases=b"", quals=b"", flag=0x100)
    out = [sec]
    for i, r in enumerate(recs):
        out.append(r)
        if i % 11 == 3:
            out += [sup, sec] if i % 2 else [none]
    return out + [sup]


@pytest.fixture(scope="module")
def eng(native):
    e = native.Engine(K, H, TILE, 1 << 20, default_seeds(H))
    yield e
    e.close()


@pytest.fixture(scope="module")
def case():
    recs = _records()
    raw, hb, _ = BC.stream(recs, text=b"@HD\tVN:1.6\tSO:coordinate\n")
    return recs, raw[hb:], BA.aligned_twin(recs)


def _bits(x):
    return struct.pack("<d", float(x))


def test_bam_parse_ex_equals_fastq_parse_of_the_aligned_twin(native, eng, case):
    recs, body, twin = case
    reads = [r for r in recs if not r["flag"] & 0x900]
    fb, rb, used, skipped = eng.bam_parse(body, accept=0x910)
    ft, rt, used_t, stopped = eng.fastq_parse(twin)
    assert used == len(body) and used_t == len(twin) and not stopped and len(rb) == len(rt) == len(reads)
    assert (skipped, int(((rb["flags"] & REVERSED) != 0).sum())) == BA.counts(recs) and skipped >= 10
    rev = [i for i, r in enumerate(reads) if r["flag"] & 0x10]
    assert len(reads) // 3 <= len(rev) <= 2 * len(reads) // 3 and {len(reads[i]["bases"]) % 2 for i in rev} == {0, 1}
    assert {len(reads[i]["bases"]) for i in rev} >= set(LENGTHS) - {0} and {len(r["bases"]) for i, r in enumerate(reads) if i not in rev} >= set(LENGTHS)
    assert {int(rb[i]["seq_off"]) % 16 for i in rev} == set(range(16)) and {int(rb[i]["qual_off"]) % 16 for i in rev} == set(range(16))
    for i, (b, t, src) in enumerate(zip(rb, rt, reads)):
        name = body[int(b["id_off"]):int(b["id_off"]) + int(b["id_len"])]
        assert name == twin[int(t["id_off"]):int(t["id_off"]) + int(t["id_len"])] == src["name"].split()[0], i
        assert int(b["seq_len"]) == int(t["seq_len"]) == len(src["bases"]) and int(b["qual_len"]) == int(t["qual_len"]), i
        # the offsets name the stored bytes, reversed or not
        assert body[int(b["seq_off"]):int(b["seq_off"]) + (len(src["bases"]) + 1) // 2] == BC.pack_bases(src["bases"], src["pad"]), i
        assert body[int(b["qual_off"]):int(b["qual_off"]) + len(src["bases"])] == src["quals"], i
        assert int(b["flags"]) & 1 == int(t["flags"]) == (1 if src["bases"].strip(b"ACGT") else 0), (i, src["bases"][:20])
        assert int(b["flags"]) & ~1 == (REVERSED if src["flag"] & 0x10 else 0), i
        assert _bits(b["phred_sum"]) == _bits(t["phred_sum"]) and _bits(b["phred_first"]) == _bits(t["phred_first"]), (i, len(src["bases"]), src["flag"] & 0x10)
    flagged = [i for i, r in enumerate(rb) if r["flags"] & 1]
    assert len(flagged) == 6 and all(rb[i]["flags"] & REVERSED for i in flagged)
    assert sum(1 for i in flagged if reads[i]["bases"][:1].strip(b"ACGT")) >= 2 and sum(1 for i in flagged if reads[i]["bases"][-1:].strip(b"ACGT")) >= 3
    # the pack of the ACGT records hashes like the twin's pack
    sel = [i for i, r in enumerate(rb) if not (r["flags"] & 1) and r["seq_len"] >= 1]
    pb = eng.fastq_pack(fb, sel, rb["seq_len"][sel])
    pt = eng.fastq_pack(ft, sel, rt["seq_len"][sel])
    last_word_checked = []
    for j, i in enumerate(sel):
        L = len(reads[i]["bases"])
        nt = L // TILE
        for t in range(nt) if nt <= 6 else (0, 1, nt // 2, nt - 2, nt - 1):
            assert np.array_equal(eng.tile_hashes(pb, j, t), eng.tile_hashes(pt, j, t)), (i, t, L, reads[i]["flag"] & 0x10)
        if L % 16 and L >= TILE and L % TILE == 0 and reads[i]["flag"] & 0x10:
            last_word_checked.append(L)
    # reversed records whose last, partial word lies inside a compared tile: of odd and of even length, short and long
    assert len(last_word_checked) >= 6 and {L % 2 for L in last_word_checked} == {0, 1} and max(last_word_checked) > 2000
    with pytest.raises(native.GrpError):
        eng.fastq_pack(fb, flagged[:1], [1])
    eng.fastq_free(fb)
    eng.fastq_free(ft)


def test_accept_zero_is_bam_parse_and_other_bits_are_invalid(native, eng, case):
    recs, body, _ = case
    reads = [r for r in recs if not r["flag"] & 0x900]
    plain = b"".join(BC.record(**dict(r, flag=r["flag"] & ~0x910)) for r in reads)
    f0, r0, u0 = eng.bam_parse(plain)
    f1, r1, u1, s1 = eng.bam_parse(plain, accept=0)
    f2, r2, u2, s2 = eng.bam_parse(plain, accept=0x910)  # (nothing to accept: the same table)
    assert u0 == u1 == u2 == len(plain) and s1 == s2 == 0 and np.array_equal(r0, r1) and np.array_equal(r0, r2) and len(r0) == len(reads)
    for f in (f0, f1, f2):
        eng.fastq_free(f)
    for accept in (0x1, 0x911, 0x4, 0x1000):
        with pytest.raises(native.GrpError) as e:
            eng.bam_parse(plain, accept=accept)
        assert e.value.code == native.GRP_ERR_INVALID, accept


@pytest.mark.parametrize("bit", [0x10, 0x100, 0x800])
def test_each_bit_of_the_mask_alone(native, eng, case, bit):
    """that bit is honoured, the other two are refused at the exact offset"""
    recs, body, _ = case
    base = [dict(r, flag=r["flag"] & ~0x910) for r in recs if not r["flag"] & 0x900][:20]
    want, _, _, _ = BA.walk(b"".join(BC.record(**r) for r in base), True, 0)
    at = want[12]["off"]
    for flag in (0x10, 0x100, 0x800):
        mine = [dict(r) for r in base]
        mine[12]["flag"] |= flag
        buf = b"".join(BC.record(**r) for r in mine)
        if flag == bit:
            fq, rec, used, skipped = eng.bam_parse(buf, accept=bit)
            assert used == len(buf) and (len(rec), skipped) == ((20, 0) if bit == 0x10 else (19, 1))
            assert int(((rec["flags"] & REVERSED) != 0).sum()) == (1 if bit == 0x10 else 0)
            eng.fastq_free(fq)
        else:
            with pytest.raises(native.GrpError) as e:
                eng.bam_parse(buf, accept=bit)
            assert e.value.code == native.GRP_ERR_INVALID and e.value.bad_offset == at and "samtools fastq" in str(e.value), (bit, flag, str(e.value))


def test_chunk_cuts_around_skipped_records(native, eng, case):
    recs, body, _ = case
    full_h, full, _, total_skipped = eng.bam_parse(body, accept=0x910)
    eng.fastq_free(full_h)
    # where every record begins, skipped ones included (a walk that skips nothing: the flags cleared in a copy)
    all_recs, _, _, _ = BA.walk(b"".join(BC.record(**dict(r, flag=0)) for r in recs), True, 0)
    k = next(i for i, r in enumerate(recs) if i > 20 and r["flag"] & 0x900 and recs[i + 1]["flag"] & 0x900)  # two skipped records in a row
    before = sum(1 for r in recs[:k] if not r["flag"] & 0x900)
    skipped_before = k - before
    o0, o1, o2 = all_recs[k]["off"], all_recs[k + 1]["off"], all_recs[k + 2]["off"]
    for what, cut, n_used, n_skip in (("inside the first", o0 + 40, o0, skipped_before), ("directly behind the first", o1, o1, skipped_before + 1), ("inside the second", o1 + 3, o1, skipped_before + 1),
                                      ("directly behind the second", o2, o2, skipped_before + 2)):
        fq, rec, used, skipped = eng.bam_parse(body[:cut], final_chunk=False, accept=0x910)
        assert (len(rec), used, skipped) == (before, n_used, n_skip), what
        assert np.array_equal(rec, full[:before]), what
        eng.fastq_free(fq)
        fq, rec2, used2, skipped2 = eng.bam_parse(body[used:], final_chunk=True, accept=0x910)
        assert (len(rec2), used2, skipped + skipped2) == (len(full) - before, len(body) - used, total_skipped), what
        shifted = full[before:].copy()
        for f in ("id_off", "seq_off", "qual_off"):
            shifted[f] -= used
        assert np.array_equal(rec2, shifted), what
        eng.fastq_free(fq)
    # a chunk of skipped records only: no record, all of its bytes used
    fq, rec, used, skipped = eng.bam_parse(body[o0:o2], final_chunk=False, accept=0x910)
    assert (len(rec), used, skipped) == (0, o2 - o0, 2)
    eng.fastq_free(fq)
    fq, rec, used, skipped = eng.bam_parse(body[o0:o2 + 7], final_chunk=False, accept=0x910)
    assert (len(rec), used, skipped) == (0, o2 - o0, 2)
    eng.fastq_free(fq)
    with pytest.raises(native.GrpError) as e:  # a final chunk that ends inside a skipped record
        eng.bam_parse(body[o0:o1 + 40], final_chunk=True, accept=0x910)
    assert e.value.code == native.GRP_ERR_INVALID and e.value.bad_offset == o1 - o0 and "truncated" in str(e.value)
    # a skipped record whose block_size is broken is refused at its offset
    broken = BC.record(b"nm", b"ACGT", b"\xff" * 4, flag=0x100, block_size=38)
    with pytest.raises(native.GrpError) as e:
        eng.bam_parse(body[:o0] + broken + body[o0:], accept=0x910)
    assert e.value.code == native.GRP_ERR_INVALID and e.value.bad_offset == o0


def test_a_body_uploaded_ahead_with_a_tail_in_front(native, eng, case):
    """as tests/test_gpu_bam.py: the body goes up first, the parse gets [tail of the chunk before | body] and finds the
    records 5 bytes into a 16-byte group — reversed records among them"""
    recs, body, _ = case
    want, _, _, _ = BA.walk(body, True, 0x910)
    cut = want[25]["off"] + 5
    fq, rec0, used0, _ = eng.bam_parse(body[:cut], final_chunk=False, accept=0x910)
    eng.fastq_free(fq)
    assert len(rec0) == 25 and cut - used0 == 5
    fq, exp, exp_used, exp_skipped = eng.bam_parse(body[used0:], accept=0x910)
    sel = [i for i, r in enumerate(exp) if not (r["flags"] & 1) and r["seq_len"] >= TILE]
    assert sum(1 for i in sel if exp[i]["flags"] & REVERSED) >= 10
    ref = eng.fastq_pack(fq, sel, exp["seq_len"][sel])
    hashes = [eng.tile_hashes(ref, j, int(exp["seq_len"][i]) // TILE - 1).copy() for j, i in enumerate(sel)]
    eng.fastq_free(fq)
    room = 4096
    buf = np.zeros(room + len(body) - cut, dtype=np.uint8)
    buf[room:] = np.frombuffer(body[cut:], dtype=np.uint8)
    assert eng.fastq_prefetch(buf[room:], buf.size - room)
    buf[room - 5:room] = np.frombuffer(body[used0:cut], dtype=np.uint8)
    view = buf[room - 5:]
    fq, rec, used, skipped = eng.bam_parse(view, final_chunk=True, accept=0x910)
    assert used == exp_used and skipped == exp_skipped and np.array_equal(rec, exp)
    batch = eng.fastq_pack(fq, sel, rec["seq_len"][sel])
    for j, i in enumerate(sel):
        assert np.array_equal(eng.tile_hashes(batch, j, int(rec["seq_len"][i]) // TILE - 1), hashes[j]), j
    eng.fastq_free(fq)
    assert eng.fastq_prefetch(None, 0)
