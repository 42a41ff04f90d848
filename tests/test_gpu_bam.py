"""GPU: grp_bam_parse (csrc/grp_ingest.inc: k_bam_records, k_fq_phred over raw qualities, k_bam_pack) against grp_fastq_parse
of the FASTQ twin on the same engine — the record table, the ACGT flag, bit-identical Phred sums, the packed bases — then
chunking, the refusals and a body uploaded ahead of its parse."""
import struct

import numpy as np
import pytest

import bam_cases as BC
from helpers import default_seeds

pytestmark = pytest.mark.gpu

K, H = 22, 4
TILE = K + H - 1  # the smallest legal tile, and an odd one: records of odd AND even length end on a tile boundary
# the lengths around the kernels' 16-byte (32-base) loads and 16-base words, a few long ones, and multiples of the tile
# that are no multiple of 16: their last, partial word lies inside a compared tile (tile_hashes covers whole tiles only)
LENGTHS = [0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 25, 50, 75, 125, 175, 525, 1025, 1550, 2975, 601, 2000]


def _records(seed=3, n=62):
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    recs = []
    for i in range(n):
        L = LENGTHS[i % len(LENGTHS)]
        bases = bytearray(acgt[rng.integers(0, 4, size=L)].tobytes())
        quals = bytes(rng.integers(0, 61, size=L).astype(np.uint8))
        if i % 9 == 1 and L:
            quals = quals[:L // 3] + b"\x5d" * (L - L // 3)  # 93, the largest quality with a character
        name = bytes(rng.integers(ord("a"), ord("z") + 1, size=1 + (i * 7) % 40).astype(np.uint8))
        if i % 6 == 2 and len(name) > 4:
            name = name[:3] + (b" " if i % 4 else b"\t") + name[4:]  # the id is cut at a whitespace
        recs.append(dict(name=name, bases=bases, quals=quals, cigar=(16 * (i + 1),) * (0, 1, 3)[i % 3], tags=(b"", b"NMC\x07z", b"t" * 300)[(i // 3) % 3],
                         pad=(0, 5, 15, 8)[i % 4], flag=4 | (0, 1 | 64, 1 | 128 | 512)[i % 3]))
    # other codes than A, C, G, T: at the first base, at the last (odd and even lengths), in the middle, and the code 0
    for i, (at, ch) in {30: (0, b"N"), 31: (-1, b"N"), 32: (-1, b"R"), 33: (-1, b"="), 34: (7, b"="), 46: (500, b"Y"), 47: (-1, b"K")}.items():
        assert len(recs[i]["bases"]) > 8
        recs[i]["bases"][at] = ch[0]
    for r in recs:
        r["bases"] = bytes(r["bases"])
    return recs


@pytest.fixture(scope="module")
def eng(native):
    e = native.Engine(K, H, TILE, 1 << 20, default_seeds(H))
    yield e
    e.close()


@pytest.fixture(scope="module")
def case():
    recs = _records()
    raw, hb, twin = BC.stream(recs, text=b"@HD\tVN:1.6\n")
    return recs, raw[hb:], twin


def _bits(x):
    return struct.pack("<d", float(x))


def test_bam_parse_equals_fastq_parse_of_the_twin(native, eng, case):
    recs, body, twin = case
    fb, rb, used = eng.bam_parse(body)
    ft, rt, used_t, stopped = eng.fastq_parse(twin)
    assert used == len(body) and used_t == len(twin) and not stopped and len(rb) == len(rt) == len(recs)  # (the last record ends the buffer exactly)
    assert {int(r["seq_off"]) % 16 for r in rb} == set(range(16)) and {int(r["qual_off"]) % 16 for r in rb} == set(range(16))
    for i, (b, t, src) in enumerate(zip(rb, rt, recs)):
        name = body[int(b["id_off"]):int(b["id_off"]) + int(b["id_len"])]
        assert name == twin[int(t["id_off"]):int(t["id_off"]) + int(t["id_len"])] == src["name"].split()[0], i
        assert int(b["seq_len"]) == int(t["seq_len"]) == len(src["bases"]) and int(b["qual_len"]) == int(t["qual_len"]), i
        assert body[int(b["seq_off"]):int(b["seq_off"]) + (len(src["bases"]) + 1) // 2] == BC.pack_bases(src["bases"], src["pad"]), i
        assert body[int(b["qual_off"]):int(b["qual_off"]) + len(src["bases"])] == src["quals"], i
        assert int(b["flags"]) == int(t["flags"]) == (1 if src["bases"].strip(b"ACGT") else 0), (i, src["bases"][:20])
        assert _bits(b["phred_sum"]) == _bits(t["phred_sum"]) and _bits(b["phred_first"]) == _bits(t["phred_first"]), i
    flagged = [i for i, r in enumerate(rb) if r["flags"] & 1]
    assert len(flagged) == 7 and any(len(recs[i]["bases"]) % 2 and recs[i]["pad"] for i in range(len(recs)) if i not in flagged)
    # the pack of the ACGT records hashes like the twin's pack
    sel = [i for i, r in enumerate(rb) if not (r["flags"] & 1) and r["seq_len"] >= 1]
    pb = eng.fastq_pack(fb, sel, rb["seq_len"][sel])
    pt = eng.fastq_pack(ft, sel, rt["seq_len"][sel])
    last_word_checked = []
    for j, i in enumerate(sel):
        L = len(recs[i]["bases"])
        nt = L // TILE
        for t in range(nt) if nt <= 6 else (0, 1, nt // 2, nt - 2, nt - 1):  # (the first words, the last ones, and one in between)
            assert np.array_equal(eng.tile_hashes(pb, j, t), eng.tile_hashes(pt, j, t)), (i, t)
        if L % 16 and L >= TILE and L % TILE == 0:
            last_word_checked.append(L)
    # records whose last, partial word lies inside a compared tile: of odd length (a padding code behind the last base) and
    # of even length, short and long
    assert len(last_word_checked) >= 8 and {L % 2 for L in last_word_checked} == {0, 1} and max(last_word_checked) > 2000
    with pytest.raises(native.GrpError):
        eng.fastq_pack(fb, flagged[:1], [1])
    eng.fastq_free(fb)
    eng.fastq_free(ft)


def test_chunking(native, eng, case):
    recs, body, _ = case
    full_h, full, _ = eng.bam_parse(body)
    eng.fastq_free(full_h)
    want, _, _ = BC.walk(body)
    k = 22  # a record with a name, CIGAR operations, bases, qualities and tags
    r = want[k]
    assert recs[k]["cigar"] and recs[k]["tags"] and r["l_seq"] > 4
    cuts = {"block_size": r["off"] + 2, "fixed part": r["off"] + 4 + 17, "name": r["off"] + 36 + 1, "bases": r["seq_off"] + 1, "qualities": r["qual_off"] + r["l_seq"] - 1,
            "tags": r["end"] - 2, "a record boundary": r["off"]}
    for what, cut in cuts.items():
        fq, rec, used = eng.bam_parse(body[:cut], final_chunk=False)
        assert len(rec) == k and used == r["off"], what  # only complete records are consumed
        assert np.array_equal(rec, full[:k]), what
        eng.fastq_free(fq)
        fq, rec2, used2 = eng.bam_parse(body[used:], final_chunk=True)  # ... and the resubmitted tail completes them
        assert len(rec2) == len(recs) - k and used2 == len(body) - used, what
        shifted = full[k:].copy()
        for f in ("id_off", "seq_off", "qual_off"):
            shifted[f] -= used
        assert np.array_equal(rec2, shifted), what
        eng.fastq_free(fq)
        if cut != r["off"]:
            with pytest.raises(native.GrpError) as e:  # a final chunk that ends inside a record
                eng.bam_parse(body[:cut], final_chunk=True)
            assert e.value.code == native.GRP_ERR_INVALID and e.value.bad_offset == r["off"] and "truncated" in str(e.value), what
    fq, rec, used = eng.bam_parse(b"")
    assert len(rec) == 0 and used == 0
    eng.fastq_free(fq)
    fq, rec, used = eng.bam_parse(body[:3], final_chunk=False)
    assert len(rec) == 0 and used == 0
    eng.fastq_free(fq)


REFUSALS = {
    "block_size below the fixed part": dict(block_size=20),
    "block_size below the fields": dict(block_size=32 + 3 + 4 + 8 - 1),
    "l_read_name 0": dict(l_read_name=0, nul=False, name=b""),
    "name without NUL": dict(nul=False),
    "flag 0x10": dict(flag=16),
    "flag 0x100": dict(flag=256),
    "flag 0x800": dict(flag=2048 | 4),
    "absent qualities": dict(quals=b"\xff" * 8),
    "a quality of 94": dict(quals=b"\x00" * 7 + b"\x5e"),
}


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_refusals(native, eng, case, what):
    recs, body, _ = case
    want, _, _ = BC.walk(body)
    at = want[12]["off"]
    bad = BC.record(**dict(dict(name=b"nm", bases=b"ACGTACGT", quals=b"\x10" * 8), **REFUSALS[what]))
    with pytest.raises(native.GrpError) as e:
        eng.bam_parse(body[:at] + bad + body[at:])
    assert e.value.code == native.GRP_ERR_INVALID and e.value.bad_offset == at, (what, str(e.value))
    if what.startswith("flag"):
        assert "samtools fastq" in str(e.value)
    # the engine stays usable
    fq, rec, used = eng.bam_parse(body)
    assert len(rec) == len(recs) and used == len(body)
    eng.fastq_free(fq)


def test_a_body_uploaded_ahead_with_a_tail_in_front(native, eng, case):
    """grp_fastq_prefetch serves a BAM chunk as it serves text (tests/test_gpu_ingest.py covers the mechanism): the body goes
    up first, the parse gets [tail of the chunk before | body] and finds the records 5 bytes into a 16-byte group"""
    recs, body, _ = case
    want, _, _ = BC.walk(body)
    cut = want[25]["off"] + 5  # the chunk before ends 5 bytes into record 25
    fq, rec0, used0 = eng.bam_parse(body[:cut], final_chunk=False)
    eng.fastq_free(fq)
    assert len(rec0) == 25 and cut - used0 == 5
    fq, exp, exp_used = eng.bam_parse(body[used0:])
    sel = [i for i, r in enumerate(exp) if not (r["flags"] & 1) and r["seq_len"] >= TILE]
    ref = eng.fastq_pack(fq, sel, exp["seq_len"][sel])
    hashes = [eng.tile_hashes(ref, j, 0).copy() for j in range(len(sel))]
    eng.fastq_free(fq)
    room = 4096
    buf = np.zeros(room + len(body) - cut, dtype=np.uint8)
    buf[room:] = np.frombuffer(body[cut:], dtype=np.uint8)
    assert eng.fastq_prefetch(buf[room:], buf.size - room)
    buf[room - 5:room] = np.frombuffer(body[used0:cut], dtype=np.uint8)
    view = buf[room - 5:]
    fq, rec, used = eng.bam_parse(view, final_chunk=True)
    assert used == exp_used and np.array_equal(rec, exp)
    batch = eng.fastq_pack(fq, sel, rec["seq_len"][sel])
    for j in range(len(sel)):
        assert np.array_equal(eng.tile_hashes(batch, j, 0), hashes[j]), j
    eng.fastq_free(fq)
    assert eng.fastq_prefetch(None, 0)
