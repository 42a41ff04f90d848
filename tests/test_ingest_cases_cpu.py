"""CPU: the edge sweeps of the device ingest (tests/ingest_cases.py, the sweeps of tests/bam_cases.py) hit what they claim
to hit, and their host model is the reader's: the coverage is asserted from the generated texts alone, the model is held
against the oracle's FASTQ reader (orc_reads_load, orc_sum_phred) and against its own restatement in numpy, the BAM sweeps'
twins against bam_aligned_cases.twin_read.  tests/test_gpu_ingest_edges.py and tests/test_gpu_bam_edges.py run the same
texts through the kernels."""
import ctypes as C

import numpy as np
import pytest

import bam_aligned_cases as BA
import bam_cases as BC
import ingest_cases as IC

# Records of S3 on which the oracle's reader and the host reader's rules (csrc/host/gr_fastq.cpp) disagree: kept in the
# device test against the host reader's rule, left out of the comparison with the oracle.  (None: both readers trim CR /
# blank / tab, cut the id at isspace and take the four lines as they come.)
ORACLE_EXCLUDED = ()


@pytest.fixture(scope="module")
def sum_phred(native):
    from goldrush_amd import host

    hl = host.load()
    return IC.PhredCache(lambda q: hl.gr_sum_phred(q, len(q)))


@pytest.fixture(scope="module")
def s1():
    return IC.s1_text()


@pytest.fixture(scope="module")
def s2():
    return IC.s2_text()


def _s1_coverage(text, lengths, aligns, want_lengths):
    recs, stopped = IC.host_parse(text)
    assert not stopped and len(recs) == len(lengths)
    seen = {}
    for (_, _, so, sl, qo, ql), L, a in zip(recs, lengths, aligns):
        assert sl == ql == L and so % 16 == a
        seen.setdefault(L, (set(), set()))
        seen[L][0].add(so % 16)
        seen[L][1].add(qo % 16)
    assert sorted(seen) == sorted(want_lengths)
    for L, (sa, qa) in seen.items():
        assert sa == set(range(16)) and qa == set(range(16)), L
    return recs


def _phred_coverage(recs):
    """whole 64-byte lines behind the prologue of phred_chain, for both halves of the walk: 0, 1, 2 and 3 or more"""
    first, second = set(), set()
    for _, _, _, _, qo, qn in recs:
        if qn >= 2:
            first.add(min(IC.phred_lines(qo, qn // 2), 3))
            second.add(min(IC.phred_lines(qo + qn // 2, qn - qn // 2), 3))
    return first, second


def test_record_dtype_is_the_engines(native):
    assert IC.RECORD_DTYPE == native.fastq_record_dtype and IC.NON_ACGT == 1


def test_s1_covers_every_length_at_every_alignment(s1):
    text, lengths, aligns = s1
    assert len(IC.S1_LENGTHS) == 343 and set(range(331)) <= set(IC.S1_LENGTHS)
    assert {1023, 1024, 1025, 1039, 1040, 1041, 2047, 2048, 2049, 2063, 2064, 2065} <= set(IC.S1_LENGTHS)
    recs = _s1_coverage(text, lengths, aligns, IC.S1_LENGTHS)
    assert len(recs) == 343 * 16 and 2_000_000 < len(text) < 3_500_000
    assert _phred_coverage(recs) == ({0, 1, 2, 3}, {0, 1, 2, 3})
    # exactly one and exactly two lines left with nothing behind them, and a prologue that eats a whole half
    exact = {(IC.phred_lines(qo, qn // 2), (qn // 2 - min((-qo) % 16, qn // 2)) % 64) for _, _, _, _, qo, qn in recs if qn >= 2}
    assert {(1, 0), (2, 0), (0, 0)} <= exact
    assert any(0 < qn // 2 <= (-qo) % 16 for _, _, _, _, qo, qn in recs)
    seqs = [text[so:so + sl] for _, _, so, sl, _, _ in recs]
    assert sum(1 for s in seqs if s and s == s.lower()) > 800 and sum(1 for s in seqs if s != s.lower() and s != s.upper()) > 800
    quals = [text[qo:qo + qn] for _, _, _, _, qo, qn in recs]
    assert sum(1 for q in quals if len(q) > 3 and set(q) == {33}) > 300 and sum(1 for q in quals if len(q) > 3 and set(q) == {126}) > 300
    assert {33, 126} <= set(b"".join(quals)) and all(33 <= c <= 126 for c in set(b"".join(quals)))


def test_a_thinned_s1_fails_the_coverage():
    """the assertions above are no formality: one alignment less, or no long records, and they fail"""
    text, lengths, aligns = IC.s1_text(lengths=[0, 1, 17, 64, 330], aligns=range(15))
    with pytest.raises(AssertionError):
        _s1_coverage(text, lengths, aligns, [0, 1, 17, 64, 330])
    text, lengths, aligns = IC.s1_text(lengths=range(200))
    recs = _s1_coverage(text, lengths, aligns, range(200))
    assert _phred_coverage(recs) != ({0, 1, 2, 3}, {0, 1, 2, 3})


def _s2_coverage(text, cases, values):
    recs, stopped = IC.host_parse(text)
    assert not stopped and len(recs) == len(cases) + len(np.unique(cases["twin"]))
    met, rounds, lanes, trimmed = {}, set(), set(), set()
    for c in cases:
        _, _, so, sl, _, _ = recs[c["rec"]]
        _, _, tso, tsl, _, _ = recs[c["twin"]]
        L, a, p, kind = int(c["len"]), int(c["align"]), int(c["pos"]), IC.S2_KINDS[c["kind"]]
        bad, clean = text[so:so + L], text[tso:tso + L]
        assert so % 16 == tso % 16 == a and tsl == L and not clean.translate(None, b"ACGT"), c
        assert bad[:p] == clean[:p] and bad[p + 1:] == clean[p + 1:] and bad[p] == c["byte"] and bad[p] not in IC.ACGT, c
        if c["byte"] in b" \t\r" and p == L - 1:  # the trim takes it: the record is clean and one shorter
            assert sl == L - 1
            trimmed.add(int(c["byte"]))
            continue
        assert sl == L
        f, t = IC.middle(so, L)
        where = {"every": p, "0": 0, "1": 1, "a0-1": f - 1, "a0": f, "a0+15": f + 15, "a0+16": f + 16, "a0+1023": f + 1023, "a0+1024": f + 1024,
                 "a1-1": t - 1, "a1": t, "L-2": L - 2, "L-1": L - 1}[kind]
        assert p == where, c
        cls, lane, rnd = IC.scan_class(so, L, p)
        if kind != "every":
            meant = {"a0-1": "front", "a0": "aligned", "a0+15": "aligned", "a0+16": "aligned", "a0+1023": "aligned", "a1-1": "aligned", "a1": "tail"}.get(kind)
            assert cls != "none" and (meant is None or cls == meant), c
            assert kind != "a0+1024" or cls == "tail" or (cls, lane, rnd) == ("aligned", 0, 1), c
            assert kind != "a0+1023" or (lane, rnd) == (63, 0), c
        met.setdefault(cls, {}).setdefault(a, set()).add(int(c["byte"]))
        if cls == "aligned":
            rounds.add(rnd)
            lanes.add(lane)
    # every class at every alignment (bytes in front of the aligned middle need a sequence that does not begin on one)
    for cls in ("front", "aligned", "tail", "none"):
        assert set(met[cls]) == set(range(16)) - ({0} if cls == "front" else set()), cls
        assert set().union(*met[cls].values()) == set(values), cls  # ... and every bad byte in every class
    assert rounds == {0, 1, 2} and {0, 1, 63} <= lanes  # the first lanes, the last one, and a lane's second and third load
    assert trimmed == {32, 9, 13}
    return recs


def test_s2_plants_every_position_it_claims(s2):
    text, cases = s2
    values = IC.bad_bytes()
    assert len(values) == len(set(values)) and not set(values) & set(IC.ACGT) and {ord("N"), ord("n"), ord("U"), ord("R"), ord("@"), ord("`"), 1, 0xC1, 32, 9, 13} <= set(values)
    assert {c ^ (1 << b) for c in IC.ACGT for b in range(8)} - set(IC.ACGT) <= set(values)
    _s2_coverage(text, cases, values)
    assert 20_000 <= len(cases) <= 26_000
    short = cases[cases["kind"] == 0]
    for L in IC.S2_SHORT:  # every position of every short length at every alignment
        for a in range(16):
            assert sorted(short["pos"][(short["len"] == L) & (short["align"] == a)]) == list(range(L)), (L, a)
    edge = cases[cases["kind"] != 0]
    assert sorted(set(edge["len"])) == IC.S2_LONG == list(range(1023, 1042)) + [2064]
    for L in IC.S2_LONG:
        for a in range(16):
            kinds = {IC.S2_KINDS[k] for k in edge["kind"][(edge["len"] == L) & (edge["align"] == a)]}
            f, t = IC.middle(a, L)
            assert kinds >= {"0", "1", "a0", "a0+15", "a0+16", "a1-1", "L-2", "L-1"} | ({"a0-1"} if f else set()) | ({"a1"} if t < L else set()) | {"a0+%d" % d for d in (1023, 1024) if f + d < L}, (L, a)


def test_a_thinned_s2_fails_the_coverage():
    """without the long records (no tail behind a second round), or with one alignment less"""
    for kw in (dict(long=[]), dict(aligns=range(1, 16)), dict(short=[], long=[1040])):
        text, cases = IC.s2_text(**kw)
        with pytest.raises((AssertionError, KeyError)):
            _s2_coverage(text, cases, IC.bad_bytes())
    # the tail positions dropped from the case list
    text, cases = IC.s2_text(short=range(1, 20))
    recs, _ = IC.host_parse(text)
    keep = np.array([IC.scan_class(recs[c["rec"]][2], int(c["len"]), int(c["pos"]))[0] != "tail" for c in cases])
    with pytest.raises((AssertionError, KeyError)):
        _s2_coverage(text, cases[keep], IC.bad_bytes())


def test_s4_blocks_are_what_the_comments_say():
    small = {what: (text, final) for what, text, final in IC.s4_small()}
    assert len(small) == 3 * len(IC.S4_CUTS) + 6
    assert {n % 16 for n in IC.S4_CUTS if n < 5000} == {n % 16 for n in IC.S4_CUTS if n > 5000} == set(range(16))
    assert {4095, 4096, 4097, 8191, 8192, 8193} <= set(IC.S4_CUTS)
    left, completes = set(), 0
    for n in IC.S4_CUTS:
        text, final = small["cut at %d, as it falls" % n]
        assert len(text) == n and final and len(small["cut at %d, a newline last" % n][0]) == n and small["cut at %d, a newline last" % n][0][-1] == 10
        assert small["cut at %d, more to come" % n] == (text, False)
        lines = IC.split_lines(text, True)
        left.add((len(lines) % 4, text[-1] == 10))
        completes += len(lines) % 4 == 0 and text[-1] != 10  # the virtual newline completes a record
        recs, stopped = IC.host_parse(text)
        assert not stopped and (len(lines) % 4 == 0) == (IC.consumed(text, True, False) == n)
        assert len(lines) % 4 == 0 or IC.consumed(text, True, False) == recs[-1][4] + recs[-1][5] + 1 < n  # ... ends behind the last complete record
    assert {k for k, _ in left} == {0, 1, 2, 3} and {(k, False) for k in range(4)} <= left and completes >= 4
    for edge in (4096, 8192):
        text, _ = small["newlines at %d and %d" % (edge - 1, edge)]
        assert text[edge - 1] == text[edge] == 10 and text[edge - 2] != 10 and len(text) > edge + 16
    text, _ = small["lines of 9000 bytes"]
    per = IC.block_newlines(text)
    assert list(per == 0) == [False, True, True, False, True, False]  # two whole blocks inside the sequence line, one inside the quality line
    text, _ = small["'@', '+' and newlines only"]
    per = IC.block_newlines(text)
    groups = (np.frombuffer(text[:8192], dtype=np.uint8) == 10).reshape(-1, 16).sum(axis=1)
    assert len(per) == 3 and per[0] >= 2730 and per[1] >= 2730 and set(groups) == {10, 11}
    text, _ = small["... and 48 newlines behind them"]
    groups = (np.frombuffer(text[:96], dtype=np.uint8) == 10).reshape(-1, 16).sum(axis=1)
    assert list(groups[3:6]) == [16, 16, 16] and IC.host_parse(text) == (IC.host_parse(text[:48])[0], True) and len(IC.host_parse(text)[0]) == 8
    assert small["... without the last newline"][0][-1] != 10


def test_s4_big_crosses_two_carries_of_the_scan(sum_phred):
    text = IC.s4_big()
    per = IC.block_newlines(text)
    assert 2 * IC.SCAN_ROUND < len(per) <= 2 * IC.SCAN_ROUND + 8 and 8 << 20 < len(text) < (8 << 20) + (64 << 10)
    for edge in (IC.SCAN_ROUND, 2 * IC.SCAN_ROUND):  # the two blocks on either side of a carry are full of lines, the rest hold a few
        assert per[edge - 2:edge + 2].min() > 1000, per[edge - 2:edge + 2]
    assert np.median(per) <= 9 and per[:IC.SCAN_ROUND].sum() > 0 and text[-1] == 10
    # the numpy model is the loop's, here and on the small texts
    got = IC.table_np(text, sum_phred)
    exp = IC.model_table(text, sum_phred)
    assert IC.table_diff(got[0], exp[0]) is None and got[1:] == exp[1:] == (len(text), False) and len(exp[0]) > 4000


def test_the_numpy_model_is_the_loop(s1, s2, sum_phred):
    texts = [(s1[0], True), (IC.s3_text()[0], True), (s2[0][:400_000], True), (s2[0][:400_000], False)] + [(t, f) for _, t, f in IC.s4_small()] + [(b"", True), (b"@a\nAC\n+\n", True), (b"\n", True)]
    for text, final in texts:
        got, exp = IC.table_np(text, sum_phred, final), IC.model_table(text, sum_phred, final)
        assert IC.table_diff(got[0], exp[0]) is None and got[1:] == exp[1:], (text[:40], len(text), final, got[1:], exp[1:])


def test_the_model_is_the_oracles_reader(oracle, native, tmp_path, s1, sum_phred):
    """S1 and S3 written to files and read by the oracle's FASTQ reader: ids, upper-cased sequences, qualities and the
    Phred sum of every record, bit for bit; the expected pack is pack_reads of these strings"""
    lib = oracle.load()
    s3, what = IC.s3_text()
    assert set(ORACLE_EXCLUDED) <= set(what)  # at most records of S3 may be left out, none of S1
    for name, text, skip in (("s1", s1[0], ()), ("s3", s3, ORACLE_EXCLUDED)):
        path = str(tmp_path / (name + ".fq"))
        with open(path, "wb") as f:
            f.write(text)
        reads = oracle.orc_reads()
        assert lib.orc_reads_load(C.byref(reads), path.encode()) == 0 and reads.is_fastq
        table, used, stopped = IC.model_table(text, sum_phred)
        assert not stopped and used == len(text) and reads.n == len(table) == (len(s1[1]) if name == "s1" else len(what))
        strings = IC.upper_strings(text, table)
        compared = 0
        for i, r in enumerate(table):
            if name == "s3" and what[i] in skip:
                continue
            o = reads.rec[i]
            qual = text[int(r["qual_off"]):int(r["qual_off"]) + int(r["qual_len"])]
            assert text[int(r["id_off"]):int(r["id_off"]) + int(r["id_len"])] == o.id, (name, i)
            assert strings[i] == o.seq and len(strings[i]) == o.len and qual == o.qual and len(qual) == o.qlen, (name, i)
            assert bool(r["flags"] & 1) == (len(o.seq.strip(b"ACGT")) != 0), (name, i)
            assert np.float64(r["phred_sum"]).tobytes() == np.float64(lib.orc_sum_phred(o.qual, o.qlen)).tobytes(), (name, i)
            half = qual[:len(qual) // 2]
            assert np.float64(r["phred_first"]).tobytes() == np.float64(lib.orc_sum_phred(half, len(half)) if len(qual) >= 2 else 0.0).tobytes(), (name, i)
            compared += 1
        assert compared == len(table) - len(skip)
        lib.orc_reads_free(C.byref(reads))
        if name == "s1":
            packed, word_off, lens = native.pack_reads(strings)
            assert list(lens) == list(s1[1]) and int(word_off[-1]) == sum((int(n) + 15) // 16 for n in s1[1]) == packed.size


def test_s3_holds_what_it_names(sum_phred):
    text, what = IC.s3_text()
    table, used, stopped = IC.model_table(text, sum_phred)
    assert not stopped and used == len(text) and len(table) == len(what) == 19 + 5 + 4 * 17
    by = {w: (r, text[int(r["id_off"]):int(r["id_off"]) + int(r["id_len"])]) for w, r in zip(what, table)}
    assert by["'@' alone, all empty"][0]["seq_len"] == by["'@' alone, all empty"][0]["qual_len"] == by["'@' alone"][0]["id_len"] == 0
    assert by["'@ x': an empty id"][1] == by["'@' and white space only"][1] == b"" and by["a header of 300 bytes"][0]["id_len"] == 299
    assert by["a header of 300 bytes with a comment"][0]["id_len"] == 150
    assert (by["quality shorter than the sequence"][0]["seq_len"], by["quality shorter than the sequence"][0]["qual_len"]) == (20, 3)
    assert (by["quality longer than the sequence"][0]["seq_len"], by["quality longer than the sequence"][0]["qual_len"]) == (3, 40)
    assert by["a blank inside the sequence"][0]["flags"] == by["a tab and a CR inside the sequence"][0]["flags"] == 1 and by["a sequence line of white space"][0]["seq_len"] == 0
    for ch in (9, 11, 12, 13, 32):
        assert by["the id ends at byte %d" % ch][1] == b"id%d" % ch
    for n in range(1, 18):
        for line in ("the header", "the sequence", "the quality", "all four"):
            r, name = by["%d trailing on %s" % (n, line)]
            assert (int(r["seq_len"]), int(r["qual_len"]), int(r["flags"]), len(name)) == (5, 5, 0, 2 + (n > 9)), (n, line)
    runs = [text[int(r["seq_off"]) + 5:text.index(b"\n", int(r["seq_off"]))] for w, r in zip(what, table) if w.endswith("trailing on the sequence")]
    assert sorted(len(x) for x in runs) == list(range(1, 18)) and {32, 9, 13} == set(b"".join(runs))


# ---- the BAM sweeps --------------------------------------------------------------------------------------------------

def _bam_twin_check(records, flag):
    """every generated record through the FASTQ model equals twin_read"""
    records = [dict(r, flag=flag) for r in records]
    twin = BA.aligned_twin(records)
    recs, stopped = IC.host_parse(twin)
    assert not stopped and len(recs) == len(records)
    for (io, il, so, sl, qo, ql), r in zip(recs, records):
        bases, qual = BA.twin_read(r["bases"], r["quals"], flag)
        assert (twin[io:io + il], twin[so:so + sl], twin[qo:qo + ql]) == (r["name"], bases, qual)
    return records


def test_bam_sweep_covers_every_length_at_every_alignment():
    recs = BC.sweep_records()
    assert set(BC.SWEEP_LENGTHS) >= set(IC.S1_LENGTHS) | {2047, 2048, 2049, 2079, 2080, 2081, 4128} and len(recs) == 16 * len(BC.SWEEP_LENGTHS) == 16 * 347
    for flag in (4, 0x10):
        mine = _bam_twin_check(recs, flag)
        body = b"".join(BC.record(**r) for r in mine)
        walked, used, bad, skipped = BA.walk(body, True, 0x10)
        assert used == len(body) and bad is None and not skipped and len(walked) == len(mine)
        seen = {}
        for w, r in zip(walked, mine):
            assert w["l_seq"] == len(r["bases"]) and w["name"] == r["name"]
            s = seen.setdefault(w["l_seq"], (set(), set(), set()))
            s[0].add(w["seq_off"] % 16)
            s[1].add(w["qual_off"] % 16)
            s[2].add(r["pad"])
        assert sorted(seen) == sorted(BC.SWEEP_LENGTHS)
        for L, (sa, qa, pads) in seen.items():
            assert sa == qa == set(range(16)) and (not L & 1 or pads == set(range(16))), L


def test_bam_bad_codes_are_planted_where_they_claim():
    recs, cases = BC.bad_code_records()
    assert sorted(BC.BAD_CODES) == [0, 3, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15] and 20_000 <= len(cases) <= 28_000
    _bam_twin_check(recs, 0x10)
    body = b"".join(BC.record(**r) for r in recs)
    walked, used, bad = BC.walk(body)
    assert bad is None and len(walked) == len(recs) == len(cases) + len(np.unique(cases["twin"]))
    met, rounds, lanes, pads = {}, set(), set(), set()
    for c in cases:
        r, t, w = recs[c["rec"]], recs[c["twin"]], walked[c["rec"]]
        L, a, p, kind = int(c["len"]), int(c["align"]), int(c["pos"]), BC.BAD_KINDS[c["kind"]]
        assert w["seq_off"] % 16 == walked[c["twin"]]["seq_off"] % 16 == a and len(r["bases"]) == len(t["bases"]) == L and not t["bases"].strip(b"ACGT")
        assert r["bases"][:p] == t["bases"][:p] and r["bases"][p + 1:] == t["bases"][p + 1:] and BC.CODE_OF[r["bases"][p]] == c["code"]
        stored = body[w["seq_off"] + p // 2]
        assert (stored >> 4 if p % 2 == 0 else stored & 15) == c["code"]
        if p == L - 1 and L & 1:
            cls, lane, rnd = "odd", 0, 0  # the high half of the byte behind the whole bytes: lane 0's own test
            pads.add(r["pad"])
        else:
            cls, lane, rnd = IC.scan_class(w["seq_off"], L // 2, p // 2)
        if kind not in ("every", "odd"):
            f, tl = IC.middle(w["seq_off"], L // 2)
            where = {"0": 0, "1": 1, "a0-1": f - 1, "a0": f, "a0+15": f + 15, "a0+16": f + 16, "a0+1023": f + 1023, "a0+1024": f + 1024, "a1-1": tl - 1, "a1": tl,
                     "L-2": L // 2 - 2, "L-1": L // 2 - 1}[kind]
            assert p // 2 == where, c
            meant = {"a0-1": "front", "a0": "aligned", "a0+15": "aligned", "a0+16": "aligned", "a0+1023": "aligned", "a1-1": "aligned", "a1": "tail"}.get(kind)
            assert meant is None or cls == meant, c
        met.setdefault(cls, {}).setdefault(a, set()).add((int(c["code"]), p % 2))
        if cls == "aligned":
            rounds.add(rnd)
            lanes.add(lane)
    for cls in ("front", "aligned", "tail", "none", "odd"):
        assert set(met[cls]) == set(range(16)) - ({0} if cls == "front" else set()), cls
        halves = {(code, 0) for code in BC.BAD_CODES} | ({(code, 1) for code in BC.BAD_CODES} if cls != "odd" else set())
        assert set().union(*met[cls].values()) == halves, cls  # the 12 codes in the high and in the low half of a byte
    assert rounds == {0, 1, 2} and {0, 1, 63} <= lanes
    assert {recs[t]["pad"] for t in np.unique(cases["twin"]) if len(recs[t]["bases"]) & 1} == set(range(16))  # clean records of odd length with every padding code


def test_bam_quality_sweep_meets_every_class():
    recs, at = BC.qual_sweep_records()
    _bam_twin_check(recs, 4)
    body = b"".join(BC.record(**r) for r in recs)
    walked, _, bad, _ = BA.walk(body, True, 0x10)
    assert bad is None and len(walked) == len(recs) and {r["flag"] for r in recs} == {4, 0x10} and len(at) <= 160
    seen, word_lanes = set(), set()
    for c in at:
        w = walked[c["rec"]]
        cls, lane, rnd = IC.scan_class(w["qual_off"], w["l_seq"], int(c["pos"]))
        seen.add((cls, rnd) if cls == "aligned" else cls)
        if cls == "aligned":
            f, t = IC.middle(w["qual_off"], w["l_seq"])
            if c["pos"] < f + 16:
                seen.add("first 16")
            if c["pos"] >= t - 16:
                seen.add("last 16")
            word_lanes.add((w["qual_off"] + int(c["pos"])) % 4)
    assert seen >= {"front", "tail", "none", ("aligned", 0), ("aligned", 1), ("aligned", 2), "first 16", "last 16"} and word_lanes == {0, 1, 2, 3}
