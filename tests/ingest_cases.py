"""FASTQ texts for the edge sweeps of the device ingest (csrc/grp_ingest.inc) and an independent host model of what the
ingest reports for them: plain Python / numpy, no engine.

The model: host_parse (the host reader's rules, csrc/host/gr_fastq.cpp: 4-line records, rtrim of CR / blank / tab, the id
cut at the first white space) + the ACGT flag + the Phred sums (the caller hands in the host library's gr_sum_phred) and
what grp_fastq_parse says about the bytes it consumed.  table_np restates it with numpy expressions for the one text that
is too large for a loop; tests/test_ingest_cases_cpu.py holds the two against each other and against the oracle's reader.

The texts:
  S1  length x alignment   every length 0..330 and the lengths round 1024 and 2048, each at all 16 values of seq_off % 16
  S2  one bad byte         every position of short records, the edges of the aligned middle of long ones, ~60 byte values
  S3  degenerate lines     empty lines, '@' alone, long runs of trailing white space, unequal lengths
  S4  the newline index    cuts round the 4096-byte blocks, blocks without and full of newlines, 8 MiB for the scan's carries
"""
import numpy as np

RECORD_DTYPE = np.dtype([("id_off", "<u8"), ("seq_off", "<u8"), ("qual_off", "<u8"), ("id_len", "<u4"), ("seq_len", "<u4"),
                         ("qual_len", "<u4"), ("flags", "<u4"), ("phred_sum", "<f8"), ("phred_first", "<f8")])
NON_ACGT = 1  # GRP_FQ_NON_ACGT
ACGT = b"ACGTacgt"
NL_BLOCK = 4096  # bytes per workgroup of k_nl_count / k_nl_scatter
SCAN_ROUND = 1024  # blocks per round of k_scan_chunks

_ACGT_U = np.frombuffer(b"ACGT", dtype=np.uint8)


# ---- the model ------------------------------------------------------------------------------------------------------------

def split_lines(text: bytes, final=True):
    """[(start, position of the line's newline)]; a final text's last line without a newline gets a virtual one at len(text)"""
    lines, pos = [], 0
    while True:
        nl = text.find(b"\n", pos)
        if nl < 0:
            if final and pos < len(text):
                lines.append((pos, len(text)))
            break
        lines.append((pos, nl))
        pos = nl + 1
    return lines


def host_parse(text: bytes, final=True):
    """The host reader's semantics (gr_fastq.cpp): 4-line records, rtrim of CR / blank / tab,
    id up to the first whitespace; stops at a header that does not start with '@'.
    -> ([(id_off, id_len, seq_off, seq_len, qual_off, qual_len)], stopped)"""
    lines = split_lines(text, final)
    recs = []
    for r in range(len(lines) // 4):
        ext = []
        for s, e in lines[4 * r: 4 * r + 4]:
            while e > s and text[e - 1:e] in (b"\r", b" ", b"\t"):
                e -= 1
            ext.append((s, e))
        (hs, he), (ss, se), _, (qs, qe) = ext
        if he == hs or text[hs:hs + 1] != b"@":
            return recs, True
        ie = hs + 1
        while ie < he and not text[ie:ie + 1].isspace():
            ie += 1
        recs.append((hs + 1, ie - hs - 1, ss, se - ss, qs, qe - qs))
    return recs, False


def consumed(text: bytes, final, stopped):
    """bytes_consumed of grp_fastq_parse: up to and with the newline of the last complete record (a virtual one is no byte);
    everything where the reader stopped at a header that is none; nothing without a complete record"""
    lines = split_lines(text, final)
    n_rec = len(lines) // 4
    if n_rec == 0:
        return 0
    return len(text) if stopped else min(lines[4 * n_rec - 1][1] + 1, len(text))


class PhredCache:
    """sum_phred(bytes) -> float (the host library's gr_sum_phred), asked once per distinct line"""

    def __init__(self, sum_phred):
        self.f, self.seen = sum_phred, {}

    def __call__(self, q: bytes):
        v = self.seen.get(q)
        if v is None:
            v = self.seen[q] = self.f(q)
        return v


def _fill(table, text, sum_phred):
    for i in range(len(table)):
        qo, qn = int(table["qual_off"][i]), int(table["qual_len"][i])
        q = text[qo:qo + qn]
        table["phred_sum"][i] = sum_phred(q)
        table["phred_first"][i] = sum_phred(q[:qn // 2]) if qn >= 2 else 0.0


def model_table(text: bytes, sum_phred, final=True):
    """-> (the record table the ingest reports, bytes_consumed, stopped)"""
    recs, stopped = host_parse(text, final)
    table = np.zeros(len(recs), dtype=RECORD_DTYPE)
    for i, (io, il, so, sl, qo, ql) in enumerate(recs):
        table[i] = (io, so, qo, il, sl, ql, NON_ACGT if text[so:so + sl].translate(None, ACGT) else 0, 0.0, 0.0)
    _fill(table, text, sum_phred)
    return table, consumed(text, final, stopped), stopped


def table_np(text: bytes, sum_phred, final=True):
    """model_table in numpy expressions over the whole text (the 8 MiB text of S4)"""
    a = np.frombuffer(text, dtype=np.uint8)
    n = a.size
    nl = np.flatnonzero(a == 10).astype(np.int64)
    if final and n and a[-1] != 10:
        nl = np.append(nl, n)
    n_rec = nl.size // 4
    if n_rec == 0:
        return np.zeros(0, dtype=RECORD_DTYPE), 0, False
    nl = nl[:4 * n_rec]
    starts = np.concatenate([[0], nl[:-1] + 1])
    ends = nl.copy()
    trim = np.zeros(256, dtype=bool)
    trim[[9, 13, 32]] = True
    while True:
        m = ends > starts
        m[m] = trim[a[ends[m] - 1]]
        if not m.any():
            break
        ends[m] -= 1
    hs, he, ss, se, qs, qe = starts[0::4], ends[0::4], starts[1::4], ends[1::4], starts[3::4], ends[3::4]
    bad = (he == hs) | (a[np.minimum(hs, n - 1)] != ord("@"))
    stopped = bool(bad.any())
    keep = int(np.argmax(bad)) if stopped else n_rec
    space = np.flatnonzero((a == 32) | ((a >= 9) & (a <= 13)))
    at = np.searchsorted(space, hs + 1)
    first = np.where(at < space.size, space[np.minimum(at, max(space.size - 1, 0))] if space.size else n, n)
    ie = np.minimum(first, he)
    other = np.concatenate([[0], np.cumsum(~np.isin(a, np.frombuffer(ACGT, dtype=np.uint8)))])
    table = np.zeros(n_rec, dtype=RECORD_DTYPE)
    table["id_off"], table["id_len"] = hs + 1, np.maximum(ie - hs - 1, 0)
    table["seq_off"], table["seq_len"] = ss, se - ss
    table["qual_off"], table["qual_len"] = qs, qe - qs
    table["flags"] = np.where(other[se] - other[ss] > 0, NON_ACGT, 0)
    table = table[:keep].copy()
    _fill(table, text, sum_phred)
    return table, (n if stopped else min(int(nl[-1]) + 1, n)), stopped


def table_diff(got, exp):
    """the first difference of two record tables, field by field, doubles as bit patterns (None: they are equal)"""
    if len(got) != len(exp):
        return "records: %d, expected %d" % (len(got), len(exp))
    for f in RECORD_DTYPE.names:
        g, e = np.ascontiguousarray(got[f]), np.ascontiguousarray(exp[f])
        if g.dtype.kind == "f":
            g, e = g.view(np.uint64), e.view(np.uint64)
        d = np.flatnonzero(g != e)
        if d.size:
            i = int(d[0])
            return "%s of record %d (of %d that differ): %r, expected %r; the record: %r" % (f, i, d.size, got[f][i], exp[f][i], exp[i])
    return None


def upper_strings(text: bytes, table):
    """the sequence lines of a table, upper-cased: what native.pack_reads packs"""
    return [text[int(o):int(o) + int(n)].upper() for o, n in zip(table["seq_off"], table["seq_len"])]


# ---- the kernels' geometry, for the coverage assertions ------------------------------------------------------------------

def middle(s0, n):
    """(a0 - s0, a1 - s0) of the bytes [s0, s0 + n): the aligned middle as k_fq_records / bam_scan_bad compute it"""
    return (-s0) % 16, n - (s0 + n) % 16


def scan_class(s0, n, p):
    """where byte p of [s0, s0 + n) is tested: ("front" | "tail" | "none", 0, 0) or ("aligned", lane, round)"""
    f, t = middle(s0, n)
    if f >= t:
        return "none", 0, 0
    if p < f:
        return "front", 0, 0
    if p >= t:
        return "tail", 0, 0
    return "aligned", (p - f) // 16 % 64, (p - f) // 1024


def phred_lines(addr, n):
    """whole 64-byte lines of phred_chain over n bytes at address addr, behind its prologue up to a 16-byte boundary"""
    return (n - min((-addr) % 16, n)) // 64


# ---- S1: length x alignment -------------------------------------------------------------------------------------------

S1_LENGTHS = list(range(331)) + [1023, 1024, 1025, 1039, 1040, 1041, 2047, 2048, 2049, 2063, 2064, 2065]


def steered_header(tag: bytes, pos: int, want: int):
    """a header at text[pos] whose comment has the length that puts the sequence line at want (mod 16)"""
    k = (want - (pos + len(tag) + 4)) % 16
    hdr = b"@" + tag + b" " + b"c" * (k + 1)
    assert (pos + len(hdr) + 1) % 16 == want
    return hdr


def s1_text(seed=101, lengths=None, aligns=range(16)):
    """-> (text, lengths per record, seq_off % 16 per record)"""
    rng = np.random.default_rng(seed)
    parts, pos, i, ls, al = [], 0, 0, [], []
    for L in S1_LENGTHS if lengths is None else lengths:
        for a in aligns:
            seq = _ACGT_U[rng.integers(0, 4, size=L)]
            if i % 3 == 2:  # every third record in lower or in mixed case
                seq = seq | (np.uint8(32) if (i // 3) % 2 else (rng.integers(0, 2, size=L).astype(np.uint8) << 5))
            qual = (b"!" * L if i % 11 == 4 else b"~" * L if i % 11 == 9 else rng.integers(33, 127, size=L).astype(np.uint8).tobytes())
            rec = steered_header(b"r%d" % i, pos, a) + b"\n" + seq.astype(np.uint8).tobytes() + b"\n+\n" + qual + b"\n"
            parts.append(rec)
            pos += len(rec)
            ls.append(L)
            al.append(a)
            i += 1
    return b"".join(parts), np.array(ls), np.array(al)


# ---- S2: one bad byte per record --------------------------------------------------------------------------------------

def bad_bytes():
    """N n U R, '@' and a backtick, 0x01 and 0xC1, every other byte one bit away from one of ACGTacgt, blank, tab, CR"""
    out = [ord(c) for c in "NnUR@`"] + [0x01, 0xC1]
    for c in ACGT:
        for bit in range(8):
            b = c ^ (1 << bit)
            if b not in ACGT and b not in out:
                out.append(b)
    assert not set(out) & {10, 32, 9, 13}
    return out + [32, 9, 13]


S2_SHORT = list(range(1, 50))
S2_LONG = list(range(1023, 1042)) + [2064]
S2_KINDS = ["every", "0", "1", "a0-1", "a0", "a0+15", "a0+16", "a0+1023", "a0+1024", "a1-1", "a1", "L-2", "L-1"]
S2_CASE = np.dtype([("rec", "<i8"), ("twin", "<i8"), ("len", "<i4"), ("align", "<i4"), ("pos", "<i4"), ("byte", "<i4"), ("kind", "<i4")])
_QPOOL = np.random.default_rng(7).integers(33, 127, size=5000).astype(np.uint8).tobytes()


def edge_positions(s0, n):
    """[(kind, position)] of the swept positions of the bytes [s0, s0 + n), those inside it"""
    f, t = middle(s0, n)
    want = [("0", 0), ("1", 1), ("a0-1", f - 1), ("a0", f), ("a0+15", f + 15), ("a0+16", f + 16), ("a0+1023", f + 1023), ("a0+1024", f + 1024),
            ("a1-1", t - 1), ("a1", t), ("L-2", n - 2), ("L-1", n - 1)]
    return [(k, p) for k, p in want if 0 <= p < n]


def s2_text(seed=102, short=None, long=None, aligns=range(16)):
    """-> (text, cases[S2_CASE]): a clean record per (length, alignment), behind it one copy per planted position with that
    one byte replaced; the bad byte takes its values in turn"""
    rng = np.random.default_rng(seed)
    values = bad_bytes()
    parts, cases, pos, n_rec, turn = [], [], 0, 0, 0

    def put(seq, L):
        nonlocal pos, n_rec
        rec = steered_header(b"b%d" % n_rec, pos, a) + b"\n" + bytes(seq) + b"\n+\n" + _QPOOL[:L] + b"\n"
        parts.append(rec)
        pos += len(rec)
        n_rec += 1
        return n_rec - 1

    for lengths, every in ((S2_SHORT if short is None else short, True), (S2_LONG if long is None else long, False)):
        for L in lengths:
            for a in aligns:
                clean = bytearray(_ACGT_U[rng.integers(0, 4, size=L)].tobytes())
                twin = put(clean, L)
                for kind, p in ([("every", p) for p in range(L)] if every else edge_positions(a, L)):
                    seq = bytearray(clean)
                    seq[p] = values[turn % len(values)]
                    cases.append((put(seq, L), twin, L, a, p, seq[p], S2_KINDS.index(kind)))
                    turn += 1
    return b"".join(parts), np.array(cases, dtype=S2_CASE)


# ---- S3: degenerate lines ---------------------------------------------------------------------------------------------

def _ws_run(n, k):
    return bytes(b"\r \t"[(i * (k + 1) + i // 3 + k) % 3] for i in range(n))


def s3_records():
    """[(what, the record's four lines with their newlines)]"""
    out = [("empty sequence and quality", b"@e\n\n+\n\n"),
           ("'@' alone, all empty", b"@\n\n+\n\n"),
           ("'@' alone", b"@\nACGT\n+\nIIII\n"),
           ("'@ x': an empty id", b"@ x\nACGTA\n+\nIIIII\n"),
           ("'@' and white space only", b"@ \t \nAC\n+\nII\n"),
           ("a header of 300 bytes", b"@" + b"h" * 299 + b"\nACGTACGTAC\n+\n" + b"5" * 10 + b"\n"),
           ("a header of 300 bytes with a comment", b"@" + b"h" * 150 + b"\t" + b"k" * 148 + b"\nACGTACGTAC\n+\n" + b"5" * 10 + b"\n"),
           ("text behind the '+'", b"@p\nACGT\n+p some text\nIIII\n"),
           ("the '+' line is something else", b"@q\nACGT\n@q\nIIII\n"),
           ("a quality line that begins with '@'", b"@a\nACGTAC\n+\n@IIIII\n"),
           ("quality shorter than the sequence", b"@s\nACGTACGTACGTACGTACGT\n+\nIII\n"),
           ("quality longer than the sequence", b"@l\nACG\n+\n" + b"I" * 40 + b"\n"),
           ("quality of one", b"@o\nA\n+\nI\n"),
           ("no quality", b"@n\nACGT\n+\n\n"),
           ("no sequence", b"@m\n\n+\nIIII\n"),
           ("a blank inside the sequence", b"@w\nACGT ACGT\n+\nIIIIIIIII\n"),
           ("a tab and a CR inside the sequence", b"@x\nAC\tGT\rAC\n+\nIIIIIIII\n"),
           ("a sequence line of white space", b"@y\n \t\r \n+\nII\n"),
           ("a quality line of white space", b"@z\nAC\n+\n\t\t \r\n")]
    for ch in (9, 11, 12, 13, 32):
        out.append(("the id ends at byte %d" % ch, b"@id%d" % ch + bytes([ch]) + b"rest\nACGT\n+\nIIII\n"))
    for n in range(1, 18):
        h, s, q = _ws_run(n, 0), _ws_run(n, 1), _ws_run(n, 2)
        out.append(("%d trailing on the header" % n, b"@t%d" % n + h + b"\nACGTT\n+\nIIIII\n"))
        out.append(("%d trailing on the sequence" % n, b"@u%d\nACGTT" % n + s + b"\n+\nIIIII\n"))
        out.append(("%d trailing on the quality" % n, b"@v%d\nACGTT\n+\nIIIII" % n + q + b"\n"))
        out.append(("%d trailing on all four" % n, b"@w%d c" % n + s + b"\nacgtt" + q + b"\n+" + h + b"\n!!~~5" + s + b"\n"))
    return out


def s3_text():
    recs = s3_records()
    return b"".join(r for _, r in recs), [w for w, _ in recs]


# ---- S4: the newline index --------------------------------------------------------------------------------------------

def _short_records(n, first=0):
    """records of 1 to 7 bases under two-byte headers: a line ends every few bytes"""
    return [b"@%c\n" % (97 + (first + i) % 26) + b"ACGTACG"[:1 + (first + i) % 7] + b"\n+\n" + b"IJKLMNO"[:1 + (first + i) % 7] + b"\n" for i in range(n)]


S4_CUTS = list(range(4080, 4113)) + list(range(8176, 8209))  # every size mod 16 twice round 4095 / 4096 / 4097 and 8191 / 8192 / 8193


def s4_small():
    """[(what, text, final_chunk)]"""
    base = b"".join(_short_records(700))
    assert len(base) > S4_CUTS[-1] + 16
    out = []
    for n in S4_CUTS:
        out.append(("cut at %d, as it falls" % n, base[:n], True))
        out.append(("cut at %d, a newline last" % n, base[:n - 1] + b"\n", True))
        out.append(("cut at %d, more to come" % n, base[:n], False))
    for edge in (NL_BLOCK, 2 * NL_BLOCK):
        # the header's newline on a block's last byte, the (empty) sequence line's on the first byte of the next block
        head = b""
        for rec in _short_records(edge // 8):
            if len(head) + len(rec) > edge - 40:
                break
            head += rec
        hdr = b"@edge " + b"c" * (edge - 1 - len(head) - 6)
        text = head + hdr + b"\n\n+\n\n" + b"".join(_short_records(5))
        assert text[edge - 1:edge + 1] == b"\n\n" and text[edge - 2] != 10
        out.append(("newlines at %d and %d" % (edge - 1, edge), text, True))
    rng = np.random.default_rng(104)
    long_seq = _ACGT_U[rng.integers(0, 4, size=9000)].tobytes()
    front = b"".join(_short_records(266))  # the long line begins a little in front of a block boundary: two whole blocks lie inside it
    assert NL_BLOCK - 200 < len(front) + 6 < NL_BLOCK
    out.append(("lines of 9000 bytes", front + b"@long\n" + long_seq + b"\n+\n" + _QPOOL[:4500] * 2 + b"\n@b\nAC\n+\nII\n", True))
    dense = b"@\n\n+\n\n" * 1400  # 8400 bytes, two of three are newlines: every 16-byte group of two whole blocks holds 10 or 11
    out.append(("'@', '+' and newlines only", dense, True))
    out.append(("... and 48 newlines behind them", b"@\n\n+\n\n" * 8 + b"\n" * 48 + b"@c\nAC\n+\nII\n", True))
    out.append(("... without the last newline", dense + b"@z\nAC\n+\nII", True))
    return out


S4_BIG_BYTES = 2 * SCAN_ROUND * NL_BLOCK + 5 * NL_BLOCK  # 2053 blocks: two carries of the scan


def s4_big(seed=105):
    """A little over 8 MiB: records of 2000 bases, and runs of short records (a newline every few bytes) over the 24 KiB
    round the 1024th and the 2048th block boundary, where the scan's carry is taken.  No trailing white space."""
    rng = np.random.default_rng(seed)
    parts, pos, i = [], 0, 0
    edges = (SCAN_ROUND * NL_BLOCK, 2 * SCAN_ROUND * NL_BLOCK)
    while pos < S4_BIG_BYTES:
        if any(e - 3 * NL_BLOCK <= pos < e + 3 * NL_BLOCK for e in edges):
            rec = b"".join(_short_records(64, i))
        else:
            L = 1990 + i % 21
            off = (i * 37) % 8
            rec = b"@g%d l=%d\n" % (i, L) + _ACGT_U[rng.integers(0, 4, size=L)].tobytes() + b"\n+\n" + _QPOOL[off:off + L] + b"\n"
        parts.append(rec)
        pos += len(rec)
        i += 1
    return b"".join(parts)


def block_newlines(text: bytes):
    """newlines per 4096-byte block"""
    a = np.frombuffer(text, dtype=np.uint8) == 10
    pad = (-a.size) % NL_BLOCK
    return np.concatenate([a, np.zeros(pad, dtype=bool)]).reshape(-1, NL_BLOCK).sum(axis=1)
