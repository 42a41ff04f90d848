"""GPU, at the C ABI: the calls a run on several files of mixed formats makes of ONE engine context — a final text chunk
that is followed by more chunks, the format changing from call to call, bodies handed over ahead across such a change, the
handle of the chunk before still alive while the next one is parsed.  Every record table (Phred sums bit for bit) and the
hashes of every pack equal those of a fresh engine that is given that one chunk alone."""
import numpy as np
import pytest

import bam_cases as BC
import bgzf_cases as B
import gzip_cases as G
from helpers import default_seeds
from test_gpu_bam import _records

pytestmark = pytest.mark.gpu

K, H = 22, 4
TILE = 25


def _engine(native):
    return native.Engine(K, H, TILE, 1 << 20, default_seeds(H))


def _arr(data):
    return np.frombuffer(data, dtype=np.uint8).copy()


def _sel(rec):
    return [i for i, r in enumerate(rec) if not (r["flags"] & 1) and r["seq_len"] >= TILE]


def _hashes(eng, fq, rec):
    sel = _sel(rec)
    batch = eng.fastq_pack(fq, sel, rec["seq_len"][sel])
    out = []
    for j, i in enumerate(sel):
        nt = int(rec["seq_len"][i]) // TILE
        out.append([eng.tile_hashes(batch, j, t).copy() for t in sorted({0, nt // 2, nt - 1})])
    return out


@pytest.fixture(scope="module")
def chunks(native, tmp_path_factory):
    """the records in five parts: text (no final newline), BAM records, the text of BGZF members, the text of gzip segments,
    BAM records again — and what a fresh engine makes of each"""
    from goldrush_amd import host

    recs = _records()
    cuts = [0, 14, 29, 43, 53, len(recs)]
    part = [recs[cuts[i]:cuts[i + 1]] for i in range(5)]
    twin = [BC.stream(p)[2] for p in part]
    body = [BC.stream(p)[0][BC.stream(p)[1]:] for p in part]
    c = {"text": twin[0][:-1], "bam1": body[1], "bgzf_text": twin[2], "gzip_text": twin[3], "bam2": body[4]}
    c["bgzf"] = B.bgzf_file(twin[2], [300, 500, 13])
    c["bgzf_blocks"] = B.walk_members(c["bgzf"])[0]
    assert len(c["bgzf_blocks"]) > 5
    p = tmp_path_factory.mktemp("switch") / "part.fq.gz"
    c["gzip"] = G.member(twin[3], 6, flush_every=1500)  # (block boundaries for the index to put its points on)
    p.write_bytes(c["gzip"])
    segs = host.gzip_index(p, 2000)["segments"]
    assert len(segs) > 2
    hist = b"".join(g["dict"] for g in segs)
    at, table = 0, []
    for g in segs:
        table.append((g["comp_bit"], g["n_bits"], at, len(g["dict"]), g["text_len"], g["crc32"], g["flags"]))
        at += len(g["dict"])
    c["gzip_hist"], c["gzip_table"] = hist, table
    want = {}
    for name, kind in (("text", "fastq"), ("bam1", "bam"), ("bgzf_text", "fastq"), ("gzip_text", "fastq"), ("bam2", "bam")):
        e = _engine(native)
        if kind == "bam":
            fq, rec, used = e.bam_parse(c[name])
        else:
            fq, rec, used, stopped = e.fastq_parse(c[name])
            assert not stopped
        assert used == len(c[name]) and len(rec) == len(part[("text", "bam1", "bgzf_text", "gzip_text", "bam2").index(name)])
        want[name] = (rec.copy(), _hashes(e, fq, rec))
        assert want[name][1], name
        e.fastq_free(fq)
        e.close()
    return c, want


def _check(eng, fq, rec, want, what):
    assert rec.tobytes() == want[0].tobytes(), what  # (the sums as bits)
    got = _hashes(eng, fq, rec)
    assert len(got) == len(want[1]), what
    for g, w in zip(got, want[1]):
        assert len(g) == len(w) and all(np.array_equal(a, b) for a, b in zip(g, w)), what


def test_the_sequence_of_a_mixed_run_on_one_context(native, chunks):
    c, want = chunks
    eng = _engine(native)
    try:
        room = 4096
        text = np.zeros(room + len(c["text"]), dtype=np.uint8)
        text[room:] = _arr(c["text"])
        bam1 = _arr(c["bam1"])
        # the bodies of the file's last chunk and of the next file's first, handed over while the text is still unparsed
        assert eng.fastq_prefetch(text[room:], len(c["text"]))
        assert eng.fastq_prefetch(bam1, bam1.size)
        # a final chunk — its last line has no newline — that is followed by more chunks
        f_text, r_text, used, stopped = eng.fastq_parse_at(text[room:], len(c["text"]), final_chunk=True)
        assert used == len(c["text"]) and not stopped
        # the next file is BAM: parsed with the text's handle alive
        f_bam1, r_bam1, used = eng.bam_parse(bam1, final_chunk=True)
        assert used == bam1.size
        _check(eng, f_text, r_text, want["text"], "text")
        eng.fastq_free(f_text)
        # BGZF members inflated, their text parsed
        z_text = eng.bgzf_inflate(c["bgzf"], c["bgzf_blocks"])
        assert z_text == c["bgzf_text"]
        z_buf = _arr(z_text)
        f_bgzf, r_bgzf, used, stopped = eng.fastq_parse_at(z_buf, z_buf.size, final_chunk=True)
        assert used == z_buf.size and not stopped
        _check(eng, f_bam1, r_bam1, want["bam1"], "bam1")
        eng.fastq_free(f_bam1)
        # gzip segments inflated, their text parsed — with the body of the BAM chunk behind it handed over first: it is not
        # this parse's, so the engine drops it and the BAM parse uploads its bytes itself
        g_text = eng.gzip_inflate(c["gzip"], c["gzip_hist"], c["gzip_table"])
        assert g_text == c["gzip_text"]
        g_buf = _arr(g_text)
        bam2 = _arr(c["bam2"])
        assert eng.fastq_prefetch(bam2, bam2.size)
        f_gzip, r_gzip, used, stopped = eng.fastq_parse_at(g_buf, g_buf.size, final_chunk=True)
        assert used == g_buf.size and not stopped
        _check(eng, f_bgzf, r_bgzf, want["bgzf_text"], "bgzf")
        eng.fastq_free(f_bgzf)
        f_bam2, r_bam2, used = eng.bam_parse(bam2, final_chunk=True)
        assert used == bam2.size
        _check(eng, f_gzip, r_gzip, want["gzip_text"], "gzip")
        eng.fastq_free(f_gzip)
        _check(eng, f_bam2, r_bam2, want["bam2"], "bam2")
        eng.fastq_free(f_bam2)
        assert eng.fastq_prefetch(None, 0)
    finally:
        eng.close()
