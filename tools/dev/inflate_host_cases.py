"""Cases for tools/dev/inflate_host_check.cpp:
  inflate_host_cases.py <out.bin>            the texts and compressor forms of tests/bgzf_cases.py, the hand-written blocks,
                                             the refused inputs, 300 streams with flipped bits
  inflate_host_cases.py --generated <dir>    the corpus of tests/deflate_gen.py and the libdeflate fixtures of tests/golden,
                                             good and refused: <dir>/members.bin (the case format above), <dir>/segments.bin
                                             (the hand-made segments, for --segments) and <dir>/gzip/*.gz (for --gzip)"""
import os, sys, struct, zlib
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, ROOT)
import bgzf_cases as B
import numpy as np


def write_cases(path, cases):
    """cases: [(name, payload, None: good | (text_len, crc): refused | "fuzz")] -> the names that are not good"""
    out = [struct.pack("<I", len(cases))]
    names = []
    for i, (name, p, bad) in enumerate(cases):
        pre = i % 7
        if bad is None:
            text, crc = B.confirm_good(p); ok = 1; tl = len(text)
        elif bad == "fuzz":
            d = zlib.decompressobj(-15)
            try:
                text = d.decompress(p); ok = 1 if (d.eof and len(text) == 30000 and not d.unused_data) else 0
            except zlib.error:
                ok = 0; text = b""
            tl = 30000; crc = zlib.crc32(text)
            if not ok: text = b"\0" * tl
        else:
            tl, crc = bad; ok = 0; text = b"\0" * tl
        if name == "wrong_crc": ok = 2
        names.append((i, name, ok))
        out.append(struct.pack("<IIIII", len(p), tl, 1 if ok == 1 else 0, crc, pre) + b"\xee" * pre + p + text[:tl].ljust(tl, b"\0"))
    open(path, "wb").write(b"".join(out))
    return names


def classic_cases():
    cases = []
    T = B.texts()
    for tn, t in T.items():
        for fn, kw in B.FORMS.items():
            cases.append((tn + "/" + fn, B.deflate(t, **kw), None))
        cases.append((tn + "/flushed", B.flushed(t), None))
    for n, p in B.hand_written().items():
        cases.append((n, p, None))
    for n, (p, tl, crc) in B.refused().items():
        cases.append((n, p, (tl, crc)))
    # fuzz: random corruptions of good streams must never crash (status irrelevant unless zlib agrees on good)
    rng = np.random.default_rng(3)
    good = B.deflate(T["fastq"][:30000], 6)
    for i in range(300):
        b = bytearray(good)
        for _ in range(int(rng.integers(1, 4))):
            b[int(rng.integers(0, len(b)))] ^= 1 << int(rng.integers(0, 8))
        cases.append(("fuzz%d" % i, bytes(b), "fuzz"))
    return cases


def generated_cases():
    """the members of deflate_gen (random, match sweep, thresholds), of the libdeflate fixtures, the hand-written blocks and
    every refused input"""
    import deflate_gen as D
    cases = [(s.name, s.payload, None) for s in D.members() + D.match_sweep()[0] + [m for m, _ in D.threshold_members()]]
    for fn in ("libdeflate_members.bgzf", "tiny_libdeflate.fq.gz"):
        buf = open(os.path.join(ROOT, "tests", "golden", fn), "rb").read()
        blocks, consumed, why = B.walk_members(buf)
        assert consumed == len(buf) and why == 1
        cases += [("%s[%d]" % (fn, i), buf[o:o + n], None) for i, (o, n, _, _) in enumerate(blocks)]
    cases += [(n, p, None) for n, p in B.hand_written().items()]
    cases += [(n, p, (tl, crc)) for n, (p, tl, crc) in B.refused().items()]
    return cases


def write_segments(path):
    """the hand-made segments of deflate_gen, good and refused, for inflate_host_check --segments: u32 n; per segment u64
    comp_bit, u64 n_bits, u32 dict_len, u32 text_len, u32 crc, u32 flags, u32 expect_ok, u32 file_len, u32 pre (bytes in
    front of the history: its alignment); the file, pre + dict_len bytes, the text"""
    import deflate_gen as D
    segs = [(f, g, text, 1) for _, f, g, text in D.hand_segments()] + [(f, g, b"\0" * g["text_len"], 0) for f, g, _ in D.refused_segments().values()]
    out = [struct.pack("<I", len(segs))]
    for i, (f, g, text, ok) in enumerate(segs):
        pre = i % 4
        out.append(struct.pack("<QQIIIIIII", g["comp_bit"], g["n_bits"], len(g["dict"]), g["text_len"], g["crc32"], g["flags"], ok, len(f), pre) + f + b"\xee" * pre + g["dict"] + text)
    open(path, "wb").write(b"".join(out))
    return len(segs)


def write_generated(outdir):
    """-> (members.bin, segments.bin, [the gzip files])"""
    import deflate_gen as D
    os.makedirs(os.path.join(outdir, "gzip"), exist_ok=True)
    members, segments = os.path.join(outdir, "members.bin"), os.path.join(outdir, "segments.bin")
    write_cases(members, generated_cases())
    write_segments(segments)
    files = []
    for s in D.gzip_streams():
        files.append(os.path.join(outdir, "gzip", s.name + ".gz"))
        open(files[-1], "wb").write(s.payload)
    files.append(os.path.join(outdir, "gzip", "tiny_libdeflate.fq.gz"))
    open(files[-1], "wb").write(open(os.path.join(ROOT, "tests", "golden", "tiny_libdeflate.fq.gz"), "rb").read())
    return members, segments, files


if __name__ == "__main__":
    if sys.argv[1] == "--generated":
        members, segments, files = write_generated(sys.argv[2])
        print(members, segments, len(files), "gzip files")
    else:
        cases = classic_cases()
        names = write_cases(sys.argv[1], cases)
        print(len(cases), "cases;", sum(1 for n in names if n[2] == 1), "good")
        for i, n, ok in names:
            if ok != 1 and not n.startswith("fuzz"): print(i, n)
