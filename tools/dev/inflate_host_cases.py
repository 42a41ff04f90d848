"""Cases for tools/dev/inflate_host_check.cpp: usage inflate_host_cases.py <out.bin>"""
import os, sys, struct, zlib
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, ROOT)
import bgzf_cases as B
import numpy as np
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
open(sys.argv[1], "wb").write(b"".join(out))
print(len(cases), "cases;", sum(1 for n in names if n[2] == 1), "good")
for i, n, ok in names:
    if ok != 1 and not n.startswith("fuzz"): print(i, n)
