#!/usr/bin/env python3
"""GPU box: the drop-in binary end to end.

  tools/cli_end_to_end.py <out.json> [reads] [genome]

Writes a FASTQ of `reads` synthetic ONT-like reads (default 100 000 x 25 kb, G = 100e6: C1's
geometry, ~5 GB of text) and runs goldrush-path on it the way bin/goldrush does — process #1
(--silver_path -M 5 -r 0.9 -m 20000, bin/goldrush:253-260) and process #2 (golden path on the
silver reads, :240-248) — with the reads kept on the device between the passes (default) and with
the second parse (GRP_RESIDENT=off); every run twice, the faster one counts.  Wall time, the program's own phase timers, reads/s
FASTQ-inclusive; bench.py on the same geometry beside it.

  tools/cli_end_to_end.py --bgzf <out.json> [reads] [genome]

The same file BGZF-compressed (a writer of its own: zlib level 1, members of 65280 bytes of text, at most 16 processes):
the rate of the inflate kernels alone (grp_debug_bgzf_stats: text bytes / kernel time, the file's members in calls of one
ingest chunk of text), and process #1 end to end, three runs each, all kept — this tree on the BGZF file (the device
inflates), the same with GRP_BGZF=off (zlib), the binary named by CLI_E2E_PARENT on the BGZF file (the parent commit:
zlib), this tree and the parent on the plain file (the floor, and what the plain path pays).

  tools/cli_end_to_end.py --gzip <out.json> [reads] [genome]

The same file as ONE gzip member at zlib level 6 (written by up to 16 processes the way pigz -i does: pieces of 64 MiB
compressed on their own and joined by sync flushes; the blocks are what gzip -6 cuts, 30 to 36 KB of text each).  The
first pass over it goes through zlib and writes down restart points (csrc/host/gr_gzidx.cpp), the passes behind it inflate
the segments on the device.  Recorded: the rate of the segment kernels alone (grp_debug_gzip_stats over the segments of
the file's first GiB of text, in calls of one ingest chunk), the index's size, and process #1 end to end, three runs
each, all kept, with the program's phase timers and its GRP_TRACE_INGEST lines (one per pass: the seconds the pass waited
for its reader, the segments the device inflated) — this tree at the default span and at the spans in CLI_E2E_SPANS, this
tree with GRP_GZIP_INDEX=off, this tree on the plain and the BGZF file, and the binary named by CLI_E2E_PARENT (the parent
commit) on all three."""
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CLI = os.path.join(ROOT, "goldrush_amd", "bin", "goldrush-path")
SEED = "1011011110110111101101"
REPEATS = int(os.environ.get("CLI_E2E_REPEATS", "2"))


def run_cli(args, env=None):
    t0 = time.perf_counter()
    r = subprocess.run([CLI] + args, capture_output=True, text=True, env=dict(os.environ, **(env or {})))
    dt = time.perf_counter() - t0
    ins = [float(x) for x in re.findall(r"^in ([0-9.]+)$", r.stderr, re.M)]
    visited = re.findall(r"Visited (\d+) reads", r.stderr)
    res = {"rc": r.returncode, "wall_s": dt, "phase_timers_s": ins, "visited": int(visited[-1]) if visited else None, "stderr_tail": r.stderr[-300:] if r.returncode else ""}
    trace = [l for l in r.stderr.splitlines() if l.startswith("GRP_TRACE_INGEST source")]
    if trace:  # one line per pass over the input
        res["passes"] = [{"waiting_for_reader_s": float(re.search(r"waiting for the reader ([0-9.e+-]+)", l).group(1)), "bgzf_blocks": int(re.search(r"BGZF blocks inflated on the device (\d+)", l).group(1)),
                          "gzip_segments": int(m.group(1)) if (m := re.search(r"gzip segments inflated on the device (\d+)", l)) else None} for l in trace]
    return res


def _bgzf_piece(job):
    import struct
    import zlib

    path, off, n = job
    with open(path, "rb") as fh:
        fh.seek(off)
        text = fh.read(n)
    out = []
    for a in range(0, len(text), 65280):
        t = text[a:a + 65280]
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        p = c.compress(t) + c.flush()
        out.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(p) + 25) + p + struct.pack("<II", zlib.crc32(t), len(t)))
    return b"".join(out)


def write_bgzf(fq, gz):
    """BGZF of `fq`: pieces of 255 members compressed by up to 16 processes, written in order; then the empty end-of-file member"""
    from multiprocessing import Pool

    size, piece = os.path.getsize(fq), 255 * 65280
    jobs = [(fq, off, piece) for off in range(0, size, piece)]
    with Pool(min(16, len(os.sched_getaffinity(0)))) as pool, open(gz, "wb") as dst:
        for blob in pool.imap(_bgzf_piece, jobs, chunksize=1):
            dst.write(blob)
        dst.write(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))


def bgzf_mode(out, fq, n_reads, genome, res):
    import numpy as np

    from goldrush_amd import host, native

    tmp = os.path.dirname(fq)
    gz = fq + ".gz"
    t0 = time.perf_counter()
    write_bgzf(fq, gz)
    res["bgzf_bytes"] = os.path.getsize(gz)
    res["bgzf_written_s"] = time.perf_counter() - t0
    # the kernels alone: the file's members in calls of one ingest chunk (256 MiB) of text each
    chunk = 256 << 20
    eng = native.Engine(22, 3, 1000, 1 << 20, [SEED[:11] + "0" * i + SEED[11:] for i in range(3)])
    calls, t0 = 0, time.perf_counter()
    with open(gz, "rb") as fh:
        carry = b""
        while True:
            buf = carry + fh.read(64 << 20)
            if not buf:
                break
            blocks, consumed, why = host.bgzf_scan(buf, 1 << 16)
            assert blocks or not buf, "not a BGZF file"
            text = 0
            keep = []
            for b in blocks:
                if text + b[2] > chunk:
                    break
                keep.append(b)
                text += b[2]
            consumed = keep[-1][0] + keep[-1][1] + 8
            eng.bgzf_inflate(np.frombuffer(buf, dtype=np.uint8)[:consumed], keep)
            calls += 1
            carry = buf[consumed:]
    st = eng.bgzf_stats()
    eng.close()
    res["inflate_kernels"] = dict(st, calls=calls, text_GB_per_s=st["text_bytes"] / max(st["kernel_us"], 1) / 1e3, wall_s_with_copies_and_python=time.perf_counter() - t0,
                                  fill_pass_needs_text_GB_per_s=29.0)
    assert st["text_bytes"] == res["fastq_bytes"], (st, res["fastq_bytes"])
    base = ["-k22", "-w16", "-t1000", "-u5", "-a1", "-o0.1", "-h3", "-j16", "-P10", "-d5", "-x10", "-s" + SEED, "-g%d" % genome, "-b10", "--verbose"]
    pdir = os.path.join(tmp, "cli_e2e_out")
    os.makedirs(pdir, exist_ok=True)
    parent = os.environ.get("CLI_E2E_PARENT")
    global CLI
    this = CLI
    runs = [("this_tree/bgzf_device", this, gz, {}), ("this_tree/bgzf_zlib", this, gz, {"GRP_BGZF": "off"}), ("this_tree/plain", this, fq, {})]
    if parent:
        runs += [("parent/bgzf_zlib", parent, gz, {}), ("parent/plain", parent, fq, {})]
    outputs = {}
    for name, binary, path, env in runs:
        CLI = binary
        tag = name.replace("/", "_")
        three = [run_cli(base + ["-r0.9", "--silver_path", "-M5", "-m20000", "-i", path, "-p", os.path.join(pdir, tag)], dict(env, GRP_TRACE_INGEST="1")) for _ in range(3)]
        r = min(three, key=lambda x: x["wall_s"])
        r["wall_s_all"] = [round(x["wall_s"], 3) for x in three]
        r["text_GB_per_s_end_to_end"] = res["fastq_bytes"] / r["wall_s"] / 1e9
        res["runs"][name] = r
        import hashlib

        outputs[name] = {f: hashlib.sha256(open(os.path.join(pdir, f), "rb").read()).hexdigest() for f in sorted(os.listdir(pdir)) if f.startswith(tag + "_")}
        outputs[name] = sorted((f[len(tag):], h) for f, h in outputs[name].items())
    CLI = this
    res["outputs_identical"] = all(o == outputs["this_tree/plain"] and o for o in outputs.values())
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res, indent=1))
    os.remove(fq)
    os.remove(gz)


def _gzip_piece(job):
    import zlib

    path, off, n, last = job
    with open(path, "rb") as fh:
        fh.seek(off)
        text = fh.read(n)
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    return c.compress(text) + c.flush(zlib.Z_FINISH if last else zlib.Z_SYNC_FLUSH), zlib.crc32(text), len(text)


def write_gzip(fq, gz):
    """one gzip member at level 6: pieces of 64 MiB compressed by up to 16 processes, each ended by a sync flush, the last
    by the final block; the member's CRC32 is that of the file read once more"""
    import struct
    import zlib
    from multiprocessing import Pool

    size, piece = os.path.getsize(fq), 64 << 20
    jobs = [(fq, off, piece, off + piece >= size) for off in range(0, size, piece)]
    with Pool(min(16, len(os.sched_getaffinity(0)))) as pool, open(gz, "wb") as dst:
        dst.write(b"\x1f\x8b\x08\0\0\0\0\0\0\x03")
        for blob, _, _ in pool.imap(_gzip_piece, jobs, chunksize=1):
            dst.write(blob)
        crc = 0
        with open(fq, "rb") as fh:
            while True:
                buf = fh.read(64 << 20)
                if not buf:
                    break
                crc = zlib.crc32(buf, crc)
        dst.write(struct.pack("<II", crc, size & 0xffffffff))


def gzip_mode(out, fq, n_reads, genome, res):
    import hashlib

    import numpy as np

    from goldrush_amd import host, native

    tmp = os.path.dirname(fq)
    gz, bg = fq + ".gz", fq + ".bgzf.gz"
    t0 = time.perf_counter()
    write_gzip(fq, gz)
    res["gzip_bytes"] = os.path.getsize(gz)
    res["gzip_written_s"] = time.perf_counter() - t0
    write_bgzf(fq, bg)
    res["bgzf_bytes"] = os.path.getsize(bg)
    # the kernels alone: the segments of the first GiB of text at the default span, in calls of one ingest chunk of text
    span, chunk = 256 << 10, 256 << 20
    t0 = time.perf_counter()
    ix = host.gzip_index(gz, span, stop_after=1 << 30)
    res["index_first_GiB"] = {"span": span, "segments": len(ix["segments"]), "index_bytes": ix["index_bytes"], "text_bytes": sum(g["text_len"] for g in ix["segments"]),
                              "max_segment_text": ix["max_text"], "built_s_zlib_and_python": time.perf_counter() - t0}
    eng = native.Engine(22, 3, 1000, 1 << 20, [SEED[:11] + "0" * i + SEED[11:] for i in range(3)])
    comp_all = np.fromfile(gz, dtype=np.uint8, count=(ix["segments"][-1]["comp_bit"] + ix["segments"][-1]["n_bits"] + 7) // 8 if ix["segments"] else 0)
    calls, i, t0 = 0, 0, time.perf_counter()
    segs = ix["segments"]
    while i < len(segs):
        j, text = i, 0
        while j < len(segs) and text + segs[j]["text_len"] <= chunk:
            text += segs[j]["text_len"]
            j += 1
        b0 = segs[i]["comp_bit"] // 8
        b1 = (segs[j - 1]["comp_bit"] + segs[j - 1]["n_bits"] + 7) // 8
        hist, table = bytearray(), []
        for g in segs[i:j]:
            table.append((g["comp_bit"] - 8 * b0, g["n_bits"], len(hist), len(g["dict"]), g["text_len"], g["crc32"], g["flags"]))
            hist += g["dict"]
        eng.gzip_inflate(comp_all[b0:b1], bytes(hist), table)
        calls += 1
        i = j
    st = eng.gzip_stats()
    eng.close()
    res["inflate_kernels"] = dict(st, calls=calls, text_GB_per_s=st["text_bytes"] / max(st["kernel_us"], 1) / 1e3, wall_s_with_copies_and_python=time.perf_counter() - t0, bgzf_kernels_text_GB_per_s=8.4,
                                  fill_pass_needs_text_GB_per_s=29.0)
    del comp_all, ix, segs
    base = ["-k22", "-w16", "-t1000", "-u5", "-a1", "-o0.1", "-h3", "-j16", "-P10", "-d5", "-x10", "-s" + SEED, "-g%d" % genome, "-b10", "--verbose"]
    pdir = os.path.join(tmp, "cli_e2e_out")
    os.makedirs(pdir, exist_ok=True)
    parent = os.environ.get("CLI_E2E_PARENT")
    global CLI
    this = CLI
    runs = []
    if parent:  # (first: how much of its time falls in the passes behind the first bounds the gain)
        runs += [("parent/gzip_zlib", parent, gz, {}, 3)]
    runs += [("this_tree/gzip_device", this, gz, {}, 3), ("this_tree/gzip_zlib", this, gz, {"GRP_GZIP_INDEX": "off"}, 3)]
    runs += [("this_tree/gzip_device_span_%d" % int(v), this, gz, {"GRP_GZIP_SPAN": str(int(v))}, 2) for v in os.environ.get("CLI_E2E_SPANS", "").split(",") if v]
    runs += [("this_tree/plain", this, fq, {}, 3), ("this_tree/bgzf", this, bg, {}, 3)]
    if parent:
        runs += [("parent/plain", parent, fq, {}, 3), ("parent/bgzf", parent, bg, {}, 3)]
    only = [v for v in os.environ.get("CLI_E2E_ONLY", "").split(",") if v]  # (a second look at some of the runs; the plain file is the reference of the outputs)
    runs = [r for r in runs if not only or r[0] in only or r[0] == "this_tree/plain"]
    outputs = {}
    for name, binary, path, env, times in runs:
        CLI = binary
        tag = name.replace("/", "_")
        many = [run_cli(base + ["-r0.9", "--silver_path", "-M5", "-m20000", "-i", path, "-p", os.path.join(pdir, tag)], dict(env, GRP_TRACE_INGEST="1")) for _ in range(times)]
        r = min(many, key=lambda x: x["wall_s"])
        r["wall_s_all"] = [round(x["wall_s"], 3) for x in many]
        r["phase_timers_s_all"] = [x["phase_timers_s"] for x in many]
        r["waiting_for_reader_s_all"] = [[p["waiting_for_reader_s"] for p in x.get("passes", [])] for x in many]
        r["text_GB_per_s_end_to_end"] = res["fastq_bytes"] / r["wall_s"] / 1e9
        res["runs"][name] = r
        outputs[name] = sorted((f[len(tag):], hashlib.sha256(open(os.path.join(pdir, f), "rb").read()).hexdigest()) for f in sorted(os.listdir(pdir)) if f.startswith(tag + "_"))
        json.dump(res, open(out, "w"), indent=1)  # (what there is so far survives a time limit)
    CLI = this
    res["outputs_identical"] = all(o == outputs["this_tree/plain"] and o for o in outputs.values())
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res, indent=1))
    for f in (fq, gz, bg):
        os.remove(f)


def main():
    gzip_m = "--gzip" in sys.argv
    if gzip_m:
        sys.argv.remove("--gzip")
    bgzf = "--bgzf" in sys.argv
    if bgzf:
        sys.argv.remove("--bgzf")
    out = sys.argv[1]
    n_reads = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000
    genome = int(float(sys.argv[3])) if len(sys.argv) > 3 else 100_000_000
    from goldrush_amd import synth

    tmp = os.environ.get("TMPDIR", "/tmp")
    fq = os.path.join(tmp, "cli_e2e.fq")
    t0 = time.perf_counter()
    # tools/fqgen.c (OpenMP: the reads of a block made by all cores, written in order) where a C compiler is at hand — the
    # Python generator wrote C1's 51 GB in 227 s, most of a GPU call; the same read model either way
    gen = os.path.join(os.environ.get("FQGEN_DIR", "/tmp"), "fqgen")  # (not TMPDIR: /dev/shm is mounted noexec)
    built = subprocess.run(["gcc", "-O3", "-fopenmp", "-o", gen, os.path.join(ROOT, "tools", "fqgen.c"), "-lm"], capture_output=True).returncode == 0
    if built and subprocess.run([gen, fq, str(n_reads), str(genome), "1"], capture_output=True).returncode == 0:
        generator = "tools/fqgen.c"
    else:
        generator = "goldrush_amd/synth.py"
        g = synth.random_genome(genome, 1)
        with open(fq, "wb") as fh:
            done = 0
            while done < n_reads:  # in slices: the Python objects of 100 k reads would not fit comfortably
                n = min(5000, n_reads - done)
                for rid, seq, qual in synth.make_reads(g, n, mean_len=25000, min_len=20000, seed=2 + done):
                    fh.write(b"@r%d\n" % done + seq + b"\n+\n" + qual + b"\n")
                    done += 1
    size = os.path.getsize(fq)
    res = {"fastq_bytes": size, "reads": n_reads, "genome": genome, "fastq_written_s": time.perf_counter() - t0, "fastq_generator": generator, "runs": {}}
    if bgzf:
        return bgzf_mode(out, fq, n_reads, genome, res)
    if gzip_m:
        return gzip_mode(out, fq, n_reads, genome, res)
    base = ["-k22", "-w16", "-t1000", "-u5", "-a1", "-o0.1", "-h3", "-j16", "-P10", "-d5", "-x10", "-s" + SEED, "-g%d" % genome, "-b10", "--verbose"]
    pdir = os.path.join(tmp, "cli_e2e_out")
    os.makedirs(pdir, exist_ok=True)
    modes = [m for m in (("resident", {}), ("second_parse", {"GRP_RESIDENT": "off"})) if m[0] in os.environ.get("CLI_E2E_MODES", "resident,second_parse").split(",")]
    for mode, env in modes:
        for name, extra in (("silver_M5", ["-r0.9", "--silver_path", "-M5", "-m20000", "-i", fq, "-p", os.path.join(pdir, "sp_" + mode)]),
                            ("golden_on_raw_reads", ["-m20000", "-i", fq, "-p", os.path.join(pdir, "gp_" + mode)])):
            runs = [run_cli(base + extra, env) for _ in range(REPEATS)]  # the first run on a fresh box also pays the code-object load
            r = min(runs, key=lambda x: x["wall_s"])
            r["wall_s_all"] = [round(x["wall_s"], 3) for x in runs]
            r["reads_per_s_fastq_inclusive"] = (r["visited"] or n_reads) / r["wall_s"]
            r["fastq_GB_per_s"] = size / r["wall_s"] / 1e9
            res["runs"][name + "/" + mode] = r
    # the pipeline's chain (bin/goldrush:239-260): process #1 writes the silver paths, `cat <p1>_*.fq > <p1>_all.fq`,
    # process #2 builds the golden path FROM THAT FILE with -m 0 (round 4)
    sp = sorted(f for f in os.listdir(pdir) if re.fullmatch(r"sp_resident_\d+\.fq", f))
    if sp:
        allfq = os.path.join(pdir, "sp_all.fq")
        t_cat = time.perf_counter()
        with open(allfq, "wb") as dst:
            for f in sp:
                with open(os.path.join(pdir, f), "rb") as src:
                    while True:
                        buf = src.read(1 << 26)
                        if not buf:
                            break
                        dst.write(buf)
        t_cat = time.perf_counter() - t_cat
        n_silver = sum(1 for _ in open(allfq, "rb")) // 4
        runs = [run_cli(base + ["-m0", "-i", allfq, "-p", os.path.join(pdir, "gp_chain")]) for _ in range(REPEATS)]
        r = min(runs, key=lambda x: x["wall_s"])
        r["wall_s_all"] = [round(x["wall_s"], 3) for x in runs]
        r["input_reads"] = n_silver
        r["input_bytes"] = os.path.getsize(allfq)
        r["cat_s"] = t_cat
        r["reads_per_s_fastq_inclusive"] = n_silver / r["wall_s"]
        res["runs"]["golden_on_silver_paths/chain"] = r
        s1 = res["runs"].get("silver_M5/resident")
        if s1:
            res["pipeline_chain"] = {"what": "goldrush-path --silver_path -M 5 on the raw reads, cat of the silver paths, goldrush-path -m 0 on them (bin/goldrush:239-260)",
                                     "raw_reads": n_reads, "silver_reads": n_silver, "seconds": s1["wall_s"] + t_cat + r["wall_s"], "raw_reads_visited_by_process_1": s1["visited"]}
    # the outputs of the two forms are the same files
    same = True
    for f in sorted(os.listdir(pdir)):
        if "_resident" in f and len(modes) == 2:
            a, b = os.path.join(pdir, f), os.path.join(pdir, f.replace("_resident", "_second_parse"))
            same = same and os.path.exists(b) and open(a, "rb").read() == open(b, "rb").read()
    res["outputs_identical"] = same
    # the kernel path alone on the same geometry (GPU-resident synthetic reads, no text)
    b = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "C1", "--reads", str(n_reads), "--genome", str(genome), "--steps", "2", "--warmup", "1", "--no-cpu-baseline",
                        "--no-pipeline-shaped"], capture_output=True, text=True)
    try:
        line = json.loads([l for l in b.stdout.splitlines() if l.startswith("{")][-1])
        res["bench_same_geometry"] = {"reads_per_s": line["value"], "wall_s": line["aux"]["wall_s"], "fill_s": line["aux"]["fill_s"], "finalize_s": line["aux"]["finalize_s"]}
    except Exception as e:
        res["bench_same_geometry"] = {"error": str(e), "stderr": b.stderr[-500:]}
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res, indent=1))
    os.remove(fq)


if __name__ == "__main__":
    main()
