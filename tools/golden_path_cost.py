#!/usr/bin/env python3
"""developer tool: what the hand-over between the two goldrush-path stages costs.  The same plain FASTQ
(tools/fqgen.c) through three forms, three rounds, the forms alternating inside a round:
  two_runs   process #1 (--silver_path), `cat`, process #2 (-m 0) — the pipeline as it was (a command without
             --golden_path runs the code it ran before the option existed)
  files      one run with --golden_path, GRP_GOLDEN_RESIDENT=off: the second stage reads the silver files back
  device     one run with --golden_path: the silver reads are handed over on the device
Per run: wall seconds of the whole form, and the seconds of the second stage from its start (the second process's start,
the first line the second stage prints) to its "assigning tiles" line — engine set-up, Phred pass, fill, finalize: what the
hand-over changes.  The golden path's md5 is printed to show that the forms agree.
usage: tools/golden_path_cost.py [work dir] [reads] [genome] > report"""
import hashlib
import os
import shutil
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(HERE, "goldrush_amd", "bin", "goldrush-path")


def run(args, env):
    """-> (wall seconds, [(seconds since start, stderr line)])"""
    t0 = time.time()
    p = subprocess.Popen([CLI] + args, stderr=subprocess.PIPE, stdout=subprocess.DEVNULL, text=True, env=env)
    lines = [(time.time() - t0, l.rstrip("\n")) for l in p.stderr]
    rc = p.wait(timeout=600)
    if rc != 0:
        sys.exit("goldrush-path %s: exit %d\n%s" % (" ".join(args), rc, "\n".join(l for _, l in lines[-20:])))
    return time.time() - t0, lines


def at(lines, text, nth):
    hits = [t for t, l in lines if l == text]
    return hits[nth]


def main():
    work = sys.argv[1] if len(sys.argv) > 1 else "/tmp/grp_golden_cost"
    reads = sys.argv[2] if len(sys.argv) > 2 else "20000"
    genome = sys.argv[3] if len(sys.argv) > 3 else "5e7"
    os.makedirs(work, exist_ok=True)
    subprocess.run(["gcc", "-O3", "-fopenmp", "-o", work + "/fqgen", HERE + "/tools/fqgen.c", "-lm"], check=True)
    subprocess.run([work + "/fqgen", work + "/all.fq", reads, genome, "7"], check=True)
    print("reads", reads, "genome", genome, "text bytes", os.path.getsize(work + "/all.fq"))
    common = "-k22 -w16 -t1000 -u5 -a1 -o0.1 -h3 -j16 -P10 -d5 -x10 -s1011011110110111101101 -b10 --verbose".split() + ["-g" + genome]
    silver = common + ["-r0.9", "--silver_path", "-M3", "-m20000", "-i", work + "/all.fq"]
    env = dict(os.environ, GRP_TRACE_INGEST="1")
    env.pop("GRP_GOLDEN_RESIDENT", None)
    for rnd in (1, 2, 3):
        for form in ("two_runs", "files", "device"):
            d = os.path.join(work, form)
            shutil.rmtree(d, ignore_errors=True)
            os.makedirs(d)
            if form == "two_runs":
                t0 = time.time()
                _, _ = run(silver + ["-p", d + "/out"], env)
                names = sorted((f for f in os.listdir(d) if f.endswith(".fq") and os.path.getsize(d + "/" + f)), key=lambda f: f.encode())
                with open(d + "/all_silver.fq", "wb") as out:
                    for f in names:
                        with open(d + "/" + f, "rb") as src:
                            shutil.copyfileobj(src, out, 1 << 24)
                silver_bytes = os.path.getsize(d + "/all_silver.fq")
                _, lines = run(common + ["-m0", "-i", d + "/all_silver.fq", "-p", d + "/gold"], env)
                wall = time.time() - t0
                stage_b = at(lines, "assigning tiles", 0)
            else:
                e = dict(env, GRP_GOLDEN_RESIDENT="off") if form == "files" else env
                wall, lines = run(silver + ["-p", d + "/out", "--golden_path", d + "/gold"], e)
                first = lines[0][1]  # a stage's first line: its second occurrence is where the second stage starts
                stage_b = at(lines, "assigning tiles", 1) - at(lines, first, 1)
            md5 = hashlib.md5(open(d + "/gold.fa", "rb").read()).hexdigest()[:12]
            trace = [l for _, l in lines if l.startswith("GRP_TRACE_INGEST golden:")]
            print("round %d form %-8s wall_s %.2f stage_b_to_assigning_tiles_s %.2f silver_bytes %d golden_md5 %s %s" % (rnd, form, wall, stage_b, silver_bytes, md5, trace[0] if trace else ""), flush=True)
    shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
