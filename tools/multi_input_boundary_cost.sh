#!/bin/bash
# developer tool: what a file boundary costs the fill pass.  The same >= 2 GB of plain FASTQ text
# (tools/fqgen.c) as 1, 4 and 64 files through goldrush-path with GRP_TRACE_INGEST, three rounds, the three forms
# alternating inside a round.  Per run: wall seconds, the "fill pass" line and the fill pass's "source:" line (seconds
# waiting for the reader, parse calls).  usage: tools/multi_input_boundary_cost.sh [work dir] [reads] > report
set -euo pipefail
work=${1:-/tmp/grp_boundary}
reads=${2:-42000}
here=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$work"
gcc -O3 -fopenmp -o "$work/fqgen" "$here/tools/fqgen.c" -lm
"$work/fqgen" "$work/all.fq" "$reads" 8e6 7
python3 - "$work" <<'PY'
import os, sys
work = sys.argv[1]
data = open(os.path.join(work, "all.fq"), "rb").read()
print("text bytes", len(data))
for parts in (4, 64):
    names, at = [], 0
    for i in range(parts):
        end = len(data) if i == parts - 1 else data.index(b"\n@", len(data) * (i + 1) // parts) + 1  # (qualities are all '5': "\n@" begins a record)
        name = os.path.join(work, "p%d_%02d.fq" % (parts, i))
        open(name, "wb").write(data[at:end])
        names.append(name)
        at = end
    open(os.path.join(work, "p%d.fofn" % parts), "w").write("\n".join(names) + "\n")
PY
args="-k22 -w16 -t1000 -u5 -a1 -o0.1 -h3 -j16 -P10 -d5 -x10 -s1011011110110111101101 -g8e6 -b10 -m20000 --verbose"
for round in 1 2 3; do
  for form in 1 4 64; do
    if [ "$form" = 1 ]; then input="$work/all.fq"; else input="$work/p$form.fofn"; fi
    t0=$(date +%s.%N)
    GRP_TRACE_INGEST=1 timeout -k 10 300 "$here/goldrush_amd/bin/goldrush-path" $args -i "$input" -p "$work/out_$form" 2> "$work/err.txt"
    t1=$(date +%s.%N)
    echo "round $round files $form wall_s $(awk "BEGIN{print $t1 - $t0}") out_md5 $(md5sum < "$work/out_$form.fa" | cut -c1-12)"
    grep -E "^GRP_TRACE_INGEST (fill pass|source):" "$work/err.txt" | sed "s/^/  /"
  done
done
rm -rf "$work"
