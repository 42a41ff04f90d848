#!/bin/bash
# developer tool: what walking the members of ONE concatenated gzip file side by side buys (DESIGN §8 N1c', §6).  About 2 GB
# of tools/fqgen.c text as one .fq.gz of 64 members (cut inside records, level 6) through goldrush-path with
# GRP_TRACE_INGEST, three rounds, the forms alternating inside a round:
#   zlib      neither switch: the first pass reads the file through zlib and builds the index
#   walk      GRP_GZIP_WALK=on: the walk's serial form, one wave, a member after the other
#   members   GRP_GZIP_WALK=on GRP_GZIP_WALK_MEMBERS=on
#   before    GRP_GZIP_WALK=on with the binary of the commit before the members switch, where BEFORE_BIN names one
# Per run: wall seconds, the md5 of the golden path, the "gzip walk" lines and the first pass's "source:" line.
# usage: tools/gzip_members_cost.sh [work dir] [reads] > report
set -euo pipefail
work=${1:-/tmp/grp_members}
reads=${2:-42000}
here=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$work"
gcc -O3 -fopenmp -o "$work/fqgen" "$here/tools/fqgen.c" -lm
"$work/fqgen" "$work/all.fq" "$reads" 8e6 7
python3 - "$work" <<'PY'
import multiprocessing, os, sys, zlib
work = sys.argv[1]
data = open(os.path.join(work, "all.fq"), "rb").read()
cuts = [len(data) * i // 64 + (977 * i) % 4001 for i in range(64)] + [len(data)]  # (inside records, wherever they fall)
cuts[0] = 0


def member(i):
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    return c.compress(data[cuts[i]:cuts[i + 1]]) + c.flush()


with multiprocessing.Pool(min(16, os.cpu_count() or 1)) as pool:
    parts = pool.map(member, range(64))
open(os.path.join(work, "all.fq.gz"), "wb").write(b"".join(parts))
print("text bytes", len(data), "compressed bytes", sum(len(p) for p in parts), "members", len(parts))
PY
rm -f "$work/all.fq"
args="-k22 -w16 -t1000 -u5 -a1 -o0.1 -h3 -j16 -P10 -d5 -x10 -s1011011110110111101101 -g8e6 -b10 -m20000 --verbose"
forms="zlib walk members"
if [ -n "${BEFORE_BIN:-}" ]; then forms="zlib before walk members"; fi
for round in 1 2 3; do
  for form in $forms; do
    bin="$here/goldrush_amd/bin/goldrush-path"
    unset GRP_GZIP_WALK GRP_GZIP_WALK_MEMBERS
    case $form in
      walk) export GRP_GZIP_WALK=on ;;
      members) export GRP_GZIP_WALK=on GRP_GZIP_WALK_MEMBERS=on ;;
      before) export GRP_GZIP_WALK=on; bin="$BEFORE_BIN" ;;
    esac
    t0=$(date +%s.%N)
    GRP_TRACE_INGEST=1 timeout -k 10 300 "$bin" $args -i "$work/all.fq.gz" -p "$work/out_$form" 2> "$work/err.txt"
    t1=$(date +%s.%N)
    echo "round $round form $form wall_s $(awk "BEGIN{print $t1 - $t0}") out_md5 $(md5sum < "$work/out_$form.fa" | cut -c1-12)"
    { grep -E "^GRP_TRACE_INGEST gzip walk" "$work/err.txt" || true; grep -E "^GRP_TRACE_INGEST source:" "$work/err.txt" | head -1; } | sed "s/^/  /"
  done
done
rm -rf "$work"
