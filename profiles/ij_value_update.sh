#!/bin/bash
# New values for an assembled IJ matrix on ONE box: an update round of this build against Destroy + Create + a full
# device assembly with the parent's build, alternating, one process per run.
#   bash profiles/ij_value_update.sh <parent.so> <this.so> <n> [rounds] [--shuffle]   -> one JSON line per run
# The first run that fails, faults or runs into its time limit ends the script: nothing more is started on that GPU.
set -o pipefail
A=$1; B=$2; n=${3:-256}; rounds=${4:-3}; extra=$5
log=$(mktemp)
for r in $(seq $rounds); do
  for v in parent this; do
    lib=$A; mode=fresh; [ $v = this ] && lib=$B && mode=update
    MI_HYPRE_LIB=$(realpath $lib) timeout -k 10 300 python3 profiles/ij_value_update.py --n $n --mode $mode --label "$v round $r" $extra > "$log" 2>&1
    rc=$?
    tail -1 "$log"
    if [ $rc -ne 0 ]; then echo "run '$v round $r' ended with status $rc: stopping" >&2; tail -5 "$log" >&2; rm -f "$log"; exit 1; fi
  done
done
rm -f "$log"
