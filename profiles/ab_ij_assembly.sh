#!/bin/bash
# A/B timing of the IJ assembly from device-pointer triples on ONE box: two builds of the library, alternating.
#   bash profiles/ab_ij_assembly.sh <parent.so> <this.so> <n> [rounds] [--shuffle]   -> one JSON line per run
# The first run that fails, faults or runs into its time limit ends the script: nothing more is started on that GPU.
set -o pipefail
A=$1; B=$2; n=${3:-256}; rounds=${4:-3}; extra=$5
log=$(mktemp)
for r in $(seq $rounds); do
  for v in parent this; do
    lib=$A; [ $v = this ] && lib=$B
    MI_HYPRE_LIB=$(realpath $lib) timeout -k 10 240 python3 profiles/ij_assembly_measure.py --n $n --label "$v round $r" $extra > "$log" 2>&1
    rc=$?
    tail -1 "$log"
    if [ $rc -ne 0 ]; then echo "run '$v round $r' ended with status $rc: stopping" >&2; rm -f "$log"; exit 1; fi
  done
done
rm -f "$log"
