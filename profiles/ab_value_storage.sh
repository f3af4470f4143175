#!/bin/bash
# A/B/C of the value storage modes on ONE box with the unchanged benchmark, alternating runs:
#   bash profiles/ab_value_storage.sh [n] [rounds] [modes] [seconds per run]   (defaults: 512, 2, "0 1", 420; mode 2 once: modes "0 1 2")
# per run: ms per solve, iterations, setup seconds, final residual, device memory in use after Setup.
# Every run has its own time limit, and the first run that does not end with status 0 ends the script with that status:
# nothing more is started on a card after a fault, an abort or a hang.
n=${1:-512}; rounds=${2:-2}; modes=${3:-"0 1"}; limit=${4:-420}
out=$(mktemp) || exit 1
trap 'rm -f "$out"' EXIT
for r in $(seq $rounds); do
  for m in $modes; do
    MI_BENCH_N=$n MI_HYPRE_VALUE_STORAGE=$m MI_HYPRE_SETUP_TIMING=1 timeout -k 10 $limit python3 bench.py --gpus 1 --steps 10 --warmup 2 > "$out"
    rc=$?
    if [ $rc -ne 0 ]; then
      echo "MI_HYPRE_VALUE_STORAGE=$m round $r: bench.py ended with status $rc; stopping" >&2
      tail -20 "$out" >&2
      exit $rc
    fi
    python3 -c "
import json,re,sys
lines=open(sys.argv[1]).read().strip().splitlines()
d=json.loads([l for l in lines if l.startswith('{')][-1])  # (the library's own lines may be flushed after it)
mem=[re.search(r'([0-9.]+) GiB in use', l).group(1) for l in lines if 'device arena' in l and 'GiB in use' in l]
print('MI_HYPRE_VALUE_STORAGE=$m round $r: ms/solve %.1f  iters %d  setup %.2f s  res %.15e  in use after Setup %s GiB' % (d['ms_per_step'], d['iterations_per_solve'], d['setup_s'], d['final_rel_residual'], mem[0] if mem else '?'))" "$out" || exit 1
  done
done
