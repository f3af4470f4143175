#!/bin/bash
# Setup reuse against the full Setup, in one session on one box:
#   [STEPS=3] bash profiles/setup_reuse.sh <dir of the parent build (hypre_app + libmi_hypre.so)> [sizes, default "256 512"] [rounds, default 3]
# Per size and round, alternating: the parent commit's driver (switch unknown there), this build with mi_setup_reuse 0 and
# with 1, each on the laplace_3d deck with mi_update_steps STEPS and mi_device_assembly 1 under MI_HYPRE_SETUP_TIMING=1.
# Prints, per run, the seconds of the first Setup, every step's Setup verdict and seconds, the refresh's own phases, the
# solves' seconds and iterations and the arena's peak.  Every run has its own time limit; the script stops at the first
# run that fails.
PARENT=$(realpath "$1"); SIZES=${2:-"256 512"}; ROUNDS=${3:-3}; STEPS=${STEPS:-3}
HERE=$(cd "$(dirname "$0")/.." && pwd)
TMP=$(mktemp -d)
deck() {  # n, extra line of boomeramg_settings
  cat > "$TMP/deck.yaml" <<EOF
linear_system:
  type: laplace_3d
  nx: $1
  ny: $1
  nz: $1
  stencil: 7
  mi_update_steps: $STEPS
  mi_device_assembly: 1

solver_settings:
  method: gmres
  preconditioner: boomeramg
  tolerance: 1.0e-8
  max_iterations: 200
  kspace: 50
  print_level: 2

boomeramg_settings:
  print_level: 1
  coarsen_type: 8
  relax_type: 8
  relax_order: 1
  num_sweeps: 1
  max_levels: 20
  strong_threshold: 0.57
$2
EOF
}
for n in $SIZES; do
  for r in $(seq "$ROUNDS"); do
    for v in parent off on; do
      app="$HERE/hypre-mini-app_amd/hypre_app"; extra=""
      [ $v = parent ] && app="$PARENT/hypre_app"
      [ $v = off ] && extra="  mi_setup_reuse: 0"
      [ $v = on ] && extra="  mi_setup_reuse: 1"
      deck "$n" "$extra"
      echo "=== n $n round $r $v"
      (cd "$TMP" && MI_HYPRE_SETUP_TIMING=1 timeout -k 10 240 "$app" deck.yaml > run.log 2>&1) || { tail -20 "$TMP/run.log"; exit 1; }
      grep -E "^mi_hypre BoomerAMG setup:|^Setup [0-9]+ :|^Solve [0-9]+ :|^Step [0-9]+ :|refresh: |device arena|Update step|[Ss]olve.*time|[Ss]etup.*time|Timer|seconds" "$TMP/run.log" | cut -c1-260
    done
  done
done
rm -rf "$TMP"
