#!/bin/bash
# Interleaved A/B of builds of the engine library on the r07 set of bench legs (GPU box, from the
# repo root): default, --config 1, 8 standard levels, --farfield, --pedestal; plain runs,
# --steps 20 --warmup 5.  Usage:
#   scripts/ab_wing_trip.sh <out> <rounds> <name>=<library .so> ...     ("tree" = the shipped one)
# e.g. scripts/ab_wing_trip.sh ab.txt 3 tree hint7=variants/liblbl_hint7.so parent=variants/liblbl_parent.so
# Afterwards the default leg's --dump-outputs of every library are compared with the first one's
# (largest absolute difference of any array).  Every run has a time limit of its own and the
# script ends at the first one that fails.
OUT=$1; ROUNDS=$2; shift 2
: > $OUT
# ONLY_LEGS="--farfield;--config 1" runs these legs instead of the five (noisy legs, more rounds).
LEGS=("" "--config 1" "--levels-per-gpu 8 --profile standard" "--farfield" "--pedestal")
if [ -n "$ONLY_LEGS" ]; then IFS=';' read -ra LEGS <<< "$ONLY_LEGS"; fi
run() {     # <name[=library]> <bench args...>: prints the bench line
  local spec=$1; shift
  if [ "$spec" = tree ]; then unset PYLBL_AMD_LIBRARY; else export PYLBL_AMD_LIBRARY=$(realpath ${spec#*=}); fi
  timeout -k 10 ${LIMIT:-240} python bench.py --gpus 1 --steps ${STEPS:-20} --warmup 5 "$@" 2>/dev/null
}
for round in $(seq 1 $ROUNDS); do
  for leg in "${LEGS[@]}"; do
    for spec in "$@"; do
      line=$(run $spec $leg) || { echo "round $round [${spec%%=*}] '$leg' failed" | tee -a $OUT; exit 1; }
      echo "$line" | python -c "
import json, sys
d = json.loads(sys.stdin.read())
print('round $round %-8s %-40s ms/step %.4f' % ('${spec%%=*}', '$leg' or 'default', d['ms_per_step']))" | tee -a $OUT || exit 1
    done
  done
done
DUMPS=$(mktemp -d)
for spec in "$@"; do
  run $spec --dump-outputs $DUMPS/${spec%%=*} > /dev/null || { echo "dump [${spec%%=*}] failed" | tee -a $OUT; exit 1; }
done
python - $DUMPS "$@" <<'EOF' | tee -a $OUT
import glob, os, sys
import numpy as np
root, names = sys.argv[1], [x.split("=")[0] for x in sys.argv[2:]]
for name in names[1:]:
    worst, same, count = 0., True, 0
    for path in sorted(glob.glob(os.path.join(root, names[0], "*.npy"))):
        a, b = np.load(path), np.load(os.path.join(root, name, os.path.basename(path)))
        worst = max(worst, float(np.max(np.abs(a - b)/np.maximum(np.abs(a), 1e-300))))
        same = same and np.array_equal(a, b)
        count += 1
    print("dump-outputs %s against %s: %d arrays, largest relative difference %.3g, same bits: %s"
          % (name, names[0], count, worst, same))
EOF
rm -rf $DUMPS
