#!/bin/bash
# A/B of bench.py between a built checkout of another commit and this tree, one process per run,
# alternating (tools/ab_lib.sh selects the other build with PCP_LIB, which needs both builds to
# export the same ABI; this one runs each tree's own bench.py over its own library).
#   bash tools/ab_bench.sh PARENT_TREE ROUNDS [bench.py arguments ...]
# NEW_ENV="K=V ..." adds a third variant: this tree with that environment.
# One line per run: variant, ms_per_step, value, and with --full roofline.avg_kernel_ms and
# reference_mode.ms_per_step.  Ends at the first run that fails.
set -u
cd "$(dirname "$0")/.."
PARENT=$1; ROUNDS=$2; shift 2
pick='import json,sys
d=json.loads([l for l in sys.stdin if l.startswith("{")][-1])
r=d.get("roofline") or {}; m=d.get("reference_mode") or {}
print(sys.argv[1], d.get("ms_per_step"), d.get("value"), r.get("avg_kernel_ms"), m.get("ms_per_step"))'
one() {   # name, directory, environment
  local out
  out=$(cd "$2" && env $3 timeout -k 10 600 python bench.py --gpus 1 "${@:4}" 2>/dev/null) || { echo "$1 failed"; exit 1; }
  echo "$out" | python -c "$pick" "$1" || exit 1
}
for r in $(seq "$ROUNDS"); do
  one parent "$PARENT" "" "$@"
  one new . "" "$@"
  [ -n "${NEW_ENV:-}" ] && one "new[$NEW_ENV]" . "$NEW_ENV" "$@"
done
exit 0
