#!/bin/bash
# Ablation A/B of the fan's "round trips" pieces: this tree's library against
# builds that take one piece out each, alternating processes of bench.py (PCP_LIB selects the
# build; the ABI is the same).
#   bash tools/fan_trips_ab.sh build            # here or anywhere with hipcc: the ablation builds
#   bash tools/fan_trips_ab.sh run ROUNDS [bench.py arguments ...]
# One line per run: variant, ms_per_step, value, roofline.avg_kernel_ms, reference ms_per_step.
set -u
cd "$(dirname "$0")/.."
LIB=pointcloud_processor_amd/_lib
VARIANTS="PCP_FAN_NO_PRO1 PCP_FAN_NO_PAIR"
if [ "$1" = build ]; then
  # each variant is the Makefile's own library target in another OUTDIR with the knob in EXTRA
  for v in $VARIANTS; do
    make -s -j"${JOBS:-16}" -C pointcloud_processor_amd/csrc OUTDIR=../_lib/alt_trips_$v EXTRA=-D$v \
      ../_lib/alt_trips_$v/libpcp.so || exit 1
  done
  ls -l $LIB/alt_trips_*/libpcp.so
  exit 0
fi
ROUNDS=$2; shift 2
pick='import json,sys
d=json.loads([l for l in sys.stdin if l.startswith("{")][-1])
r=d.get("roofline") or {}; m=d.get("reference_mode") or {}
print(sys.argv[1], d.get("ms_per_step"), d.get("value"), r.get("avg_kernel_ms"), m.get("ms_per_step"))'
one() {   # name, library ("" = this tree's)
  local out
  out=$(env ${2:+PCP_LIB=$2} timeout -k 10 600 python bench.py --gpus 1 "${@:3}" 2>/dev/null) || { echo "$1 failed"; exit 1; }
  echo "$out" | python -c "$pick" "$1" || exit 1
}
for r in $(seq "$ROUNDS"); do
  one new "" "$@"
  for v in $VARIANTS; do one "minus_$v" "$PWD/$LIB/alt_trips_$v/libpcp.so" "$@"; done
done
exit 0
