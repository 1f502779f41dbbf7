#!/bin/bash
# usage: tools/ab.sh <A> <B> [rounds] [bench args]   -- alternates two settings on one box, one untimed heat-up run first (the
# chip's clock settles under load).  A setting is a build -- <lib.so>, or "-" for the in-tree build -- or an environment switch
# of the in-tree build: env:NAME=VALUE[,NAME=VALUE...] (e.g. env:BB_EVAL_CACHE=0).  Every run is a plain bench.py (plus the
# bench args) under its own time limit.  Prints games/s (`value`), node evaluations/s (simulations) and tower runs/s of every
# run, and the medians.  (Tower runs/s is not a yardstick once the evaluation cache answers some evaluations without one.)
# Each run's JSON line is kept as $AB_OUT/ab_<label>.json (default directory: ab_out).
A=$1; B=$2; N=${3:-4}; shift 3
OUT=${AB_OUT:-ab_out}
mkdir -p "$OUT"
run() { # label setting [bench args]
  L=$1; S=$2; shift 2
  local envs=() P=bench.py
  case "$S" in
    env:*) IFS=',' read -ra envs <<< "${S#env:}" ;;
    -) ;;
    *) P=tools/bench_lib.py; envs=("BB_LIB=$S") ;;
  esac
  timeout -k 10 300 env "${envs[@]}" python $P "$@" 2>/dev/null | tail -1 > "$OUT/ab_$L.json" || { echo "$L FAILED"; exit 1; }
}
run heat "$A" "$@"
for i in $(seq 1 $N); do run A$i "$A" "$@" && run B$i "$B" "$@" || exit 1; done
python - <<PY
import json, statistics
for k, s in (("A", "$A"), ("B", "$B")):
    r = [json.load(open("$OUT/ab_%s%d.json" % (k, i))) for i in range(1, $N + 1)]
    for key, name, scale in (("value", "games/s", 1.0), ("node_evals_per_sec", "node evals/s (M)", 1e-6),
                             ("net_evals_per_sec_rank0", "tower runs/s (M)", 1e-6)):
        v = [x[key] * scale for x in r]
        print(k, s, name + ":", " ".join("%.1f" % x for x in v), "median %.1f" % statistics.median(v))
PY
