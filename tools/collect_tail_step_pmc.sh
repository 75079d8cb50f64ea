#!/bin/bash
# HBM bytes of the segmentation step's forward forms (tools/bench_tail.py --forward): rocprofv3 --pmc FETCH_SIZE WRITE_SIZE with
# --kernel-trace only, one form and one grad mode per run.  usage: collect_tail_step_pmc.sh REPO_ROOT OUT_FILE TAG TOKENS WIDTH FORM...
# (REPO_ROOT: the tree whose build is measured; all kernels of the run are summed and divided by the calls made.)
set -o pipefail
root=$1; out=$2; tag=$3; tokens=$4; width=$5; shift 5
iters=2; calls=$((iters + 2))
for form in "$@"; do
  for grad in train valid; do
    d=$(mktemp -d)
    (cd "$root" && timeout -k 10 240 rocprofv3 --pmc FETCH_SIZE WRITE_SIZE --kernel-trace -d "$d" -o t -- \
        python tools/bench_tail.py --forward --forms "$form" --grad $grad --tokens "$tokens" --width "$width" --iters $iters) > "$d/log" 2>&1 \
      || { tail -5 "$d/log"; exit 1; }
    python - "$root" "$d" "$tag" "$form" "$grad" $calls <<'PY' | tee -a "$out"
import sys
sys.path.insert(0, sys.argv[1] + "/tools")
import pmc_db
res, calls = pmc_db.read(sys.argv[2]), int(sys.argv[6])
tot = {"FETCH_SIZE": 0.0, "WRITE_SIZE": 0.0}
for k, v in res.items():
    for c in tot:
        if c in v:
            tot[c] += v[c]["avg"] * v[c]["samples"] * 1024 / calls  # KiB per dispatch x dispatches / calls
print(f"{sys.argv[3]} {sys.argv[5]} forward {sys.argv[4]:9s} per call, all kernels: FETCH_SIZE {tot['FETCH_SIZE'] / 1e6:9.1f} MB  "
      f"WRITE_SIZE {tot['WRITE_SIZE'] / 1e6:9.1f} MB  (raw counters x 1 KiB)")
PY
    rm -rf "$d"
  done
done
