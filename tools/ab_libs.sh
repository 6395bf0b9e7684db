#!/bin/bash
# A/B timing of library builds (tuning aid, GPU box): bash tools/ab_libs.sh name1 name2 ...  -> kernel_ms (the launch) and
# ms_per_step (the step as the host sees it: what the call does around its kernels shows only there) of the headline
# bench with cnf2freq_amd/libcnf2hip_x_<name>.so in place of the product library ("base" = the product library).  A name that
# is a directory holding another checkout with its library built (say, the parent commit's tree) runs that tree's own bench.py
# on its own library: for a parent whose library lacks an export this tree's capi.py asks for.  Repeat names to alternate.
# The first run that fails ends the script.  The runs' logs go to the directory $AB_OUT (default ab_out/, kept out of git).
AB_OUT=${AB_OUT:-$PWD/ab_out}
mkdir -p "$AB_OUT"
n=0
for v in "$@"; do
    n=$((n+1))
    tree=$PWD
    lib=$PWD/cnf2freq_amd/libcnf2hip_x_$v.so
    tag=$v
    if [ "$v" = base ]; then lib=$PWD/cnf2freq_amd/libcnf2hip.so; fi
    if [ -f "$v/bench.py" ]; then tree=$(cd "$v" && pwd); lib=$tree/cnf2freq_amd/libcnf2hip.so; tag=$(basename "$tree"); fi
    log=$AB_OUT/ab_${n}_$tag.log
    (cd "$tree" && CNF2HIP_LIB=$lib timeout -k 10 200 python bench.py --full --steps 3 --warmup 1 --cpu-seconds 0 --no-iteration-probe --no-merge-probe ${AB_FLAGS}) \
        > "$log" 2>&1 || { echo "$tag failed"; tail -3 "$log"; exit 1; }
    python - "$tag" "$log" <<'PY' || exit 1
import json, sys
v = sys.argv[1]
r = json.loads(open(sys.argv[2]).read().strip().split("\n")[-1])
print("%-12s kernel_ms %.2f  ms_per_step %.2f  frac %.4f  loglik_checksum %r  checks %s" % (v, r["roofline"]["kernel_ms"], r["ms_per_step"], r["roofline"]["frac"],
      r.get("loglik_checksum", r.get("checks_detail", {}).get("loglik_checksum")), all(r["checks"].values())))
PY
done
