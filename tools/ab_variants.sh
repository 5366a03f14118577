#!/bin/bash
# A/B of library variants on the driver-shaped run (build/variants/libsddp_<name>.so, built with SDDP_LIB / SDDP_CXXFLAGS, e.g. from
# a tree with profiles/r05/experiments/lds_dma.diff applied and the diff's flag in SDDP_CXXFLAGS):
#   bash tools/ab_variants.sh base lds_dma base lds_dma        (bench lines and stderr under $OUT, default build/ab)
O=${OUT:-build/ab}
mkdir -p $O
for v in "$@"; do
  if [ $v = base ]; then unset SDDP_LIB; else export SDDP_LIB=/root/repo/build/variants/libsddp_$v.so; fi
  python bench.py --full --steps 20 --warmup 5 --no-extras --no-cpu-baseline > $O/ab_$v.json 2> $O/ab_$v.err
  python - <<PY
import json
d=json.loads(open("$O/ab_$v.json").read().strip().splitlines()[-1]); print("$v", round(d["value"]), [round(x) for x in d["value_runs"]], round(d["roofline"]["kernel_ms"],2), d["roofline"]["resources"])
PY
done
