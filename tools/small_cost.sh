#!/bin/bash
# NUMERICS (environment, default contract): the build of the kernel library, pinned on every bench.py line
# OUT (environment, default bench_out): where the bench lines go
OUT=${OUT:-bench_out}
mkdir -p $OUT
for n in 64 128 256; do
  python bench.py --numerics ${NUMERICS:-contract} --ncell $n --steps 20 --warmup 5 --full --no-cpu-baseline --no-contract-leg --no-extras > $OUT/sm.json 2> $OUT/sm.err || tail -3 $OUT/sm.err
  python - <<PY
import json
d=json.load(open("$OUT/sm.json"))
k={a: b["ms_per_step"] for a, b in d["roofline"]["kernel_utilisation"].items()}
print("n=$n: ms/step %.3f  kernels %.3f  -> %.3f G cell-updates/s" % (d["ms_per_step"], sum(k.values()), d["value"]/1e9), {a: round(b,3) for a,b in k.items()})
PY
done
