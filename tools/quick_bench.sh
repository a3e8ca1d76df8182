#!/bin/bash
# NUMERICS (environment, default contract): the build of the kernel library, pinned on every bench.py line
# parity tests, then the 256^3 bench with per-kernel times; OUT (environment, default bench_out): where its line goes
OUT=${OUT:-bench_out}
mkdir -p $OUT
python -m pytest tests/test_gpu_parity.py -x -q 2>&1 | tail -3
python bench.py --numerics ${NUMERICS:-contract} --steps 10 --warmup 3 --full --no-cpu-baseline --no-contract-leg > $OUT/qb.json 2> $OUT/qb.err || tail -5 $OUT/qb.err
python - <<PY
import json
d=json.load(open("$OUT/qb.json"))
print("ms/step %.2f" % d["ms_per_step"], {k: round(v,2) for k,v in {a: b["ms_per_step"] for a, b in d["roofline"]["kernel_utilisation"].items()}.items()})
PY
