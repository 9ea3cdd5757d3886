#!/bin/bash
# A/B helper (run on the GPU box): the scan-bound workloads, one line each
cd ${GRAFT_REPO_ROOT:-/root/repo}
OUT=${OUT:-bench_out}; mkdir -p $OUT
py() { python - "$1" <<'PY'
import json,sys
d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]); r=d["roofline"]
print(sys.argv[1], "value=%.0f ms=%.4f kernel_ms=%.4f" % (d["value"], d["ms_per_step"], r["kernel_ms"]), "ids_match", d["cpu_baseline"].get("ids_match_gpu"))
PY
}
python bench.py --full --workload ivfpq > $OUT/q_ivfpq_c3.json 2>/dev/null; py $OUT/q_ivfpq_c3.json
python bench.py --full --workload ivfpq --n 12500000 --nlist 8192 --nprobe 8 --batch 4096 --steps 10 --warmup 2 > $OUT/q_c5.json 2>/dev/null; py $OUT/q_c5.json
python bench.py --full --workload flat --n 1000000 > $OUT/q_flat_b1.json 2>/dev/null; py $OUT/q_flat_b1.json
python bench.py --full --workload flat --n 1000000 --batch 64 > $OUT/q_flat_b64.json 2>/dev/null; py $OUT/q_flat_b64.json
python bench.py --full --workload flat > $OUT/q_flat_c1.json 2>/dev/null; py $OUT/q_flat_c1.json
python bench.py --full --workload spann --steps 20 --warmup 3 > $OUT/q_spann.json 2>/dev/null; py $OUT/q_spann.json
