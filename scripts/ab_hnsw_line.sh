#!/bin/bash
# one line for scripts/ab_run.sh: the C2 headline's first / median region and kernel time
cd ${GRAFT_REPO_ROOT:-/root/repo}
python bench.py --full --workload hnsw --streams 0 --no-cpu-baseline ${1:-} > /dev/null 2>&1
python - <<'P'
import json
j = json.load(open("bench_out/bench_full.json"))
d = j["dispersion"]["region_ms_per_step"]
print("first %.5f median %.5f min %.5f kernel_ms %.5f recall %s" % (j["ms_per_step"], d["median"], d["min"], j["roofline"]["kernel_ms"], j["recall_at_10"]))
P
