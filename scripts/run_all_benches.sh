#!/bin/bash
# Every bench.py workload once, with --full (run on a GPU box); JSON lines land in $OUT/bench_<name>.json (default bench_out/)
REPO=${GRAFT_REPO_ROOT:-/root/repo}
OUT=${OUT:-$REPO/bench_out}
mkdir -p $OUT
cd $REPO
python bench.py --full                                                  > $OUT/bench_hnsw_c2.json      2> $OUT/bench_hnsw_c2.err
python bench.py --full --workload flat                                  > $OUT/bench_flat_c1.json      2> $OUT/bench_flat_c1.err
python bench.py --full --workload flat --n 1000000                      > $OUT/bench_flat_1m_b1.json   2> $OUT/bench_flat_1m_b1.err
python bench.py --full --workload flat --n 1000000 --batch 64           > $OUT/bench_flat_1m_b64.json  2> $OUT/bench_flat_1m_b64.err
python bench.py --full --workload ivfpq                                 > $OUT/bench_ivfpq_c3.json     2> $OUT/bench_ivfpq_c3.err
python bench.py --full --workload spann --steps 20 --warmup 3           > $OUT/bench_spann_128u.json   2> $OUT/bench_spann_128u.err
for f in $OUT/bench_*.json; do echo "== $f"; tail -c 400 $f; echo; done
