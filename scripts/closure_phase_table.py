#!/usr/bin/env python3
"""Phase table of the frontier form (mdb_hnsw_closure.hip.h) from the `[hnsw dbg]` lines of an MDB_PIPE_DBG build.

  MDB_HNSW_DBG=4 python bench.py --full --workload hnsw --streams 0 --steps 200 --warmup 20 2> l1.txt    (layer-1 launch)
  MDB_HNSW_DBG=8 ...                                                                        2> top.txt   (top launch)
  scripts/closure_phase_table.py l1.txt top.txt [--json out.json]

One line per call (a batch) after the word of counters[3]: fallbacks | row | theta | clear | rounds | #trips | #rounds | pops | #pops |
hand-over | total | #blocks (CL_DBG_*).  Prints, per file, thread 0's cycles per block (mean over all batches, and the median batch) and
the events per block.  Shares, not times: a stamped build is slower than the real one."""
import json
import statistics
import sys

NAMES = ["row", "theta", "clear", "rounds", "n_trips", "n_rounds", "pops", "n_pops", "hand_over", "total", "blocks"]
COUNTS = {"n_trips", "n_rounds", "n_pops", "blocks"}


def table(path):
    rows = []
    for line in open(path):
        if "[hnsw dbg]" not in line:
            continue
        w = [int(v) for v in line.split("]")[1].split()]
        rows.append(dict(zip(NAMES, w[2:13]), fallbacks=w[1]))
    # a batch with a flagged query is left out: the sequential kernels that re-run it add THEIR stamps to the same words of a stamped
    # build (the fallback word among them), so only the clean batches can be read — `batches_with_a_rerun` says how many were dropped
    everything = len(rows)
    rows = [r for r in rows if r["blocks"] and r["fallbacks"] == 0]
    out = {"batches": len(rows), "batches_with_a_rerun": everything - len(rows)}
    nb = sum(r["blocks"] for r in rows)
    for k in NAMES[:-1]:
        out[k] = {"mean_per_block": sum(r[k] for r in rows) / nb, "median_batch_per_block": statistics.median(r[k] / r["blocks"] for r in rows)}
    other = sum(r["total"] - r["theta"] - r["clear"] - r["rounds"] - r["pops"] - r["hand_over"] for r in rows) / nb
    out["traverse_unaccounted"] = {"mean_per_block": other}
    return out


def main(argv):
    js = argv[argv.index("--json") + 1] if "--json" in argv else None
    paths = [a for a in argv if a != "--json" and a != js]
    res = {p: table(p) for p in paths}
    for p, t in res.items():
        whole = t["row"]["mean_per_block"] + t["total"]["mean_per_block"]
        print("%s: %d clean batches (%d with a re-run left out)" % (p, t["batches"], t["batches_with_a_rerun"]))
        for k in NAMES[:-1] + ["traverse_unaccounted"]:
            v = t[k]["mean_per_block"]
            if k in COUNTS:
                print("  %-22s %10.2f per block" % (k, v))
            else:
                print("  %-22s %10.0f cycles per block  %5.1f %%" % (k, v, 100.0 * v / whole))
    if js:
        json.dump(res, open(js, "w"), indent=1)


if __name__ == "__main__":
    main(sys.argv[1:])
