#!/usr/bin/env python3
"""Launch-for-launch record of the HNSW dispatch, to compare two builds of the library (a refactor of the host-side dispatch must
leave every call's kernels, grids, blocks and LDS what they were).

  rocprofv3 --kernel-trace --output-format csv -d DIR -o trace -- python scripts/hnsw_route_trace.py run > markers.txt
  python scripts/hnsw_route_trace.py summary DIR/.../trace_kernel_trace.csv markers.txt > profiles/NAME_hnsw_route_trace.csv
  python scripts/hnsw_route_trace.py compare A.csv B.csv

`run` issues the calls of tests/test_gpu_hnsw_route.py (its four graphs; b in 1, 31, 32; ef in 200, 209, 300, 449; default options,
MDB_HNSW_RANK 0 and 3, MDB_HNSW_NO_SPLIT, MDB_HNSW_CLOSURE 0) one after another in ONE process, synchronising between them.  In front of
every step (a load or a call) it launches a one-pair mdb_l2_distance as a separator the trace shows, and writes one marker row per step
to stdout: `load NAME` or `call NAME b ef OPTIONS | described launches` (the text of mdb_hnsw_describe_search where the library has it).
`summary` cuts the trace at the separators and prints, per call, its HNSW kernels as `step,marker,kernel_key,grid,workgroup,lds`; where
the marker carries a description it must name the same kernels with the same grid and block, else the summary fails.  (The trace's
LDS_Block_Size is the kernel's STATIC LDS — 0 for these kernels: the dynamic size of a launch is not in a kernel trace, so the lds column
only shows that no kernel gained static LDS.)  `compare` wants two summaries equal."""
import csv
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEPARATOR = "pair_distance_kernel<0>"   # what a one-pair mdb_l2_distance launches
ROUTED = ("hnsw_beam_kernel", "hnsw_search_kernel", "hnsw_closure_kernel", "hnsw_upper_", "pq_quantize", "pq_rows_kernel")


def run():
    import numpy as np
    import oracle
    from muopdb_amd import lib
    from tests import test_gpu_hnsw_route as T
    ctx = lib.Context(0)
    one = np.ones((1, 16), np.float32)

    def step(text):
        ctx.l2_distance(one, one)
        print(text, flush=True)

    for _ in range(5):
        ctx.l2_distance(one, one)
    ctx.sync()
    can_describe = hasattr(ctx.lib, "mdb_hnsw_describe_search")
    for name, (build, n, d, upper, _) in T.GRAPHS.items():
        step("load %s" % name)
        g, _, q = build(oracle, ctx, n, d, upper, seed=len(name))
        ctx.sync()
        for opts in T.OPTION_SETS:
            for k, v in opts.items():
                ctx.set_option(k, v)
            for b in T.BATCHES:
                for ef in T.EFS:
                    text = ""
                    if can_describe:
                        text = "; ".join("%s %d,%d %d %d" % (key, gx, gy, block, lds) for _, key, (gx, gy), block, lds in g.describe_search(b, 10, ef)[1])
                    step("call %s %d %d %s | %s" % (name, b, ef, ",".join("%s=%d" % kv for kv in sorted(opts.items())) or "-", text))
                    g.ann_search(q[:b], 10, ef)
                    ctx.sync()
            for k in opts:
                ctx.set_option(k, {"MDB_HNSW_RANK": 2, "MDB_HNSW_NO_SPLIT": 0, "MDB_HNSW_CLOSURE": 1}[k])
        g.close()
    step("end")
    ctx.close()


def summary(trace_csv, markers_txt):
    from tests.helpers import kernel_key
    with open(trace_csv, newline="") as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    with open(markers_txt) as f:
        markers = [ln.rstrip("\n") for ln in f if ln.startswith(("load ", "call ", "end"))]
    segments, cur, seen = [], None, 0
    for r in rows:
        if kernel_key(r["Kernel_Name"]) == SEPARATOR:
            seen += 1
            if seen > 5:   # the first five: run()'s warm-up of the separator itself
                cur = []
                segments.append(cur)
        elif cur is not None:
            cur.append(r)
    assert len(segments) == len(markers), "%d separators after the first five, %d marker rows" % (len(segments), len(markers))
    out = csv.writer(sys.stdout, lineterminator="\n")
    out.writerow(["step", "marker", "kernel_key", "grid", "workgroup", "lds"])
    bad = 0
    for i, (marker, seg) in enumerate(zip(markers, segments)):
        if not marker.startswith("call "):
            continue
        head, _, described = marker.partition(" | ")
        got = [(kernel_key(r["Kernel_Name"]), int(r["Grid_Size_X"]), int(r["Grid_Size_Y"]), int(r["Workgroup_Size_X"]), int(r["LDS_Block_Size"]))
               for r in seg if kernel_key(r["Kernel_Name"]).startswith(ROUTED)]
        for key, gx, gy, wg, lds in got:
            out.writerow([i, head, key, "%d,%d" % (gx, gy), wg, lds])
        if described.strip():
            want = []
            for item in described.split("; "):
                key, grid, block, lds = item.rsplit(" ", 3)
                bx, by = (int(x) for x in grid.split(","))
                want.append((key, bx * int(block), by, int(block), int(lds)))
            same = len(want) == len(got) and all(w[:4] == g[:4] for w, g in zip(want, got))
            if not same:
                bad += 1
                print("step %d (%s): described %s, traced %s" % (i, head, want, got), file=sys.stderr)
    return 1 if bad else 0


def compare(a_csv, b_csv):
    def load(p):
        with open(p, newline="") as f:
            return [tuple(r[c] for c in ("step", "marker", "kernel_key", "grid", "workgroup", "lds")) for r in csv.DictReader(f)]
    a, b = load(a_csv), load(b_csv)
    diff = [(x, y) for x, y in zip(a, b) if x != y]
    print("%d / %d launches; differing: %d" % (len(a), len(b), len(diff) + abs(len(a) - len(b))))
    for x, y in diff[:10]:
        print("  %s\n  %s" % (x, y))
    return 1 if diff or len(a) != len(b) else 0


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "run":
        sys.exit(run())
    if len(sys.argv) == 4 and sys.argv[1] == "summary":
        sys.exit(summary(sys.argv[2], sys.argv[3]))
    if len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    sys.exit(__doc__)
