#!/usr/bin/env python
"""bench.py — measures BASELINE.json's metric on MI355X.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...
(a plain `python bench.py --gpus N` with N > 1 starts its N ranks itself through torch.distributed.run — one process per GPU over
RCCL — and fails loudly when fewer than N devices are visible; `n_gpus` in the line is always the number of ranks that ran)

A plain run sets up, warms up, times the K steps of the headline and prints ONE JSON line (`metric`, `value`, `unit`,
`ms_per_step` = milliseconds per timed step, ...); `--dump-outputs DIR` writes what the last timed step returned (dump_outputs).
Everything else below (recall, roofline, cpu_baseline, dispersion, multi-stream runs, sweeps, the `workloads` block, the full
record) runs with `--full` only.

Headline (`value`, `ms_per_step`, `roofline`, `cpu_baseline` at the top level of the ONE JSON line) =
BASELINE.json configs[1]: SIFT-1M-like 1M x 128 f32 (synthetic), HNSW ef=200, top-10, batch=64,
through the C ABI (libmuopdb_hip.so) with queries and outputs resident in HBM.  A "step" is one batch of 64 queries
through BlockBasedHnsw::ann_search.  N>1: HNSW does not shard (replicas only) — every rank holds the
graph and runs its own batches, so per-GPU work is fixed ("weak") and value = all ranks' queries / max time.
The graph of the headline is built the way MuopDB builds it (HnswBuilder::insert's algorithm, `--graph insert`, the default since
round 6); the bulk k-NN build is the workload `hnsw_c2_knn_graph`.  `value` is the K-step region's; `dispersion.long_region` adds one
region of 200 steps (K = 20 steps are ~15 ms: inside the 3-8 % two boxes differ by).

A --full run also times the other north-star workloads and reports them under `workloads` (each entry with its own
value / ms_per_step / recall_at_10 / roofline / cpu_baseline, every one bracketed by the same barrier +
synchronize and max-over-ranks rule):
    hnsw_c2_b1, hnsw_c2_ef400 the metric's other batch size / ef above 256, over the same resident graph
    flat_c1_10k_b1 (_b64)     BASELINE configs[0]: 10 k x 128 (py/create_test_hdf5.py-shaped rows), batch 1
    flat_1m_b1, flat_1m_b64   brute-force L2 over the same 1M x 128 base (batch 1: HBM stream; batch 64: MFMA filter)
    ivfpq_c3                  IVF nlist=4096 + PQ m=16 nbits=8 (the reference's symmetric distance), batch 256,
                              nprobe sweep {1, 8, 16, 32, 64} as (recall@10, QPS) pairs
    spann_c4_128u             multi-user SPANN, 128 users x 9766 x 768 (C4's shape at 1/8 of its users; the full
                              1024 users: --workload spann --users 1024), num_explored_centroids / ratio sweep
For N>1 the list-sharded workloads (ivfpq, spann) run with posting lists sharded over the ranks and ONE packed RCCL
all-gather of the per-shard top-k per batch ("strong": the same batch on every rank).
`--workload hnsw|flat|ivfpq|spann|c5` runs a single workload as the line (profiling, other sizes).

`roofline.achieved` = algorithmic bytes per launch (SURVEY.md §8d per-unit bytes x units) / the dominant
kernel's mean duration from HIP events recorded on the launch stream inside the library (mdb_set_profiling).
`cpu_baseline` = the CPU oracle (oracle/, a port of the reference's algorithm) timed on this box's host cores.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# The `concurrent` extra of the HNSW workload keeps 4 batches in flight on 4 HIP streams; with the runtime's default
# of 4 hardware queues two of them share a queue with torch's own stream and only 2 batches overlap (117 k
# queries/s); 8 queues give every stream its own (235 k queries/s).  No effect on the single-stream headline.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

import numpy as np
import torch
import torch.distributed as dist

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8.0 TB/s spec (6.29 TB/s measured copy ceiling)
LONG_STEPS = 200       # steps of the headline's extra long region (dispersion.long_region)
DISP_REGIONS = 4       # extra timed regions per workload for the dispersion entry (Env.timed)
WARM_MIN_S = 0.05      # Env.timed: the untimed warm-up lasts at least this long (the W steps repeated)
PROF_EVERY = 8         # steps of the timed region between two steps whose dominant kernels are bracketed by HIP events
METRIC = "QPS @ recall@10, SIFT-1M d=128 top-10, batch=1/64; 1/2/4/8 GPUs"
FULL_JSON_DEFAULT = os.path.join("bench_out", "bench_full.json")   # --full: the full record, relative to the repository root
DUMP_OUTPUTS_LIMIT = 64 << 20   # --dump-outputs: bytes in all; a larger output is cut to a fixed, seeded sample of its rows


def measured_traffic(kind, cfg):
    """roofline.traffic: HBM bytes per launch of the dominant kernel from the committed PMC passes
    (profiles/r*_traffic.json; rocprofv3 --pmc cannot run inside this process), only when the
    workload matches the profiled one; else None."""
    import glob
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_traffic.json")), reverse=True):
        with open(path) as f:
            e = json.load(f).get(kind)
        # round 1's passes (no "data" key) were taken on the legacy generators
        if e and e["match"].get("data", "legacy") == cfg.get("data") and all(cfg.get(k) == v for k, v in e["match"].items() if k != "data"):
            return (e["fetch_kib"] * e["fetch_correction"] + e["write_kib"]) * 1024.0, os.path.relpath(path, ROOT)
    return None, None


def measured_mfma(kind, cfg):
    """roofline.mfma_busy: SQ_VALU_MFMA_BUSY_CYCLES / SQ_BUSY_CYCLES of the matrix-core filter kernel from the committed PMC pass
    (profiles/r*_traffic.json "_mfma"; same matching rule as measured_traffic), else None."""
    import glob
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_traffic.json")), reverse=True):
        with open(path) as f:
            j = json.load(f)
        e, t = j.get("_mfma", {}).get(kind), j.get(kind)
        if e and t and t["match"].get("data", "legacy") == cfg.get("data") and all(cfg.get(k) == v for k, v in t["match"].items() if k != "data"):
            # SQ_VALU_MFMA_BUSY_CYCLES sums the busy cycles of all 1024 SIMDs' matrix cores (32 per v_mfma_f32_32x32x16_bf16,
            # MI355X_MICROARCH.md); GRBM_GUI_ACTIVE sums the 8 XCCs' active cycles over the launch
            cyc = e["grbm_gui_active"] / 8.0 if e.get("grbm_gui_active") else None
            return dict(mfma_busy_frac_of_chip=e["mfma_busy_cycles"] / (1024.0 * cyc) if cyc else None,
                        mfma_busy_cycles=e["mfma_busy_cycles"], kernel_cycles=cyc, simds=1024, sq_busy_cycles=e.get("sq_busy_cycles"),
                        source=e["source"])
    return None


def dump(args, rank, sub, **files):
    """--dump-dir: the workload's files for examples/replay_search.cpp (torch-free PMC passes)."""
    if not args.dump_dir or rank != 0:
        return
    d = os.path.join(args.dump_dir, sub)
    os.makedirs(d, exist_ok=True)
    for name, data in files.items():
        with open(os.path.join(d, name), "wb") as f:
            f.write(data if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data).tobytes())
    log("dumped %s to %s" % (", ".join(files), d))


def log(*a):
    if int(os.environ.get("RANK", "0")) == 0:
        print("[bench]", *a, file=sys.stderr, flush=True)


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--workload", default="all", choices=["all", "hnsw", "flat", "ivfpq", "spann", "c5", "c5full"])
    p.add_argument("--data", default="lowrank", choices=["lowrank", "legacy"],
                   help="lowrank: muopdb_amd.build.SiftLike / EmbedLike; legacy: round 1's isotropic Gaussian generators")
    p.add_argument("--n", "--base-n", dest="n", type=int, default=None,
                   help="base vectors (default: the config's size); spell it --base-n under a torch.distributed.run launch (its own "
                        "argument parser rejects --n as an ambiguous prefix of --nnodes / --nproc-per-node / ...)")
    p.add_argument("--dim", type=int, default=None)
    p.add_argument("--batch", type=int, default=None)
    p.add_argument("--ef", type=int, default=200)
    p.add_argument("--k", type=int, default=10)
    p.add_argument("--nprobe", type=int, default=None)
    p.add_argument("--ratio", type=float, default=None, help="spann: centroid_distance_ratio of the primary setting")
    p.add_argument("--nlist", type=int, default=None, help="ivfpq: number of posting lists (default min(4096, n/244))")
    p.add_argument("--users", type=int, default=128, help="spann workload: number of users (1024 = full C4)")
    p.add_argument("--max-neighbors", type=int, default=32)
    p.add_argument("--no-cpu-baseline", action="store_true")
    p.add_argument("--no-sweep", action="store_true")
    p.add_argument("--no-c5", action="store_true", help="all: skip the C5 per-GPU shard workload (~50 s of build)")
    p.add_argument("--no-c5-full", action="store_true", help="all: skip the whole-C5-on-one-GPU workload (100M codes, ~2-3 min of build)")
    p.add_argument("--no-c4-full", action="store_true", help="all: skip the full-size C4 workload (1024 users, 30.7 GB, ~60 s)")
    p.add_argument("--streams", type=int, default=4, help="hnsw: extra measurement with this many batches in flight (0/1 = skip)")
    p.add_argument("--dump-dir", default=None, help="write index files + queries for examples/replay_search.cpp")
    p.add_argument("--dump-big", action="store_true", help="--dump-dir also for workloads above 8 GB (full C4: 30 GB)")
    p.add_argument("--cpu-seconds", type=float, default=10.0)
    p.add_argument("--sift-dir", default=None, help="directory holding sift_base.fvecs / sift_query.fvecs / sift_groundtruth.ivecs: "
                                                    "the C2/C3 workloads then run on the real SIFT-1M (data: sift1m) instead of synthetic rows")
    p.add_argument("--graph", default="insert", choices=["knn", "insert"],
                   help="hnsw: how the base graph of the HEADLINE is built — insert (default): HnswBuilder::insert's algorithm, the graph MuopDB "
                        "itself would write, wave-batched on the GPU (muopdb_amd.build.insert_hnsw); knn: exact k-NN + the reference's selection "
                        "heuristic (fast bulk build)")
    p.add_argument("--no-insert-graph", "--no-second-graph", dest="no_insert_graph", action="store_true",
                   help="all: skip the second HNSW line on the graph built the OTHER way")
    p.add_argument("--insert-n", type=int, default=None, help="all: base size of the second-graph HNSW workload (default: --n)")
    p.add_argument("--shard", default="lists", choices=["lists", "users", "batch"],
                   help="world > 1, single workloads: posting-list shards + exact merge (default, what north_star names), or a QUERY "
                        "partitioning with an all-gather of finished rows only: users (spann: user slot u on rank u %% world) / batch (ivfpq, "
                        "c5full: replicas, contiguous batch slices).  --workload all runs list shards AND the comparators (SURVEY 8e: measure both)")
    p.add_argument("--share-closure", default="auto", choices=["auto", "on", "off"],
                   help="spann, list shards, world > 1: run the centroid-graph closure ONCE per (user, query) pair — each rank for its slice "
                        "of the batch, probe rows in one more all-gather (mdb_multi_spann_probes / _search_shard_probes) — instead of on "
                        "every rank.  auto: from batch 1024 (the closure is one wave per pair: 36-39 us flat up to batch 256, 55 us at 512, 94 us at 1024)")
    p.add_argument("--plan", action="store_true",
                   help="print what `--gpus N` (workload all) will build and hold — per workload: who builds, estimated build / load "
                        "seconds, host bytes private to a rank and shared through the page cache, HBM per rank — and exit (no GPU needed)")
    p.add_argument("--full", action="store_true",
                   help="measure and check everything besides the headline timing: the `workloads` block, CPU baselines, recall, "
                        "roofline brackets, dispersion regions, multi-stream runs, sweeps and the full record (off: set up, warm up, "
                        "time the K steps, print the line)")
    p.add_argument("--dump-outputs", default=None, metavar="DIR",
                   help="after the timed steps, write what the line's workload computed in its last timed step (ids, scores, counts) "
                        "as DIR/<name>.npy in float32 / float64, at most %d MB in all" % (DUMP_OUTPUTS_LIMIT >> 20))
    p.add_argument("--full-json", default=None, help="--full: where rank 0 writes the full record (default %s); stdout "
                                                     "carries ONE compact line of at most %d bytes" % (FULL_JSON_DEFAULT, LINE_LIMIT))
    p.add_argument("--sift-clusters", type=int, default=None, help="SiftLike mixture components (generator exploration)")
    p.add_argument("--sift-sigma", type=float, default=None)
    p.add_argument("--sift-noise", type=float, default=None)
    return p.parse_args()


def cpu_stamp(threads_all):
    """CPU model, core count and the thread counts used, recorded with every cpu_baseline"""
    model = "unknown"
    try:
        with open("/proc/cpuinfo") as f:
            for ln in f:
                if ln.lower().startswith("model name"):
                    model = ln.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    return dict(cpu_model=model, host_cores=os.cpu_count(), threads_single=1, threads_all=int(threads_all),
                omp_places=os.environ.get("OMP_PLACES"), omp_proc_bind=os.environ.get("OMP_PROC_BIND"))


def cpu_baseline(single_fn, multi_fn, nq, seconds, probe, match_fn, sample_fmt):
    """Times the oracle on a bounded sample of the timed queries: `single_fn(n)` runs the first n on ONE thread and returns its
    result, `multi_fn(n, threads)` the same on all cores; match_fn(result, n) compares the one-thread rows with the GPU's."""
    import oracle
    t0 = time.perf_counter(); single_fn(probe); dt = time.perf_counter() - t0
    ns = int(min(nq, max(probe, seconds / (dt / probe))))
    t0 = time.perf_counter(); r = single_fn(ns); dt1 = time.perf_counter() - t0
    nt = oracle.num_threads()
    na = int(min(nq, max(ns, 8 * nt)))
    multi_fn(min(na, nt), nt)   # warm the thread pool
    t0 = time.perf_counter(); multi_fn(na, nt); dta = time.perf_counter() - t0
    out = dict(value=ns / dt1, unit="queries/s", cores=1, kind="port", sample=sample_fmt % ns, all_cores_value=na / dta, all_cores=nt,
               all_cores_sample="%d queries, one query per thread" % na, ids_match_gpu=bool(match_fn(r, ns)))
    out.update(cpu_stamp(nt))
    return out


class Env:
    def __init__(self, args, ctx, rank, world):
        self.args, self.ctx, self.rank, self.world = args, ctx, rank, world
        self.cpu = rank == 0 and world == 1 and args.full and not args.no_cpu_baseline
        self.outputs = None        # --dump-outputs: host copies of the first timed region's last step (Env.timed)
        self._sift = None
        self._real = None
        self.hnsw_cache = {}
        self.keep_tags = set()     # shared builds that a later entry of the plan maps again (their files stay until drop_kept_builds)
        self.kept_builds = {}

    def barrier(self):
        if self.world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def loaded(self, make, file_bytes):
        """make() -> index handle, with what the load left resident in HBM (free bytes before - after, mdb_device_mem_info: tiles / codes /
        graphs AND the load-time accelerators — bf16 fragments, row-major copies, samples, tables) next to the bytes of the files it was
        built from: `hbm` goes into the workload's entry as hbm_resident_bytes / hbm_over_file_bytes"""
        torch.cuda.synchronize()
        f0 = self.ctx.mem_info()[0]
        h = make()
        torch.cuda.synchronize()
        used = f0 - self.ctx.mem_info()[0]
        self.last_hbm = dict(hbm_resident_bytes=int(used), file_bytes=int(file_bytes), hbm_over_file_bytes=used / file_bytes if file_bytes else None)
        return h

    def shared_build(self, tag, build_fn):
        """Index files of a list-sharded workload, built ONCE per job: world == 1 -> build_fn() as is.  world > 1 -> rank 0 builds
        (on its GPU), writes every bytes-like value of the returned dict under MDB_BENCH_TMP (default /tmp) and the small values
        into a pickle; the other ranks wait at a barrier and np.memmap the files — every rank then hands the loader the SAME bytes
        (it keeps the posting lists it owns: mdb_*_load(.., shard_rank, shard_world)), the host holds them once (page cache)
        instead of once per rank (full C4: 30.7 GB -> 250 GB at 8 ranks), and nothing is generated / clustered eight times over.
        Returns (dict, cleanup): call cleanup() once the indexes are loaded."""
        if self.world == 1:
            return build_fn(), (lambda: None)
        import pickle
        import shutil
        base = os.path.join(os.environ.get("MDB_BENCH_TMP", "/tmp"), "mdb_bench_%s_%s" % (os.environ.get("MASTER_PORT", "0"), tag))
        t0 = time.time()
        reuse = tag in self.kept_builds   # a second partitioning of the same collection (keep_tags) maps the files of the first
        if self.rank == 0 and not reuse:
            shutil.rmtree(base, ignore_errors=True)
            os.makedirs(base)
        if self.rank == 0:
            built = build_fn() if not reuse else {}
            small = {}
            for key, val in built.items():
                if isinstance(val, (bytes, bytearray, memoryview)) or (isinstance(val, np.ndarray) and val.nbytes >= (1 << 20)):
                    arr = np.frombuffer(val, np.uint8) if not isinstance(val, np.ndarray) else val
                    arr.tofile(os.path.join(base, key + ".bin"))
                    small[key] = ("file", str(arr.dtype), arr.shape)
                else:
                    small[key] = ("value", val)
            if not reuse:
                with open(os.path.join(base, "meta.pkl"), "wb") as f:
                    pickle.dump(small, f)
            del built
        dist.barrier()
        with open(os.path.join(base, "meta.pkl"), "rb") as f:
            small = pickle.load(f)
        out = {}
        for key, rec in small.items():
            if rec[0] == "file":
                out[key] = np.memmap(os.path.join(base, key + ".bin"), dtype=np.dtype(rec[1]), mode="r", shape=tuple(rec[2]))
            else:
                out[key] = rec[1]
        log("%s: shared build %.1fs (rank 0 builds, %d ranks map %s)" % (tag, time.time() - t0, self.world, base))

        def cleanup():
            dist.barrier()   # every rank has uploaded what it owns
            if tag in self.keep_tags:
                self.kept_builds[tag] = base
            elif self.rank == 0:
                shutil.rmtree(base, ignore_errors=True)
        return out, cleanup

    def drop_kept_builds(self):
        import shutil
        if self.world > 1:
            dist.barrier()
        if self.rank == 0:
            for base in self.kept_builds.values():
                shutil.rmtree(base, ignore_errors=True)
        self.kept_builds = {}

    def same_on_all_ranks(self, arr):
        """world > 1: every rank ends a sharded step with the SAME rows (each merges / permutes the same gathered blocks): a checksum of the
        timed batches' doc ids must agree across the ranks (None on one rank)"""
        if self.world == 1:
            return None
        chk = float(np.asarray(arr, np.int64).astype(np.float64).sum() % 1e15)
        return bool(self.max_over_ranks(chk) == -self.max_over_ranks(-chk))

    def max_over_ranks(self, seconds):
        if self.world > 1:
            t = torch.tensor([seconds], dtype=torch.float64, device="cuda")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            return float(t.item())
        return seconds

    def timed(self, step, steps, warm, profiling=True, disperse=True, long_steps=0, outputs=None):
        """W untimed warm-up steps, then exactly K steps between barrier + synchronize; max over ranks.
        Returns (seconds, dominant-kernel ms summed, launches).  The region that is returned is the FIRST one; `last_dispersion`
        then holds how much the same K steps vary when repeated (a 17 ms region alone cannot tell a 3 % change
        from noise): DISP_REGIONS more regions bracketed the same way (region-level min / median / max of ms per step, the
        returned region included), and one region with an event after every step on the launch stream (per-step GPU time).
        The dispersion regions run with --full only.  outputs() -> {name: device tensor}: the buffers a step writes, copied to the
        host right after the first region (its last step) for --dump-outputs, by the first workload of the run that passes them."""
        for i in range(warm):
            step(i)
        self.ctx.sync()
        # ... and at least WARM_MIN_S of device work: a workload whose W steps are a few hundred microseconds starts its timed region
        # on a GPU that has idled through the host-side preparation before it (r05a: ONE region of flat 1M batch 1 at 0.80 ms per
        # step, the five repeats of the same region at 0.10; the host had issued all of it in 0.5 ms).  The same W steps, repeated.
        t_w = time.perf_counter()
        while warm > 0 and time.perf_counter() - t_w < WARM_MIN_S:
            for i in range(warm):
                step(i)
            self.ctx.sync()
        self.ctx.set_profiling(False)
        self.ctx.get_profile()
        self.barrier()
        host = []   # host time of every step's call in the returned region: where a region loses time to ONE blocking call, it shows here
        t0 = time.perf_counter()
        for j, i in enumerate(range(warm, warm + steps)):
            # the HIP events around the dominant kernel(s) are recorded on every PROF_EVERY-th step of the timed region only: an event
            # pair drains the queue around the kernels it brackets (measured: +9 us per HNSW batch of 64, +40 us at batch 1, +6 us
            # of a 50 us IVF-PQ step) — `kernel_ms` is the mean over the sampled launches
            if j % PROF_EVERY == 0:
                self.ctx.set_profiling(profiling)
            elif j % PROF_EVERY == 1:
                self.ctx.set_profiling(False)
            th = time.perf_counter()
            step(i)
            host.append(time.perf_counter() - th)
        t_issue = time.perf_counter() - t0
        self.barrier()
        elapsed = time.perf_counter() - t0
        kernel_ms, launches = self.ctx.get_profile()
        self.ctx.set_profiling(False)
        elapsed = self.max_over_ranks(elapsed)
        if outputs is not None and self.args.dump_outputs and self.outputs is None:
            self.outputs = {name: t.cpu().numpy() for name, t in outputs().items()}
        self.last_dispersion = None
        if disperse and self.args.full and steps > 0:
            regions = [1000 * elapsed / steps]
            for _ in range(DISP_REGIONS):
                self.barrier()
                t0 = time.perf_counter()
                for i in range(warm, warm + steps):
                    step(i)
                self.barrier()
                regions.append(1000 * self.max_over_ranks(time.perf_counter() - t0) / steps)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
            self.barrier()
            ev[0].record()
            for j, i in enumerate(range(warm, warm + steps)):
                step(i)
                ev[j + 1].record()
            self.barrier()
            per = sorted(ev[j].elapsed_time(ev[j + 1]) for j in range(steps))
            rs = sorted(regions)
            hs = sorted(host)
            self.last_dispersion = dict(
                regions=len(regions), region_ms_per_step=dict(first=regions[0], min=rs[0], median=rs[len(rs) // 2], max=rs[-1]),
                first_region_host=dict(issue_ms=1000 * t_issue, slowest_call_ms=1000 * hs[-1], slowest_call_step=int(np.argmax(host)),
                                       median_call_ms=1000 * hs[len(hs) // 2]),
                per_step_gpu_ms=dict(min=per[0], median=per[len(per) // 2], max=per[-1], steps=steps,
                                     note="events on the launch stream after every step of one more region (this rank)"))
            if long_steps > 0:
                self.barrier()
                t0 = time.perf_counter()
                for j in range(long_steps):
                    step(warm + j % steps)
                self.barrier()
                el = self.max_over_ranks(time.perf_counter() - t0)
                self.last_dispersion["long_region"] = dict(steps=long_steps, ms_per_step=1000 * el / long_steps,
                                                           note="one region of this many steps (the timed batches cycled), bracketed like the timed one")
        return elapsed, kernel_ms, launches

    def sift(self, n, d, nq, qseed):
        """(base rows, queries, description) of the C2/C3 synthetic SIFT-1M; the base is cached across workloads."""
        from muopdb_amd import build as B, synth as S
        if self.args.sift_dir:   # the real dataset, when the box has it
            if self._real is None:
                from muopdb_amd import datasets as DS
                r = DS.load_sift(self.args.sift_dir)
                if r is None:
                    raise SystemExit("--sift-dir %s: sift_base.fvecs / sift_query.fvecs not found" % self.args.sift_dir)
                self._real = (torch.from_numpy(r[0]).cuda(), torch.from_numpy(r[1]).cuda())
            xb, xq = self._real
            if xb.shape[1] != d:
                raise SystemExit("--sift-dir holds %d-d rows, the workload wants %d" % (xb.shape[1], d))
            g = torch.Generator(device="cpu"); g.manual_seed(qseed)
            pick = torch.randint(0, xq.shape[0], (nq,), generator=g).cuda()   # the 10 k queries, drawn with replacement to fill the batches
            return xb[:n].contiguous(), xq[pick].contiguous(), "SIFT-1M (sift_base.fvecs[:%d], sift_query.fvecs)" % min(n, xb.shape[0])
        if self.args.data == "legacy":
            ncl = max(1, min(4096, n // 244))
            if self._sift is None or self._sift[0] != (n, d):
                self._sift = ((n, d), S.gaussian_clusters(n, d, n_clusters=ncl, seed=1))
            g = torch.Generator(device="cpu"); g.manual_seed(1)
            centers = (torch.rand((ncl, d), generator=g) * 218.0).cuda()
            gq = torch.Generator(device="cpu"); gq.manual_seed(qseed)
            qa = torch.randint(0, ncl, (nq,), generator=gq).cuda()
            q = torch.clamp(torch.round(centers[qa] + (torch.randn((nq, d), generator=gq) * 20.0).cuda()), 0, 218).contiguous()
            return self._sift[1], q, "%d isotropic Gaussian clusters, sigma 20, clipped [0,218] (round-1 generator)" % ncl
        kw = {k: v for k, v in (("n_clusters", self.args.sift_clusters), ("sigma", self.args.sift_sigma), ("noise", self.args.sift_noise))
              if v is not None}
        gen = S.SiftLike(d, seed=1, **kw)
        if self._sift is None or self._sift[0] != (n, d):
            self._sift = ((n, d), gen.draw(n, seed=11))
        return self._sift[1], gen.draw(nq, seed=qseed).contiguous(), \
            "block low-rank (32 latent dims) + noise, clipped [0,218], rounded: muopdb_amd.build.SiftLike"


def recall_at_k(found_lo, gt_idx, k):
    hits = 0
    for row, g in zip(found_lo, gt_idx):
        hits += len(set(row[:k].tolist()) & set(g[:k].tolist()))
    return hits / (len(gt_idx) * k)


def hbm_roofline(kernel, abytes_per_launch, kernel_ms, launches, **extra):
    ms = kernel_ms / max(launches, 1)
    ach = abytes_per_launch / (ms * 1e-3) / 1e9 if launches else None
    r = dict(bound="hbm", kernel=kernel, achieved=ach, peak=HBM_PEAK_GBS, unit="GB/s", frac=ach / HBM_PEAK_GBS if ach else None,
             traffic=None, bytes_per_launch=abytes_per_launch, kernel_ms=ms)
    r.update(extra)
    return r


def exchange_times(env, step, steps, warm):
    """world > 1: one more (untimed) pass over the timed steps with events around every collective and merge call
    (muopdb_amd.distributed.StepTimer): the all-gathers' own device time and the merge kernels', per step, max over ranks."""
    if env.world == 1:
        return None
    from muopdb_amd import distributed as D
    D.TIMER = D.StepTimer()
    env.barrier()
    for i in range(warm, warm + steps):
        step(i)
    env.barrier()
    ms = D.TIMER.ms()
    D.TIMER = None
    out = {}
    for kind in ("probes_allgather", "coarse_allgather", "merge_coarse", "points_allgather", "merge_points", "rows_allgather", "rows_permute"):
        if kind in ms:
            out[kind + "_ms_per_step"] = env.max_over_ranks(ms[kind]["total_ms"] / steps)
    out["ranks"] = env.world
    out["backend"] = dist.get_backend()
    return out


def partitioning(shard, world):
    """how a workload's data and queries are divided among the job's ranks (both partitionings are measured)"""
    if world == 1:
        return "one GPU"
    return {"lists": "posting lists sharded x%d, every rank sees the whole batch, all-gather of points blocks + exact (distance, point id) merge",
            "users": "users sharded x%d (user slot u on rank u %% world), pairs routed to their owner, all-gather of finished rows only",
            "batch": "replicas x%d, contiguous batch slices, all-gather of finished rows only"}[shard] % world


def finish(out, disp, step_bytes):
    """every workload: `step_frac` = the step's algorithmic bytes / ms_per_step / 8 TB/s (the whole step against the HBM roof, not
    only its dominant kernel) and the dispersion of the timed region (Env.timed)."""
    out["step_frac"] = step_bytes / (out["ms_per_step"] * 1e-3) / 1e9 / HBM_PEAK_GBS if step_bytes else None
    out["step_bytes"] = step_bytes
    out["dispersion"] = disp
    return out


# ------------------------------------------------------------------------------------------ HNSW (headline)
def run_hnsw(env, batch=None, graph=None, n=None, extras=True, steps=None, warm=None, ef=None):
    """BASELINE config C2.  batch 64 = the headline; batch 1 = the metric's other batch size (same resident graph);
    graph "insert" = the same workload on a graph built by HnswBuilder::insert's algorithm (what MuopDB itself would write)."""
    from muopdb_amd import build as B, synth as S
    from muopdb_amd.index import BlockBasedHnsw
    args, ctx, rank, world = env.args, env.ctx, env.rank, env.world
    n = n or args.n or 1_000_000
    d = args.dim or 128
    batch = batch or args.batch or 64
    graph = graph or args.graph
    k, ef = args.k, ef or args.ef
    steps, warm = steps or args.steps, warm if warm is not None else args.warmup
    t0 = time.time()
    nq = (steps + warm) * batch
    x, queries, desc = env.sift(n, d, nq, 1000 + rank)
    n = x.shape[0]
    log("data %.1fs" % (time.time() - t0))
    key = (n, d, graph, args.max_neighbors)
    if key not in env.hnsw_cache:
        t0 = time.time()
        if graph == "insert":
            index_bytes, vec_bytes = B.hnsw_files_by_insertion(ctx, x, max_neighbors=args.max_neighbors, max_layers=8, ef_construction=100, seed=1)
        else:
            index_bytes, vec_bytes = S.hnsw_files(x, max_neighbors=args.max_neighbors, max_layers=8, kcand=2 * args.max_neighbors, seed=1)
        build_s = time.time() - t0
        log("graph build (%s) %.1fs (%d MiB index)" % (graph, build_s, len(index_bytes) >> 20))
        t0 = time.time()
        env.hnsw_cache.clear()   # one resident graph at a time
        env.hnsw_cache[key] = (env.loaded(lambda: BlockBasedHnsw(ctx, index_bytes, vec_bytes, d), len(index_bytes) + len(vec_bytes)), index_bytes, vec_bytes, build_s)
        env.hnsw_hbm = getattr(env, "hnsw_hbm", {})
        env.hnsw_hbm[key] = env.last_hbm
        log("load %.1fs" % (time.time() - t0))
    hnsw, index_bytes, vec_bytes, build_s = env.hnsw_cache[key]
    if batch == 64 and graph == args.graph and (ef or args.ef) == args.ef:
        dump(args, rank, "hnsw", index=index_bytes, vectors=vec_bytes, **{"queries.f32": queries.cpu().numpy()})
    ids = torch.zeros((batch, k, 2), dtype=torch.int64, device="cuda")
    sc = torch.zeros((batch, k), dtype=torch.float32, device="cuda")
    cn = torch.zeros(batch, dtype=torch.int32, device="cuda")

    def step(i, keep=None):
        q = queries[i * batch:(i + 1) * batch]
        hnsw.ann_search_device(q.data_ptr(), batch, k, ef, ids.data_ptr(), sc.data_ptr(), cn.data_ptr())
        if keep is not None:
            keep.append(ids[:, :, 0].clone())

    # the headline also runs one LONG region (>= 200 steps, the timed batches cycled): K = 20 steps are ~15 ms, inside the 3-8 % two
    # boxes differ by, and a round-to-round delta of that size cannot be told from noise; `value` stays the K-step region's.
    # Without --full the timed region carries no kernel brackets and nothing else follows it.
    elapsed, kernel_ms, launches = env.timed(step, steps, warm, profiling=args.full, long_steps=max(LONG_STEPS, steps) if extras else 0,
                                             outputs=lambda: dict(ids=ids, scores=sc, counts=cn))
    disp = env.last_dispersion
    how = ("exact k-NN + select_neighbors_heuristic (bulk build)" if graph == "knn"
           else "HnswBuilder::insert's algorithm, wave-batched (muopdb_amd.build.insert_hnsw, ef_construction=100)")
    config = {"workload": "%s %dx%d f32 (%s); HNSW max_neighbors=%d ef=%d top-%d batch=%d per GPU; graph: %s; replicas"
                          % ("SIFT-1M" if args.sift_dir else "SIFT-1M-like synthetic", n, d, desc, args.max_neighbors, ef, k, batch, how),
              "n": n, "dim": d, "batch": batch, "ef": ef, "k": k, "index": "hnsw", "graph": graph,
              "data": "sift1m" if args.sift_dir else args.data, "parallelism": "replica x%d" % world, "graph_build_s": build_s}
    if not args.full:
        return dict(value=world * steps * batch / elapsed, ms_per_step=1000 * elapsed / steps, config=config, steps=steps, warmup=warm)
    # untimed re-run of the timed batches: results for recall + exact traversal counters per launch
    found, evals, expanded, abytes = [], 0, 0, 0
    for i in range(warm, warm + steps):
        step(i, found)
        st = ctx.stats()
        evals += st["distance_evals"]; expanded += st["expanded_nodes"]; abytes += st["algorithmic_bytes"]
    found = torch.cat(found).cpu().numpy()
    tq = queries[warm * batch:(warm + steps) * batch]
    gt, _ = S.exact_knn(x, k, queries=tq, f64=True)
    rec = recall_at_k(found, gt.cpu().numpy(), k)
    out = dict(
        value=world * steps * batch / elapsed, ms_per_step=1000 * elapsed / steps, recall_at_10=rec, config=config,
        # ef <= 448: the traversal is three kernels — the upper layers' distance table (fused with the top layers' traversal — on sorted
        # positions since round 6, mdb_hnsw_rank.hip.h — for batches >= 32), layer 1's single-wave traversal and the layer-0 instance of
        # the beam kernel (mdb_hnsw_upper.hip); the bracket is their sum, the algorithmic bytes are the whole traversal's
        roofline=hbm_roofline("hnsw_upper_top_rank_kernel|hnsw_upper_table*_kernel+hnsw_upper_kernel+hnsw_beam_kernel<L0>" if ef <= 448 else "hnsw_search_kernel",
                              abytes / steps, kernel_ms, launches,
                              evals_per_query=evals / (steps * batch), expanded_per_query=expanded / (steps * batch)),
    )
    finish(out, disp, abytes / steps)
    out.update(getattr(env, "hnsw_hbm", {}).get(key) or {})
    out["steps"], out["warmup"] = steps, warm
    if batch == 64 and graph == args.graph:
        out["roofline"]["traffic"], out["roofline"]["traffic_source"] = measured_traffic("hnsw", out["config"])
    if extras and args.streams > 1:
        # Extra, NOT the headline: the same K batches issued round-robin on several HIP streams (one context +
        # attached index handle each, all over the same resident graph), i.e. several batches of 64 in flight.  One batch occupies 64 of the 256 CUs for
        # its whole latency-bound traversal, so a serving process overlaps batches to fill the chip.
        from muopdb_amd import lib as L
        lanes = []
        for _ in range(args.streams):
            st_ = torch.cuda.Stream()
            c_ = L.Context(torch.cuda.current_device()); c_.set_stream(st_.cuda_stream)
            # one resident index, one handle per stream over it (mdb_hnsw_attach)
            lanes.append((st_, c_, hnsw.attach(c_), torch.zeros_like(ids), torch.zeros_like(sc), torch.zeros_like(cn)))
        torch.cuda.synchronize()

        def cstep(i):
            _, _, h_, i_, s_, c_n = lanes[i % len(lanes)]
            q = queries[i * batch:(i + 1) * batch]
            h_.ann_search_device(q.data_ptr(), batch, k, ef, i_.data_ptr(), s_.data_ptr(), c_n.data_ptr())

        for i in range(warm):
            cstep(i)
        env.barrier()
        t0 = time.perf_counter()
        for i in range(warm, warm + steps):
            cstep(i)
        env.barrier()
        el = env.max_over_ranks(time.perf_counter() - t0)
        same = True
        for j, i in enumerate(range(warm + steps - len(lanes), warm + steps)):  # last batch of every lane vs the serial run
            same &= bool(torch.equal(lanes[i % len(lanes)][3][:, :, 0].cpu(), torch.from_numpy(found[(i - warm) * batch:(i - warm + 1) * batch])))
        out["concurrent"] = dict(streams=args.streams, value=world * steps * batch / el, ms_per_step=1000 * el / steps,
                                 ids_equal_serial=same, note="same batches, several in flight on attached handles over one resident index "
                                      "(GPU_MAX_HW_QUEUES=%s); not the headline value" % os.environ.get("GPU_MAX_HW_QUEUES"))
        for lane_ in lanes:
            lane_[2].close(); lane_[1].close()
    if env.cpu:
        import oracle
        o = oracle.BlockBasedHnsw(index_bytes, vec_bytes, d)
        qh = tq.cpu().numpy()
        out["cpu_baseline"] = cpu_baseline(
            lambda m: o.ann_search(qh[:m], k, ef, threads=1), lambda m, t: o.ann_search(qh[:m], k, ef, threads=t), len(qh),
            args.cpu_seconds if extras else min(args.cpu_seconds, 4.0), min(64, len(qh)),
            lambda r, m: all(r.doc_ids(i) == [int(v) for v in found[i][:int(r.counts[i])]] for i in range(min(m, 256))),
            "%d of the timed queries, one thread (the reference runs one query per task, no intra-query parallelism); index fully memory-resident")
    return out


# ------------------------------------------------------------------------------------------ flat
def run_flat(env, n=None, batch=None, steps=None, warm=None):
    """flat brute-force L2: the C2/C3 1M base (default inside --workload all) or BASELINE config C1 (10k x 128, batch 1,
    py/create_test_hdf5.py-shaped data) with --workload flat."""
    from muopdb_amd import build as B, synth as S
    from muopdb_amd.index import FlatIndex
    args, ctx, rank, world = env.args, env.ctx, env.rank, env.world
    n = n or args.n or 10_000
    d = args.dim or 128
    batch = batch or args.batch or 1
    k = args.k
    steps, warm = steps or args.steps, args.warmup if warm is None else warm
    nq = (steps + warm) * batch
    if n >= 100_000:  # "flat SIFT-1M" of the north star: the C2/C3 synthetic SIFT-like base
        x, queries, desc = env.sift(n, d, nq, 2000 + rank)
        x = x.contiguous()
    else:             # C1: py/create_test_hdf5.py-shaped data
        desc = "create_test_hdf5-like: 10 clusters, centre i*100, N(0, 5^2)"
        g = torch.Generator(device="cpu"); g.manual_seed(42)
        lab = torch.arange(n) % 10
        x = (lab[:, None].float() * 100.0 + torch.randn((n, d), generator=g) * 5.0)
        x = x[torch.randperm(n, generator=g)].cuda().contiguous()
        ql = torch.randint(0, 10, (nq,), generator=g)
        queries = (ql[:, None].float() * 100.0 + torch.randn((nq, d), generator=g) * 5.0).cuda().contiguous()
    # rows are sharded across ranks (SURVEY.md §8e flat: row-range shards); here every rank scans its shard
    lo, hi = rank * n // world, (rank + 1) * n // world
    idx = env.loaded(lambda: FlatIndex(ctx, None, device_ptr=x[lo:hi].data_ptr(), n=hi - lo, d=d), (hi - lo) * d * 4)
    hbm = env.last_hbm
    if args.dump_dir:
        from muopdb_amd import formats as F
        dump(args, rank, "flat_b%d" % batch, vectors=F.write_vector_file(x.cpu().numpy()), **{"queries.f32": queries.cpu().numpy()})
    ids = torch.zeros((batch, k), dtype=torch.int32, device="cuda")
    ds = torch.zeros((batch, k), dtype=torch.float32, device="cuda")

    def step(i):
        idx.search_device(queries[i * batch:(i + 1) * batch].data_ptr(), batch, k, ids.data_ptr(), ds.data_ptr())

    elapsed, kernel_ms, launches = env.timed(step, steps, warm, outputs=lambda: dict(ids=ids, scores=ds))
    disp = env.last_dispersion
    abytes = (hi - lo) * d * 4 + batch * d * 4 + batch * k * 8
    # recall@k of the last timed batch against the f64 brute force (untimed re-run of that batch)
    last = warm + steps - 1
    step(last)
    gt, _ = S.exact_knn(x[lo:hi], k, queries=queries[last * batch:(last + 1) * batch], f64=True)
    rec = recall_at_k(ids.cpu().numpy().astype(np.int64), gt.cpu().numpy(), k)
    batched = batch >= 8 and (hi - lo) >= 65536  # mdb_flat_mfma.hip: sample bound + MFMA filter + exact refine
    out = dict(value=steps * batch / elapsed, ms_per_step=1000 * elapsed / steps, recall_at_10=rec,
               config={"workload": "flat brute-force L2 %dx%d f32 (%s), batch=%d, top-%d (row-sharded x%d)" % (n, d, desc, batch, k, world),
                       "n": n, "dim": d, "batch": batch, "k": k, "index": "flat", "data": args.data},
               # batches <= 4 over bases of <= 1024 tiles (C1) take flat_small_scan_kernel (one wave per tile, no block selector)
               roofline=hbm_roofline("flat_bf16_filter_kernel" if batched else
                                     ("flat_small_scan_kernel" if batch <= 4 and (hi - lo) <= 65536 and d % 16 == 0 and d <= 128 and k <= 64 else "flat_scan_kernel"),
                                     abytes, kernel_ms, launches))
    finish(out, disp, abytes)   # the step's algorithmic bytes: the base once (however many passes the filter takes)
    out.update(hbm)
    out["steps"], out["warmup"] = steps, warm
    if (hi - lo) * d * 4 < (64 << 20):
        out["note"] = "launch-latency bound: the base (%.1f MB) sits in the Infinity Cache, SURVEY 8d" % ((hi - lo) * d * 4 / 1e6)
    if batched:
        # the filter streams a bf16 copy of the base in matrix-core fragment order — the hi halves only (2 bytes per element, one
        # MFMA product per pair: MDB_BF_X1, the default for L2 stores) or hi + lo (4 bytes, three products) — plus a 4-byte norm per
        # row, once per group of queries: 32 QB per block (QB = 1 / 2 / 4 for batches up to 32 / 64 / more), 512 in the block-shared
        # form of batches >= 512.  The roofline is priced on THOSE bytes: what the launch has to read.
        x1 = int(os.environ.get("MDB_BF_X1", "1")) >= 1
        blocked = x1 and d <= 128 and d > 112 and batch >= int(os.environ.get("MDB_BF_BLOCK_MIN_B", "512"))
        qb = 4 if batch > 64 else 2 if batch > 32 else 1
        groups = (batch + 511) // 512 if blocked else (batch + 32 * qb - 1) // (32 * qb)
        dpad = (d + 15) // 16 * 16
        r = out["roofline"]
        r["kernel"] = "flat_bf16x1_block_kernel (filter pass)" if blocked else "flat_bf16_filter_kernel"
        r["operand"] = "bf16 hi fragments (2 B/element) + norms" if x1 else "bf16 hi + lo fragments (4 B/element) + norms"
        r["bytes_per_launch"] = float((hi - lo) * (dpad * (2 if x1 else 4) + 4) * groups)
        r["achieved"] = r["bytes_per_launch"] / (r["kernel_ms"] * 1e-3) / 1e9
        r["frac"] = r["achieved"] / HBM_PEAK_GBS
        r["mfma_tflops"] = (1 if x1 else 3) * 2.0 * batch * (hi - lo) * d / (r["kernel_ms"] * 1e-3) / 1e12
        r["mfma_frac_of_bf16_peak"] = r["mfma_tflops"] / 2500.0
    out["roofline"]["traffic"], out["roofline"]["traffic_source"] = measured_traffic("flat_b64" if batched else "flat", out["config"])
    if batched:
        out["roofline"]["mfma_busy"] = measured_mfma("flat_b64", out["config"])
    if env.cpu:
        import oracle
        xb, qh = x[lo:hi].cpu().numpy(), queries[warm * batch:].cpu().numpy()
        got = []                                    # the GPU's rows for the first timed queries (untimed re-run)
        for i in range(warm, warm + min(steps, max(1, 32 // batch))):
            step(i)
            got.append(ids.cpu().numpy().astype(np.int64))
        got = np.concatenate(got)
        out["cpu_baseline"] = cpu_baseline(
            lambda m: oracle.flat_topk(0, xb, qh[:m], k, threads=1), lambda m, t: oracle.flat_topk(0, xb, qh[:m], k, threads=t), len(qh),
            args.cpu_seconds, min(4, len(qh)),
            lambda r, m: bool(np.array_equal(np.asarray(r[0])[:min(m, len(got))].astype(np.int64), got[:min(m, len(got))])),
            "%d queries, one thread")
    idx.close()
    return out


# ------------------------------------------------------------------------------------------ IVF-PQ
def pq_scan_kernel_name(batch):
    """the library's choice (mdb_ivf.hip): two-phase scan (bounds, then exact distances of the candidates) from 512 queries per batch;
    below, the fused step (ivf_prep_kernel + ivf_pq_fused_kernel: the bracketed kernel is the per-query one)"""
    return "ivf_scan_pq3_kernel+ivf_pq3_refine_kernel" if batch >= 512 else "ivf_pq_fused_kernel"


def ivfpq_measure(env, ivf, x, queries, batch, k, P, steps, warm, gt=None, nrec=0, disperse=True, shard="lists"):
    """one (nprobe) setting: timed steps + untimed re-run for results / counters"""
    from muopdb_amd import lib as L
    from muopdb_amd import distributed as D
    ctx, world = env.ctx, env.world
    by_batch = world > 1 and shard == "batch"
    # world > 1: the EXACT sharded step — the search writes this rank's (distance, point id) rows straight into its points block
    gather = D.PointsGather(ctx, batch, k, "cuda") if (world > 1 and not by_batch) else None
    # ... or replicas: this rank answers its contiguous slice of the batch whole, ONE all-gather of finished rows (no merge)
    rows = D.RowsExchange(batch, k, D.route_by_batch(batch, world), env.rank, "cuda") if by_batch else None
    ids = torch.zeros((batch, k, 2), dtype=torch.int64, device="cuda")
    sc = torch.zeros((batch, k), dtype=torch.float32, device="cuda")
    cn = torch.zeros(batch, dtype=torch.int32, device="cuda")

    def step(i, keep=None):
        q = queries[i * batch:(i + 1) * batch]
        if by_batch:
            ql = rows.local_queries(q)
            ctx.check(ctx.lib.mdb_ivf_search(ivf.h, C.c_void_p(ql.data_ptr()), C.c_size_t(rows.n_local), None, C.c_size_t(P), C.c_size_t(k),
                                             C.c_int(L.MEM_DEVICE), C.c_void_p(rows.ids.data_ptr()), C.c_void_p(rows.scores.data_ptr()),
                                             C.c_void_p(rows.counts.data_ptr())))
            res = rows.gather()[0]
        elif world > 1:
            # the coarse quantizer is sharded too: 1/world of the centroids per rank + one all-gather of (distance, id) rows
            probes = D.sharded_probes(ctx, ivf, q.data_ptr(), batch, P, q.device)
            ctx.check(ctx.lib.mdb_ivf_search_shard(ivf.h, C.c_void_p(q.data_ptr()), C.c_size_t(batch), C.c_void_p(probes.data_ptr()),
                                                   C.c_size_t(P), C.c_size_t(k), C.c_int(L.MEM_DEVICE), None, C.c_size_t(0), C.c_size_t(0),
                                                   C.c_void_p(gather.send.data_ptr())))
            # ONE RCCL all-gather of the points blocks + merge by (distance, point id), then remap
            res, _, _ = gather.gather_merge_ivf(ivf)
        else:
            ctx.check(ctx.lib.mdb_ivf_search(ivf.h, C.c_void_p(q.data_ptr()), C.c_size_t(batch), None, C.c_size_t(P), C.c_size_t(k),
                                             C.c_int(L.MEM_DEVICE), C.c_void_p(ids.data_ptr()), C.c_void_p(sc.data_ptr()),
                                             C.c_void_p(cn.data_ptr())))
            res = ids
        if keep is not None:
            keep.append(res[:, :, 0].clone())

    outputs = (lambda: dict(ids=ids, scores=sc, counts=cn)) if world == 1 else None
    elapsed, kernel_ms, launches = env.timed(step, steps, warm, disperse=disperse, outputs=outputs)
    disp = env.last_dispersion
    found, scored, abytes = [], 0, 0
    for i in range(warm, warm + steps):
        step(i, found)
        st = ctx.stats(); scored += st["scored_vectors"]; abytes += st["algorithmic_bytes"]
    found = torch.cat(found).cpu().numpy()
    rec = recall_at_k(found[:nrec], gt, k) if gt is not None else None
    ex = exchange_times(env, step, steps, warm) if disperse else None
    across = env.same_on_all_ranks(found)
    same = None
    if by_batch:   # every rank holds the whole index: the gathered rows of the last timed batch against ONE unsharded call over that batch
        i = warm + steps - 1
        q = queries[i * batch:(i + 1) * batch]
        ctx.check(ctx.lib.mdb_ivf_search(ivf.h, C.c_void_p(q.data_ptr()), C.c_size_t(batch), None, C.c_size_t(P), C.c_size_t(k),
                                         C.c_int(L.MEM_DEVICE), C.c_void_p(ids.data_ptr()), C.c_void_p(sc.data_ptr()), C.c_void_p(cn.data_ptr())))
        step(i)                                  # this rank's slice -> its block, all-gather ...
        g_ids, g_sc, g_cn, _ = rows.gather()     # ... and the rows in batch order once more (the same blocks)
        same = bool(torch.equal(g_ids, ids) and torch.equal(g_sc.view(torch.int32), sc.view(torch.int32)) and torch.equal(g_cn, cn))
        same = bool(env.max_over_ranks(0.0 if same else 1.0) == 0.0)
    return dict(elapsed=elapsed, kernel_ms=kernel_ms, launches=launches, found=found, scored=scored, abytes=abytes, recall=rec, disp=disp,
                exchange=ex, rows_equal_unsharded=same, rows_equal_across_ranks=across)


def build_ivfpq(env, x, nlist, seed=3):
    """IVF centroids + PQ codebook + codes + files for device rows x (build side: muopdb_amd.build)"""
    from muopdb_amd import build as B, formats as F, synth as S
    from muopdb_amd.index import ProductQuantizer
    n, d = x.shape
    ctx = env.ctx
    cent = B.kmeans(ctx, x, nlist, iters=6, seed=seed, sample=min(n, 400_000))
    assign = B.assign_nearest(ctx, x, cent)
    cb = B.train_pq_codebook(ctx, x, 8, 8, iters=6, seed=seed + 1, sample=100_000)
    pq = ProductQuantizer(d, 8, 8, cb)
    codes = pq.quantize(env.ctx, x.cpu().numpy())
    pls = B.posting_lists_from_assignment(assign, nlist)
    index_bytes = F.write_ivf_index(cent.cpu().numpy(), np.arange(n, dtype=np.uint64), pls, quantized_dimension=d // 8)
    return index_bytes, F.write_vector_file(codes), pq, cb


def run_ivfpq(env, shard=None, no_sweep=False):
    """BASELINE config C3: SIFT-1M-like, IVF nlist=4096 + PQ m=16 (subdim 8) nbits=8, batch 256; nprobe sweep.
    world > 1: posting-list shards + exact merge, or (shard="batch") replicas answering contiguous slices of the batch."""
    from muopdb_amd import build as B, synth as S
    from muopdb_amd.index import BlockBasedIvf
    args, ctx, rank, world = env.args, env.ctx, env.rank, env.world
    n = args.n or 1_000_000
    d = args.dim or 128
    batch = args.batch or 256
    k, P = args.k, args.nprobe or 16
    steps, warm = args.steps, args.warmup
    nlist = args.nlist or max(1, min(4096, n // 244))
    nq = (steps + warm) * batch
    shard = (shard or args.shard) if world > 1 else "lists"
    by_batch = shard == "batch"
    x, queries, desc = env.sift(n, d, nq, 3000)  # every rank sees the SAME batch (list shards: all of it; batch split: its slice of it)
    t0 = time.time()
    index_bytes, vec_bytes, pq, cb = build_ivfpq(env, x, nlist)
    log("ivf-pq build %.1fs" % (time.time() - t0))
    ivf = env.loaded(lambda: BlockBasedIvf(ctx, index_bytes, vec_bytes, pq, shard_rank=0 if by_batch else rank, shard_world=1 if by_batch else world),
                     len(index_bytes) + len(vec_bytes))
    hbm = env.last_hbm
    dump(args, rank, "ivfpq", index=index_bytes, vectors=vec_bytes, **{"queries.f32": queries.cpu().numpy(), "codebook.f32": cb})
    tq = queries[warm * batch:(warm + steps) * batch]
    nrec = min(len(tq), 2560, max(256, int(1.3e10 // n)))  # f64 ground truth for a bounded number of the timed queries
    gt = S.exact_knn(x, k, queries=tq[:nrec], f64=True)[0].cpu().numpy()
    m = ivfpq_measure(env, ivf, x, queries, batch, k, P, steps, warm, gt, nrec, shard=shard)
    part = partitioning(shard, world)
    out = dict(value=steps * batch / m["elapsed"], ms_per_step=1000 * m["elapsed"] / steps, recall_at_10=m["recall"], scaling="strong",
               partitioning=part, shard=shard if world > 1 else None,
               config={"workload": "SIFT-1M-like synthetic %dx%d (%s), IVF nlist=%d + PQ m=16 nbits=8 (symmetric distance), nprobe=%d, "
                                   "batch=%d, top-%d, %s" % (n, d, desc, nlist, P, batch, k, part),
                       "n": n, "dim": d, "batch": batch, "k": k, "nprobe": P, "index": "ivf-pq", "data": args.data, "parallelism": part},
               roofline=hbm_roofline(pq_scan_kernel_name(batch), m["abytes"] / steps, m["kernel_ms"], m["launches"],
                                     scored_per_query=m["scored"] / (steps * batch)))
    finish(out, m["disp"], m["abytes"] / steps)
    out.update(hbm)
    if m["exchange"]:
        out["exchange"] = m["exchange"]
    if m.get("rows_equal_unsharded") is not None:
        out["rows_equal_unsharded"] = m["rows_equal_unsharded"]
    if m.get("rows_equal_across_ranks") is not None:
        out["rows_equal_across_ranks"] = m["rows_equal_across_ranks"]
    out["roofline"]["traffic"], out["roofline"]["traffic_source"] = measured_traffic("ivfpq", out["config"])
    if args.full and args.streams > 1 and world == 1:
        # Extra: the same batches round-robin on several HIP streams, each through its own handle ATTACHED to the one resident
        # index (mdb_ivf_attach: shared posting lists / tombstones, own scratch + stream) — several batches in flight.
        from muopdb_amd import lib as L
        lanes = []
        for _ in range(args.streams):
            st_ = torch.cuda.Stream()
            c_ = L.Context(torch.cuda.current_device()); c_.set_stream(st_.cuda_stream)
            lanes.append((st_, c_, ivf.attach(c_), torch.zeros((batch, k, 2), dtype=torch.int64, device="cuda"),
                          torch.zeros((batch, k), dtype=torch.float32, device="cuda"), torch.zeros(batch, dtype=torch.int32, device="cuda")))
        torch.cuda.synchronize()

        def cstep(i):
            _, c_, h_, i_, s_, n_ = lanes[i % len(lanes)]
            q = queries[i * batch:(i + 1) * batch]
            c_.check(c_.lib.mdb_ivf_search(h_.h, C.c_void_p(q.data_ptr()), C.c_size_t(batch), None, C.c_size_t(P), C.c_size_t(k),
                                           C.c_int(L.MEM_DEVICE), C.c_void_p(i_.data_ptr()), C.c_void_p(s_.data_ptr()), C.c_void_p(n_.data_ptr())))

        for i in range(warm):
            cstep(i)
        env.barrier()
        t0 = time.perf_counter()
        for i in range(warm, warm + steps):
            cstep(i)
        env.barrier()
        el = time.perf_counter() - t0
        same = True
        for i in range(max(warm, warm + steps - len(lanes)), warm + steps):  # last batch of every lane vs the serial run
            same &= bool(np.array_equal(lanes[i % len(lanes)][3][:, :, 0].cpu().numpy(), m["found"][(i - warm) * batch:(i - warm + 1) * batch]))
        out["concurrent"] = dict(streams=args.streams, value=steps * batch / el, ms_per_step=1000 * el / steps, ids_equal_serial=same,
                                 note="same batches, several in flight on handles attached to ONE resident index; not the workload's value")
        for lane_ in lanes:
            lane_[2].close(); lane_[1].close()
    if args.full and not (args.no_sweep or no_sweep):
        sweep = []
        for p in (1, 8, 16, 32, 64):
            if p > nlist:
                continue
            s = m if p == P else ivfpq_measure(env, ivf, x, queries, batch, k, p, steps, warm, gt, nrec, disperse=False, shard=shard)
            sweep.append(dict(nprobe=p, recall_at_10=s["recall"], value=steps * batch / s["elapsed"], ms_per_step=1000 * s["elapsed"] / steps,
                              scan_kernel_ms=s["kernel_ms"] / max(s["launches"], 1), scored_per_query=s["scored"] / (steps * batch)))
        out["sweep"] = sweep
    if env.cpu:
        import oracle
        o = oracle.BlockBasedIvf(index_bytes, vec_bytes, oracle.Quant(oracle.QUANT_PQ, oracle.METRIC_L2, 8, 8, cb))
        qh = tq.cpu().numpy()
        out["cpu_baseline"] = cpu_baseline(
            lambda m_: o.search(qh[:m_], k, num_probes=P, threads=1), lambda m_, t: o.search(qh[:m_], k, num_probes=P, threads=t), len(qh),
            args.cpu_seconds, min(32, len(qh)),
            lambda r, m_: all(r.doc_ids(i) == [int(v) for v in m["found"][i][:int(r.counts[i])]] for i in range(min(m_, 256))),
            "%d queries, one thread")
    ivf.close()
    return out


def run_c5_full(env, steps=None, warm=None):
    """BASELINE config C5 WHOLE on ONE GPU: all 100M x 128 rows as 16-byte PQ codes (1.6 GB) in 65 536 posting lists, nprobe 64,
    batch 4096 — the N = 1 point C5's strong scaling is read against (8 x the per-GPU shard step of c5_shard_per_gpu vs this)."""
    from muopdb_amd import synth as S
    from muopdb_amd.index import BlockBasedIvf
    args, ctx = env.args, env.ctx
    batch = args.batch or 4096
    k, P = args.k, args.nprobe or 64
    steps, warm = steps or args.steps, args.warmup if warm is None else warm
    total = args.n or 100_000_000
    t0 = time.time()
    full = S.c5_index(ctx, total=total, world=1, rank=0, nlist=args.nlist or 65536, log=log)
    build_s = time.time() - t0
    log("C5 full build %.1fs: %d vectors in %d lists" % (build_s, full["n"], full["owned_lists"]))
    torch.cuda.empty_cache()
    t0 = time.time()
    ivf = env.loaded(lambda: BlockBasedIvf(ctx, full["index"], full["vectors"], full["pq"]), len(full["index"]) + len(full["vectors"]))
    hbm = env.last_hbm
    load_s = time.time() - t0
    queries = full["gen"].draw((steps + warm) * batch, seed=5000).contiguous()
    dump(args, env.rank, "c5full", index=full["index"], vectors=full["vectors"], **{"queries.f32": queries.cpu().numpy(), "codebook.f32": full["codebook"]})
    m = ivfpq_measure(env, ivf, None, queries, batch, k, P, steps, warm)
    out = dict(value=steps * batch / m["elapsed"], ms_per_step=1000 * m["elapsed"] / steps, recall_at_10=None, scaling="strong",
               config={"workload": "C5 on ONE GPU: %d x 128 SiftLike rows as 16-byte PQ codes in %d posting lists (all resident), nprobe=%d, "
                                   "batch=%d, top-%d" % (full["n"], full["nlist"], P, batch, k),
                       "n": full["n"], "dim": 128, "batch": batch, "k": k, "nprobe": P, "index": "ivf-pq", "data": "lowrank",
                       "build_s": build_s, "load_s": load_s},
               roofline=hbm_roofline(pq_scan_kernel_name(batch), m["abytes"] / steps, m["kernel_ms"], m["launches"],
                                     scored_per_query=m["scored"] / (steps * batch)))
    finish(out, m["disp"], m["abytes"] / steps)
    out.update(hbm)
    out["steps"], out["warmup"] = steps, warm
    out["roofline"]["traffic"], out["roofline"]["traffic_source"] = measured_traffic("c5full", out["config"])
    if env.cpu:
        import oracle
        o = oracle.BlockBasedIvf(full["index"], full["vectors"], oracle.Quant(oracle.QUANT_PQ, oracle.METRIC_L2, 8, 8, full["codebook"]))
        qh = queries[warm * batch:].cpu().numpy()
        out["cpu_baseline"] = cpu_baseline(
            lambda m_: o.search(qh[:m_], k, num_probes=P, threads=1), lambda m_, t: o.search(qh[:m_], k, num_probes=P, threads=t), len(qh),
            min(args.cpu_seconds, 6.0), min(8, len(qh)),
            lambda r, m_: all(r.doc_ids(i) == [int(v) for v in m["found"][i][:int(r.counts[i])]] for i in range(min(m_, 256))),
            "%d queries, one thread")
    ivf.close()
    env.c5_full = full   # run_c5 reads rank 0's shard of 8 out of the same files instead of generating its own
    return out


def run_c5_sharded(env, steps=None, warm=None, shard=None):
    """BASELINE config C5 over the ranks of this job (world > 1): the 100M-code index is built ONCE (rank 0, Env.shared_build), every
    rank loads the posting lists it owns from the same files (size-balanced owners, mdb_ivf_load(.., rank, world)) plus the
    replicated coarse quantizer, and a step is the EXACT sharded search: coarse search over 1/world of the centroids + one all-gather
    of [b][P] keys, search of the owned lists into a points block, ONE all-gather of the blocks, (distance, point id) merge and
    remap on every rank.  Strong scaling: the same batch on every rank; compare with c5_full_1gpu (N = 1)."""
    from muopdb_amd import synth as S
    from muopdb_amd.index import BlockBasedIvf
    args, ctx, rank, world = env.args, env.ctx, env.rank, env.world
    batch = args.batch or 4096
    k, P = args.k, args.nprobe or 64
    steps, warm = steps or args.steps, args.warmup if warm is None else warm
    total = args.n or 100_000_000
    shard = shard or args.shard
    by_batch = shard == "batch"    # replicas (1.6 GB of codes fits a GPU 180 times over): the comparator SURVEY 8e asks for
    t0 = time.time()

    def build():
        full = S.c5_index(ctx, total=total, world=1, rank=0, nlist=args.nlist or 65536, log=log)
        return dict(index=full["index"], vectors=full["vectors"], codebook=np.asarray(full["codebook"], np.float32), n=full["n"],
                    nlist=full["nlist"])

    full, cleanup = env.shared_build("c5", build)
    build_s = time.time() - t0
    from muopdb_amd.index import ProductQuantizer
    pq = ProductQuantizer(128, 8, 8, full["codebook"])
    t0 = time.time()
    ivf = env.loaded(lambda: BlockBasedIvf(ctx, full["index"], full["vectors"], pq, shard_rank=0 if by_batch else rank, shard_world=1 if by_batch else world),
                     len(full["index"]) + len(full["vectors"]))
    hbm = env.last_hbm
    load_s = time.time() - t0
    cleanup()
    queries = S.SiftLike(128, seed=4).draw((steps + warm) * batch, seed=5000).contiguous()   # the same batch on every rank
    m = ivfpq_measure(env, ivf, None, queries, batch, k, P, steps, warm, shard=shard)
    part = partitioning(shard, world)
    out = dict(value=steps * batch / m["elapsed"], ms_per_step=1000 * m["elapsed"] / steps, recall_at_10=None, scaling="strong",
               partitioning=part, shard=shard if world > 1 else None,
               config={"workload": "C5 x%d ranks: %d x 128 SiftLike rows as 16-byte PQ codes in %d posting lists, nprobe=%d, batch=%d, top-%d; %s"
                                   % (world, full["n"], full["nlist"], P, batch, k, part),
                       "n": full["n"], "dim": 128, "batch": batch, "k": k, "nprobe": P, "index": "ivf-pq", "data": "lowrank",
                       "build_s": build_s, "load_s": load_s, "parallelism": part},
               roofline=hbm_roofline(pq_scan_kernel_name(batch), m["abytes"] / steps, m["kernel_ms"], m["launches"],
                                     scored_per_query_this_rank=m["scored"] / (steps * batch)))
    finish(out, m["disp"], m["abytes"] / steps)
    out.update(hbm)
    if m["exchange"]:
        out["exchange"] = m["exchange"]
    if m.get("rows_equal_unsharded") is not None:
        out["rows_equal_unsharded"] = m["rows_equal_unsharded"]
    if m.get("rows_equal_across_ranks") is not None:
        out["rows_equal_across_ranks"] = m["rows_equal_across_ranks"]
    out["steps"], out["warmup"] = steps, warm
    ivf.close()
    return out


def run_c5(env, steps=None, warm=None):
    """BASELINE config C5 as ONE GPU of the 8 sees it: rank 0's share (size-balanced owners, 1/8 of the entries) of the posting lists
    of a 100M x 128 index stored as 16-byte PQ codes, loaded from the WHOLE index's files the way a rank of the 8-GPU job loads them,
    the FULL coarse quantizer (65 536 centroids, replicated), nprobe 64, batch 4096."""
    from muopdb_amd import build as B, synth as S
    from muopdb_amd.index import BlockBasedIvf
    args, ctx = env.args, env.ctx
    batch = args.batch or 4096
    k, P = args.k, args.nprobe or 64
    steps, warm = steps or args.steps, args.warmup if warm is None else warm
    total = args.n or 100_000_000
    t0 = time.time()
    full = getattr(env, "c5_full", None)
    if full is None or full["n"] != total:   # (c5_full_1gpu leaves its files behind when it ran first)
        full = S.c5_index(ctx, total=total, world=1, rank=0, nlist=args.nlist or 65536, log=log)
        torch.cuda.empty_cache()
    # what rank 0 of an 8-rank job loads from the whole index's files (size-balanced owners, mdb_ivf_load(.., 0, 8)) — exactly what
    # run_c5_sharded's ranks do
    ivf = env.loaded(lambda: BlockBasedIvf(ctx, full["index"], full["vectors"], full["pq"], shard_rank=0, shard_world=8), len(full["index"]) + len(full["vectors"]))
    hbm = env.last_hbm
    from muopdb_amd import distributed as D0
    owner = np.asarray(D0.balanced_owners(full["list_sizes"], 8))
    sh = dict(full, n=int(ivf.num_resident_vectors()), owned_lists=int(((owner == 0) & (full["list_sizes"] > 0)).sum()))
    assert sh["n"] == int(full["list_sizes"][owner == 0].sum()), "the library's owner rule and distributed.balanced_owners differ"
    owner_rule = "size-balanced owners"
    env.c5_full = full = None
    log("C5 shard build+load %.1fs: %d vectors in %d owned lists" % (time.time() - t0, sh["n"], sh["owned_lists"]))
    queries = sh["gen"].draw((steps + warm) * batch, seed=5000).contiguous()
    dump(args, env.rank, "c5", index=sh["index"], vectors=sh["vectors"], **{"queries.f32": queries.cpu().numpy(), "codebook.f32": sh["codebook"]})
    m = ivfpq_measure(env, ivf, None, queries, batch, k, P, steps, warm)
    out = dict(value=steps * batch / m["elapsed"], ms_per_step=1000 * m["elapsed"] / steps, recall_at_10=None, scaling="strong",
               config={"workload": "C5 per-GPU: rank 0's shard (%s: %d vectors, %d lists) of a %d x 128 SiftLike index as 16-byte PQ "
                                   "codes, full coarse quantizer nlist=%d, nprobe=%d, batch=%d, top-%d"
                                   % (owner_rule, sh["n"], sh["owned_lists"], total, sh["nlist"], P, batch, k),
                       "n": sh["n"], "dim": 128, "batch": batch, "k": k, "nprobe": P, "index": "ivf-pq", "data": "lowrank"},
               roofline=hbm_roofline(pq_scan_kernel_name(batch), m["abytes"] / steps, m["kernel_ms"], m["launches"],
                                     scored_per_query=m["scored"] / (steps * batch)))
    finish(out, m["disp"], m["abytes"] / steps)
    out.update(hbm)
    out["steps"], out["warmup"] = steps, warm
    out["roofline"]["traffic"], out["roofline"]["traffic_source"] = measured_traffic("c5", out["config"])
    out["roofline"]["coarse_filter_mfma_busy"] = measured_mfma("c5", out["config"])
    out["recall_note"] = "a shard's rows are a partial result (1/8 of the probed lists): recall is defined after the all-gather merge only"
    # What a rank of the 8-GPU job REALLY runs per batch (muopdb_amd.distributed.sharded_probes + the exact sharded step): the coarse
    # search over ITS 1/8 of the centroids (mdb_ivf_coarse_keys), the merge of the 8 ranks' coarse rows (here: 8 copies of its own —
    # the all-gather itself needs 8 devices), then the search of its lists with the merged probes written as a points block.  The
    # probes used by the search are the true ones (precomputed, untimed), so the scan does exactly the replicated step's work.
    from muopdb_amd import distributed as D
    from muopdb_amd import lib as L
    nlist = sh["nlist"]
    first, count = D.coarse_range(nlist, 0, 8)
    ckeys = torch.empty((batch, P), dtype=torch.int64, device="cuda")
    gathered = torch.empty((batch, 8, P), dtype=torch.int64, device="cuda")
    mprobes = torch.empty((batch, P), dtype=torch.int32, device="cuda")
    true_probes = torch.empty((steps + warm, batch, P), dtype=torch.int32, device="cuda")
    for i in range(steps + warm):
        q = queries[i * batch:(i + 1) * batch]
        ctx.check(ctx.lib.mdb_ivf_find_nearest_centroids(ivf.h, C.c_void_p(q.data_ptr()), C.c_size_t(batch), C.c_size_t(P), C.c_int(L.MEM_DEVICE),
                                                         C.c_void_p(true_probes[i].data_ptr())))
    block = torch.zeros(D.points_block_bytes(batch, k), dtype=torch.uint8, device="cuda")
    ctx.sync()

    def rank_step(i):
        q = queries[i * batch:(i + 1) * batch]
        ctx.check(ctx.lib.mdb_ivf_coarse_keys(ivf.h, C.c_void_p(q.data_ptr()), C.c_size_t(batch), C.c_size_t(P), C.c_size_t(first), C.c_size_t(count),
                                              C.c_int(L.MEM_DEVICE), C.c_void_p(ckeys.data_ptr())))
        gathered.copy_(ckeys.view(batch, 1, P).expand(batch, 8, P))   # stand-in for the all-gather of 8 x [b][P] u64 rows
        ctx.check(ctx.lib.mdb_ivf_merge_coarse_keys(ivf.h, C.c_void_p(gathered.data_ptr()), C.c_size_t(batch), C.c_size_t(8), C.c_size_t(P),
                                                    C.c_int(L.MEM_DEVICE), C.c_void_p(mprobes.data_ptr())))
        ctx.check(ctx.lib.mdb_ivf_search_shard(ivf.h, C.c_void_p(q.data_ptr()), C.c_size_t(batch), C.c_void_p(true_probes[i].data_ptr()), C.c_size_t(P),
                                               C.c_size_t(k), C.c_int(L.MEM_DEVICE), None, C.c_size_t(0), C.c_size_t(0), C.c_void_p(block.data_ptr())))

    el, kms, nl = env.timed(rank_step, steps, warm)
    out["rank_of_8_step"] = dict(ms_per_step=1000 * el / steps, value=steps * batch / el, scan_kernel_ms=kms / max(nl, 1),
                                 dispersion=env.last_dispersion,
                                 coarse_centroids=count, note="coarse search over 1/8 of the centroids + merge of 8 coarse rows + search_shard with the "
                                 "probes; excludes the two all-gathers (8 x 8 P and 8 x (8 k + 5) bytes per query: latency-bound on xGMI, needs 8 devices)")
    ivf.close()
    return out


# ------------------------------------------------------------------------------------------ multi-user SPANN
def run_spann(env, users=None, no_sweep=False, steps=None, warm=None, shard=None):
    """BASELINE.md C4 shape: multi-user SPANN over unit-norm f32 rows, one (user, query) pair per user
    per batch, posting lists sharded l % world, one all-gather + merge per batch.  Defaults are a
    1/8 slice (128 users x 9766 x 768 = 3.8 GB); --users 1024 is the full 10M x 768 (30.7 GB)."""
    from muopdb_amd import build as B, synth as S
    from muopdb_amd import formats as F
    from muopdb_amd import distributed as D
    from muopdb_amd.index import MultiSpannIndex, SearchParams
    from muopdb_amd import lib as L
    args, ctx, rank, world = env.args, env.ctx, env.rank, env.world
    U = users or args.users
    per = (args.n // U) if args.n else 9766
    d = args.dim or 768
    batch = args.batch or U
    k, P = args.k, args.nprobe or 16
    ratio = args.ratio if args.ratio is not None else 0.1
    steps, warm = steps or args.steps, args.warmup if warm is None else warm
    nlist = max(1, per // 64)
    t0 = time.time()
    gen = S.EmbedLike(d, seed=3) if args.data == "lowrank" else None
    ucent = [gen.user(u) for u in range(U)] if gen is not None else []
    base = []   # the users' rows on the device (rank 0 / single process): exact ground truth, legacy queries

    def build():
        users_ = {}
        for u in range(U):
            if gen is not None:
                x = gen.draw(ucent[u], per, seed=3_000_000 + u)
            else:
                x = S.unit_gaussian(per, d, seed=3_000_000 + u)
            cent = B.kmeans(ctx, x, nlist, iters=4, seed=u)
            pls = B.posting_lists_from_assignment(B.assign_nearest(ctx, x, cent), cent.shape[0])
            hi, hv = S.hnsw_files(cent, max_neighbors=16, max_layers=4, kcand=32, seed=u)
            docs = np.arange(u * per, (u + 1) * per, dtype=np.uint64)
            users_[u + 1] = dict(hnsw_index=hi, hnsw_vectors=hv, ivf_index=F.write_ivf_index(cent.cpu().numpy(), docs, pls),
                                 ivf_vectors=F.write_vector_file(x.cpu().numpy()))
            base.append(x)
        cat_ = F.concat_multi_spann(users_)
        del users_
        return {key: cat_[key] for key in ("user_table", "hnsw_index", "hnsw_vectors", "ivf_index", "ivf_vectors")}

    if world > 1 and gen is None:
        raise SystemExit("the sharded SPANN workload needs --data lowrank (queries are drawn from the generator, not from rank-local rows)")
    # world > 1: rank 0 builds the collection ONCE and the ranks map the same files (Env.shared_build) — every rank used to build all
    # 1024 users itself: 35 s and 30.7 GB of host bytes PER RANK
    cat, cleanup = env.shared_build("spann_%du" % U, build)
    log("multi-user SPANN build: %d users x %d x %d, %.1fs, ivf_vectors %.2f GB" % (U, per, d, time.time() - t0,
                                                                                    len(cat["ivf_vectors"]) / 1e9))
    t0 = time.time()
    shard = (shard or args.shard) if world > 1 else "lists"
    by_user = shard == "users"
    if shard == "batch":
        raise SystemExit("spann: --shard batch is not offered (the collection does not fit one GPU at scale: shard by lists or by users)")
    if by_user:
        # user slot u -> rank u % world: this rank loads ONLY its users' records (112-byte UserIndexInfo rows carry absolute offsets into
        # the shared files: graphs, centroids, lists and doc ids of the other users are never uploaded), whole, unsharded
        table = np.frombuffer(bytes(cat["user_table"]), np.uint8).reshape(U, -1)
        mine = D.users_of_rank(U, rank, world)
        ms = env.loaded(lambda: MultiSpannIndex(ctx, table[mine].tobytes(), d, cat["hnsw_index"], cat["hnsw_vectors"], cat["ivf_index"], cat["ivf_vectors"], None, 0, 1),
                        sum(len(cat[k_]) for k_ in ("hnsw_index", "hnsw_vectors", "ivf_index", "ivf_vectors")))
    else:
        ms = env.loaded(lambda: MultiSpannIndex(ctx, cat["user_table"], d, cat["hnsw_index"], cat["hnsw_vectors"], cat["ivf_index"], cat["ivf_vectors"],
                                                None, rank, world), sum(len(cat[k_]) for k_ in ("hnsw_index", "hnsw_vectors", "ivf_index", "ivf_vectors")))
    log("load %.1fs" % (time.time() - t0))
    hbm = env.last_hbm
    cleanup()
    have_base = len(base) == U
    nq = (steps + warm) * batch
    quser = (torch.arange(nq) % U)
    if gen is not None:  # queries: fresh draws of each user's own distribution (same pairs on every rank: lists are sharded)
        per_user = (nq + U - 1) // U
        qs = torch.stack([gen.draw(ucent[u], per_user, seed=7_000_000 + u) for u in range(U)])  # [U][per_user][d]
        queries = qs.permute(1, 0, 2).reshape(-1, d)[:nq].contiguous()                       # query i -> user i % U
        desc = "low-rank (48) + noise unit-norm rows: muopdb_amd.build.EmbedLike"
    else:
        gq = torch.Generator(device="cpu"); gq.manual_seed(77)
        qrow = torch.randint(0, per, (nq,), generator=gq)
        noise = torch.randn((nq, d), generator=gq) * (0.3 / d ** 0.5)
        queries = torch.stack([base[int(u)][int(r)] for u, r in zip(quser.tolist(), qrow.tolist())]) + noise.cuda()
        queries = (queries / queries.norm(dim=1, keepdim=True)).contiguous()
        desc = "isotropic Gaussian unit-norm rows (round-1 generator)"
    if args.dump_dir and (U * per * d * 4 < (8 << 30) or args.dump_big):   # (the full C4 writes 30 GB: --dump-big)
        dump(args, rank, "spann", hnsw_index=cat["hnsw_index"], hnsw_vectors=cat["hnsw_vectors"], ivf_index=cat["ivf_index"],
             vectors=cat["ivf_vectors"], user_table=cat["user_table"],
             **{"queries.f32": queries.cpu().numpy(), "users.u64": (quser + 1).numpy().astype(np.uint64)})
    gather = D.PointsGather(ctx, batch, k, "cuda") if (world > 1 and not by_user) else None   # the EXACT sharded step (points blocks)
    # user sharding: the routing of a batch's pairs is host integer work on the user ids (the aggregator's role); it is prepared per
    # step next to the u128 user-id arrays, outside the timed region like them; the row gather of the routed queries is inside it
    rows_ex = [D.RowsExchange(batch, k, D.route_by_user(quser[i * batch:(i + 1) * batch].tolist(), world), rank, "cuda")
               for i in range(steps + warm)] if by_user else None
    if by_user:   # steps with the same routing share one exchange object (query i -> user i % U with batch = U: all of them)
        for i in range(1, len(rows_ex)):
            if torch.equal(rows_ex[i].perm, rows_ex[0].perm):
                rows_ex[i] = rows_ex[0]
        uid_local = [L.u128_array([int(u) + 1 for u in quser[i * batch:(i + 1) * batch][rows_ex[i].local.cpu()].tolist()]) for i in range(steps + warm)]
    ids = torch.zeros((batch, k, 2), dtype=torch.int64, device="cuda")
    sc = torch.zeros((batch, k), dtype=torch.float32, device="cuda")
    cn = torch.zeros(batch, dtype=torch.int32, device="cuda")
    fo = torch.zeros(batch, dtype=torch.uint8, device="cuda")
    uid_arrays = [L.u128_array([int(u) + 1 for u in quser[i * batch:(i + 1) * batch].tolist()]) for i in range(steps + warm)]
    # exact per-user ground truth (f64) of the timed queries (the rank that built the collection holds the rows)
    gts = None
    if have_base:
        gts = []
        for j in range(steps * batch):
            qi = warm * batch + j
            u = int(quser[qi])
            dd = ((base[u].double() - queries[qi].double()[None, :]) ** 2).sum(1)
            gts.append((torch.topk(dd, k, largest=False).indices + u * per))
        gts = torch.stack(gts).cpu().numpy()

    share = world > 1 and not by_user and (args.share_closure == "on" or (args.share_closure == "auto" and batch >= 1024))
    uid_slices = None

    def measure(P_, ratio_, disperse=True):
        nonlocal uid_slices
        params = SearchParams(k, args.ef).with_num_explored_centroids(P_).with_centroid_distance_ratio(ratio_).to_c()
        psh = D.ProbeRowsShare(ctx, batch, int(ctx.lib.mdb_spann_probe_row_words(C.byref(params))), "cuda") if share else None
        if share and uid_slices is None:
            lo_, hi_ = psh.slice
            uid_slices = [L.u128_array([int(u) + 1 for u in quser[i * batch + lo_:i * batch + hi_].tolist()]) for i in range(steps + warm)]

        def step(i, keep=None):
            q = queries[i * batch:(i + 1) * batch]
            if by_user:
                ex = rows_ex[i]
                ql = ex.local_queries(q)
                ctx.check(ctx.lib.mdb_multi_spann_search(ms.h, uid_local[i], C.c_void_p(ql.data_ptr()), C.c_size_t(ex.n_local), C.byref(params),
                                                         C.c_int(L.MEM_DEVICE), C.c_void_p(ex.ids.data_ptr()), C.c_void_p(ex.scores.data_ptr()),
                                                         C.c_void_p(ex.counts.data_ptr()), C.c_void_p(ex.found.data_ptr())))
                res = ex.gather()[0]
            elif share:
                # the centroid stage of THIS rank's slice of the pairs -> one all-gather of probe rows -> every rank scans its lists
                lo_, hi_ = psh.slice
                if hi_ > lo_:
                    ctx.check(ctx.lib.mdb_multi_spann_probes(ms.h, uid_slices[i], C.c_void_p(q[lo_:hi_].data_ptr()), C.c_size_t(hi_ - lo_),
                                                             C.byref(params), C.c_int(L.MEM_DEVICE), C.c_void_p(psh.send.data_ptr())))
                rows = psh.gather()
                ctx.check(ctx.lib.mdb_multi_spann_search_shard_probes(ms.h, uid_arrays[i], C.c_void_p(q.data_ptr()), C.c_size_t(batch),
                                                                      C.byref(params), C.c_int(L.MEM_DEVICE), C.c_void_p(rows.data_ptr()), None,
                                                                      C.c_size_t(0), C.c_size_t(0), C.c_void_p(gather.send.data_ptr())))
                res, _, _ = gather.gather_merge_multi(ms, uid_arrays[i])
            elif world > 1:
                ctx.check(ctx.lib.mdb_multi_spann_search_shard(ms.h, uid_arrays[i], C.c_void_p(q.data_ptr()), C.c_size_t(batch),
                                                               C.byref(params), C.c_int(L.MEM_DEVICE), None, C.c_size_t(0), C.c_size_t(0),
                                                               C.c_void_p(gather.send.data_ptr())))
                res, _, _ = gather.gather_merge_multi(ms, uid_arrays[i])
            else:
                ctx.check(ctx.lib.mdb_multi_spann_search(ms.h, uid_arrays[i], C.c_void_p(q.data_ptr()), C.c_size_t(batch), C.byref(params),
                                                         C.c_int(L.MEM_DEVICE), C.c_void_p(ids.data_ptr()), C.c_void_p(sc.data_ptr()),
                                                         C.c_void_p(cn.data_ptr()), C.c_void_p(fo.data_ptr())))
                res = ids
            if keep is not None:
                keep.append(res[:, :, 0].clone())

        outputs = (lambda: dict(ids=ids, scores=sc, counts=cn)) if world == 1 else None
        elapsed, kernel_ms, launches = env.timed(step, steps, warm, profiling=1, disperse=disperse, outputs=outputs)  # 1: posting-list scan only
        disp = env.last_dispersion
        found, scored, abytes, evals, expanded = [], 0, 0, 0, 0
        ctx.set_profiling(2); ctx.get_profile()  # untimed re-run: centroid-graph traversal kernel time
        for i in range(warm, warm + steps):
            step(i, found)
            st = ctx.stats(); scored += st["scored_vectors"]; abytes += st["algorithmic_bytes"]
            evals += st["distance_evals"]; expanded += st["expanded_nodes"]
        hnsw_ms, hnsw_launches = ctx.get_profile(); ctx.set_profiling(False)
        found = torch.cat(found).cpu().numpy()
        across = env.same_on_all_ranks(found)
        # a SPANN call's algorithmic bytes = the centroid graphs' traversal (evaluations x (4 d + 4) + expansions x 16: ANOTHER kernel,
        # hnsw_closure_kernel) + the posting-list scan (scored x bytes per scored vector): each kernel is priced with its own bytes
        graph_bytes = evals * (d * 4 + 4) + expanded * 16
        ex = exchange_times(env, step, steps, warm) if disperse else None
        return dict(exchange=ex, rows_equal_across_ranks=across, elapsed=elapsed, kernel_ms=kernel_ms, launches=launches, found=found, scored=scored, abytes=abytes,
                    scan_bytes=abytes - graph_bytes, graph_bytes=graph_bytes, evals=evals, disp=disp,
                    recall=recall_at_k(found, gts, k) if gts is not None else None, hnsw_ms=hnsw_ms / max(hnsw_launches, 1))

    m = measure(P, ratio)
    part = partitioning(shard, world)
    out = dict(value=steps * batch / m["elapsed"], ms_per_step=1000 * m["elapsed"] / steps, recall_at_10=m["recall"], scaling="strong",
               partitioning=part, shard=shard if world > 1 else None,
               config={"workload": "multi-user SPANN, %d users x %d x %d f32 (%s; BASELINE.md C4 shape), batch=%d (user,query) "
                                   "pairs, ef=%d, num_explored_centroids=%d, ratio=%g, top-%d, %s"
                                   % (U, per, d, desc, batch, args.ef, P, ratio, k, part),
                       "users": U, "n": U * per, "dim": d, "batch": batch, "k": k, "nprobe": P, "ratio": ratio, "index": "multi-spann",
                       "data": args.data, "parallelism": part},
               roofline=hbm_roofline("ivf_scan_f32_kernel", m["scan_bytes"] / steps, m["kernel_ms"], m["launches"],
                                     scored_per_query=m["scored"] / (steps * batch)))
    if world > 1 and not by_user:
        out["closure"] = "once per pair: each rank its slice of the batch, probe rows all-gathered" if share else "replicated on every rank"
    # the centroid-graph kernel as its own entry (r3 divided its bytes by the scan kernel's time: VERDICT r3 weak #1)
    out["roofline"]["centroid_graph"] = hbm_roofline("hnsw_closure_kernel", m["graph_bytes"] / steps, m["hnsw_ms"], 1,
                                                     evals_per_query=m["evals"] / (steps * batch))
    finish(out, m["disp"], m["abytes"] / steps)
    out.update(hbm)
    if m["exchange"]:
        out["exchange"] = m["exchange"]
    if m.get("rows_equal_across_ranks") is not None:
        out["rows_equal_across_ranks"] = m["rows_equal_across_ranks"]
    out["roofline"]["traffic"], out["roofline"]["traffic_source"] = measured_traffic("spann_full" if U >= 1024 else "spann", out["config"])
    out["steps"], out["warmup"] = steps, warm
    if args.full and not (args.no_sweep or no_sweep):
        sweep = []
        for p_, r_ in ((4, 0.1), (16, 0.1), (64, 0.1), (4, 0.3), (16, 0.3), (64, 0.3), (16, 1.0)):
            s = m if (p_, r_) == (P, ratio) else measure(p_, r_, disperse=False)
            sweep.append(dict(num_explored_centroids=p_, centroid_distance_ratio=r_, recall_at_10=s["recall"],
                              value=steps * batch / s["elapsed"], ms_per_step=1000 * s["elapsed"] / steps,
                              scan_kernel_ms=s["kernel_ms"] / max(s["launches"], 1), scored_per_query=s["scored"] / (steps * batch)))
        out["sweep"] = sweep
    if env.cpu:
        import oracle
        o = oracle.MultiSpannIndex(cat["user_table"], d, cat["hnsw_index"], cat["hnsw_vectors"], cat["ivf_index"], cat["ivf_vectors"])
        op = oracle.SearchParams(k, args.ef, num_explored_centroids=P, centroid_distance_ratio=ratio)
        qh = queries[warm * batch:(warm + steps) * batch].cpu().numpy()
        uh = [int(u) + 1 for u in quser[warm * batch:(warm + steps) * batch].tolist()]
        out["cpu_baseline"] = cpu_baseline(
            lambda m_: o.search_for_user(uh[:m_], qh[:m_], op, threads=1), lambda m_, t: o.search_for_user(uh[:m_], qh[:m_], op, threads=t),
            len(qh), args.cpu_seconds, min(16, len(qh)),
            lambda r, m_: all(r.doc_ids(i) == [int(v) for v in m["found"][i][:int(r.counts[i])]] for i in range(min(m_, 256))),
            "%d (user,query) pairs, one thread")
    ms.close()
    return out


LINE_LIMIT = 6144   # bytes of the ONE stdout line (the driver parses it from a bounded stdout tail; round 4's 24.8 KB line did not parse)


def _r(v, sig=5):
    """floats to `sig` significant digits (the line is a record, not a checkpoint)"""
    if isinstance(v, float):
        return float("%.*g" % (sig, v)) if v == v and abs(v) != float("inf") else None
    return v


def _compact_roofline(r):
    if not r:
        return None
    out = {"bound": r.get("bound"), "kernel": str(r.get("kernel"))[:96], "bytes_per_launch": _r(float(r["bytes_per_launch"])) if r.get("bytes_per_launch") else None,
           "kernel_ms": _r(r.get("kernel_ms")), "achieved": _r(r.get("achieved")), "peak": r.get("peak"), "unit": r.get("unit"),
           "frac": _r(r.get("frac")), "traffic": _r(float(r["traffic"])) if r.get("traffic") else None}
    mb = r.get("mfma_busy")
    if isinstance(mb, dict) and mb.get("mfma_busy_frac_of_chip") is not None:
        out["mfma_busy"] = _r(mb["mfma_busy_frac_of_chip"])
    return out


def _compact_cpu(c):
    if not c:
        return None
    return {"value": _r(c.get("value")), "unit": c.get("unit"), "cores": c.get("cores"), "kind": c.get("kind"),
            "sample": str(c.get("sample"))[:64], "all_cores_value": _r(c.get("all_cores_value")), "all_cores": c.get("all_cores"),
            "cpu_model": str(c.get("cpu_model"))[:48], "ids_match_gpu": c.get("ids_match_gpu")}


def _compact_workload(w):
    """one entry of `workloads`: the numbers a reader recomputes from, nothing else (prose, dispersion, sweeps: the full record)"""
    if "error" in w:
        return {"error": str(w["error"])[:120]}
    r, c, cfg = w.get("roofline") or {}, w.get("cpu_baseline") or {}, w.get("config") or {}
    out = {"value": _r(w.get("value")), "ms_per_step": _r(w.get("ms_per_step")), "steps": w.get("steps"), "recall": _r(w.get("recall_at_10"), 4),
           "batch": cfg.get("batch"), "kernel_ms": _r(r.get("kernel_ms")), "frac": _r(r.get("frac"), 4), "step_frac": _r(w.get("step_frac"), 4),
           "cpu1": _r(c.get("value"), 4), "cpuN": _r(c.get("all_cores_value"), 4), "ids_match": c.get("ids_match_gpu")}
    if w.get("scaling") == "strong":
        out["scaling"] = "strong"
    if w.get("shard"):
        out["partitioning"] = w["shard"]     # lists | users | batch (prose: the full record's `partitioning`)
    if w.get("rows_equal_unsharded") is not None:
        out["rows_ok"] = w["rows_equal_unsharded"]
    if w.get("rows_equal_across_ranks") is not None:
        out["ranks_agree"] = w["rows_equal_across_ranks"]
    ex = w.get("exchange")
    if ex:
        out["exchange_ms"] = _r(sum(v for k_, v in ex.items() if k_.endswith("_ms_per_step")), 4)
    mb = r.get("mfma_busy")
    if isinstance(mb, dict) and mb.get("mfma_busy_frac_of_chip") is not None:
        out["mfma_busy"] = _r(mb["mfma_busy_frac_of_chip"], 3)
    if w.get("hbm_resident_bytes"):
        out["hbm_gb"] = _r(w["hbm_resident_bytes"] / 1e9, 3)
    return {k_: v for k_, v in out.items() if v is not None}


def compact_line(line):
    """The ONE stdout line of the contract, bounded (LINE_LIMIT): top level = the headline's metric / value / ms_per_step / roofline /
    cpu_baseline / recall, `config` with a short `workload` string, `workloads` = one compact dict per entry.  Everything else
    (dispersion, notes, sweeps, prose) goes to the full record (`emit`)."""
    cfg = dict(line.get("config") or {})
    short = {"workload": short_workload(cfg)}
    for k_ in ("n", "dim", "batch", "ef", "k", "nprobe", "users", "index", "graph", "data", "parallelism", "ratio"):
        if k_ in cfg:
            short[k_] = cfg[k_]
    out = {k_: line.get(k_) for k_ in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                                       "vs_baseline", "dtype", "data")}
    out["value"], out["ms_per_step"] = _r(out["value"], 7), _r(out["ms_per_step"], 7)
    out["config"] = short
    out["recall_at_10"] = _r(line.get("recall_at_10"), 4)
    out["roofline"] = _compact_roofline(line.get("roofline"))
    out["cpu_baseline"] = _compact_cpu(line.get("cpu_baseline"))
    out["step_frac"] = _r(line.get("step_frac"), 4)
    for k_ in ("rccl_ranks", "collective_backend", "shard", "rows_equal_unsharded", "rows_equal_across_ranks"):
        if line.get(k_) is not None:
            out[k_] = line[k_]
    if line.get("exchange"):
        out["exchange"] = {k_: _r(v) for k_, v in line["exchange"].items()}
    if isinstance(line.get("concurrent"), dict):
        out["concurrent"] = {"streams": line["concurrent"].get("streams"), "value": _r(line["concurrent"].get("value"))}
    if line.get("workloads"):
        out["workloads"] = {name: _compact_workload(w) for name, w in line["workloads"].items()}
    if line.get("full_record"):
        out["full_record"] = line["full_record"]
    text = json.dumps(out, separators=(",", ":"))
    if len(text) > LINE_LIMIT and "workloads" in out:   # never exceed the bound: drop per-workload fields from the back, then entries
        for drop in ("hbm_gb", "mfma_busy", "steps", "batch", "kernel_ms", "cpuN", "exchange_ms"):
            for w in out["workloads"].values():
                w.pop(drop, None)
            text = json.dumps(out, separators=(",", ":"))
            if len(text) <= LINE_LIMIT:
                break
        names = list(out["workloads"])
        while len(text) > LINE_LIMIT and names:
            out["workloads"].pop(names.pop())
            out["workloads_truncated"] = True
            text = json.dumps(out, separators=(",", ":"))
    return text


def short_workload(cfg):
    """`config.workload`: a name a reader maps to BASELINE.json's configs, no prose"""
    idx = cfg.get("index")
    if idx == "hnsw":
        return "C2 sift1m-like %dx%d hnsw ef=%d k=%d b=%d" % (cfg.get("n", 0), cfg.get("dim", 0), cfg.get("ef", 0), cfg.get("k", 0), cfg.get("batch", 0))
    if idx == "flat":
        return "%s flat L2 %dx%d k=%d b=%d" % ("C1" if cfg.get("n", 0) < 100_000 else "flat-1m", cfg.get("n", 0), cfg.get("dim", 0), cfg.get("k", 0), cfg.get("batch", 0))
    if idx == "ivf-pq":
        return "%s ivf-pq m=16 %dx%d nprobe=%d k=%d b=%d" % ("C5" if cfg.get("n", 0) > 2_000_000 else "C3", cfg.get("n", 0), cfg.get("dim", 0),
                                                            cfg.get("nprobe", 0), cfg.get("k", 0), cfg.get("batch", 0))
    if idx == "multi-spann":
        return "C4 multi-spann %du x %dx%d k=%d b=%d" % (cfg.get("users", 0), cfg.get("n", 0) // max(cfg.get("users", 1), 1), cfg.get("dim", 0),
                                                         cfg.get("k", 0), cfg.get("batch", 0))
    return str(cfg.get("workload", ""))[:80]


def emit(args, line):
    """rank 0: with --full, the full record (every workload's config prose, dispersion, sweeps, notes) goes to --full-json (default
    FULL_JSON_DEFAULT under the repository root, when that directory can be made) and to stderr; stdout gets exactly ONE bounded line."""
    if not args.full:
        sys.stdout.write(compact_line(line) + "\n")
        sys.stdout.flush()
        return
    path = args.full_json or os.path.join(ROOT, FULL_JSON_DEFAULT)
    try:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(line, f)
        line["full_record"] = os.path.relpath(path, ROOT) if os.path.abspath(path).startswith(ROOT) else path
    except OSError:
        pass
    sys.stderr.write("[bench-full] " + json.dumps(line) + "\n")
    sys.stderr.flush()
    sys.stdout.write(compact_line(line) + "\n")
    sys.stdout.flush()


def dump_outputs(directory, outputs):
    """--dump-outputs: the arrays Env.timed kept from the last step of the first timed region, as DIR/<name>.npy — integers as
    float64 (exact below 2^53: doc ids, counts), floats as float32.  Above DUMP_OUTPUTS_LIMIT bytes in all, the same fixed, seeded
    sample of rows (first axis) is taken from every array, and rows.npy says which."""
    if outputs is None:
        sys.stderr.write("bench.py: --dump-outputs: this workload keeps no outputs of its timed steps\n")
        sys.exit(2)
    arrs = {name: a.astype(np.float32 if a.dtype.kind == "f" else np.float64) for name, a in outputs.items()}
    total = sum(a.nbytes for a in arrs.values())
    if total > DUMP_OUTPUTS_LIMIT:
        n = min(a.shape[0] for a in arrs.values())
        rows = np.sort(np.random.default_rng(0).choice(n, size=max(1, n * DUMP_OUTPUTS_LIMIT // (2 * total)), replace=False))
        arrs = {name: a[rows] for name, a in arrs.items()}
        arrs["rows"] = rows.astype(np.float64)
    os.makedirs(directory, exist_ok=True)
    for name, a in arrs.items():
        np.save(os.path.join(directory, name + ".npy"), np.ascontiguousarray(a))
    log("outputs of the last timed step: %s in %s" % (", ".join("%s%s" % (k_, list(a.shape)) for k_, a in arrs.items()), directory))


def launch_ranks(args):
    """`python bench.py --gpus N` (N > 1) without a launcher: start the N ranks through torch.distributed.run — one process per
    GPU, RCCL over xGMI — exactly the command the driver uses.  Fewer than N visible devices is an ERROR (never a silent
    1-rank run), unless the one-GPU validation hook below is set."""
    import socket
    ndev = torch.cuda.device_count()
    if ndev < args.gpus and not os.environ.get("MDB_BENCH_DEVICE"):
        sys.stderr.write("bench.py: --gpus %d but only %d HIP device(s) visible; refusing to measure fewer ranks than asked "
                         "(one-GPU plumbing check: MDB_BENCH_BACKEND=gloo MDB_BENCH_DEVICE=0)\n" % (args.gpus, ndev))
        sys.exit(2)
    sock = socket.socket(); sock.bind(("127.0.0.1", 0)); port = sock.getsockname()[1]; sock.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    log("starting %d ranks: %s" % (args.gpus, " ".join(cmd)))
    os.execv(sys.executable, cmd)


def print_plan(args):
    """--plan: the dry run of `bench.py --gpus N` (VERDICT r3 next #7d).  Seconds are this round's single-GPU measurements (gpurun
    boxes: 2 x EPYC 9575F, one MI355X), bytes follow from the sizes; nothing here touches a device."""
    w = max(1, args.gpus)
    GB = 1e9
    rows = []
    rows.append(dict(workload="hnsw C2 (headline: insert-built graph, replicas) + batch 1 + ef 400", builder="every rank, on its own GPU", build_s=60, load_s=3,
                     host_private_gb=0.8, host_shared_gb=0, hbm_per_rank_gb=2.4,
                     note="1M x 128 graph per rank: 0.77 GB of files, no collective in the step"))
    rows.append(dict(workload="flat 1M b1 / b64 (row shards)", builder="every rank (shares the C2 base)", build_s=0, load_s=1,
                     host_private_gb=0, host_shared_gb=0, hbm_per_rank_gb=1.1 / w + 0.6))
    rows.append(dict(workload="ivfpq C3 (list shards)", builder="every rank (k-means + PQ training on the device, ~10 s)", build_s=10, load_s=1,
                     host_private_gb=0.1, host_shared_gb=0, hbm_per_rank_gb=0.7))
    rows.append(dict(workload="spann_c4_128u (list shards)", builder="rank 0, files shared" if w > 1 else "the process", build_s=5, load_s=1,
                     host_private_gb=0.1 if w > 1 else 3.9, host_shared_gb=3.9 if w > 1 else 0, hbm_per_rank_gb=3.9 / w + 3.9 * (w > 1)))
    if w > 1:
        rows.append(dict(workload="spann_c4_full_sharded (1024 users x 9766 x 768)", builder="rank 0, files shared", build_s=35 + 25, load_s=12,
                         host_private_gb=0.3, host_shared_gb=31.0, host_rank0_peak_gb=62.0,
                         hbm_per_rank_gb=30.7 + 30.7 / w, note="rank 0 holds the collection once more while it writes it (peak 2 x 30.7 GB); "
                         "every rank uploads the shared vector file (30.7 GB, released after the gather of its lists) and keeps 1/%d" % w))
        rows.append(dict(workload="c5_sharded (100M x 16-byte codes, 65 536 lists)", builder="rank 0, files shared", build_s=70 + 8, load_s=3,
                         host_private_gb=0.3, host_shared_gb=3.9, host_rank0_peak_gb=12.0, hbm_per_rank_gb=3.9 + 1.6 / w + 0.3,
                         note="the other ranks wait at a barrier for ~80 s: well inside the process group's timeout (10 min)"))
        rows.append(dict(workload="spann_c4_full_by_user (user slot u on rank u %% %d, rows all-gather only)" % w, builder="maps spann_c4_full_sharded's files", build_s=0,
                         load_s=6, host_private_gb=0.3, host_shared_gb=31.0, hbm_per_rank_gb=2 * 30.7 / w, note="each rank uploads only its users' byte ranges"))
        rows.append(dict(workload="c5_by_batch (replicas, batch slices, rows all-gather only)", builder="maps c5_sharded's files", build_s=0, load_s=3,
                         host_private_gb=0.3, host_shared_gb=3.9, hbm_per_rank_gb=3.9 + 1.6 + 0.3))
        rows.append(dict(workload="ivfpq_c3_by_batch (replicas)", builder="every rank", build_s=10, load_s=1, host_private_gb=0.1, host_shared_gb=0, hbm_per_rank_gb=0.7))
    else:
        rows.append(dict(workload="c5_full_1gpu", builder="the process", build_s=66, load_s=1, host_private_gb=12.0, host_shared_gb=0, hbm_per_rank_gb=4.5))
        rows.append(dict(workload="c5_shard_per_gpu", builder="the process (reads c5_full_1gpu's files)", build_s=0, load_s=2, host_private_gb=12.0, host_shared_gb=0, hbm_per_rank_gb=1.0))
        rows.append(dict(workload="spann_c4_full_1024u", builder="the process", build_s=35, load_s=4, host_private_gb=62.0, host_shared_gb=0, hbm_per_rank_gb=61.4))
        rows.append(dict(workload="hnsw_c2_knn_graph", builder="the process", build_s=25, load_s=3, host_private_gb=0.8, host_shared_gb=0, hbm_per_rank_gb=2.4))
    total_s = sum(r["build_s"] + r["load_s"] for r in rows) + 60   # + timed regions, dispersion, recall / ground truth
    print(json.dumps(dict(gpus=w, estimated_wall_s=total_s, peak_host_gb=max(r.get("host_rank0_peak_gb", 0) + w * r["host_private_gb"] for r in rows),
                          workloads=rows, tmp_dir=os.environ.get("MDB_BENCH_TMP", "/tmp"),
                          note="estimates from round 4's one-GPU runs; shared = one copy in the page cache (np.memmap of rank 0's files)"), indent=1))


def main():
    args = parse()
    if args.plan:
        print_plan(args)
        return
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        launch_ranks(args)   # does not return
    if os.environ.get("MDB_BENCH_WATCHDOG"):   # seconds: every thread's Python stack to stderr, then exit (a rank stuck in a collective says where)
        import faulthandler
        faulthandler.dump_traceback_later(float(os.environ["MDB_BENCH_WATCHDOG"]), exit=True)
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        sys.stderr.write("bench.py: --gpus %d but WORLD_SIZE=%d: the launcher and the flag disagree\n" % (args.gpus, world))
        sys.exit(2)
    # Validation hooks for boxes with ONE GPU (the multi-rank logic of every workload — sharding, gathers, merges, max over ranks —
    # without RCCL, which needs one device per rank): MDB_BENCH_DEVICE pins every rank to that device, MDB_BENCH_BACKEND=gloo
    # moves the collectives to gloo.  Never set by the driver; numbers from such a run are not bench results.
    if os.environ.get("MDB_BENCH_DEVICE"):
        local = int(os.environ["MDB_BENCH_DEVICE"])
    if local >= torch.cuda.device_count():
        sys.stderr.write("bench.py: rank %d wants device %d, %d visible\n" % (rank, local, torch.cuda.device_count()))
        sys.exit(2)
    torch.cuda.set_device(local)
    backend = None
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("MDB_BENCH_BACKEND", "nccl")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend)
    from muopdb_amd import lib as L
    ctx = L.Context(local)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    env = Env(args, ctx, rank, world)
    single = {"hnsw": run_hnsw, "flat": run_flat, "ivfpq": run_ivfpq, "spann": run_spann, "c5": run_c5,
              "c5full": run_c5_full if world == 1 else run_c5_sharded}
    if args.workload != "all":
        res = single[args.workload](env)
    else:
        res = run_hnsw(env, batch=64, graph=args.graph)   # the headline: the reference-shaped (insert-built) graph unless --graph knn
        extra = {}
        # the metric's other batch size over the same resident graph (one sequential chain on one CU: latency, not throughput)
        plan = [("hnsw_c2_b1", lambda: run_hnsw(env, batch=1, graph=args.graph, extras=False, steps=max(args.steps, 200), warm=max(args.warmup, 20))),
                # ef above 256: the 8-register beam of the table path (up to 448; beyond: hnsw_search_kernel), the same resident graph
                ("hnsw_c2_ef400", lambda: run_hnsw(env, batch=64, graph=args.graph, extras=False, ef=400)),
                # BASELINE configs[0]: 10 k x 128 (py/create_test_hdf5.py-shaped rows), batch 1 (+ a batch-64 point): launch latency, not HBM
                ("flat_c1_10k_b1", lambda: run_flat(env, n=10_000, batch=1, steps=max(args.steps, 200), warm=max(args.warmup, 20))),
                ("flat_c1_10k_b64", lambda: run_flat(env, n=10_000, batch=64, steps=max(args.steps, 100), warm=max(args.warmup, 10))),
                ("flat_1m_b1", lambda: run_flat(env, n=1_000_000, batch=1)), ("flat_1m_b64", lambda: run_flat(env, n=1_000_000, batch=64)),
                ("ivfpq_c3", lambda: run_ivfpq(env)), ("spann_c4_128u", lambda: run_spann(env, users=128))]
        if world > 1:   # the list-sharded configurations at full size over this job's ranks (C4: 1024 users; C5: 100M codes)
            env.keep_tags = {"spann_1024u", "c5"}   # the second partitioning of a collection maps the first one's files
            # both partitionings of SURVEY 8e: list shards (what north_star names; default) and the query partitionings next to them
            if not args.no_c4_full:
                plan.append(("spann_c4_full_sharded", lambda: run_spann(env, users=1024, no_sweep=True, steps=min(args.steps, 10), warm=min(args.warmup, 3), shard="lists")))
                plan.append(("spann_c4_full_by_user", lambda: run_spann(env, users=1024, no_sweep=True, steps=min(args.steps, 10), warm=min(args.warmup, 3), shard="users")))
            if not args.no_c5_full:
                plan.append(("c5_sharded", lambda: run_c5_sharded(env, steps=min(args.steps, 6), warm=min(args.warmup, 2), shard="lists")))
                plan.append(("c5_by_batch", lambda: run_c5_sharded(env, steps=min(args.steps, 6), warm=min(args.warmup, 2), shard="batch")))
            plan.append(("ivfpq_c3_by_batch", lambda: run_ivfpq(env, shard="batch", no_sweep=True)))
        if world == 1 and not args.no_c5_full:  # the whole of C5 on one GPU: the N = 1 anchor of its strong scaling
            plan.append(("c5_full_1gpu", lambda: run_c5_full(env, steps=min(args.steps, 6), warm=min(args.warmup, 2))))
        if world == 1 and not args.no_c5:  # one GPU's share of C5: rank 0's 1/8 of the lists, read from c5_full_1gpu's files when it ran
            plan.append(("c5_shard_per_gpu", lambda: run_c5(env, steps=min(args.steps, 8), warm=min(args.warmup, 2))))
        if world == 1 and not args.no_c4_full:  # the whole of C4 on one GPU: 1024 users x 9766 x 768 = 30.7 GB resident (~60 s of build + load)
            plan.append(("spann_c4_full_1024u", lambda: run_spann(env, users=1024, no_sweep=True, steps=min(args.steps, 10), warm=min(args.warmup, 3))))
        if world == 1 and not args.no_insert_graph:  # C2 again on the graph built the other way (default: the bulk k-NN build next to the insert-built headline)
            other = "knn" if args.graph == "insert" else "insert"
            plan.append(("hnsw_c2_%s_graph" % other, lambda: run_hnsw(env, batch=64, graph=other, n=args.insert_n, extras=False)))
        for name, fn in (plan if args.full else []):   # the other workloads: --full only
            t0 = time.time()
            try:  # a failing extra workload must never take the headline line with it
                torch.cuda.empty_cache()
                w = fn()
                w.update(unit="queries/s", scaling=w.get("scaling", "weak"))
                w.setdefault("steps", args.steps)
                w.setdefault("warmup", args.warmup)
                extra[name] = w
            except Exception as e:  # noqa: BLE001
                extra[name] = {"error": "%s: %s" % (type(e).__name__, e)}
            log("%s: %.1fs" % (name, time.time() - t0))
        if args.full:
            res["workloads"] = extra
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, env.outputs)
    env.drop_kept_builds()
    for h in env.hnsw_cache.values():
        h[0].close()
    res.pop("steps", None); res.pop("warmup", None)
    line = {"metric": METRIC, "value": res.pop("value"), "unit": "queries/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": res.pop("ms_per_step"), "higher_is_better": True, "scaling": res.pop("scaling", "weak"),
            "vs_baseline": None, "dtype": "f32", "data": "sift1m" if args.sift_dir else "synthetic",
            # ranks that took part in the collectives (RCCL when the backend is nccl; 0 for a single process)
            "rccl_ranks": dist.get_world_size() if (world > 1 and backend == "nccl") else 0, "collective_backend": backend}
    line.update(res)
    if rank == 0:
        emit(args, line)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
