#!/usr/bin/env python3
"""bench.py -- headline benchmark of the MI355X SpMV path.

    python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full]
    python bench.py --workload queen|kkt|webbase|powerlaw [--format csr|coo|ell|hybrid]
    python bench.py --matrix Queen_4147.tar.gz [--expand-symmetric] [--format ...]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A "step" is one pass of the hot path, y += A*x, over the workload with all inputs already
resident in HBM.  Default workload (BASELINE.json configs[1]): Poisson 5-point stencil CSR on a
4096 x 4096 grid, N = 16 777 216 rows, Z = 83 869 696 stored entries, fp64 values / int32
indices.  The other BASELINE configurations run from their files (--matrix, through the repo's
own loader, libspmv_host.so; symmetric files are multiplied as stored unless --expand-symmetric)
or, where the files cannot be fetched, from structure-faithful generators of the same size
(--workload queen | kkt | webbase, host/matrix/synthetic.hpp).

With N > 1 GPUs the SAME matrix is row-partitioned (ceil(rows/N) rows per rank, the reference's
static chunk rule), x is replicated, and every step ends with ONE all-gather of the y segments
(RCCL): total work is fixed, so scaling is "strong".

Prints ONE JSON line on rank 0.  `value` = 2*Z*K / t in GFLOP/s (whole job); `ms_per_step` = t / K, K = --steps.
--dump-outputs DIR writes y as the K timed steps left it (warm-up + K multiplies accumulated from y = 0) to DIR/y.npy,
float64; beyond 64 MB a fixed seeded sample of rows, their numbers in DIR/y_rows.npy.  Inputs are seeded: the same
arguments give the same inputs on every run, so two builds can be compared output for output.

A plain run does only what `value` needs: it sets up, warms up, times the K steps, dumps y if asked and prints the line
(config, the roofline figures of the timed launch itself, build).  Everything else described below -- the STREAM triad,
`cold`, `plan_ms`, `compressed`, PMC `traffic`, the companions, `drop_in_multi_gpu`, `cpu_baseline` and its parity gate,
`host_boundary`, `reference_protocol` and, for N > 1, the collective alone, the gather check, the link probe and the deferred
gather -- runs only with --full.  The --no-* switches below pick legs out of a --full run.

The timed launch READS THE VALUE ARRAY (plan flag SPMV_HIP_FLAG_NO_VALUE_INDEX: what the kernel does for a matrix of this
structure with arbitrary values), and `roofline` follows SURVEY section 8(d) to the letter: `achieved` = ALGORITHMIC bytes
per launch (CSR 12 Z + 4 (N+1) + 16 N + 8 M) / the launch's mean duration measured with HIP events on the launch stream,
`frac` = achieved / 8 TB/s, `traffic` = PMC bytes of a committed profile of the same device code.  Beside it, as
information: `streamed` (the bytes the plan's tile classes really move, their fraction of the peak and of the STREAM triad
timed in the same process), `cold` (the same launch with L2 and Infinity Cache evicted before every run), `plan_ms` (what
building the plan cost, stage by stage) and `compressed`: the launch the product runs BY DEFAULT for a matrix with at most
128 distinct values (value dictionary, constant-row tiles -- bit-identical y, far fewer bytes than the algorithmic figure:
its own us, GFLOP/s, streamed bytes, cold time and plan cost; `--headline product` makes that launch the timed one).
Companions on the default workload (never part of `value`): `config2_queen`, `config3_kkt`, `config4_webbase` -- the
stand-ins of BASELINE configs[2..4] at full size, each with ms per step, the section-8(d) fraction and a whole-vector
parity check against the CPU kernel; `config2_queen_stored`, `config3_kkt_stored` -- the same two matrices as the reference
multiplies their FILES (the stored lower triangle of a `symmetric` Matrix Market file, nothing mirrored).
`drop_in_multi_gpu` (every N): the same workload through the drop-in's own multi-GPU path -- spmv_hip_create_multi, ONE process
over N devices, timed by a fresh child process of rank 0 (t_local / t_allgather / t_total per gather scheme, the RCCL rank count,
the speed-up bound at the measured link rate); `value` for N > 1 is the one-process-per-GPU path the bench contract launches.  `cpu_baseline` (rank 0, N = 1 only) times the reference's own OpenMP kernel
(oracle/_ref, kind "reference") or the C oracle (kind "port") on the host cores; the same leg is the parity gate.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "spmv-cache-trace_amd", "python"))
# the host driver only supports dmabuf IPC: without this RCCL cannot share buffers across ranks
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

HBM_PEAK_GBS = 8000.0      # MI355X HBM3E spec peak (MI355X_MICROARCH.md); ~6300 GB/s is the measured copy ceiling
XGMI_LINK_GBS = 64.0       # per direction and link, 7 links per GPU: the conservative figure DESIGN.md section 6 uses
XGMI_LINK_GBS_QUOTED = 153.0  # the per-link figure usually quoted for MI355X; the truth for one direction lies in between


def strong_scaling_model(rows, t1_us, measured_gbs=None):
    """What the replicated-y design can reach on one node: every GPU multiplies rows / G and must RECEIVE
    the other G - 1 segments, each over its own xGMI link (direct all-to-all: segment bytes / link rate, whatever G is), fully
    overlapped with the multiply at best: step = max(t1 / G, 8 rows / G / rate).  Rates per link and direction: 64 GB/s (what
    MI300X-class links deliver), 76.8 (half of the 153.6 GB/s bidirectional figure quoted for MI355X)."""
    out = {"formula": "step_us(G) = max(t1_us / G, 8 * rows / G / link_rate); speedup = t1_us / step_us", "t1_us": round(t1_us, 1), "rows": int(rows)}
    rates = [("link_64.0_GBs", 64.0), ("link_76.8_GBs", 76.8)]
    if measured_gbs:
        rates.append(("link_measured_%.1f_GBs" % measured_gbs, float(measured_gbs)))
    for key, rate in rates:
        row = {}
        for G in (2, 4, 8):
            gather = 8.0 * rows / G / (rate * 1e9) * 1e6
            step = max(t1_us / G, gather)
            row["G%d" % G] = {"local_us": round(t1_us / G, 1), "gather_us": round(gather, 1), "speedup": round(t1_us / step, 2)}
        out[key] = row
    # 4 x at G = 8 needs step <= t1 / 4, i.e. the segment (8 rows / 8 bytes) received within t1 / 4 over ONE link
    out["link_GBs_needed_for_4x_at_G8"] = round(8.0 * rows / 8 / (t1_us / 4 * 1e-6) / 1e9, 1)
    out["needs"] = ("speedup >= 4 at G = 8 needs >= %.0f GB/s per link and direction, transfer fully hidden behind the multiply"
                    % out["link_GBs_needed_for_4x_at_G8"])
    return out


def link_probe(torch, dist, capi, o, rank, world, reps=5):
    """What the links between the ranks' devices deliver for THIS path's traffic: every rank stores its y segment (the doubles
    the gather moves) into its slot of one peer's vector at a time -- rank r -> (r + k) mod G for k = 1 .. G-1, all ranks at
    once, so every link carries one sender per direction: the pattern of tools/probes/xgmi_bw.hip -- and then into all peers
    at once (the fused store's pattern).  Timed with HIP events on the launch stream; a few ms in total.  The stores rewrite
    the values the slots already hold (the segment was delivered by the last multiply), so nothing changes.
    Returns (this rank's {peer: GB/s}, GB/s leaving this rank with all peers at once) or None."""
    v = o.vectors
    n = int(o.end - o.begin)
    stream = torch.cuda.current_stream().cuda_stream
    src = v.addr + 8 * rank * o.chunk

    def timed(peers):
        dsts = [v.peer_addr[h] + 8 * rank * o.chunk for h in peers]
        if n > 0:
            capi.peer_push(src, dsts, n, stream)
        torch.cuda.synchronize()
        dist.barrier()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            if n > 0:
                capi.peer_push(src, dsts, n, stream)
        b.record()
        torch.cuda.synchronize()
        dist.barrier()
        ms = a.elapsed_time(b)
        return round(8.0 * n * len(dsts) * reps / (ms * 1e-3) / 1e9, 2) if (n > 0 and ms > 0) else None
    per_peer = {}
    for k in range(1, world):
        h = (rank + k) % world
        per_peer[h] = timed([h])
    together = timed(sorted(v.peer_addr)) if world > 1 else None
    return per_peer, together
CLI = os.path.join(ROOT, "spmv-cache-trace_amd", "spmv-cache-trace-hip")


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--workload", default="poisson2d",
                    choices=["poisson2d", "queen", "kkt", "queen_stored", "kkt_stored", "webbase", "powerlaw", "banded", "random24", "stencil27", "random"],
                    help="poisson2d = BASELINE configs[1]; queen / kkt / webbase = generated stand-ins of configs[2..4] "
                         "at full size (symmetric structure EXPANDED, the entry counts BASELINE.json quotes); queen_stored / kkt_stored = the stored "
                         "lower triangle of the same matrices: what a `symmetric` Matrix Market file holds and the reference multiplies "
                         "(it mirrors nothing); powerlaw = webbase with uniformly scattered columns; banded / random24 = north_star's synthetic banded / "
                         "random CSR of ~100 M entries (SURVEY 8d S-banded, S-random); stencil27 / random: round-1 numpy stand-ins")
    ap.add_argument("--matrix", default=None, help="Matrix Market file (.mtx, .gz, .tgz, .tar.gz) or synthetic:<spec>; overrides --workload")
    ap.add_argument("--expand-symmetric", action="store_true",
                    help="mirror the entries of a symmetric file (EXTENSION; the reference multiplies the stored triangle)")
    ap.add_argument("--format", default="csr", choices=["csr", "coo", "ell", "hybrid"],
                    help="storage format (coo / ell / hybrid: one GPU, through the context API)")
    ap.add_argument("--grid", type=int, default=4096, help="poisson2d grid edge (4096 = BASELINE configs[1])")
    ap.add_argument("--kkt-grid", type=int, default=200, help="kkt grid edge (200 = nlpkkt200's size)")
    ap.add_argument("--algorithm", default="auto", choices=["auto", "scalar", "vector", "adaptive", "wavetile"])
    ap.add_argument("--lanes", type=int, default=0)
    ap.add_argument("--xcd-remap", action="store_true")
    ap.add_argument("--flags", type=lambda v: int(v, 0), default=0, help="extra SPMV_HIP_FLAG_* bits")
    ap.add_argument("--full", action="store_true",
                    help="beside the timed steps, run every other measurement and check of the line (CPU baseline and parity, cold "
                         "and compressed launches, plan cost, triad, PMC traffic, companions, the drop-in and reference-protocol legs, "
                         "N > 1: gather check, link probe); a plain run times the steps and prints the line")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="budget for the CPU baseline sample")
    ap.add_argument("--cpu-threads", type=int, default=0, help="0 = all host cores visible to this process")
    ap.add_argument("--no-parity-check", action="store_true")
    ap.add_argument("--cold", action="store_true",
                    help="reference_protocol: a second CLI run with --flush-caches (the device's L2 and Infinity Cache evicted before "
                         "every timed run) next to the warm one")
    ap.add_argument("--no-reference-protocol", action="store_true",
                    help="skip the extra run of the C++ CLI that times the multiply the reference's way (sync per run)")
    ap.add_argument("--events", choices=["launch", "region"], default="region",
                    help="one HIP event pair around the K timed launches (default; mean launch duration = span / K, "
                         "launch gaps included), or a pair around every launch (adds ~5 us of gap per step)")
    ap.add_argument("--no-north-star", action="store_true",
                    help="skip the short measurements of north_star's synthetic banded / random CSR matrices that the default "
                         "workload's line carries beside config3_kkt")
    ap.add_argument("--no-host-boundary", action="store_true",
                    help="skip the host_boundary leg (upload from host arrays; one multiply with x sent and y fetched over PCIe)")
    ap.add_argument("--partition", choices=["rows", "nnz"], default="rows",
                    help="N > 1: the reference's static row chunks (default), or a split on row boundaries with "
                         "equal stored entries per rank (uneven rows)")
    ap.add_argument("--no-overlap", action="store_true",
                    help="N > 1: wait for each all-gather before the next multiply (default: gather k overlaps multiply k+1)")
    ap.add_argument("--snapshot", action="store_true",
                    help="N > 1 with overlap: accumulate in place and copy the segment to a send buffer (round 1's way) "
                         "instead of alternating two segment buffers")
    ap.add_argument("--gather", default="auto", choices=["auto", "rccl", "peer-fused", "peer-push"],
                    help="N > 1: how the y segments reach the other ranks.  rccl = one in-place all-gather per step; peer-fused = "
                         "the multiply kernel stores its row sums into every rank's vector (inter-process device memory); "
                         "peer-push = the multiply, then one kernel that pushes the segment; auto (default) = time a few steps "
                         "of each scheme that can be set up and take the fastest")
    ap.add_argument("--headline", choices=["general", "product"], default="general",
                    help="which plan the timed region runs.  general (default): SPMV_HIP_FLAG_NO_VALUE_INDEX, the launch reads the "
                         "value array -- the roofline row of SURVEY 8(d); product: the plan the library builds by default (a value "
                         "dictionary where the matrix has <= 128 distinct values: fewer bytes than the algorithmic figure)")
    ap.add_argument("--no-companions", action="store_true",
                    help="skip config2_queen / config4_webbase (the stand-ins of BASELINE configs[2] and [4]) on the default workload")
    ap.add_argument("--no-cold", action="store_true", help="skip the flushed-cache timing of the headline launch")
    ap.add_argument("--no-config3", action="store_true",
                    help="skip the companion measurement of BASELINE configs[3] (the nlpkkt200-like KKT matrix, the configuration "
                         "BASELINE.json partitions over 8 GPUs) that the default workload's --full line carries as `config3_kkt`")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                    help="process-group backend; gloo is for rehearsing N > 1 on a box with one GPU")
    ap.add_argument("--share-gpu", action="store_true",
                    help="rehearsal: every rank uses device 0 (needs --backend gloo; RCCL refuses duplicate GPUs)")
    ap.add_argument("--reject-scheme", default=None, choices=["peer-fused", "peer-push"],
                    help="rehearsal: treat this gather scheme as if its gathered y had failed the check against RCCL's")
    ap.add_argument("--no-live-pmc", action="store_true",
                    help="do not measure roofline.traffic in this run (two short rocprofv3 --pmc passes -- FETCH_SIZE, WRITE_SIZE -- over a child "
                         "that launches the timed plan a few times); the figure then comes from a committed profile of the same device sources")
    ap.add_argument("--pmc-child", action="store_true", help=argparse.SUPPRESS)  # internal: this process IS the profiled child
    ap.add_argument("--no-drop-in", action="store_true",
                    help="skip the `drop_in_multi_gpu` leg: the same workload through spmv_hip_create_multi in ONE fresh process over "
                         "N devices -- the path the reference-side adapter binds (the reference is one process, src/profile-kernel.cpp:227)")
    ap.add_argument("--drop-in-child", type=int, default=0, help=argparse.SUPPRESS)   # internal: this process IS that child, over G devices
    ap.add_argument("--drop-in-specs", default="", help=argparse.SUPPRESS)            # internal: name=spec;name=spec
    ap.add_argument("--force-collective", action="store_true",
                    help="initialise the process group and run the all-gather even with one rank (rehearsal)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write y as the last timed step left it to DIR/<name>.npy (float64; a fixed seeded sample of rows "
                         "where the whole vector passes %d MB)" % (DUMP_LIMIT_BYTES >> 20))
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return args


DUMP_LIMIT_BYTES = 64 << 20  # everything --dump-outputs writes, all files together
DUMP_SAMPLE_SEED = 20240531


def dump_outputs(dirname, y):
    """--dump-outputs: y (what a caller of the timed path receives) as DIR/y.npy.  A vector larger than the budget is
    written as a sample: rows drawn once with a fixed seed (the same rows for the same --grid / --matrix), sorted, their
    values in y.npy and their indices in y_rows.npy (float64, exact below 2^53)."""
    os.makedirs(dirname, exist_ok=True)
    y = np.ascontiguousarray(y, dtype=np.float64)
    files = {}
    if y.nbytes <= DUMP_LIMIT_BYTES - 4096:
        files["y"] = y
    else:
        n = (DUMP_LIMIT_BYTES - 4096) // 16  # values and row indices, 8 bytes each
        rows = np.sort(np.random.default_rng(DUMP_SAMPLE_SEED).choice(y.size, size=n, replace=False))
        files["y"] = y[rows]
        files["y_rows"] = rows.astype(np.float64)
    for name, arr in files.items():
        np.save(os.path.join(dirname, name + ".npy"), arr)
    return {"dir": dirname, "files": {k: int(v.size) for k, v in files.items()}, "rows": int(y.size),
            "sampled": "y_rows" in files}


QUEEN_STORED_NAME = "queen-like 110x71x177 mesh x 3 dof, stored lower triangle (Queen_4147.mtx as the reference multiplies it)"
KKT_STORED_NAME = "kkt-27pt-%d^3, stored lower triangle (nlpkkt%d.mtx as the reference multiplies it)"


def workload_spec(args):
    """(spec for the host library or None, short name)."""
    if args.matrix:
        return args.matrix, os.path.basename(args.matrix)
    if args.workload == "poisson2d":
        return "synthetic:poisson2d:%d" % args.grid, "poisson2d-5pt-%dx%d" % (args.grid, args.grid)
    if args.workload == "kkt":
        return "synthetic:kkt:%d" % args.kkt_grid, "kkt-27pt-%d^3 (nlpkkt%d-like)" % (args.kkt_grid, args.kkt_grid)
    if args.workload == "queen":
        return "synthetic:queen", "queen-like 110x71x177 mesh x 3 dof (Queen_4147-like)"
    if args.workload == "queen_stored":
        return "synthetic:queen:tril", QUEEN_STORED_NAME
    if args.workload == "kkt_stored":
        return "synthetic:kkt:%d:tril" % args.kkt_grid, KKT_STORED_NAME % (args.kkt_grid, args.kkt_grid)
    if args.workload == "webbase":
        return "synthetic:webbase", "webbase-like power law, 75% host-local links (webbase-1M-like)"
    if args.workload == "powerlaw":
        return "synthetic:powerlaw", "power-law rows, uniformly scattered columns"
    if args.workload == "banded":  # north_star: "synthetic banded ... CSR of stated nnz": 4 M rows x 27 diagonals = 108 M entries
        return "synthetic:banded:4000000,13", "banded-4M-27diagonals"
    if args.workload == "random24":  # ... and random: 4 M rows x 24 uniform columns = 96 M entries (host generator)
        return "synthetic:random:4000000,24,3", "random-4M-24perrow (host generator)"
    return None, {"stencil27": "stencil27-253^3", "random": "random-4M-24perrow"}[args.workload]


def load_csr(args, rank, world):
    """This rank's rows of the workload as CSR arrays: (rows_total, cols, nnz_total or None, p, c, v, begin, end,
    ranges or None, keep-alive object)."""
    from spmv_amd import hostapi, partition, synth
    spec, _ = workload_spec(args)
    ranges = None
    if spec is None:  # numpy generators of round 1 (whole matrix, then cut)
        if args.workload == "stencil27":
            rows, cols, p, c, v = synth.stencil27_like(253, 253, 253)
        else:
            rows, cols, p, c, v = synth.random_uniform(4000000, 4000000, 24, seed=3)
        keep = None
    elif world > 1 and spec.startswith("synthetic:") and args.partition == "rows":
        # a generated matrix: only this rank's rows are made (the row count comes from an empty range)
        probe = hostapi.load_csr_rows(spec, 0, 0)
        rows = probe.rows_total
        probe.close()
        begin, end = partition.row_range(rows, rank, world)
        keep = hostapi.load_csr_rows(spec, begin, end)
        return rows, keep.cols, None, keep.row_ptr, keep.column_index, keep.value, begin, end, None, keep
    elif world > 1 and spec.startswith("synthetic:") and args.partition == "nnz":
        # equal stored entries per rank WITHOUT any rank holding the whole matrix: every rank generates its static chunk, the
        # ranks exchange their entry counts, each finds the cut rows that fall into its chunk (partition.nnz_balanced_ranges'
        # rule: first row whose row_ptr >= g * nnz / G), and then generates the rows it really owns
        import torch.distributed as dist
        probe = hostapi.load_csr_rows(spec, 0, 0)
        rows = probe.rows_total
        probe.close()
        b0, e0 = partition.row_range(rows, rank, world)
        part = hostapi.load_csr_rows(spec, b0, e0)
        lp = np.asarray(part.row_ptr, dtype=np.int64)
        counts = [None] * world
        dist.all_gather_object(counts, int(lp[-1]))
        offset, total = sum(counts[:rank]), sum(counts)
        cuts = {}
        for g in range(1, world):
            t = g * total // world
            if offset < t <= offset + counts[rank]:
                cuts[g] = b0 + int(np.searchsorted(lp, t - offset, side="left"))
            elif t <= 0 and rank == 0:
                cuts[g] = 0
        part.close()
        every = [None] * world
        dist.all_gather_object(every, cuts)
        bounds = [0] * (world + 1)
        bounds[world] = rows
        for g in range(1, world):
            bounds[g] = min(c[g] for c in every if g in c)
        bounds = [int(v) for v in np.maximum.accumulate(np.minimum(bounds, rows))]
        ranges = [(bounds[g], bounds[g + 1]) for g in range(world)]
        begin, end = ranges[rank]
        keep = hostapi.load_csr_rows(spec, begin, end)
        return rows, keep.cols, total, keep.row_ptr, keep.column_index, keep.value, begin, end, ranges, keep
    else:
        keep = hostapi.load(spec, "csr", expand_symmetric=args.expand_symmetric)
        rows, cols, p, c, v = keep.rows, keep.cols, keep.row_ptr, keep.column_index, keep.value
    nnz = int(p[-1])
    begin, end = 0, rows
    if world > 1:
        if args.partition == "nnz":
            ranges = partition.nnz_balanced_ranges(p, world)
            begin, end = ranges[rank]
        else:
            begin, end = partition.row_range(rows, rank, world)
        p, c, v = partition.csr_slice(p, c, v, begin, end)
    return rows, cols, nnz, p, c, v, begin, end, ranges, keep


def host_cores():
    """Cores this process may really use: the affinity mask capped by the cgroup CPU quota
    (a GPU box exposes all host CPUs but grants one GPU's share of them)."""
    n = len(os.sched_getaffinity(0))
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                quota, period = txt[0], txt[1]
            else:
                quota, period = txt[0], open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read().split()[0]
            if quota not in ("max", "-1"):
                n = min(n, max(1, int(int(quota) / int(period))))
            break
        except (OSError, ValueError, IndexError):
            continue
    return n


def pmc_traffic(kernel_name, workload, algorithmic_bytes, streamed_bytes=None, build=None, kernel_us=None):
    """HBM bytes per launch of the dominant kernel from the newest committed rocprofv3 PMC summary
    (profiles/*_summary.json, written by tools/profile_gpu.sh: FETCH_SIZE x2 + WRITE_SIZE, the
    gfx950 correction of MI355X_MICROARCH.md).  Counters cannot be read from inside this process,
    so the figure is only reported when the summary was taken (a) on the same kernel and workload --
    same algorithmic and streamed bytes -- and (b) with the same device code: the summary's bench
    line carries `build.source_sha256` (hash of csrc/ + include/spmv_hip.h) and it must equal the
    running library's.  A profiled process runs several variants of one kernel template (the timed
    plan and, e.g., the general-values companion): the variant is told by its average duration,
    the one closest to `kernel_us`.  Returns (bytes, file name, lib hash equal too?, variant, its avg us) or None."""
    import glob
    best = None
    seq = -1
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "*_summary.json"))):
        try:
            d = json.load(open(f))
            bl = d.get("bench_line") or {}
            rl = bl.get("roofline", {})
            if rl.get("algorithmic_bytes_per_launch") != algorithmic_bytes:
                continue
            # the same tile classes too (a plan with and one without a value dictionary run different kernel variants)
            if streamed_bytes is not None and rl.get("streamed_bytes_per_launch") not in (None, streamed_bytes):
                continue
            theirs = bl.get("build") or {}
            if not build or not theirs.get("source_sha256") or theirs["source_sha256"] != build.get("source_sha256"):
                continue  # another binary (or a summary from before the stamp existed): not evidence for this one
            if d.get("sequence", 0) <= seq:
                continue
            names = (kernel_name,) if isinstance(kernel_name, str) else tuple(kernel_name)
            cands = [k for k in d["kernels"] if any(n in k["kernel"] for n in names) and "hbm_traffic_bytes_per_launch" in k and k.get("avg_us")]
            if not cands:
                continue
            k = min(cands, key=lambda q: abs(q["avg_us"] - kernel_us)) if kernel_us else cands[0]
            if kernel_us and abs(k["avg_us"] - kernel_us) > 0.25 * kernel_us:
                continue  # no variant of that duration in the profile: not this launch
            seq = d.get("sequence", 0)
            best = (k["hbm_traffic_bytes_per_launch"], os.path.basename(f), theirs.get("lib_sha256") == build.get("lib_sha256"), k["kernel"], k["avg_us"])
        except (OSError, ValueError, KeyError):
            continue
    return best


# (whole kernel names: "csr_blockwin" alone would also match the plan-time csr_blockwin_mark_kernel, whose duration on the
# queen-like matrix happens to equal the multiply's)
MULTIPLY_KERNELS = ("csr_wavetile_kernel", "csr_segtile_kernel", "csr_segwin_kernel", "csr_blockwin_kernel", "csr_blockwin_stream_kernel",
                    "coo_wide_kernel", "spmv::ell_kernel")


def attach_traffic(d, build, triad_gbs):
    """a companion (config2_queen, config3_kkt, config4_webbase.*, north_star_synthetic.*) carries the PMC
    traffic of its launch when profiles/ holds a rocprofv3 summary of that workload taken with the running device code
    (tools/profile_gpu.sh --all); looked up exactly like the headline's (pmc_traffic).  Never measured in this run."""
    if not isinstance(d, dict) or not d.get("algorithmic_bytes_per_launch") or not d.get("kernel_us"):
        return
    if triad_gbs and d.get("streamed_bytes_per_launch"):
        d["frac_streamed_of_triad"] = round(d["streamed_bytes_per_launch"] / (d["kernel_us"] * 1e-6) / 1e9 / triad_gbs, 4)
    tr = pmc_traffic(MULTIPLY_KERNELS, d.get("workload"), int(d["algorithmic_bytes_per_launch"]), d.get("streamed_bytes_per_launch"), build, d["kernel_us"])
    if tr:
        d["traffic"] = tr[0]
        d["traffic_over_algorithmic_bytes"] = round(tr[0] / max(1, int(d["algorithmic_bytes_per_launch"])), 3)
        d["frac_traffic"] = round(tr[0] / (d["kernel_us"] * 1e-6) / 1e9 / HBM_PEAK_GBS, 4)
        d["traffic_source"] = "profiles/%s, kernel %s (%.1f us average under rocprofv3), same device sources %s; not measured in this run" % (
            tr[1], tr[3], tr[4], build["source_sha256"])
    else:
        d["traffic"] = None
        d["traffic_source"] = "none: no committed profiles/*_summary.json of this workload was taken with device sources %s" % build["source_sha256"]


def format_bytes(fmt, rows, cols, nnz, stored=None, coo_entries=0):
    """Algorithmic bytes of one y += A*x (SURVEY 8d / BASELINE.md section 3)."""
    from spmv_amd import synth
    if fmt == "csr":
        return synth.csr_bytes(rows, cols, nnz)
    if fmt == "coo":
        return synth.coo_bytes(rows, cols, nnz)
    if fmt == "ell":
        return 12 * stored + 16 * rows + 8 * cols
    return 12 * stored + 16 * coo_entries + 16 * rows + 8 * cols  # hybrid: ELL part + COO remainder


def cpu_model():
    """The host CPU's model name (core count and CPU model go into the result)."""
    try:
        for line in open("/proc/cpuinfo"):
            if line.lower().startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return None


def cpu_baseline(args, fmt, rows, cols, A, x, y_gpu=None, budget=None):
    """The reference's OpenMP kernel (or the C oracle) on the host cores, bounded sample.  Also the
    parity gate: one CPU multiply from y = 0 is compared with the GPU's (y_gpu), whole vector,
    tolerance 1e-10 relative (BASELINE.json).  A = dict of the format's arrays.  Returns (cpu_baseline, parity)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle_py
    threads = args.cpu_threads or host_cores()
    budget = args.cpu_seconds if budget is None else budget
    nnz = A["nnz"]
    if fmt == "csr":
        p, c, v = A["p"], A["c"], A["v"]
    spec, _ = workload_spec(args)
    child = None
    if fmt == "csr" and spec is not None and oracle_py.RefLib.available() and not args.cpu_threads and budget >= 2 and \
            os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libref_profile.so")):
        child = cpu_baseline_protocol(args, spec, threads, budget)
    if fmt == "csr" and child is not None and "error" not in child:
        # SURVEY 8(d)'s protocol, run in a process of its own (the OpenMP runtime reads its placement variables at start-up);
        # here only the y for the parity gate is computed, by the same reference kernel
        R = oracle_py.RefLib()
        M = R.csr_from_arrays(rows, cols, p, c, v)
        y_cpu = R.csr_spmv(M, x, num_threads=min(threads, 16)) if y_gpu is not None else None
        R.csr_free(M)
        threads = child["threads"]
        ns = np.array([child["median_ns"], child["min_ns"]])
        med_override = child["median_ns"] * 1e-9
        ns1 = np.array([2.0 * nnz / child["single_thread_gflops"]])
        kind = "reference"
    elif fmt == "csr" and oracle_py.RefLib.available():
        R = oracle_py.RefLib()
        M = R.csr_from_arrays(rows, cols, p, c, v)
        t = time.perf_counter()
        if not args.cpu_threads:
            # the box may expose more CPUs than it grants: probe a few team sizes briefly
            best = None
            for cand in sorted({min(threads, 16), min(threads, 32), min(threads, 64), threads} if budget >= 8 else {threads}):
                ns, _ = R.csr_spmv_timed(M, x, cand, 2)
                if best is None or np.median(ns) < best[0]:
                    best = (float(np.median(ns)), cand)
            threads = best[1]
        ns, _ = R.csr_spmv_timed(M, x, threads, 2)  # 1 warm-up + 2 timed, to size the sample
        per = max(float(np.median(ns)) * 1e-9, 1e-4)
        runs = int(max(3, min(200, (budget - (time.perf_counter() - t)) / per)))
        ns, _ = R.csr_spmv_timed(M, x, threads, runs)
        ns1, _ = R.csr_spmv_timed(M, x, 1, 3)  # one thread, as BASELINE configs[0] is defined
        y_cpu = R.csr_spmv(M, x, num_threads=threads) if y_gpu is not None else None
        R.csr_free(M)
        kind = "reference"
    else:
        O = oracle_py.Oracle()
        if fmt == "csr":
            run = lambda y, T: O.csr_spmv_inplace(rows, p, c, v, x, y, T)
            fresh = lambda T: O.csr_spmv(rows, p, c, v, x, num_threads=T)
        elif fmt == "coo":
            # the atomic form is what the GPU kernel implements (coo-matrix.cpp:287-309)
            fresh = lambda T: O.coo_spmv_atomic(rows, A["r"], A["c"], A["v"], x, num_threads=T)
            run = lambda y, T: fresh(T)
        elif fmt == "ell":
            fresh = lambda T: O.ell_spmv(rows, A["L"], A["c"], A["v"], x, num_threads=T)
            run = lambda y, T: fresh(T)
        else:
            H = dict(row_length=A["L"], ell_col=A["c"], ell_val=A["v"], coo_row=A["cr"], coo_col=A["cc"], coo_val=A["cv"],
                     skip_padding=False)
            fresh = lambda T: O.hybrid_spmv(rows, H, x, num_threads=T)
            run = lambda y, T: fresh(T)
        y = np.zeros(rows)
        run(y, threads)  # warm-up
        ns = []
        t_end = time.perf_counter() + budget
        while len(ns) < 3 or (time.perf_counter() < t_end and len(ns) < 200):
            t0 = time.perf_counter_ns()
            run(y, threads)
            ns.append(time.perf_counter_ns() - t0)
        ns = np.array(ns)
        ns1 = []
        for _ in range(3):
            t0 = time.perf_counter_ns()
            run(y, 1)
            ns1.append(time.perf_counter_ns() - t0)
        ns1 = np.array(ns1)
        y_cpu = fresh(threads if fmt in ("csr", "ell") else 1) if y_gpu is not None else None
        kind = "port"
    med = float(np.median(ns)) * 1e-9
    if child is not None and "error" not in child:
        med = med_override
    parity = None
    if y_gpu is not None:
        diff = np.abs(y_gpu - y_cpu)
        finite = bool(np.isfinite(y_gpu).all())
        err = float(np.max(diff) / max(float(np.max(np.abs(y_cpu))), 1e-300)) if finite else float("nan")
        # per row |y_gpu - y_cpu| <= 1e-10 * max(|y_cpu_i|, 1e-6 * ||y_cpu||_inf); norm-wise 1e-10
        ninf = float(np.max(np.abs(y_cpu))) if rows else 0.0
        row_bound = 1e-10 * np.maximum(np.abs(y_cpu), 1e-6 * ninf) + 1e-300
        worst_row = float(np.max(diff / row_bound)) if (finite and rows) else float("nan")
        parity = {"against": "cpu_baseline kernel (%s), one multiply from y = 0" % kind, "rows_checked": int(rows),
                  "max_rel_err": err if finite else "nan", "tolerance": 1e-10, "pass": bool(finite and err <= 1e-10),
                  "worst_row_over_8d_bound": round(worst_row, 4) if finite else "nan",
                  "rows_outside_8d_bound": int(np.count_nonzero(diff > row_bound)) if finite else None,
                  "bitexact": bool(np.array_equal(y_gpu, y_cpu))}
    out = {"value": round(2.0 * nnz / med / 1e9, 3), "unit": "GFLOP/s", "cores": threads, "kind": kind,
           "sample": "full workload (%s), %d timed runs after 1 warm-up, median %.2f ms (min %.2f ms), %d OpenMP threads"
                     % (fmt, child["runs"] if (child and "error" not in child) else len(ns), med * 1e3, float(np.min(ns)) * 1e-6, threads),
           "gbs": round(A["bytes"] / med / 1e9, 2),
           "single_thread_gflops": round(2.0 * nnz / (float(np.median(ns1)) * 1e-9) / 1e9, 3),
           "cpu_model": cpu_model(), "host_logical_cpus": os.cpu_count(),
           "omp": {k: os.environ.get(k) for k in ("OMP_NUM_THREADS", "OMP_PROC_BIND", "OMP_PLACES")}}
    if child is not None and "error" not in child:
        out.update({"omp": child["omp"], "sweep": child["sweep"], "cpus": child["cpus"], "numa_nodes_of_the_team": sorted(set(child["numa_nodes"])),
                    "numa_nodes_configured": child["numa_nodes_configured"], "pages_distributed": child["pages_distributed"],
                    "protocol": "SURVEY 8(d): a process of its own with OMP_PROC_BIND=close OMP_PLACES=cores; arrays first touched by the master as the "
                                "reference's init does, then moved page by page to the NUMA node of the owning thread by the reference's own "
                                "distribute_pages (src/util/aligned-allocator.hpp:216-271, as csr-spmv.cpp:48-62 calls it); 1 warm-up run, then runs timed "
                                "like profile_kernel_run (src/profile-kernel.cpp:137-179); team size = the fastest of `sweep` (3 runs each)"})
    elif child is not None:
        out["protocol_error"] = child["error"]
    return out, parity


def cpu_baseline_protocol(args, spec, granted, budget):
    """oracle/cpu_baseline_child.py in a process of its own: the OpenMP runtime must see OMP_PROC_BIND / OMP_PLACES when it starts."""
    env = dict(os.environ)
    env.update(OMP_PROC_BIND="close", OMP_PLACES="cores")
    env.pop("OMP_NUM_THREADS", None)
    visible = len(os.sched_getaffinity(0))  # the affinity mask; `granted` is that capped by the cgroup CPU quota
    teams = sorted({t for t in (16, 32, 64, granted) if 0 < t <= visible} | {granted})
    cmd = [sys.executable, os.path.join(ROOT, "oracle", "cpu_baseline_child.py"), "--spec", spec, "--budget", str(budget),
           "--threads", ",".join(str(t) for t in teams)]
    if args.expand_symmetric:
        cmd.append("--expand-symmetric")
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=max(120.0, 20 * budget))
    except (OSError, subprocess.TimeoutExpired) as e:
        return {"error": str(e)[:300]}
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    if r.returncode != 0 or not lines:
        return {"error": (r.stderr or r.stdout).strip()[-300:]}
    return json.loads(lines[-1])


def reference_protocol(args, fmt, runs, flush=False):
    """The same multiply timed the reference's way (src/profile-kernel.cpp:137-179): the C++ CLI
    (host/main.cpp) loads or generates the matrix itself, uploads it through the C ABI, and times
    `runs` runs each bracketed by barriers with the device idle at both ends; --check compares y
    with the CPU CSR kernel after the same number of accumulating runs.  Returns a dict, or a
    dict with "error"."""
    spec, _ = workload_spec(args)
    if spec is None or not os.path.exists(CLI):
        return None
    cmd = [CLI, "--matrix", spec, "--spmv-format", "hip-" + fmt, "--threads", "1", "--profile", str(runs),
           "--x", "uniform", "--check"]
    if args.expand_symmetric:
        cmd.append("--expand-symmetric")
    if flush:
        cmd.append("--flush-caches")
    t0 = time.perf_counter()
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    except (OSError, subprocess.TimeoutExpired) as e:
        return {"error": str(e)}
    if r.returncode != 0 and not r.stdout.strip():
        return {"error": (r.stderr or "").strip()[-300:]}
    try:
        d = json.loads(r.stdout)
    except ValueError:
        return {"error": "unparsable output: " + r.stdout[-200:]}
    et = d["execution_time"]
    flops = d.get("throughput", {}).get("flops_per_run", 0.0)
    out = {"command": " ".join(os.path.basename(c) if c == CLI else c for c in cmd),
           "protocol": "1 warm-up + %d runs, each: barrier, t0, barrier, run + device sync, barrier, t1 (host steady_clock)" % runs,
           "execution_time_ns": {k: et[k] for k in ("samples", "min", "median", "mean", "max")},
           "gflops_median": round(flops / et["median"], 2) if et["median"] else None,
           "device_ns_last_run": d.get("kernel", {}).get("device", {}).get("last_run_device_ns"),
           "parity": d.get("parity"), "wall_s": round(time.perf_counter() - t0, 1),
           # (VERDICT r05 weak point 11: this and the headline are two different launches)
           "plan": "the library's DEFAULT plan through the adapter's context API -- a value dictionary where the matrix has <= 128 distinct values "
                   "(Poisson: two): NOT the value-reading launch that `value` / `roofline` time; compare with roofline.compressed",
           "init_seconds": d.get("kernel", {}).get("device", {}).get("init_seconds"),
           "init_note": "Kernel::init (load / generate, upload over PCIe, plan) is outside the reference's timed window (src/profile-kernel.cpp:262-266) "
                        "but costs the equivalent of ~190 runs for Poisson 4096^2: a --profile=10 session never amortises it"}
    return out


class ContextOperator:
    """COO / ELLPACK / hybrid through the Level-1 context API (what the C++ adapters bind), launched
    on torch's current stream so that the events of the timed region see it."""

    def __init__(self, fmt, M, x, device_index, flags, stream):
        from spmv_amd import capi
        self.ctx = capi.Context(device_index, flags)
        self.ctx.set_stream(stream)
        if fmt == "coo":
            self.ctx.upload_coo(M.rows, M.cols, M.row_index, M.column_index, M.value)
        elif fmt == "ell":
            self.ctx.upload_ell(M.rows, M.cols, M.row_length, M.column_index, M.value)
        else:
            self.ctx.upload_hybrid(M.rows, M.cols, M.row_length, M.column_index, M.value,
                                   M.coo_row_index, M.coo_column_index, M.coo_value)
        self.ctx.set_x(x)
        self.rows = M.rows

    def step(self):
        self.ctx.run(1, sync=False)

    def zero_y(self):
        self.ctx.set_y(np.zeros(self.rows))

    def y(self):
        return self.ctx.get_y()


def host_boundary(capi, device_index, rows, cols, A, x, nnz, runs=5):
    """What the Level-1 boundary costs when the caller's arrays live in HOST memory (the reference's adapters: init uploads the matrix
    once, run multiplies on the device): the upload (PCIe + plan), and one multiply with x sent and y fetched around it -- the
    PCIe-inclusive rate of a caller that keeps nothing resident.  Never `value`."""
    import torch
    # Kernel::init sends arrays the driver has never seen: fresh copies (their pages were never locked for a transfer), as after
    # loading a file.  Beside it: what a plain copy of such an array reaches (pageable hipMemcpy, first touch): the library's own
    # copies are that kind, issued from a helper thread while the caller's thread cuts the tiles (csrc/context.hip, StagedUpload).
    fresh = {k: np.array(A[k], copy=True) for k in ("p", "c", "v")}
    probe = np.array(A["v"], copy=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tprobe = torch.from_numpy(probe).to(torch.device("cuda", device_index))
    torch.cuda.synchronize()
    pageable_s = time.perf_counter() - t0
    del tprobe
    t0 = time.perf_counter()
    ctx = capi.Context(device_index, 0)
    t_create = time.perf_counter()
    ctx.upload_csr(rows, cols, fresh["p"], fresh["c"], fresh["v"])
    t_upload = time.perf_counter()
    ctx.set_x(x)
    ctx.run(1)  # first multiply: the plan's one-time checks
    upload_s = time.perf_counter() - t0
    init_ms = {"create": round((t_create - t0) * 1e3, 2), "upload_csr (copy on a helper thread beside the host tiler; index check, compress, repack, dictionary)":
               round((t_upload - t_create) * 1e3, 2), "set_x + first multiply": round((time.perf_counter() - t_upload) * 1e3, 2)}
    del fresh
    ts = []
    for _ in range(runs):
        t1 = time.perf_counter()
        ctx.set_x(x)
        ctx.run(1)
        y = ctx.get_y()
        ts.append(time.perf_counter() - t1)
    del y
    ctx.close()
    ts.sort()
    med = ts[len(ts) // 2]
    matrix_bytes = 12.0 * nnz + 4.0 * (rows + 1)
    return {"upload_ms": round(upload_s * 1e3, 1), "upload_bytes": int(matrix_bytes),
            "upload_gbs": round(matrix_bytes / upload_s / 1e9, 2), "init_ms": init_ms,
            "pageable_first_touch_gbs": round(probe.nbytes / pageable_s / 1e9, 2),
            "set_x_run_get_y_ms": round(med * 1e3, 3), "vector_bytes_over_pcie": int(8 * (rows + cols)),
            "gflops_pcie_inclusive": round(2.0 * nnz / med / 1e9, 1),
            "note": "spmv_hip_create + upload_csr (host arrays -> device, plan, first multiply) once; then the median of %d x "
                    "(set_x from host, run, get_y to host), pageable host memory, host clock; the arrays are fresh copies (never page-locked before), "
                    "`pageable_first_touch_gbs` = a plain copy of such an array (the value array).  The timed region of `value` has x, y "
                    "and the matrix resident in HBM, as the reference's run() has them resident in DRAM" % runs}


def time_launches(torch, fn, steps, warmup):
    """Mean duration of one launch in seconds: `warmup` launches, then ONE HIP event pair on torch's current stream (the
    stream the launches go to) around `steps` back-to-back launches."""
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / steps


class CacheFlusher:
    """What --flush-caches does between two timed runs (src/profile-kernel.cpp:181-192: flush_cache of 10 x the largest
    cache), on the device: a read-modify-write pass over 1 GiB -- four times the 256 MiB Infinity Cache, 32 times the
    L2s -- so that the next launch finds neither its matrix nor its vectors on the chip."""

    def __init__(self, torch, device):
        self.buf = torch.zeros(128 * 1024 * 1024, dtype=torch.float64, device=device)

    def __call__(self):
        self.buf.add_(1.0)


def cold_launches(torch, fn, flusher, n=10):
    """`n` launches, each after a cache flush, each with its own event pair: (median, min) seconds."""
    t = []
    for _ in range(n):
        flusher()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1) * 1e-3)
    return float(np.median(t)), float(np.min(t))


def build_plan_timed(torch, capi, rows, cols, p, tp, tc, tv, algo, lanes, flags, stream, first_multiply=None):
    """A Level-2 plan built stage by stage with the device idle at both ends of every stage: what the plan costs, in ms.
    `first_multiply(plan)`: one multiply (the first one re-checks the plan's checksums: one pass + a stream sync)."""
    ms = {}

    def stage(name, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms[name] = round((time.perf_counter() - t0) * 1e3, 3)
        return out
    plan = stage("tiles_from_host_row_ptr", lambda: capi.CsrPlan(rows, cols, p, algo, lanes, flags))
    if not (flags & capi.FLAG_NO_INDEX_COMPRESSION):
        stage("confirm_blocks (row groups of a block-tile candidate, tiles cut on them)", lambda: plan.confirm_blocks(tp.data_ptr(), tc.data_ptr(), p, stream))
        stage("compress (tile classes, 16-bit columns, patterns, windows)", lambda: plan.compress(tc.data_ptr(), stream))
        stage("repack (column panels, where the matrix is scattered)", lambda: plan.repack(tp.data_ptr(), tc.data_ptr(), tv.data_ptr(), stream))
        stage("index_values (dictionary, constant-row marks, re-cut tiles)", lambda: plan.index_values(tv.data_ptr(), stream))
    if first_multiply is not None:
        stage("first_multiply (checksum verification + launch)", lambda: first_multiply(plan))
    ms["total"] = round(sum(ms.values()), 3)
    return plan, ms


def companion(torch, capi, hostapi, synth, args, device, stream, spec, fmt, name, flags, algo, steps=30, warmup=10):
    """One of BASELINE's other configurations at full size on this GPU, short: whole-step time (host clock around `steps`
    steps, device idle at both ends), the launch by HIP events, the section-8(d) fraction, and the whole vector of one
    multiply against the CPU kernel (the reference library for CSR, the C oracle for the other formats).  Never `value`."""
    t_all = time.perf_counter()
    M = hostapi.load(spec, fmt)
    rows, cols, nnz = M.rows, M.cols, M.num_entries
    x = synth.x_vector(cols, "uniform", seed=12345)
    if fmt == "csr":
        p, c, v = M.row_ptr, M.column_index, M.value
        tp, tc, tv, tx = (torch.from_numpy(np.ascontiguousarray(t)).to(device) for t in (p, c, v, x))
        ty = torch.zeros(rows, dtype=torch.float64, device=device)
        plan, plan_ms = build_plan_timed(torch, capi, rows, cols, p, tp, tc, tv, algo, args.lanes, flags, stream)
        ptrs = (tp.data_ptr(), tc.data_ptr(), tv.data_ptr(), tx.data_ptr(), ty.data_ptr())
        step = lambda: plan.spmv(*ptrs, stream)
        step()
        torch.cuda.synchronize()
        y_check = ty.cpu().numpy()
        ty.zero_()
        info = plan.info()
        alg_bytes = synth.csr_bytes(rows, cols, nnz)
        host_arrays = {"p": p, "c": c, "v": v}
        extra = {"tiles": info["row_blocks"], "tiles_with_16bit_columns": info["narrow_tiles"], "shifted_tiles": info["shifted_tiles"],
                 "segment_window_tiles": info["segwin_tiles"], "block_row_tiles": info.get("block_tiles", 0),
                 "masked_block_tiles": info.get("masked_block_tiles", 0), "stencil_mask_tiles": info.get("stencil_mask_tiles", 0),
                 "group_tiles": info.get("group_tiles", 0), "multi_window_tiles": info.get("multi_window_tiles", 0),
                 "entries_in_block_tiles": info.get("block_entries", 0) + info.get("masked_block_entries", 0), "entries_in_shifted_tiles": info.get("shifted_entries", 0),
                 "balanced_tiles": bool(info["balanced"]),
                 "value_dictionary_size": info["indexed_values"], "plan_ms": plan_ms}
    else:
        op = ContextOperator(fmt, M, x, device.index or 0, flags | capi.FLAG_NO_RUN_EVENTS, stream)
        step = op.step
        step()
        torch.cuda.synchronize()
        y_check = op.y()
        op.zero_y()
        info = op.ctx.info()
        alg_bytes = format_bytes(fmt, rows, cols, nnz, M.stored, M.num_coo_entries)
        if fmt == "coo":
            host_arrays = {"r": M.row_index, "c": M.column_index, "v": M.value}
        elif fmt == "ell":
            host_arrays = {"L": M.row_length, "c": M.column_index, "v": M.value}
        else:
            host_arrays = {"L": M.row_length, "c": M.column_index, "v": M.value, "cr": M.coo_row_index,
                           "cc": M.coo_column_index, "cv": M.coo_value}
        extra = {"tiles": info["row_blocks"], "tiles_with_16bit_columns": info["narrow_tiles"], "column_panel_tiles": info["panel_tiles"],
                 "ell_row_length": getattr(M, "row_length", None) if fmt != "coo" else None,
                 "coo_remainder_entries": M.num_coo_entries if fmt == "hybrid" else None}
    streamed = int(info["streamed_bytes"])
    for _ in range(warmup):
        step()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    c0 = time.perf_counter()
    e0.record()
    for _ in range(steps):
        step()
    e1.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - c0) / steps
    kern = e0.elapsed_time(e1) * 1e-3 / steps
    host_arrays.update(nnz=nnz, bytes=alg_bytes)
    cpu, parity = (None, None)
    if not args.no_cpu_baseline:
        cpu, parity = cpu_baseline(args, fmt, rows, cols, host_arrays, x, y_check, budget=1.5)
    out = {"workload": name, "format": fmt, "rows": rows, "cols": cols, "nnz": nnz, "steps": steps, "warmup": warmup,
           "ms_per_step": round(wall * 1e3, 5), "gflops": round(2.0 * nnz / wall / 1e9, 2),
           "kernel_us": round(kern * 1e6, 2), "gflops_kernel_only": round(2.0 * nnz / kern / 1e9, 1),
           "algorithmic_bytes_per_launch": int(alg_bytes), "frac_algorithmic": round(alg_bytes / kern / 1e9 / HBM_PEAK_GBS, 4),
           "streamed_bytes_per_launch": streamed, "frac_streamed": round(streamed / kern / 1e9 / HBM_PEAK_GBS, 4),
           "parity": parity, "cpu_gflops": cpu["value"] if cpu else None, "cpu_cores": cpu["cores"] if cpu else None,
           "cpu_kind": cpu["kind"] if cpu else None}
    out.update(extra)
    if fmt == "csr":
        plan.close()
        del tp, tc, tv, tx, ty
    else:
        op.ctx.close()
    M.close()
    torch.cuda.empty_cache()
    out["wall_s"] = round(time.perf_counter() - t_all, 1)
    return out


DROP_IN_SCHEMES = (  # name, SPMV_HIP_FLAG_* bits (capi names), what it is
    ("rccl", (), "one grouped in-place ncclAllGather per run on every device's stream"),
    ("rccl-pipelined", ("FLAG_PIPELINE_GATHER",), "the same collective on a second stream per device beside the next run's multiply"),
    ("peer-push", ("FLAG_PEER_GATHER",), "one push kernel per device and run: the slot stored into the other devices' y over xGMI"),
    ("peer-push-pipelined", ("FLAG_PEER_GATHER", "FLAG_PIPELINE_GATHER"), "the push on a second stream beside the next run's multiply"),
    ("peer-fused", ("FLAG_FUSED_PEER_STORE",), "the multiply kernel stores its row sums into every device's y itself"),
)


def drop_in_child(args):
    """`bench.py --drop-in-child G`: ONE process, G devices, the drop-in's own multi-GPU path (csrc/multi_gpu.hip behind
    include/spmv_hip.h): spmv_hip_create_multi -> ncclCommInitAll, rows cut by ceil(rows / G) (src/matrix/csr-matrix.cpp:77-95),
    x replicated, a grouped in-place ncclAllGather per run -- and the same with the gather as peer stores, fused into the multiply,
    or pipelined behind the next run.  Started fresh by rank 0 of the benchmark (no GPU call has been made in THIS process before
    the library's own); imports neither torch nor anything under oracle/.  Prints one JSON document.

    Two protocols per scheme: `t_total_us` = K runs enqueued back to back, one sync (bench.py's step); `sync_per_run` = the
    reference's timed loop (run, sync, clock: src/profile-kernel.cpp:159-163) with the library's own event split --
    t_local (the slowest device's multiply), t_allgather (the longest span from a device's multiply to the end of its gather)."""
    from spmv_amd import capi, hostapi, synth
    G = args.drop_in_child
    out = {"devices_visible": capi.device_count(), "devices": G, "steps": args.steps, "warmup": args.warmup, "process": "one process, %d device%s" % (G, "" if G == 1 else "s"),
           "workloads": {}}
    share = os.environ.get("SPMV_HIP_SHARE_DEVICES") == "1"  # rehearsal on fewer devices than parts (peer schemes only; RCCL refuses)
    out["rehearsal_shared_devices"] = share and out["devices_visible"] < G
    if out["devices_visible"] < G and not share:
        out["error"] = "%d devices asked for, %d visible" % (G, out["devices_visible"])
        print(json.dumps(out), flush=True)
        return 0
    K, W = max(1, args.steps), max(0, args.warmup)
    base = capi.FLAG_NO_VALUE_INDEX if args.headline == "general" else 0
    for item in [q for q in args.drop_in_specs.split(";") if q]:
        name, spec = item.split("=", 1)
        t_load = time.perf_counter()
        A = hostapi.load(spec, "csr")
        rows, cols, nnz = A.rows, A.cols, int(A.row_ptr[-1])
        x = synth.x_vector(cols, "uniform", seed=12345)
        w = {"spec": spec, "rows": rows, "nnz": nnz, "algorithmic_bytes_per_launch": int(synth.csr_bytes(rows, cols, nnz)),
             "segment_bytes_per_link": int(8 * -(-rows // G)) if G > 1 else 0, "load_s": round(time.perf_counter() - t_load, 2), "schemes": {}}
        signatures = {}
        one = (("one-device", (), "spmv_hip_create_multi with one device: no gather (t1 of the speed-ups below)"),)
        for sname, bits, what in (one + DROP_IN_SCHEMES if G > 1 else one):
            flags = base
            for b in bits:
                flags |= getattr(capi, b)
            r = {"what": what}
            Gs = 1 if sname == "one-device" else G
            try:
                # (a) K runs back to back, no per-run events (what bench.py's step is)
                with capi.Context(num_gpus=Gs, flags=flags | capi.FLAG_NO_RUN_EVENTS) as ctx:
                    t0 = time.perf_counter()
                    ctx.upload_csr(rows, cols, A.row_ptr, A.column_index, A.value)
                    ctx.set_x(x)
                    r["init_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                    info = ctx.info()
                    r["rccl_ranks"] = int(info["rccl_ranks"])
                    r["pipelined"] = bool(info["pipelined"])
                    ctx.run(1)
                    y1 = ctx.get_y()
                    signatures[sname] = (float(y1.sum()), float(np.abs(y1).sum()))
                    ctx.run(W)
                    t0 = time.perf_counter()
                    ctx.run(K)  # K x spmv_hip_run, then one spmv_hip_sync
                    t = (time.perf_counter() - t0) / K
                    r["t_total_us"] = round(t * 1e6, 2)
                    r["gflops"] = round(2.0 * nnz / t / 1e9, 1)
                    r["frac_algorithmic_of_%dx8TBs" % Gs] = round(w["algorithmic_bytes_per_launch"] / t / 1e9 / (HBM_PEAK_GBS * Gs), 4)
                # (b) the reference's protocol: every run waited for, with the library's event split
                with capi.Context(num_gpus=Gs, flags=flags) as ctx:
                    ctx.upload_csr(rows, cols, A.row_ptr, A.column_index, A.value)
                    ctx.set_x(x)
                    ctx.run(3)
                    wall, loc, gat = [], [], []
                    for _ in range(min(K, 20)):
                        t0 = time.perf_counter()
                        ctx.run(1)
                        wall.append(time.perf_counter() - t0)
                        k_ns, g_ns = ctx.last_run_times()
                        loc.append(k_ns)
                        gat.append(g_ns)
                    r["sync_per_run"] = {"t_total_us_median": round(float(np.median(wall)) * 1e6, 2), "t_local_us_median": round(float(np.median(loc)) * 1e-3, 2),
                                         "t_allgather_us_median": round(float(np.median(gat)) * 1e-3, 2), "runs": len(wall)}
                    if Gs > 1 and np.median(gat) > 0 and sname != "peer-fused":
                        r["sync_per_run"]["gather_gbs_per_link"] = round(w["segment_bytes_per_link"] / (float(np.median(gat)) * 1e-9) / 1e9, 2)
            except capi.SpmvHipError as e:
                r["error"] = str(e)[:300]
            w["schemes"][sname] = r
        ok = [k for k, v in w["schemes"].items() if "t_total_us" in v and k != "one-device"] or [k for k, v in w["schemes"].items() if "t_total_us" in v]
        t1 = (w["schemes"].get("one-device") or {}).get("t_total_us")
        if G > 1 and t1:
            # speed-up vs one device on t_total; and what the links allow: every device must RECEIVE G - 1 segments, one
            # per link (direct all-to-all), so a step cannot beat max(t1 / G, segment bytes / link rate) however the gather is done
            links = [v["sync_per_run"]["gather_gbs_per_link"] for v in w["schemes"].values() if (v.get("sync_per_run") or {}).get("gather_gbs_per_link")]
            for k in ok:
                w["schemes"][k]["speedup_vs_one_device"] = round(t1 / w["schemes"][k]["t_total_us"], 3)
            if links:
                link = max(links)
                bound_us = max(t1 / G, w["segment_bytes_per_link"] / (link * 1e9) * 1e6)
                w["speedup_bound_at_measured_link"] = {"link_gbs": link, "step_us_at_best": round(bound_us, 2), "speedup": round(t1 / bound_us, 2),
                                                       "is": "t1 / max(t1 / G, 8 * ceil(rows / G) bytes / the best per-link rate any scheme's gather reached)"}
        if ok:
            best = min(ok, key=lambda k: w["schemes"][k]["t_total_us"])
            w["fastest"] = best
            w["t_total_us"] = w["schemes"][best]["t_total_us"]
            ref = signatures.get("one-device") or signatures.get(ok[0])
            # (sum and absolute sum of y after one run; the row blocks cut their tiles by themselves, so a row of more than 16
            # entries may be added in another lane order than on one device: 1e-12, not bits)
            w["every_scheme_delivers_the_same_y"] = all(abs(signatures[k][0] - ref[0]) <= 1e-12 * ref[1] and abs(signatures[k][1] - ref[1]) <= 1e-12 * ref[1]
                                                        for k in signatures)
        out["workloads"][name] = w
        A.close()
    print(json.dumps(out), flush=True)
    return 0


def drop_in_leg(args, torch, dist, rank, world, use_dist, specs, timeout_s=420):
    """beside the one-process-per-GPU measurement (what the bench contract launches), the SAME workloads through
    the drop-in's own multi-GPU path -- spmv_hip_create_multi in one fresh child process over `world` devices.  Rank 0 starts the
    child (a child process, not an exec; its first GPU call is the library's) while the other ranks wait on the HOST (a key of the
    process group's store: an RCCL barrier would keep a kernel spinning on their devices); every rank has synchronised its device and
    released its caches before.  Never part of `value`; a failure or a timeout is reported in the line, never fatal."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    store = None
    if use_dist:
        try:
            store = dist.distributed_c10d._get_default_store()
        except Exception:
            store = None
        dist.barrier()
        torch.cuda.synchronize()
    result = None
    if rank == 0:
        cmd = [sys.executable, os.path.abspath(__file__), "--drop-in-child", str(world), "--drop-in-specs", ";".join("%s=%s" % kv for kv in specs),
               "--steps", str(min(args.steps, 50)), "--warmup", str(min(args.warmup, 10)), "--headline", args.headline]
        env = dict(os.environ)
        for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "GROUP_RANK", "ROLE_RANK", "MASTER_ADDR", "MASTER_PORT",
                  "TORCHELASTIC_RUN_ID", "HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES", "OMP_NUM_THREADS"):
            if k in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
                continue  # what the launcher made visible stays visible
            env.pop(k, None)
        if args.share_gpu:  # rehearsal: the child's parts share the one device too (peer schemes only; RCCL refuses and says so)
            env["SPMV_HIP_SHARE_DEVICES"] = "1"
        t0 = time.perf_counter()
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=timeout_s)
            lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
            if r.returncode == 0 and lines:
                result = json.loads(lines[-1])
            else:
                result = {"error": "child exited with %d: %s" % (r.returncode, (r.stderr or r.stdout)[-400:])}
        except subprocess.TimeoutExpired:
            result = {"error": "child did not finish within %d s" % timeout_s}
        except (OSError, ValueError) as e:
            result = {"error": str(e)[:300]}
        result["wall_s"] = round(time.perf_counter() - t0, 1)
        result["command"] = " ".join(cmd[1:])
        result["what"] = ("the drop-in's multi-GPU path: ONE process, spmv_hip_create_multi over %d device%s (csrc/multi_gpu.hip: ncclCommInitAll, "
                          "grouped in-place ncclAllGather), started fresh by rank 0 while the other ranks idle; `value` above is the "
                          "one-process-per-GPU path the bench contract launches" % (world, "" if world == 1 else "s"))
        if use_dist and store is not None:
            store.set("drop_in_done", "1")
    if use_dist:
        if store is not None:
            try:
                if rank != 0:
                    store.wait(["drop_in_done"], __import__("datetime").timedelta(seconds=timeout_s + 60))
            except Exception:
                pass
        dist.barrier()
        torch.cuda.synchronize()
    return result


def pmc_child(args):
    """`bench.py --pmc-child` (under `rocprofv3 --pmc <counter> -- python3 bench.py --pmc-child ...`): the headline workload's timed
    plan -- the same flags, the same planning calls as the timed region's -- launched a few times on device 0, nothing else.  No
    checker library, no timing; the counters are read by the parent from rocprofv3's CSV."""
    import torch
    from spmv_amd import capi, hostapi, synth
    spec, _ = workload_spec(args)
    A = hostapi.load(spec, "csr", expand_symmetric=args.expand_symmetric)
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    stream = torch.cuda.current_stream().cuda_stream
    algo = {"auto": capi.CSR_AUTO, "scalar": capi.CSR_SCALAR, "vector": capi.CSR_VECTOR, "adaptive": capi.CSR_ADAPTIVE, "wavetile": capi.CSR_WAVETILE}[args.algorithm]
    flags = (capi.FLAG_XCD_REMAP if args.xcd_remap else 0) | args.flags | (capi.FLAG_NO_VALUE_INDEX if args.headline == "general" else 0)
    x = synth.x_vector(A.cols, "uniform", seed=12345)
    tp, tc, tv, tx = (torch.from_numpy(np.ascontiguousarray(t)).to(device) for t in (A.row_ptr, A.column_index, A.value, x))
    ty = torch.zeros(A.rows, dtype=torch.float64, device=device)
    plan, _ = build_plan_timed(torch, capi, A.rows, A.cols, A.row_ptr, tp, tc, tv, algo, args.lanes, flags, stream)
    for _ in range(max(1, args.steps) + max(0, args.warmup)):
        plan.spmv(tp.data_ptr(), tc.data_ptr(), tv.data_ptr(), tx.data_ptr(), ty.data_ptr(), stream)
    torch.cuda.synchronize()
    print(json.dumps({"pmc_child": True, "streamed_bytes_per_launch": int(plan.info()["streamed_bytes"]), "launches": max(1, args.steps) + max(0, args.warmup)}), flush=True)
    plan.close()
    return 0


def live_pmc_traffic(args, kernel_names, streamed_bytes, timeout_s=100):
    """roofline.traffic MEASURED IN THIS RUN (VERDICT r05 weak point 5): HBM-side bytes per launch of the dominant kernel from the PMC
    counters, collected exactly as MI355X_MICROARCH.md prescribes -- FETCH_SIZE and WRITE_SIZE in SEPARATE rocprofv3 --pmc passes
    (the TCC block cannot hold both), no trace domain beside them, KiB units, FETCH_SIZE doubled (gfx950 counts a 128-byte request as
    64) -- over a child process that launches the timed plan ten times (pmc_child).  rocprofv3 stands directly in front of the python
    interpreter (no env / shell hop).  Returns a dict for the line, or {"error": ...}: the caller then falls back to the committed
    profile of the same device sources."""
    import csv
    import glob
    import shutil
    import tempfile
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(rocprof):
        return {"error": "rocprofv3 not found"}
    child = [sys.executable, os.path.abspath(__file__), "--pmc-child", "--steps", "8", "--warmup", "2", "--headline", args.headline,
             "--workload", args.workload, "--grid", str(args.grid), "--kkt-grid", str(args.kkt_grid), "--algorithm", args.algorithm,
             "--lanes", str(args.lanes), "--flags", hex(args.flags)]
    if args.matrix:
        child += ["--matrix", args.matrix]
    if args.expand_symmetric:
        child.append("--expand-symmetric")
    if args.xcd_remap:
        child.append("--xcd-remap")
    env = dict(os.environ, TMPDIR="/tmp")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    got, took = {}, {}
    for counter in ("FETCH_SIZE", "WRITE_SIZE"):
        outdir = tempfile.mkdtemp(prefix="spmv_pmc_", dir="/tmp")
        t0 = time.perf_counter()
        try:
            r = subprocess.run([rocprof, "--pmc", counter, "--output-format", "csv", "-d", outdir, "--"] + child, cwd="/tmp", env=env,
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout_s)
            if r.returncode != 0:
                return {"error": "rocprofv3 --pmc %s exited with %d: %s" % (counter, r.returncode, (r.stderr or r.stdout)[-300:])}
            info = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{") and "pmc_child" in l]
            if not info or info[-1]["streamed_bytes_per_launch"] != int(streamed_bytes):
                return {"error": "the profiled child built another plan than the timed one (streamed bytes %s against %s)" % (
                    info[-1]["streamed_bytes_per_launch"] if info else None, int(streamed_bytes))}
            vals = []
            for f in glob.glob(os.path.join(outdir, "**", "*counter_collection.csv"), recursive=True):
                for row in csv.DictReader(open(f)):
                    if row.get("Counter_Name") == counter and any(n in row.get("Kernel_Name", "") for n in kernel_names):
                        vals.append(float(row["Counter_Value"]))
            if len(vals) < 4:
                return {"error": "rocprofv3 --pmc %s: %d dispatches of the multiply kernel in its output" % (counter, len(vals))}
            got[counter] = float(np.median(vals))  # KiB per launch
            got[counter + "_launches"] = len(vals)
        except subprocess.TimeoutExpired:
            return {"error": "rocprofv3 --pmc %s did not finish within %d s" % (counter, timeout_s)}
        except (OSError, ValueError, KeyError) as e:
            return {"error": "%s: %s" % (type(e).__name__, str(e)[:200])}
        finally:
            took[counter] = round(time.perf_counter() - t0, 1)
            shutil.rmtree(outdir, ignore_errors=True)
    traffic = int(got["FETCH_SIZE"] * 1024 * 2 + got["WRITE_SIZE"] * 1024)
    return {"traffic": traffic, "FETCH_SIZE_KiB_per_launch": round(got["FETCH_SIZE"], 1), "WRITE_SIZE_KiB_per_launch": round(got["WRITE_SIZE"], 1),
            "launches_counted": [got["FETCH_SIZE_launches"], got["WRITE_SIZE_launches"]], "pass_seconds": took,
            "how": "two rocprofv3 --pmc passes (FETCH_SIZE; WRITE_SIZE) over a child process that launches the timed plan 10 times; "
                   "per launch: median over the multiply kernel's dispatches; bytes = FETCH_SIZE KiB x 1024 x 2 (gfx950) + WRITE_SIZE KiB x 1024"}


def launch_ranks(args):
    """`python bench.py --gpus N` typed plainly (no launcher): start the N ranks as FRESH child processes -- one
    `python -m torch.distributed.run --nnodes=1 --nproc-per-node N` with this command line -- before this process has imported
    torch or made any HIP call, let them write to this process's stdout / stderr (rank 0 prints the one JSON line), and leave
    with their exit code.  Nothing is exec'ed and no process that has initialised the GPU starts another."""
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("OMP_NUM_THREADS", "1")  # what torch.distributed.run would set (and warn about) per rank anyway
    sys.stderr.write("bench.py: --gpus %d without a launcher: starting %d ranks: %s\n" % (args.gpus, args.gpus, " ".join(cmd)))
    sys.stderr.flush()
    return subprocess.call(cmd, env=env)


def main():
    args = parse_args()
    if args.drop_in_child > 0:
        sys.exit(drop_in_child(args))
    if args.pmc_child:
        sys.exit(pmc_child(args))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(args))
    import torch
    import torch.distributed as dist
    from spmv_amd import capi, hostapi, partition, synth
    from spmv_amd.distributed import DistributedCsrSpmv

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            sys.exit("bench.py: --gpus %d needs torch.distributed.run with %d ranks" % (args.gpus, args.gpus))
        args.gpus = world
    if not torch.cuda.is_available():
        sys.exit("bench.py: no GPU visible; this benchmark has no CPU fallback")
    fmt = args.format
    if fmt != "csr" and (world > 1 or args.force_collective):
        sys.exit("bench.py: --format %s runs on one GPU (the row partition of the N > 1 path is CSR)" % fmt)
    if args.share_gpu:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    use_dist = world > 1 or args.force_collective
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        if args.backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)
        else:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        pg_world = dist.get_world_size()
        if pg_world != world:
            sys.exit("bench.py: the process group has %d ranks, WORLD_SIZE says %d" % (pg_world, world))

    def finish(code=0, message=None):
        """Every rank leaves together: the verdict travels before the last barrier."""
        if use_dist:
            flag = torch.tensor([code], dtype=torch.int32, device=device if args.backend == "nccl" else "cpu")
            dist.all_reduce(flag, op=dist.ReduceOp.MAX)
            code = int(flag.item())
            dist.barrier()
            dist.destroy_process_group()
        if code:
            sys.exit(message or "bench.py: a check failed on another rank")
        sys.exit(0)

    # ---- workload ------------------------------------------------------------------------------
    t_setup = time.perf_counter()
    spec, wname = workload_spec(args)
    wname = "%s-%s" % (wname, fmt)
    algo = {"auto": capi.CSR_AUTO, "scalar": capi.CSR_SCALAR, "vector": capi.CSR_VECTOR,
            "adaptive": capi.CSR_ADAPTIVE, "wavetile": capi.CSR_WAVETILE}[args.algorithm]
    flags = (capi.FLAG_XCD_REMAP if args.xcd_remap else 0) | args.flags
    # the timed plan: by default one that READS THE VALUE ARRAY (SURVEY 8(d)'s launch); `flags` alone = the product's default plan
    hflags = flags | (capi.FLAG_NO_VALUE_INDEX if args.headline == "general" else 0)
    stream = torch.cuda.current_stream().cuda_stream
    host_arrays = None  # what the cpu_baseline leg multiplies
    if fmt == "csr":
        rows, cols, nnz, p, c, v, begin, end, ranges, keep = load_csr(args, rank, world)
        if nnz is None:  # only this rank's rows were generated: the total is the sum over ranks
            t = torch.tensor([float(p[-1])], dtype=torch.float64, device=device if args.backend == "nccl" else "cpu")
            dist.all_reduce(t)
            nnz = int(t.item())
        x = synth.x_vector(cols, "uniform", seed=12345)
        op = DistributedCsrSpmv.on_gpu(rows, cols, rank, world, device, p, c, v, x, algo, args.lanes, hflags,
                                       overlap=not args.no_overlap, ranges=ranges, pingpong=not args.snapshot)
        ops = {"rccl": op}
        peer_note = None
        if use_dist and args.gather != "rccl":
            # the same rows, plan and device arrays behind vectors the other ranks can store into (spmv_amd/peer.py)
            from spmv_amd.peer import PeerCsrSpmv, PeerUnavailable
            try:
                for name, fused in (("peer-fused", True), ("peer-push", False)):
                    if args.gather in ("auto", name):
                        ops[name] = PeerCsrSpmv.on_gpu(rows, cols, rank, world, device, p, c, v, x, algo, args.lanes, hflags,
                                                       ranges=ranges, fused=fused, uploaded=op.uploaded)
            except PeerUnavailable as e:
                # (the construction is collective: every rank lands here together) whatever was already set up is closed -- its
                # inter-process mappings before their owners free the memory -- and the run goes on with RCCL alone
                peer_note = "peer stores not available: %s" % e
                for name in [k for k in ops if k != "rccl"]:
                    ops.pop(name).close()
                ops = {"rccl": op}
        local_rows, local_nnz = end - begin, int(p[-1])
        local_bytes = synth.csr_bytes(local_rows, cols, local_nnz)
        total_bytes = synth.csr_bytes(rows, cols, nnz)
        info = op.plan.info()
        streamed = info["streamed_bytes"]
        if world == 1:
            host_arrays = {"p": p, "c": c, "v": v, "nnz": nnz, "bytes": total_bytes}
        step = op.step
        kernel_name = "csr_%s" % capi.CSR_ALGORITHM_NAMES[info["algorithm"]]
    else:
        if spec is None:
            sys.exit("bench.py: --format %s needs --matrix or a generated --workload" % fmt)
        M = hostapi.load(spec, fmt, expand_symmetric=args.expand_symmetric)
        keep = M
        rows, cols, nnz = M.rows, M.cols, M.num_entries
        begin, end, ranges = 0, rows, None
        x = synth.x_vector(cols, "uniform", seed=12345)
        # the timed region brackets K runs with its own event pair: no per-run events inside it
        op = ContextOperator(fmt, M, x, local_rank, flags | capi.FLAG_NO_RUN_EVENTS, stream)
        local_rows, local_nnz = rows, nnz
        local_bytes = total_bytes = format_bytes(fmt, rows, cols, nnz, M.stored, M.num_coo_entries)
        info = op.ctx.info()
        streamed = info["streamed_bytes"]
        step = op.step
        kernel_name = {"coo": "coo_wide", "ell": "csr_wavetile" if info["row_blocks"] else "ell", "hybrid": "csr_wavetile+coo_wide"}[fmt]
        if fmt == "coo":
            host_arrays = {"r": M.row_index, "c": M.column_index, "v": M.value}
        elif fmt == "ell":
            host_arrays = {"L": M.row_length, "c": M.column_index, "v": M.value}
        else:
            host_arrays = {"L": M.row_length, "c": M.column_index, "v": M.value, "cr": M.coo_row_index,
                           "cc": M.coo_column_index, "cv": M.coo_value}
        host_arrays.update(nnz=nnz, bytes=total_bytes)
    torch.cuda.synchronize()
    setup_s = time.perf_counter() - t_setup

    # ---- one multiply into a zero y, kept for the cpu_baseline leg (the only place the checker
    # libraries under oracle/ are loaded), which compares it with the CPU kernel's y.  A plain run
    # makes and fetches it too, unused: the timed steps start from the same device state as in a
    # --full run (the plan's first multiply re-checks its checksums; the fetch idles the device) ----------
    y_check = None
    if world == 1 and not use_dist and not args.no_cpu_baseline and not args.no_parity_check:
        if fmt == "csr":
            op.multiply_local()
            torch.cuda.synchronize()
            y_check = op.y_local[:local_rows].cpu().numpy()
            op.zero()
        else:
            op.step()
            torch.cuda.synchronize()
            y_check = op.y()
            op.zero_y()

    # ---- N > 1: which gather?  A few steps of every scheme that could be set up, max over ranks, fastest wins ----------
    schemes = None
    if fmt == "csr" and use_dist:
        def timed_steps(o, n):
            torch.cuda.synchronize()
            dist.barrier()
            c0 = time.perf_counter()
            for _ in range(n):
                o.multiply_local()
                if o.collective:
                    o.gather_async() if o.overlap else o.gather()
            o.finish()
            torch.cuda.synchronize()
            dist.barrier()
            t = torch.tensor([time.perf_counter() - c0], dtype=torch.float64, device=device)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            return t.item() / n
        # Before anything is timed, every scheme without a collective must deliver what the RCCL all-gather delivers: one multiply
        # from y = 0 with each, the gathered vector's sum and absolute sum compared on every rank (the row sums are the same kernel's:
        # equal bits).  A scheme that does not (peer stores that a platform maps but does not carry) is closed -- collectively, every
        # rank takes the same branch -- and the run goes on without it.  `--reject-scheme NAME` rehearses that branch.
        def signature(o):
            o.zero()
            o.multiply_local()
            if o.collective:
                o.gather()
            o.finish()
            yf = o.y_full
            return torch.stack([yf.sum(), yf.abs().sum()])
        rejected = {}
        if len(ops) > 1:
            ref_sig = signature(ops["rccl"])
            for name in [n for n in ops if n != "rccl"]:
                sig = signature(ops[name])
                bad = bool(((sig - ref_sig).abs() > 1e-9 * ref_sig.abs().clamp_min(1e-300)).any()) or name == args.reject_scheme
                flag = torch.tensor([1.0 if bad else 0.0], dtype=torch.float64, device=device)
                dist.all_reduce(flag, op=dist.ReduceOp.MAX)
                if flag.item() > 0:
                    ops.pop(name).close()
                    rejected[name] = "closed before timing: its gathered y differed from the RCCL scheme's after one multiply" + (
                        " (forced by --reject-scheme)" if name == args.reject_scheme else "")
            for o in ops.values():
                o.zero()
        schemes = {}
        ncal = max(5, min(20, args.warmup))
        for name, o in ops.items():
            timed_steps(o, 3)
            schemes[name] = {"t_total_us": round(timed_steps(o, ncal) * 1e6, 2), "calibration_steps": ncal}
            if not o.collective:
                schemes[name]["multiply_forwards_row_sums"] = bool(o.fused)
        for name, why in rejected.items():
            schemes[name] = {"rejected": why}
        timed = {k: v for k, v in schemes.items() if "t_total_us" in v}
        chosen = args.gather if args.gather in ops else min(timed, key=lambda k: timed[k]["t_total_us"])
        if args.gather != "auto" and args.gather not in ops:
            chosen = "rccl"
        op = ops[chosen]
        step = op.step
        op.zero()  # y accumulates warm-up + K multiplies from here on (gather_check)

    # ---- warm-up, then K timed steps -------------------------------------------------------
    for _ in range(args.warmup):
        step()
    ev0 = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps)]
    ev1 = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps)]
    torch.cuda.synchronize()
    if use_dist:
        dist.barrier()
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    # with a collective in the step the compute stream also carries the waits for earlier gathers,
    # so the span is no longer K launches: time every launch there
    per_launch = args.events == "launch" or use_dist
    if not per_launch:
        ev0[0].record()
    for k in range(args.steps):
        if per_launch:
            ev0[k].record()
        if fmt == "csr":
            op.multiply_local()
        else:
            step()
        if per_launch:
            ev1[k].record()
        if use_dist:
            if op.overlap:
                op.gather_async()
            else:
                op.gather()
    if not per_launch:
        ev1[0].record()
    if fmt == "csr":
        op.finish()
    torch.cuda.synchronize()
    if use_dist:
        dist.barrier()
        torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    # --dump-outputs: y as the last timed step left it (warm-up + K accumulated multiplies), taken before anything below
    # multiplies into the same vector.  With a gather, op.y() waits for it and meets the other ranks: every rank calls it;
    # without one, the rank's segment is the whole vector
    dumped = None
    if args.dump_outputs:
        y_out = op.y() if (fmt != "csr" or use_dist) else op.y_local[:local_rows]
        if rank == 0:
            dumped = dump_outputs(args.dump_outputs, y_out if fmt != "csr" else y_out.cpu().numpy())
        del y_out
    if per_launch:
        kernel_ms = np.array([a.elapsed_time(b) for a, b in zip(ev0, ev1)])
    else:
        kernel_ms = np.array([ev0[0].elapsed_time(ev1[0]) / args.steps])

    stats = torch.tensor([elapsed, float(kernel_ms.mean())], dtype=torch.float64, device=device)
    if use_dist:
        dist.all_reduce(stats, op=dist.ReduceOp.MAX)
    elapsed_max, kern_ms_max = stats.tolist()

    # ---- --full: the empirical denominator, STREAM triad on 3 x 512 MiB in the same process -------------
    triad_gbs = None
    if args.full:
        try:
            nt = 64 * 1024 * 1024
            ta = torch.zeros(nt, dtype=torch.float64, device=device)
            tb = torch.ones(nt, dtype=torch.float64, device=device)
            tc_ = torch.ones(nt, dtype=torch.float64, device=device)
            for _ in range(3):
                capi.triad(nt, ta.data_ptr(), tb.data_ptr(), tc_.data_ptr(), 3.1, stream)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                capi.triad(nt, ta.data_ptr(), tb.data_ptr(), tc_.data_ptr(), 3.1, stream)
            e1.record()
            torch.cuda.synchronize()
            triad_gbs = 24.0 * nt * 20 / (e0.elapsed_time(e1) * 1e-3) / 1e9
            del ta, tb, tc_
        except (RuntimeError, capi.SpmvHipError):
            triad_gbs = None

    # ---- --full, beside the headline launch: its cold time, what its plan cost, and the product's default plan -------------
    # The timed plan reads the value array.  For a matrix with <= 128 distinct values (this Poisson operator has two) the
    # library by default builds a value dictionary and the launch streams one index byte per entry -- or, in constant-row
    # tiles, none -- instead of eight: far fewer bytes than SURVEY 8(d) prices, so that launch is reported BESIDE the
    # roofline row, as `compressed`: same process, same device arrays, same K and warm-up, bit-identical y.
    cold = plan_ms = compressed = None
    single = fmt == "csr" and world == 1 and not use_dist and args.full
    flusher = None
    if single and not args.no_cold:
        flusher = CacheFlusher(torch, device)
        tp, tc, tv, tx = op._keep
        yc = torch.zeros(local_rows, dtype=torch.float64, device=device)
        hp = (tp.data_ptr(), tc.data_ptr(), tv.data_ptr(), tx.data_ptr(), yc.data_ptr())
        med, mn = cold_launches(torch, lambda: op.plan.spmv(*hp, stream), flusher)
        cold = {"kernel_us_median": round(med * 1e6, 2), "kernel_us_min": round(mn * 1e6, 2), "launches": 10,
                "frac": round(local_bytes / med / 1e9 / HBM_PEAK_GBS, 4),
                "flush": "before every launch a read-modify-write pass over 1 GiB (4 x the Infinity Cache), one event pair per launch"}
        del yc
    if single:
        tp, tc, tv, tx = op._keep
        yg = torch.zeros(local_rows, dtype=torch.float64, device=device)
        ptrs = (tp.data_ptr(), tc.data_ptr(), tv.data_ptr(), tx.data_ptr(), yg.data_ptr())
        first = lambda pl: pl.spmv(*ptrs, stream)
        # what the timed plan cost: the same plan built once more, stage by stage (never inside the timed region)
        plan_h, plan_ms = build_plan_timed(torch, capi, local_rows, cols, p, tp, tc, tv, algo, args.lanes, hflags, stream, first)
        plan_h.close()
        other = flags if args.headline == "general" else (flags | capi.FLAG_NO_VALUE_INDEX)
        yg.zero_()
        plan_o, plan_o_ms = build_plan_timed(torch, capi, local_rows, cols, p, tp, tc, tv, algo, args.lanes, other, stream, first)
        oinfo = plan_o.info()
        differs = oinfo["indexed_values"] != info["indexed_values"]
        if differs:
            torch.cuda.synchronize()
            same = bool(y_check is not None and np.array_equal(yg.cpu().numpy(), y_check))
            o_s = time_launches(torch, lambda: plan_o.spmv(*ptrs, stream), args.steps, args.warmup)
            o_cold = cold_launches(torch, lambda: plan_o.spmv(*ptrs, stream), flusher) if flusher else None
            ob = int(oinfo["streamed_bytes"])
            compressed = {"plan": "the library's default (value dictionary of %d values; %d tiles read no value stream at all)" % (
                              oinfo["indexed_values"], oinfo.get("value_row_tiles", 0)) if args.headline == "general"
                          else "SPMV_HIP_FLAG_NO_VALUE_INDEX (values read as doubles)",
                          "kernel_us": round(o_s * 1e6, 2), "gflops": round(2.0 * local_nnz / o_s / 1e9, 1),
                          "streamed_bytes_per_launch": ob,
                          "streamed_over_algorithmic_bytes": round(ob / local_bytes, 4),
                          "frac_streamed": round(ob / o_s / 1e9 / HBM_PEAK_GBS, 4),
                          "frac_streamed_of_triad": round(ob / o_s / 1e9 / triad_gbs, 4) if triad_gbs else None,
                          "frac_algorithmic": round(local_bytes / o_s / 1e9 / HBM_PEAK_GBS, 4),
                          "speedup_over_headline_launch": round(kern_ms_max * 1e-3 / o_s, 3),
                          "cold_kernel_us_median": round(o_cold[0] * 1e6, 2) if o_cold else None,
                          "value_dictionary_size": int(oinfo["indexed_values"]),
                          "tiles_reading_no_value_stream": int(oinfo.get("value_row_tiles", 0)),
                          "tiles_of_the_dictionary_launch": int(oinfo.get("dictionary_launch_tiles", 0)),
                          "plan_ms": plan_o_ms,
                          "bitexact_vs_headline_plan": same if y_check is not None else None,
                          "events": "one pair around the %d timed launches, after %d warm-up launches" % (args.steps, args.warmup)}
        plan_o.close()
        del yg
    del flusher
    torch.cuda.empty_cache()

    # N > 1, --full: the collective on its own (after the timed region, not part of `value`): a few
    # blocking all-gathers, max over ranks, so the line shows where a step's time goes.
    gather_us = None
    if use_dist and args.full:
        op.finish()
        rc_op = ops["rccl"] if fmt == "csr" else op
        times = []
        for _ in range(5):
            torch.cuda.synchronize()
            dist.barrier()
            g0 = time.perf_counter()
            dist.all_gather_into_tensor(rc_op.y_full, rc_op.y_local, group=rc_op.group)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - g0)
        gt = torch.tensor([float(np.median(times))], dtype=torch.float64, device=device)
        dist.all_reduce(gt, op=dist.ReduceOp.MAX)
        gather_us = gt.item() * 1e6

    # N > 1, --full: the gathered y must hold what the OTHER ranks computed.  Rank 0 recomputes a strip of
    # the last rank's rows on its own GPU (product kernel, one multiply) and compares it with the
    # gathered segment, which has accumulated warm-up + K multiplies.
    gather_check = None
    if use_dist:
        op.finish()  # every rank (the peer schemes meet at a barrier here); below, rank 0 reads its vector without one
    if use_dist and args.full and world > 1 and rank == 0 and spec is not None and spec.startswith("synthetic:"):
        ob, oe = ranges[world - 1] if ranges is not None else partition.row_range(rows, world - 1, world)
        strip = min(4096, oe - ob)
        S = hostapi.load_csr_rows(spec, ob, ob + strip)
        tps, tcs, tvs = (torch.from_numpy(np.array(t)).to(device) for t in (S.row_ptr, S.column_index, S.value))
        ys = torch.zeros(strip, dtype=torch.float64, device=device)
        plan_s = capi.CsrPlan(strip, cols, S.row_ptr, algo, args.lanes, flags)
        plan_s.spmv(tps.data_ptr(), tcs.data_ptr(), tvs.data_ptr(), op._keep[3].data_ptr(), ys.data_ptr(), stream)
        torch.cuda.synchronize()
        want = ys * float(args.steps + args.warmup)
        got = op.y_full[(world - 1) * op.chunk:(world - 1) * op.chunk + strip]  # the last rank's slot (static row chunks: = y[ob:])
        err = float((got - want).abs().max() / want.abs().max().clamp_min(1e-300))
        gather_check = {"rows_checked": strip, "of_rank": world - 1, "max_rel_err": err, "pass": bool(err <= 1e-10)}
        plan_s.close()
        S.close()
    if use_dist:
        dist.barrier()  # rank 0 is done reading its vector: the ranks may multiply on

    if use_dist and args.full and schemes is not None:
        # per scheme: the local multiply alone (no delivery of any kind), the delivery alone where it is a launch
        # or a call of its own, and the whole step from the calibration above
        def events_us(fn, n=10):
            fn()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            dist.barrier()
            a.record()
            for _ in range(n):
                fn()
            b.record()
            torch.cuda.synchronize()
            t = torch.tensor([a.elapsed_time(b) * 1e3 / n], dtype=torch.float64, device=device)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            return round(t.item(), 2)
        t_local = events_us(ops["rccl"].multiply_local)
        ops["rccl"].finish()
        for name in schemes:
            if "rejected" in schemes[name]:
                continue
            schemes[name]["t_local_us"] = t_local
        schemes["rccl"]["t_gather_us"] = round(gather_us, 2)
        if "peer-push" in ops:
            schemes["peer-push"]["t_gather_us"] = events_us(ops["peer-push"].deliver) if ops["peer-push"].deliver else 0.0
        if "peer-fused" in ops:
            schemes["peer-fused"]["t_gather_us"] = None  # inside the multiply: t_total - t_local is what it adds
        for o in ops.values():
            o.finish()

    # N > 1, --full, for information only (never `value`): the same K multiplies with ONE all-gather after the
    # last of them -- what a caller pays who, like the reference's timed loop, looks at y only after
    # the loop.  `value` above gathers after every multiply.
    deferred = None
    if use_dist and args.full:
        dop = ops["rccl"] if fmt == "csr" else op
        torch.cuda.synchronize()
        dist.barrier()
        d0 = time.perf_counter()
        for _ in range(args.steps):
            dop.multiply_local()
        dop.gather()
        torch.cuda.synchronize()
        dist.barrier()
        dt = torch.tensor([time.perf_counter() - d0], dtype=torch.float64, device=device)
        dist.all_reduce(dt, op=dist.ReduceOp.MAX)
        deferred = {"steps": args.steps, "all_gathers": 1, "ms_total": round(dt.item() * 1e3, 4),
                    "gflops": round(2.0 * nnz * args.steps / dt.item() / 1e9, 2)}

    # ---- N > 1, --full: what do the links deliver?  (after the timed region; a few ms; never part of `value`) ----------------
    # The y segments travel as stores into the other ranks' vectors (or as RCCL's transfers over the same links): the rate of
    # exactly those stores, per peer and with all peers at once, so that the line explains its own step time.
    probe = None
    if use_dist and args.full and fmt == "csr":
        po = ops.get("peer-push") or ops.get("peer-fused")
        if po is None or world < 2:
            probe = {"link_probe_gbs": None, "why": peer_note or ("one rank" if world < 2 else "no peer-store operator was set up (--gather rccl)")}
        else:
            po.finish()
            tpr = time.perf_counter()
            mine = link_probe(torch, dist, capi, po, rank, world)
            took_ms = (time.perf_counter() - tpr) * 1e3
            everyone = [None] * world
            dist.all_gather_object(everyone, mine)
            po.finish()
            rates = [r for per, _ in everyone for r in per.values() if r]
            tog = [t for _, t in everyone if t]
            probe = {"link_probe_gbs": {"rank%d" % r: {"to_rank%d" % h: g for h, g in sorted(per.items())} for r, (per, _) in enumerate(everyone)},
                     "all_peers_at_once_gbs_per_rank": [t for _, t in everyone],
                     "min_link_gbs": min(rates) if rates else None, "median_link_gbs": float(np.median(rates)) if rates else None,
                     "per_link_gbs_with_all_peers_at_once": round(min(tog) / (world - 1), 2) if tog else None,
                     "bytes_per_store_pass": int(8 * (end - begin)), "took_ms": round(took_ms, 1),
                     "pattern": "rank r stores its y segment into rank (r + k) mod G's vector, k = 1 .. G-1, every rank at once (one sender "
                                "per link and direction), 5 passes per peer after one untimed pass; then into all peers at once",
                     "same_device": bool(args.share_gpu)}

    # ---- --full, companion: BASELINE configs[3] on the same ranks ---------------------------------------------------------
    # The headline workload (configs[1], Poisson: 5 entries per row) cannot scale strongly with a replicated y; the
    # configuration BASELINE.json partitions over 8 GPUs is nlpkkt200 (27 entries per row).  So that a run at N = 1, 2, 4, 8
    # also says what THAT matrix does on the same ranks with the same gather scheme, the default workload's --full line carries
    # a short measurement of its stand-in (30 timed steps after 10 warm-up steps; never part of `value`).
    def partitioned_companion(spec3, label3, note3):
        import argparse as _ap
        a3 = _ap.Namespace(**vars(args))
        a3.matrix, a3.expand_symmetric = spec3, False  # the partition is the headline's (--partition rows | nnz)
        t3 = time.perf_counter()
        rows3, cols3, nnz3, p3, c3, v3, b3, e3, ranges3, keep3 = load_csr(a3, rank, world)
        if nnz3 is None:
            tt = torch.tensor([float(p3[-1])], dtype=torch.float64, device=device if args.backend == "nccl" else "cpu")
            dist.all_reduce(tt)
            nnz3 = int(tt.item())
        x3 = synth.x_vector(cols3, "uniform", seed=12345)
        scheme3 = chosen if (use_dist and schemes is not None) else None
        if scheme3 in ("peer-fused", "peer-push"):
            from spmv_amd.peer import PeerCsrSpmv
            op3 = PeerCsrSpmv.on_gpu(rows3, cols3, rank, world, device, p3, c3, v3, x3, algo, args.lanes, flags, fused=(scheme3 == "peer-fused"),
                                     ranges=ranges3)
        else:
            op3 = DistributedCsrSpmv.on_gpu(rows3, cols3, rank, world, device, p3, c3, v3, x3, algo, args.lanes, flags,
                                            overlap=use_dist and not args.no_overlap, ranges=ranges3)

        def steps3(n):
            for _ in range(n):
                op3.multiply_local()
                if use_dist and op3.collective:
                    op3.gather_async() if op3.overlap else op3.gather()
            op3.finish()
        K3, W3 = 30, 10  # (10 / 3 in round 3: the first launches of a 5 GB matrix run 10 % slower than the rest)
        steps3(W3)
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()
        c0 = time.perf_counter()
        steps3(K3)
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()
        el3 = torch.tensor([time.perf_counter() - c0], dtype=torch.float64, device=device)
        if use_dist:
            dist.all_reduce(el3, op=dist.ReduceOp.MAX)
        # the local multiply alone (no delivery of any kind): one event pair around K3 launches into a scratch vector
        tloc3 = None
        if use_dist:
            op3.finish()
            tp3, tc3, tv3, tx3 = op3._keep
            ys3 = torch.zeros(max(1, e3 - b3), dtype=torch.float64, device=device)
            ptr3 = (tp3.data_ptr(), tc3.data_ptr(), tv3.data_ptr(), tx3.data_ptr(), ys3.data_ptr())
            for _ in range(3):
                op3.plan.spmv(*ptr3, stream)
            ea, eb = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            dist.barrier()
            ea.record()
            for _ in range(K3):
                op3.plan.spmv(*ptr3, stream)
            eb.record()
            torch.cuda.synchronize()
            tl = torch.tensor([ea.elapsed_time(eb) * 1e3 / K3], dtype=torch.float64, device=device)
            dist.all_reduce(tl, op=dist.ReduceOp.MAX)
            tloc3 = tl.item()
            del ys3
        t1_est = tloc3 * world if tloc3 else el3.item() / K3 * 1e6
        i3 = op3.plan.info()
        out3 = {"workload": "%s, csr, %s" % (label3, (("rows/%d static chunks" % world) if ranges3 is None else
                                                       ("%d row ranges of equal stored entries" % world)) if use_dist else "single GPU"),
                "local_rows_min_max": [int(min(e - b for b, e in ranges3)), int(max(e - b for b, e in ranges3))] if ranges3 else None,
                "rows": rows3, "nnz": nnz3, "steps": K3, "warmup": W3, "gather": scheme3 or ("rccl" if use_dist else None),
                "ms_per_step": round(el3.item() / K3 * 1e3, 5), "gflops": round(2.0 * nnz3 * K3 / el3.item() / 1e9, 2),
                "frac_algorithmic_whole_step": round(synth.csr_bytes(rows3, cols3, nnz3) / (el3.item() / K3) / 1e9 / (HBM_PEAK_GBS * world), 4),
                "algorithmic_bytes_per_launch": int(synth.csr_bytes(rows3, cols3, nnz3)) if not use_dist else None,
                "streamed_bytes_per_launch": int(i3["streamed_bytes"]) if not use_dist else None,
                "kernel_us": round(el3.item() / K3 * 1e6, 2) if not use_dist else None, # one GPU: a step IS the launch (host clock, device idle at both ends)
                "local_tiles": i3["row_blocks"], "local_shifted_tiles": i3["shifted_tiles"], "local_x_window_tiles": i3["xwin_tiles"],
                "local_column_panel_tiles": i3["panel_tiles"],
                "setup_s": round(time.perf_counter() - t3 - el3.item(), 1),
                "local_multiply_us": round(tloc3, 2) if tloc3 else None,
                "strong_scaling_model": strong_scaling_model(rows3, t1_est, (probe or {}).get("per_link_gbs_with_all_peers_at_once")),
                "note": note3 + "; strong_scaling_model: t1 = "
                        + ("the slowest rank's local multiply alone (HIP events, no delivery) x ranks: an estimate of the single-GPU time"
                           + ("; NOT meaningful in this rehearsal, where the ranks share one device and its memory" if args.share_gpu else "")
                           if use_dist else "this run's step time")}
        if not op3.collective:
            op3.close()
        del op3, keep3, p3, c3, v3
        torch.cuda.empty_cache()
        return out3

    config3 = None
    north_star = {}
    if args.full and fmt == "csr" and args.matrix is None and args.workload == "poisson2d" and args.grid == 4096 and not args.no_config3:
        config3 = partitioned_companion("synthetic:kkt:200", "kkt-27pt-200^3 (nlpkkt200-like)",
                                        "whole-job GFLOP/s of BASELINE configs[3]'s stand-in on these ranks; parity of this matrix and "
                                        "path: tests/test_gpu_fullsize.py, tests/test_gpu_peer.py")
        # north_star: "throughput on synthetic banded/random CSR of stated nnz is reported at 1, 2, 4 and 8 GPUs": the same short
        # measurement for the two synthetic families (108 M and 96 M entries), on the same ranks, never part of `value`
        if not args.no_north_star:
            north_star["banded"] = partitioned_companion("synthetic:banded:4000000,13", "banded-4M-27diagonals",
                                                         "whole-job GFLOP/s on these ranks; parity: tests/test_gpu_parity.py, bench.py --workload banded")
            north_star["random"] = partitioned_companion("synthetic:random:4000000,24,3", "random-4M-24perrow",
                                                         "whole-job GFLOP/s on these ranks; parity: tests/test_gpu_parity.py, bench.py --workload random24")

    # ---- --full, companions: BASELINE configs[2] and [4] on this GPU (default workload, one GPU) ------------------------------
    companions = {}
    if (args.full and fmt == "csr" and args.matrix is None and args.workload == "poisson2d" and args.grid == 4096 and world == 1
            and not use_dist and not args.no_companions):
        companions["config2_queen"] = companion(torch, capi, hostapi, synth, args, device, stream, "synthetic:queen", "csr",
                                                "queen-like 110x71x177 mesh x 3 dof (Queen_4147-like), csr", flags, algo)
        # round 6: the reference's DEFAULT semantics for the two SuiteSparse files -- a `symmetric` file's stored
        # triangle, nothing mirrored (src/matrix/matrix-market.cpp:396-414, :530-555): section-8(d) bytes of the STORED matrix
        companions["config2_queen_stored"] = companion(torch, capi, hostapi, synth, args, device, stream, "synthetic:queen:tril", "csr",
                                                       QUEEN_STORED_NAME + ", csr", flags, algo)
        companions["config3_kkt_stored"] = companion(torch, capi, hostapi, synth, args, device, stream, "synthetic:kkt:200:tril", "csr",
                                                     KKT_STORED_NAME % (200, 200) + ", csr", flags, algo)
        companions["config4_webbase"] = {
            f: companion(torch, capi, hostapi, synth, args, device, stream, "synthetic:webbase", f,
                         "webbase-like power law, 75%% host-local links (webbase-1M-like), %s" % f, flags, algo, steps=50, warmup=10)
            for f in ("coo", "hybrid", "csr")}
        companions["config4_webbase"]["ell"] = "not representable: rows x longest row overflows int32, the converter throws like the reference's (ell-matrix.cpp:201-205)"

    # ---- --full: the drop-in's own multi-GPU path (one process over all devices) beside the one-process-per-GPU measurement -----
    drop_in = None
    if args.full and fmt == "csr" and spec is not None and not args.no_drop_in and not args.force_collective:
        dspecs = [("headline", spec)]
        if world > 1 and config3 is not None and not args.share_gpu:  # (a rehearsal on one shared device keeps to the headline matrix)
            dspecs.append(("config3_kkt", "synthetic:kkt:200"))
        # (the child holds its own copy of every matrix: this rank's device arrays stay, there is room for both in 288 GB)
        drop_in = drop_in_leg(args, torch, dist, rank, world, use_dist, dspecs)

    code, message = 0, None
    if rank == 0:
        from spmv_amd import buildinfo
        build = buildinfo.build_info(capi.LIB_PATH)
        ms_per_step = elapsed_max / args.steps * 1e3
        gflops = 2.0 * nnz * args.steps / elapsed_max / 1e9
        kern_s = kern_ms_max * 1e-3  # slowest rank's mean launch duration
        achieved = local_bytes / kern_s / 1e9
        streamed_gbs = streamed / kern_s / 1e9
        config = {"workload": wname, "rows": rows, "cols": cols, "nnz": nnz, "format": fmt,
                  "index_dtype": "int32", "x": "uniform(-1,1) seed 12345",
                  "symmetric_file_expanded": bool(getattr(keep, "expanded", False)),
                  "partition": ("%s, x replicated, %s" % (
                      ("rows/%d static chunks" % world) if ranges is None else ("%d row ranges of equal stored entries" % world),
                      ("1 all-gather(y)/step" + ((", gather k overlaps multiply k+1 (%s)" % ("two alternating segment buffers" if op.pingpong else "snapshot copy"))
                                                 if op.overlap else "")) if op.collective else
                      ("y segments stored into every rank's vector by %s" % ("the multiply kernel itself" if getattr(op, "fused", False) else "a push kernel after the multiply")))
                      ) if use_dist else "single GPU",
                  "backend": args.backend if use_dist else None, "rehearsal_shared_gpu": bool(args.share_gpu)}
        if fmt == "csr":
            config.update({"algorithm": capi.CSR_ALGORITHM_NAMES[info["algorithm"]], "lanes_per_row": info["lanes_per_row"],
                           "workgroups": info["workgroups"], "tiles": info["row_blocks"],
                           "tiles_with_16bit_columns": info["narrow_tiles"], "uniform_tiles": info["uniform_tiles"],
                           "shifted_tiles": info["shifted_tiles"], "tiles_with_x_window": info["xwin_tiles"],
                           "block_window_tiles": info["blockwin_tiles"], "column_panel_tiles": info["panel_tiles"],
                           "balanced_tiles": bool(info["balanced"]), "value_dictionary_size": info["indexed_values"],
                           "tiles_reading_no_value_stream": info.get("value_row_tiles", 0),
                           "tiles_of_the_dictionary_launch": info.get("dictionary_launch_tiles", 0),
                           "block_tiles": info.get("block_tiles", 0), "masked_block_tiles": info.get("masked_block_tiles", 0),
                           "group_tiles": info.get("group_tiles", 0), "rows_per_group": info.get("group_rows", 0),
                           "masked_stencil_tiles": info.get("stencil_mask_tiles", 0), "multi_window_tiles": info.get("multi_window_tiles", 0),
                           "long_row_tiles": info.get("long_blocks", 0)})
        else:
            config.update({"ell_row_length": getattr(keep, "row_length", None), "coo_remainder_entries": getattr(keep, "num_coo_entries", None),
                           "tiles": info["row_blocks"], "shifted_tiles": info["shifted_tiles"],
                           "tiles_with_16bit_columns": info["narrow_tiles"], "column_panel_tiles": info["panel_tiles"]})
        # `achieved` = ALGORITHMIC bytes per launch (CSR 12 Z + 4 (N+1) + 16 N + 8 M; COO 16 Z + 16 N + 8 M;
        # ELL 12 N L + 16 N + 8 M) / the launch's mean duration; `frac` = achieved / 8 TB/s.  The bytes the plan's tile
        # classes really stream (values 8 B or an index byte, columns 4 / 2 / 0 B, row_ptr where it is read, y in and out,
        # x once, descriptors) stand beside it under `streamed`: below the algorithmic figure wherever the plan found a
        # cheaper encoding of the columns (shifted tiles read one row of them), so `frac` may pass the rate HBM delivered.
        roofline = {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": None,
                    #  `achieved` / `frac` are SURVEY 8(d)'s ALGORITHMIC figure, not a bandwidth HBM delivered: where the
                    # plan streams fewer bytes than the formula counts they pass the ~6.3 TB/s a copy reaches.  The bandwidth
                    # figures to read beside them: frac_streamed (bytes the tile classes move / time / 8 TB/s), its ratio to the
                    # triad timed in this process, and frac_traffic (PMC bytes / time / 8 TB/s, from a committed profile of the
                    # same device code -- counters cannot be read inside this run: traffic_measured_in_this_run is always false)
                    "achieved_is": "algorithmic bytes / time (SURVEY 8(d)); not a measured bandwidth: see frac_streamed, frac_streamed_of_triad, frac_traffic",
                    "frac_streamed": round(streamed_gbs / HBM_PEAK_GBS, 4),
                    "frac_streamed_of_triad": round(streamed_gbs / triad_gbs, 4) if triad_gbs else None,
                    "frac_traffic": None, "traffic_measured_in_this_run": False,
                    "kernel": kernel_name, "kernel_us": round(kern_s * 1e6, 2),
                    "kernel_us_min": round(float(kernel_ms.min()) * 1e3, 2) if per_launch else None,
                    "events": "per launch" if per_launch else "one pair around the %d timed launches" % args.steps,
                    "bytes_per_launch": int(local_bytes), "bytes_are": "algorithmic (SURVEY 8(d)); the launch reads the value array"
                    if (fmt != "csr" or info.get("indexed_values", 0) == 0) else "algorithmic (SURVEY 8(d)); NOTE: this launch reads a value dictionary, not the value array (--headline product)",
                    "algorithmic_bytes_per_launch": int(local_bytes),
                    "streamed": {"bytes_per_launch": int(streamed), "gbs": round(streamed_gbs, 1), "frac": round(streamed_gbs / HBM_PEAK_GBS, 4),
                                 "frac_of_triad": round(streamed_gbs / triad_gbs, 4) if triad_gbs else None,
                                 "over_algorithmic_bytes": round(streamed / max(1, local_bytes), 4)},
                    "streamed_bytes_per_launch": int(streamed),
                    "triad_gbs": round(triad_gbs, 1) if triad_gbs else None,
                    "gflops_kernel_only": round(2.0 * local_nnz / kern_s / 1e9, 1)}
        if cold is not None:
            roofline["cold"] = cold
        if plan_ms is not None:
            roofline["plan_ms"] = plan_ms
        if single:
            roofline["compressed"] = compressed if compressed is not None else (
                "none: the matrix has more than 128 distinct values (or the plan has its own variant): the library's default plan IS the timed one")
        if fmt == "csr" and local_nnz > 0:
            roofline["share_of_entries_not_reading_column_index"] = round(info["shifted_entries"] / local_nnz, 4)
            roofline["share_of_entries_with_16bit_columns"] = round(info["narrow_entries"] / local_nnz, 4)
            roofline["share_of_rows_not_reading_row_ptr"] = round(info["uniform_rows"] / max(1, local_rows), 4)
            # > 0: the matrix has that many distinct values and the kernel streams ONE byte per entry instead of eight
            roofline["value_dictionary_size"] = info["indexed_values"]
        out = {
            "metric": "spmv_%s_gflops" % fmt, "value": round(gflops, 2), "unit": "GFLOP/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 5), "higher_is_better": True, "scaling": "strong",
            "vs_baseline": None, "dtype": "f64", "data": "synthetic" if (spec is None or spec.startswith("synthetic:")) else "file",
            "config": config, "roofline": roofline,
            "hbm_gbs_whole_step": round(total_bytes / (ms_per_step * 1e-3) / 1e9, 1),
            "setup_s": round(setup_s, 1),
        }
        config["timed_plan"] = ("reads the value array (SPMV_HIP_FLAG_NO_VALUE_INDEX)" if (hflags & capi.FLAG_NO_VALUE_INDEX)
                                else "the library's default plan") if fmt == "csr" else "context upload (library default)"
        if gather_us is not None:
            recv = 8.0 * op.chunk * (world - 1)
            # what the step can reach at best: the local multiply and the gather fully overlapped; the gather is bounded
            # by the bytes a rank must RECEIVE over its 7 xGMI links (direct all-gather, all links busy)
            model_gather_us = recv / (7 * XGMI_LINK_GBS * 1e9) * 1e6 if world > 1 else 0.0
            model_gather_us_fast = recv / (7 * XGMI_LINK_GBS_QUOTED * 1e9) * 1e6 if world > 1 else 0.0
            out["multi_gpu"] = {"local_kernel_us": round(kern_s * 1e6, 2), "all_gather_us": round(gather_us, 2),
                                "all_gather_bytes_received_per_rank": int(recv),
                                "all_gather_gbs_received_per_rank": round(recv / (gather_us * 1e-6) / 1e9, 1) if world > 1 else None,
                                "overlap": bool(op.overlap),
                                "model": {"formula": "predicted_us = max(local_kernel_us, received_bytes / (7 links x %.0f GB/s))" % XGMI_LINK_GBS,
                                          "gather_us_at_link_rate": round(model_gather_us, 1),
                                          "gather_us_at_%.0f_GBs_per_link" % XGMI_LINK_GBS_QUOTED: round(model_gather_us_fast, 1),
                                          "predicted_us": round(max(kern_s * 1e6, model_gather_us), 1),
                                          "predicted_us_at_%.0f_GBs_per_link" % XGMI_LINK_GBS_QUOTED: round(max(kern_s * 1e6, model_gather_us_fast), 1),
                                          "measured_us": round(ms_per_step * 1e3, 1)},
                                "gather": chosen if schemes is not None else "rccl",
                                "schemes": schemes, "peer_note": peer_note if fmt == "csr" else None,
                                "note": "all_gather_us: blocking collective alone, median of 5 after the timed region; schemes: t_total = a "
                                        "whole step (max over ranks) timed before the warm-up, `gather` = the one the timed region ran",
                                "one_all_gather_after_the_k_multiplies": deferred,
                                "ranks": {"world_size": world, "process_group_world_size": int(pg_world), "backend": args.backend,
                                          "devices": "every rank on device 0 (rehearsal)" if args.share_gpu else "one device per rank (LOCAL_RANK)"}}
            if probe is not None:
                out["multi_gpu"].update(probe)
        for k in sorted(companions):
            out[k] = companions[k]
            attach_traffic(companions[k], build, triad_gbs)
            if isinstance(companions[k], dict):
                for sub in companions[k].values():
                    attach_traffic(sub, build, triad_gbs)
        if config3 is not None:
            out["config3_kkt"] = config3
            attach_traffic(config3, build, triad_gbs)
        if north_star:
            out["north_star_synthetic"] = north_star
            for sub in north_star.values():
                attach_traffic(sub, build, triad_gbs)
        if drop_in is not None:
            h = (drop_in.get("workloads") or {}).get("headline") or {}
            if h.get("t_total_us"):
                # N = 1: the same launch through the context API in another process must reproduce the timed region within box spread
                h["over_this_run_ms_per_step"] = round(h["t_total_us"] * 1e-3 / ms_per_step, 3)
            k3 = (drop_in.get("workloads") or {}).get("config3_kkt") or {}
            if k3.get("t_total_us") and config3 is not None and config3.get("ms_per_step"):
                k3["over_the_per_process_path_ms_per_step"] = round(k3["t_total_us"] * 1e-3 / config3["ms_per_step"], 3)
            out["drop_in_multi_gpu"] = drop_in
        if gather_check:
            out["gather_check"] = gather_check
            if not gather_check["pass"]:
                code, message = 1, "bench.py: gathered y does not match the owning rank's rows"
        out["build"] = build
        if dumped is not None:
            out["dumped_outputs"] = dumped
        tr = pmc_traffic(kernel_name, wname, int(local_bytes), out["roofline"].get("streamed_bytes_per_launch"), build, kern_s * 1e6) if args.full else None
        live = None
        under_profiler = any("ROCPROF" in k or k.startswith("ROCP_") for k in os.environ)  # (this run is itself a rocprofv3 child: no nesting)
        if args.full and world == 1 and not use_dist and fmt == "csr" and spec is not None and not args.no_live_pmc and code == 0 and not under_profiler:
            live = live_pmc_traffic(args, MULTIPLY_KERNELS, streamed)
        if live is not None and "traffic" in live:
            # measured in THIS run, on THIS box, with the library that was just timed; the committed profile (another run, another
            # box, the same device sources) stands beside it as a cross-check
            out["roofline"]["traffic"] = live["traffic"]
            out["roofline"]["traffic_measured_in_this_run"] = True
            out["roofline"]["traffic_over_bytes"] = round(live["traffic"] / max(1, int(streamed)), 3)
            out["roofline"]["traffic_over_algorithmic_bytes"] = round(live["traffic"] / max(1, int(local_bytes)), 3)
            out["roofline"]["frac_traffic"] = round(live["traffic"] / kern_s / 1e9 / HBM_PEAK_GBS, 4)
            out["roofline"]["traffic_source"] = live["how"]
            out["roofline"]["traffic_live"] = {k: live[k] for k in ("FETCH_SIZE_KiB_per_launch", "WRITE_SIZE_KiB_per_launch", "launches_counted", "pass_seconds")}
            if tr:
                out["roofline"]["traffic_committed_profile"] = {"bytes": tr[0], "file": "profiles/" + tr[1], "over_live": round(tr[0] / live["traffic"], 4)}
        elif tr:
            if live is not None:
                out["roofline"]["traffic_live"] = live  # why the live measurement did not happen
            out["roofline"]["traffic"] = tr[0]
            out["roofline"]["traffic_over_bytes"] = round(tr[0] / max(1, int(streamed)), 3)
            out["roofline"]["frac_traffic"] = round(tr[0] / kern_s / 1e9 / HBM_PEAK_GBS, 4)
            out["roofline"]["traffic_source"] = ("profiles/%s, kernel %s (%.1f us average under rocprofv3; PMC passes of the same command on the "
                                                 "same device code: source_sha256 %s matches%s)" % (tr[1], tr[3], tr[4], build["source_sha256"],
                                                                                                    "" if tr[2] else "; the .so was rebuilt from it since"))
            out["roofline"]["traffic_over_algorithmic_bytes"] = round(tr[0] / max(1, int(local_bytes)), 3)
            if compressed is not None:  # the other launch was profiled in the same process
                tg = pmc_traffic(kernel_name, wname, int(local_bytes), out["roofline"].get("streamed_bytes_per_launch"), build, compressed["kernel_us"])
                if tg and tg[3] != tr[3]:
                    compressed["traffic"] = tg[0]
                    compressed["traffic_over_streamed_bytes"] = round(tg[0] / max(1, compressed["streamed_bytes_per_launch"]), 3)
        else:
            if live is not None:
                out["roofline"]["traffic_live"] = live
            out["roofline"]["traffic_source"] = ("none: no committed profiles/*_summary.json of this workload was taken with device "
                                                 "sources %s" % build["source_sha256"]) if args.full else "not looked for: bench.py --full"
        if args.full and world == 1 and not use_dist and not args.no_cpu_baseline:
            out["cpu_baseline"], out["parity"] = cpu_baseline(args, fmt, rows, cols, host_arrays, x, y_check)
            if out["parity"] and not out["parity"]["pass"]:
                code, message = 1, "bench.py: parity check failed: max relative error %s > 1e-10" % out["parity"]["max_rel_err"]
        else:
            out["cpu_baseline"] = None
        if args.full and world == 1 and not use_dist and fmt == "csr" and not args.no_host_boundary and host_arrays is not None and code == 0:
            try:
                out["host_boundary"] = host_boundary(capi, device.index or 0, rows, cols, host_arrays, x, nnz)
            except Exception as e:  # reported, never fatal: the line's value does not depend on it
                out["host_boundary"] = {"error": str(e)[:200]}
        if args.full and world == 1 and not use_dist and not args.no_reference_protocol and code == 0:
            big = nnz > 200e6
            rp = reference_protocol(args, fmt, 10 if big else 20)
            if rp is not None:
                out["reference_protocol"] = rp
                if args.cold and "error" not in rp:
                    cold = reference_protocol(args, fmt, 10, flush=True)
                    if cold is not None:
                        rp["flushed"] = {k: cold.get(k) for k in ("command", "execution_time_ns", "gflops_median", "device_ns_last_run", "error") if k in cold}
        print(json.dumps(out), flush=True)
    if fmt == "csr":
        for o in ops.values():
            if not o.collective:
                o.close()  # collective: mappings are closed before their owners free the memory
    finish(code, message)


if __name__ == "__main__":
    main()
