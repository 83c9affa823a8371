#!/usr/bin/env python3
"""Transposed multiply y += A' x from the arrays of A (include/spmv_hip_transpose.h) against the ways the project had before,
one process, torch tensors, interleaved rounds after a warm-up:

    spmv_t      spmv_hip_csr_spmv_t on A as it is stored: no transposed copy
    transposed  the default CSR plan (what spmv_hip_upload_csr builds) on A', transposed on the host and uploaded beside A
    symv        for stored triangles only: spmv_hip_csr_symv on the same arrays (it adds T x + T' x - D x: a superset of the work)

Per matrix: microseconds per multiply (median and min over the rounds, each round the mean of --reps back-to-back launches),
the largest difference of spmv_t against transposed scaled by (|A'| |x|)_i, the device bytes each way needs beside A, the
transposed plan's info, the time its atomic adds would take at the chip-wide rate of fp64 atomics, and how long each plan
took to build.  The log goes to stdout and to profiles/transpose_ab.log.

    python tools/transpose_ab.py                       # queen, kkt, Delaunay RCM, Poisson 4096^2, webbase-like, queen:tril
    python tools/transpose_ab.py --only queen_tril --rounds 25 --reps 1
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spmv-cache-trace_amd", "python"))

MATRICES = [
    ("queen_tril", "synthetic:queen:tril", "Queen_4147-like stored triangle (full size): the gate against symv"),
    ("queen", "synthetic:queen", "Queen_4147-like, both triangles (full size)"),
    ("kkt", "synthetic:kkt:200", "nlpkkt200-like, both triangles"),
    ("delaunay_rcm", "delaunay:250000,3,1,rcm", "Delaunay 3-D mesh, 3 unknowns per node, RCM order"),
    ("poisson", "synthetic:poisson2d:4096", "5-point Poisson 4096^2"),
    ("webbase", "synthetic:webbase", "webbase-1M-like graph"),
]
ATOMIC_RATES_TBS = {"guide": 1.3, "measured": 0.92}  # chip-wide fp64 atomic adds: the guide's figure, and DESIGN 3.8's


def load(spec):
    """(rows, cols, A arrays, A' arrays): CSR with ascending columns; A' by scipy (a stable transposition)."""
    import scipy.sparse as sp
    from spmv_amd import hostapi, synth
    if spec.startswith("delaunay:"):
        q = spec[9:].split(",")
        rows, cols, p, c, v = synth.delaunay_mesh(int(q[0]), int(q[1]), seed=int(q[2]), order=q[3])
    else:
        H = hostapi.load(spec, "csr")
        rows, cols, p, c, v = H.rows, H.cols, np.array(H.row_ptr), np.array(H.column_index), np.array(H.value)
        H.close()
    p, c, v = p.astype(np.int32), c.astype(np.int32), v.astype(np.float64)
    At = sp.csr_matrix((v, c, p), shape=(rows, cols)).T.tocsr()
    At.sort_indices()
    return rows, cols, (p, c, v), (At.indptr.astype(np.int32), At.indices.astype(np.int32), At.data.astype(np.float64))


def default_plan(capi, rows, cols, host_p, tp, tc, tv, stream):
    """The plan spmv_hip_upload_csr builds (context.hip): tiles, block confirmation, compression, panels, value dictionary."""
    plan = capi.CsrPlan(rows, cols, host_p, capi.CSR_AUTO, 0, 0)
    plan.confirm_blocks(tp.data_ptr(), tc.data_ptr(), host_p, stream)
    plan.compress(tc.data_ptr(), stream)
    plan.repack(tp.data_ptr(), tc.data_ptr(), tv.data_ptr(), stream)
    plan.index_values(tv.data_ptr(), stream)
    return plan


def measure(torch, capi, synth, name, spec, rounds, reps):
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    t0 = time.time()
    rows, cols, (ap, ac, av), (bp, bc, bv) = load(spec)
    load_s = time.time() - t0
    nnz = int(ap[-1])
    A = [torch.from_numpy(a).to(dev) for a in (ap, ac, av)]
    B = [torch.from_numpy(a).to(dev) for a in (bp, bc, bv)]
    tx = torch.from_numpy(synth.x_vector(rows, "uniform", seed=12345)).to(dev)
    torch.cuda.synchronize()

    t0 = time.time()
    tr = capi.TrPlan(rows, cols, ap, A[1].data_ptr(), 0, 0, stream)
    tr_plan_s = time.time() - t0
    t0 = time.time()
    tplan = default_plan(capi, cols, rows, bp, *B, stream)
    torch.cuda.synchronize()
    tplan_s = time.time() - t0
    ways = {
        "spmv_t": lambda y: tr.spmv_t(A[0].data_ptr(), A[1].data_ptr(), A[2].data_ptr(), tx.data_ptr(), y, stream),
        "transposed": lambda y: tplan.spmv(B[0].data_ptr(), B[1].data_ptr(), B[2].data_ptr(), tx.data_ptr(), y, stream),
    }
    sym = None
    if rows == cols and capi.csr_triangle(rows, ap, ac)[0] in (capi.TRIANGLE_LOWER, capi.TRIANGLE_UPPER):
        sym = capi.SymPlan(rows, ap, A[1].data_ptr(), capi.SYMMETRIC, 0, 0, stream)
        ways["symv"] = lambda y: sym.symv(A[0].data_ptr(), A[1].data_ptr(), A[2].data_ptr(), tx.data_ptr(), y, stream)

    # one multiply each into y = 0: spmv_t against transposed, scaled by (|A'| |x|)_i
    ys = {}
    for k in ("spmv_t", "transposed"):
        y = torch.zeros(cols, dtype=torch.float64, device=dev)
        ways[k](y.data_ptr())
        torch.cuda.synchronize()
        ys[k] = y
    scale = torch.zeros(cols, dtype=torch.float64, device=dev).index_add_(
        0, A[1].long(), A[2].abs() * torch.repeat_interleave(tx.abs(), A[0][1:].long() - A[0][:-1].long()))
    diff = float(torch.max(torch.abs(ys["spmv_t"] - ys["transposed"]) / torch.clamp(scale, min=1e-300)).item()) if cols and nnz else 0.0
    del ys, scale

    y = torch.zeros(cols, dtype=torch.float64, device=dev)
    times = {k: [] for k in ways}
    for rnd in range(rounds + 1):  # round 0 warms up
        for k, run in ways.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                run(y.data_ptr())
            e1.record()
            torch.cuda.synchronize()
            if rnd > 0:
                times[k].append(e0.elapsed_time(e1) / reps * 1e3)
    info = tr.info()
    tinfo = tplan.info()
    res = {
        "matrix": name, "spec": spec, "rows": rows, "cols": cols, "stored_entries": nnz, "load_s": round(load_s, 1),
        "us": {k: {"median": round(float(np.median(t)), 2), "min": round(float(np.min(t)), 2)} for k, t in times.items()},
        "spmv_t_vs_transposed_max_scaled_diff": diff,
        "extra_device_bytes": {
            "spmv_t": info["device_bytes"],
            "transposed": 12 * nnz + 4 * (cols + 1) + tinfo["meta_bytes"] + (12 * nnz if tinfo["value_snapshot"] else 0),
        },
        "tr_plan": info,
        "atomic_us_at": {k: round(info["atomic_bytes"] / r / 1e6, 1) for k, r in ATOMIC_RATES_TBS.items()},
        "plan_s": {"spmv_t": round(tr_plan_s, 3), "transposed": round(tplan_s, 3)},
    }
    tr.close()
    tplan.close()
    if sym:
        sym.close()
    del A, B, tx, y
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", nargs="*", help="names among: " + ", ".join(m[0] for m in MATRICES))
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "transpose_ab.log"))
    args = ap.parse_args()
    import torch
    from spmv_amd import capi, synth

    log = open(args.log, "a")

    def say(text):
        print(text, flush=True)
        log.write(text + "\n")
        log.flush()

    say("spmv_t = spmv_hip_csr_spmv_t on A as stored; transposed = default CSR plan on A' (host-transposed, uploaded beside A); "
        "symv = spmv_hip_csr_symv on the same stored triangle (rounds %d, reps %d)" % (args.rounds, args.reps))
    for name, spec, what in MATRICES:
        if args.only and name not in args.only:
            continue
        r = measure(torch, capi, synth, name, spec, args.rounds, args.reps)
        us, i = r["us"], r["tr_plan"]
        say("%-14s %s: %d x %d, %d stored entries" % (name, what, r["rows"], r["cols"], r["stored_entries"]))
        for k in us:
            say("    %-10s median %9.2f us  min %9.2f us" % (k, us[k]["median"], us[k]["min"]))
        say("    spmv_t / transposed (median) %.3f;  max |spmv_t - transposed| / (|A'||x|)_i = %.2e" % (
            us["spmv_t"]["median"] / us["transposed"]["median"], r["spmv_t_vs_transposed_max_scaled_diff"]))
        if "symv" in us:
            say("    spmv_t / symv (median) %.3f  (the gate of tests/test_gpu_transpose.py: <= 1.10)" % (us["spmv_t"]["median"] / us["symv"]["median"]))
        say("    device bytes beside A: spmv_t %.6f GB, transposed %.3f GB;  plan time: spmv_t %.2f s, transposed %.2f s" % (
            r["extra_device_bytes"]["spmv_t"] / 1e9, r["extra_device_bytes"]["transposed"] / 1e9, r["plan_s"]["spmv_t"], r["plan_s"]["transposed"]))
        say("    plan: %d ranges of %d rows (most entries in one: %d), %d windows (%.2f per range), LDS %d B per workgroup, "
            "%d spilled entries (%.2f %%), atomic adds %.1f MB per multiply (window slots %.2f x cols): %.0f us at 1.3 TB/s, %.0f us at 0.92 TB/s" % (
                i["ranges"], i["rows_per_range"], i["most_entries_in_a_range"], i["windows"], i["windows"] / max(1, i["ranges"]), i["lds_bytes"],
                i["spilled_entries"], 100.0 * i["spilled_entries"] / max(1, i["stored_entries"]), i["atomic_bytes"] / 1e6,
                i["window_slots"] / max(1, i["cols"]), r["atomic_us_at"]["guide"], r["atomic_us_at"]["measured"]))
        say(json.dumps(r))
    log.close()


if __name__ == "__main__":
    main()
