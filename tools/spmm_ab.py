#!/usr/bin/env python3
"""Y += A X for k vectors in one multiply (include/spmv_hip_multivec.h) against k single-vector multiplies, one process, torch
tensors, interleaved rounds after a warm-up:

    spmm     one spmv_hip_csr_spmm with X (cols, k) and Y (rows, k) row-major: every stored entry read once per pass
    single   k back-to-back spmv_hip_csr_spmv calls of the default plan (what spmv_hip_upload_csr builds) on the same columns

Per matrix and k in 1, 2, 4, 8, 16: microseconds per multiply and per vector (median and min over the rounds, each round the
mean of --reps back-to-back launches), the share of the box's STREAM triad (timed in this process) that the bytes model
B(k) = passes (12 nnz + 4 (rows + 1)) + 8 k cols + 16 k rows reaches at the spmm time, and the largest difference of the two
results scaled by (|A| |x_c|)_i.

    python tools/spmm_ab.py                          # queen, kkt, Delaunay RCM, Poisson 4096^2, webbase
    python tools/spmm_ab.py --only queen --ks 4 8 --rounds 9
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
    ("queen", "synthetic:queen", "Queen_4147-like, expanded (full size)"),
    ("kkt", "synthetic:kkt:200", "nlpkkt200-like, expanded"),
    ("delaunay_rcm", "delaunay:250000,3,1,rcm", "Delaunay 3-D mesh, 3 unknowns per node, RCM order"),
    ("poisson", "synthetic:poisson2d:4096", "5-point Poisson 4096^2"),
    ("webbase", "synthetic:webbase", "webbase-1M-like graph"),
]


def load(spec):
    from spmv_amd import hostapi, synth
    if spec.startswith("delaunay:"):
        q = spec[9:].split(",")
        rows, cols, p, c, v = synth.delaunay_mesh(int(q[0]), int(q[1]), seed=int(q[2]), order=q[3])
        return rows, cols, np.asarray(p, dtype=np.int32), np.asarray(c, dtype=np.int32), np.asarray(v, dtype=np.float64)
    H = hostapi.load(spec, "csr")
    out = (H.rows, H.cols, np.array(H.row_ptr, dtype=np.int32), np.array(H.column_index, dtype=np.int32), np.array(H.value))
    H.close()
    return out


def default_plan(capi, rows, cols, host_p, tp, tc, tv, stream):
    """The plan spmv_hip_upload_csr builds (context.hip): tiles, block confirmation, compression, panels, value dictionary."""
    plan = capi.CsrPlan(rows, cols, host_p, capi.CSR_AUTO, 0, 0)
    plan.confirm_blocks(tp.data_ptr(), tc.data_ptr(), host_p, stream)
    plan.compress(tc.data_ptr(), stream)
    plan.repack(tp.data_ptr(), tc.data_ptr(), tv.data_ptr(), stream)
    plan.index_values(tv.data_ptr(), stream)
    return plan


def triad_gbs(torch, capi, dev, stream):
    nt = 64 * 1024 * 1024
    ta = torch.zeros(nt, dtype=torch.float64, device=dev)
    tb = torch.ones(nt, dtype=torch.float64, device=dev)
    tc = torch.ones(nt, dtype=torch.float64, device=dev)
    for _ in range(3):
        capi.triad(nt, ta.data_ptr(), tb.data_ptr(), tc.data_ptr(), 3.1, stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        capi.triad(nt, ta.data_ptr(), tb.data_ptr(), tc.data_ptr(), 3.1, stream)
    e1.record()
    torch.cuda.synchronize()
    return 24.0 * nt * 20 / (e0.elapsed_time(e1) * 1e-3) / 1e9


def measure(torch, capi, synth, name, spec, ks, rounds, reps, triad):
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    t0 = time.time()
    rows, cols, p, c, v = load(spec)
    load_s = time.time() - t0
    nnz = int(p[-1])
    A = [torch.from_numpy(a).to(dev) for a in (p, c, v)]
    single = default_plan(capi, rows, cols, p, *A, stream)
    arow = torch.repeat_interleave(torch.arange(rows, device=dev), A[0][1:].long() - A[0][:-1].long())
    x = torch.from_numpy(synth.x_vector(cols, "uniform", seed=12345)).to(dev)
    out = []
    for k in ks:
        X = (x[:, None] * (torch.arange(k, device=dev, dtype=torch.float64)[None, :] + 1.0)).contiguous()  # (cols, k)
        Xc = X.t().contiguous()                                                                          # (k, cols): k vectors
        Y = torch.zeros(rows, k, dtype=torch.float64, device=dev)
        Yc = torch.zeros(k, rows, dtype=torch.float64, device=dev)
        mv = capi.MvPlan(rows, cols, p, k, 0, stream)
        ways = {
            "spmm": lambda: mv.spmm(A[0].data_ptr(), A[1].data_ptr(), A[2].data_ptr(), X, Y, stream=stream),
            "single": lambda: [single.spmv(A[0].data_ptr(), A[1].data_ptr(), A[2].data_ptr(), Xc[q].data_ptr(), Yc[q].data_ptr(), stream)
                               for q in range(k)],
        }
        for run in ways.values():  # one multiply each into zero: the scaled difference
            run()
        torch.cuda.synchronize()
        diff = 0.0
        for q in range(k):
            scale = torch.zeros(rows, dtype=torch.float64, device=dev).index_add_(0, arow, A[2].abs() * Xc[q][A[1].long()].abs())
            diff = max(diff, float(torch.max(torch.abs(Y[:, q] - Yc[q]) / torch.clamp(scale, min=1e-300)).item()))
            del scale
        times = {w: [] for w in ways}
        for rnd in range(rounds + 1):  # round 0 warms up
            for w, run in ways.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    run()
                e1.record()
                torch.cuda.synchronize()
                if rnd > 0:
                    times[w].append(e0.elapsed_time(e1) / reps * 1e3)
        info = mv.info()
        med = {w: float(np.median(t)) for w, t in times.items()}
        r = {
            "matrix": name, "k": k, "rows": rows, "cols": cols, "entries": nnz,
            "us": {w: {"median": round(med[w], 2), "min": round(float(np.min(t)), 2)} for w, t in times.items()},
            "us_per_vector": {w: round(med[w] / k, 2) for w in ways},
            "spmm_over_one_single": round(med["spmm"] / (med["single"] / k), 3),
            "spmm_over_k_single": round(med["spmm"] / med["single"], 3),
            "bytes_model": info["streamed_bytes"], "passes": info["passes"], "tiles": info["tiles"], "long_rows": info["long_rows"],
            "spmm_share_of_triad": round(info["streamed_bytes"] / (med["spmm"] * 1e-6) / 1e9 / triad, 3) if triad else None,
            "max_scaled_diff": diff,
        }
        out.append(r)
        mv.close()
        del X, Xc, Y, Yc
    single.close()
    del A, arow, x
    torch.cuda.empty_cache()
    return out, load_s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ks", type=int, nargs="*", default=[1, 2, 4, 8, 16])
    ap.add_argument("--only", nargs="*", help="names among: " + ", ".join(m[0] for m in MATRICES))
    args = ap.parse_args()
    import torch
    from spmv_amd import capi, synth

    dev = torch.device("cuda:0")
    triad = triad_gbs(torch, capi, dev, torch.cuda.current_stream().cuda_stream)
    print("spmm = one spmv_hip_csr_spmm for k vectors; single = k default-plan spmv_hip_csr_spmv calls; triad %.0f GB/s" % triad)
    for name, spec, what in MATRICES:
        if args.only and name not in args.only:
            continue
        res, load_s = measure(torch, capi, synth, name, spec, args.ks, args.rounds, args.reps, triad)
        r0 = res[0]
        print("%-13s %s: rows %d, cols %d, entries %d (loaded in %.0f s)" % (name, what, r0["rows"], r0["cols"], r0["entries"], load_s))
        for r in res:
            us, pv = r["us"], r["us_per_vector"]
            print("    k=%-2d spmm %9.1f us (%8.1f per vector, %d pass%s, %.2f of triad)   single x k %9.1f us (%8.1f per vector)   "
                  "spmm / one single %.2f   max diff %.1e" % (
                      r["k"], us["spmm"]["median"], pv["spmm"], r["passes"], "" if r["passes"] == 1 else "es", r["spmm_share_of_triad"],
                      us["single"]["median"], pv["single"], r["spmm_over_one_single"], r["max_scaled_diff"]))
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
