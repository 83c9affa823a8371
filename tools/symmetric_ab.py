#!/usr/bin/env python3
"""Symmetric multiply of a stored triangle against the two ways the project had before (include/spmv_hip_symmetric.h), one
process, torch tensors, interleaved rounds after a warm-up:

    sym       spmv_hip_csr_symv on the stored triangle T: y += (T + T' - D) x, every stored value read once
    expanded  the default CSR plan (what spmv_hip_upload_csr builds) on E = T + T' - D, mirrored on the host
    stored    the default CSR plan on T as if it were general: y += T x (the reference's semantics; not the matrix's product)

Per matrix: microseconds per multiply (median and min over the rounds, each round the mean of --reps back-to-back launches),
the largest difference of sym against expanded scaled by (|E| |x|)_i, the device bytes of the matrix + plan of sym and of
expanded, the symmetric plan's info, and how long each plan took to build.

    python tools/symmetric_ab.py                       # queen, kkt, Delaunay RCM / random, Poisson 4096^2
    python tools/symmetric_ab.py --only queen --rounds 9
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
    ("queen", "synthetic:queen:tril", "Queen_4147-like stored triangle, 3-D mesh in natural order (full size)"),
    ("kkt", "synthetic:kkt:200:tril", "nlpkkt200-like stored triangle"),
    ("delaunay_rcm", "delaunay:250000,3,1,rcm", "Delaunay 3-D mesh, 3 unknowns per node, RCM order"),
    ("delaunay_random", "delaunay:250000,3,1,random", "the same mesh, points in random order"),
    ("poisson", "synthetic:poisson2d:4096:tril", "5-point Poisson 4096^2, stored triangle"),
]


def load_pair(spec):
    """(rows, T arrays, E arrays): the stored triangle and its expansion T + T' - D, CSR with ascending columns."""
    from spmv_amd import hostapi, synth
    if spec.startswith("delaunay:"):
        import scipy.sparse as sp
        q = spec[9:].split(",")
        rows, _, p, c, v = synth.delaunay_mesh(int(q[0]), int(q[1]), seed=int(q[2]), order=q[3])
        A = sp.csr_matrix((v, c, p), shape=(rows, rows))
        T = sp.tril(A, format="csr")
        E = (T + T.T - sp.diags(T.diagonal())).tocsr()
        out = []
        for M in (T, E):
            M.sort_indices()
            out.append((M.indptr.astype(np.int32), M.indices.astype(np.int32), M.data.astype(np.float64)))
        return rows, out[0], out[1]
    arrays = []
    for expand in (False, True):
        H = hostapi.load(spec, "csr", expand_symmetric=expand)
        rows = H.rows
        arrays.append((np.array(H.row_ptr), np.array(H.column_index), np.array(H.value)))
        H.close()
    return rows, arrays[0], arrays[1]


def default_plan(capi, rows, host_p, tp, tc, tv, stream):
    """The plan spmv_hip_upload_csr builds (context.hip): tiles, block confirmation, compression, panels, value dictionary."""
    plan = capi.CsrPlan(rows, rows, host_p, capi.CSR_AUTO, 0, 0)
    plan.confirm_blocks(tp.data_ptr(), tc.data_ptr(), host_p, stream)
    plan.compress(tc.data_ptr(), stream)
    plan.repack(tp.data_ptr(), tc.data_ptr(), tv.data_ptr(), stream)
    plan.index_values(tv.data_ptr(), stream)
    return plan


def measure(torch, capi, synth, name, spec, rounds, reps):
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    t0 = time.time()
    rows, (tp_h, tc_h, tv_h), (ep_h, ec_h, ev_h) = load_pair(spec)
    load_s = time.time() - t0
    nnz_t, nnz_e = int(tp_h[-1]), int(ep_h[-1])
    T = [torch.from_numpy(a).to(dev) for a in (tp_h, tc_h, tv_h)]
    E = [torch.from_numpy(a).to(dev) for a in (ep_h, ec_h, ev_h)]
    tx = torch.from_numpy(synth.x_vector(rows, "uniform", seed=12345)).to(dev)
    torch.cuda.synchronize()

    t0 = time.time()
    sym = capi.SymPlan(rows, tp_h, T[1].data_ptr(), capi.SYMMETRIC, 0, 0, stream)
    sym_plan_s = time.time() - t0
    t0 = time.time()
    exp_plan = default_plan(capi, rows, ep_h, *E, stream)
    torch.cuda.synchronize()
    exp_plan_s = time.time() - t0
    t0 = time.time()
    sto_plan = default_plan(capi, rows, tp_h, *T, stream)
    torch.cuda.synchronize()
    sto_plan_s = time.time() - t0

    ways = {
        "sym": lambda y: sym.symv(T[0].data_ptr(), T[1].data_ptr(), T[2].data_ptr(), tx.data_ptr(), y, stream),
        "expanded": lambda y: exp_plan.spmv(E[0].data_ptr(), E[1].data_ptr(), E[2].data_ptr(), tx.data_ptr(), y, stream),
        "stored": lambda y: sto_plan.spmv(T[0].data_ptr(), T[1].data_ptr(), T[2].data_ptr(), tx.data_ptr(), y, stream),
    }
    # one multiply each into y = 0: sym against expanded, scaled by (|E| |x|)_i
    ys = {}
    for k in ("sym", "expanded"):
        y = torch.zeros(rows, dtype=torch.float64, device=dev)
        ways[k](y.data_ptr())
        torch.cuda.synchronize()
        ys[k] = y
    erow = torch.repeat_interleave(torch.arange(rows, device=dev), E[0][1:].long() - E[0][:-1].long())
    scale = torch.zeros(rows, dtype=torch.float64, device=dev).index_add_(0, erow, E[2].abs() * tx[E[1].long()].abs())
    del erow
    diff = float(torch.max(torch.abs(ys["sym"] - ys["expanded"]) / torch.clamp(scale, min=1e-300)).item()) if rows else 0.0
    del ys, scale

    y = torch.zeros(rows, dtype=torch.float64, device=dev)
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
    info = sym.info()
    einfo = exp_plan.info()
    res = {
        "matrix": name, "spec": spec, "rows": rows, "stored_entries": nnz_t, "expanded_entries": nnz_e, "load_s": round(load_s, 1),
        "us": {k: {"median": round(float(np.median(t)), 2), "min": round(float(np.min(t)), 2)} for k, t in times.items()},
        "sym_vs_expanded_max_scaled_diff": diff,
        "device_bytes": {
            "sym": 12 * nnz_t + 4 * (rows + 1) + info["device_bytes"],
            "expanded": 12 * nnz_e + 4 * (rows + 1) + einfo["meta_bytes"] + (12 * nnz_e if einfo["value_snapshot"] else 0),
        },
        "sym_plan": info,
        "plan_s": {"sym": round(sym_plan_s, 3), "expanded": round(exp_plan_s, 3), "stored": round(sto_plan_s, 3)},
    }
    sym.close()
    exp_plan.close()
    sto_plan.close()
    del T, E, tx, y
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", nargs="*", help="names among: " + ", ".join(m[0] for m in MATRICES))
    args = ap.parse_args()
    import torch
    from spmv_amd import capi, synth

    print("sym = spmv_hip_csr_symv on the stored triangle; expanded = default CSR plan on T + T' - D; stored = default plan on T alone")
    results = []
    for name, spec, what in MATRICES:
        if args.only and name not in args.only:
            continue
        r = measure(torch, capi, synth, name, spec, args.rounds, args.reps)
        results.append(r)
        us, i = r["us"], r["sym_plan"]
        print("%-16s %s: rows %d, stored %d, expanded %d" % (name, what, r["rows"], r["stored_entries"], r["expanded_entries"]))
        for k in ("sym", "expanded", "stored"):
            print("    %-9s median %9.2f us  min %9.2f us" % (k, us[k]["median"], us[k]["min"]))
        print("    sym / expanded (median) %.3f;  max |sym - expanded| / (|E||x|)_i = %.2e" % (
            us["sym"]["median"] / us["expanded"]["median"], r["sym_vs_expanded_max_scaled_diff"]))
        print("    device bytes: sym %.3f GB, expanded %.3f GB;  plan time: sym %.2f s, expanded %.2f s, stored %.2f s" % (
            r["device_bytes"]["sym"] / 1e9, r["device_bytes"]["expanded"] / 1e9, r["plan_s"]["sym"], r["plan_s"]["expanded"], r["plan_s"]["stored"]))
        print("    sym plan: %d ranges of %d rows, %d windows (%.2f per range), LDS %d B per workgroup, %d spilled entries (%.2f %%), "
              "atomic adds %.1f MB per multiply (window slots %.2f x rows)" % (
                  i["ranges"], i["rows_per_range"], i["windows"], i["windows"] / max(1, i["ranges"]), i["lds_bytes"], i["spilled_entries"],
                  100.0 * i["spilled_entries"] / max(1, i["stored_entries"]), i["atomic_bytes"] / 1e6, i["window_slots"] / max(1, i["rows"])))
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
