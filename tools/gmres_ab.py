#!/usr/bin/env python3
"""The GMRES updates (include/spmv_hip_gmres.h) against what a caller had to do without them, at Level 2, in ONE process on one
stream, for double and float vectors:

  vectors alone (n = 2^22; at k = 16 the basis of doubles is 537 MB, beyond the Infinity Cache), torch events, no host read in
  either way:
    pair        spmv_hip_gmres_project_* + spmv_hip_gmres_update_*   against   h = torch.mv(V, w), w.addmv_(V.T, h, alpha=-1),
                                                                               torch.dot(w, w)            at k = 4, 8, 16, 32
    correct     spmv_hip_gmres_correct_* (no minv)                   against   x.addmv_(V.T, y)           at k = 16
    triad       a = b + s c over three vectors of the pair's size: the same-process bandwidth that each side's bytes are a share of

  one whole right-preconditioned GMRES(m) cycle through a C16Plan (c16_f64 for doubles, c16_f32xy for floats), minv = 1 / |diag|,
  wall clock around one cycle (m Arnoldi steps, the solve, the correction, the residual and the restart) with one synchronisation
  at the end:
    direct      the header's walk-through: enqueue-only calls, nothing read by the host
    graph       the same cycle captured once, replayed (reported only)
    composed    the scaled multiply, torch.mv / addmv_ twice, torch.dot(w, w).item() per step, the Hessenberg bookkeeping and the
                triangular solve on the host

on Poisson 4096^2 and on the webbase-like graph (the cycle is timed, not solved).  Three warm-up rounds, then --rounds rounds
alternating the ways, medians.  Everything is reported, nothing gated.  The log goes to stdout and to profiles/gmres_ab.log (--log).

    python tools/gmres_ab.py
    python tools/gmres_ab.py --only vectors poisson --rounds 25
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spmv-cache-trace_amd", "python"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from compact_ab import load  # noqa: E402
from scaled_ab import alternate  # noqa: E402

MATRICES = [
    ("poisson", "synthetic:poisson2d:4096", "5-point Poisson 4096^2 (134 MB per double vector)"),
    ("webbase", "synthetic:webbase", "webbase-1M-like graph, nonsymmetric (8 MB per double vector)"),
]
WARM = 3
KS = (4, 8, 16, 32)


def vectors(rounds):
    import torch
    from spmv_amd import capi
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    n = 2 ** 22
    out = {"n": n, "rounds": rounds, "library": os.path.basename(capi.LIB_PATH), "cases": {}}
    gen = torch.Generator(device=dev)
    gen.manual_seed(12)
    for dtype, name in ((torch.float64, "f64"), (torch.float32, "f32")):
        es = 8 if dtype == torch.float64 else 4
        basis = (torch.randn(max(KS), n, dtype=torch.float64, device=dev, generator=gen) * (1.0 / math.sqrt(n))).to(dtype)
        w, x = (torch.randn(n, dtype=torch.float64, device=dev, generator=gen).to(dtype) for _ in range(2))
        h = torch.zeros(max(KS) + 2, dtype=torch.float64, device=dev)
        y = (torch.randn(max(KS), dtype=torch.float64, device=dev, generator=gen) * 1e-3)
        dots = torch.zeros(2, dtype=torch.float64, device=dev)
        work = torch.zeros(capi.gmres_workspace_bytes(n, max(KS)) // 8, dtype=torch.float64, device=dev)
        for k in KS:
            V = basis[:k]
            got = {}

            def torch_pair():
                got["h"] = torch.mv(V, w)
                w.addmv_(V.T, got["h"], alpha=-1.0)
                got["ww"] = torch.dot(w, w)

            def fused_pair():
                capi.gmres_project(n, k, V, n, w, h, work, None, s)
                capi.gmres_update(n, k, V, n, h, w, dots, work, None, s)

            # a = b + s c over three arrays of (2 k + 3) n / 3 elements: a triad moving what the fused pair moves
            ta, tb, tc = (torch.zeros((2 * k + 3) * n // 3, dtype=dtype, device=dev) for _ in range(3))

            def triad():
                torch.add(tb, tc, alpha=0.5, out=ta)

            med = alternate(torch, {"torch": torch_pair, "fused": fused_pair, "triad": triad}, rounds)
            triad_bw = 3 * ta.numel() * es / med["triad"]  # bytes per us
            fused_bytes, torch_bytes = (2 * k + 3) * n * es, (2 * k + 4) * n * es
            case = {"pair_us": {key: round(u, 2) for key, u in med.items()}, "ratio": round(med["fused"] / med["torch"], 3),
                    "ratio_by_bytes": round(fused_bytes / torch_bytes, 3), "triad_GBps": round(triad_bw / 1e3, 1),
                    "fused_share_of_triad_bandwidth": round(fused_bytes / med["fused"] / triad_bw, 3),
                    "torch_share_of_triad_bandwidth": round(torch_bytes / med["torch"] / triad_bw, 3)}
            if k == 16:
                yk = y[:k].to(dtype)

                def torch_correct():
                    x.addmv_(V.T, yk)

                def fused_correct():
                    capi.gmres_correct(n, k, V, n, y, None, x, s)

                medc = alternate(torch, {"torch": torch_correct, "fused": fused_correct}, rounds)
                case["correct_us"] = {key: round(u, 2) for key, u in medc.items()}
                case["correct_ratio"] = round(medc["fused"] / medc["torch"], 3)
            out["cases"]["%s_k%d" % (name, k)] = case
            del ta, tb, tc
        del basis, w, x, work
        torch.cuda.empty_cache()
    return out


def cycle(name, spec, rounds, m):
    import torch
    from spmv_amd import capi
    dev = torch.device("cuda:0")
    rows, cols, p_h, c_h, v_h = load(spec)
    assert rows == cols
    nnz = int(p_h[-1])
    row = np.repeat(np.arange(rows), np.diff(p_h))
    diag = np.zeros(rows)
    diag[row[c_h == row]] = np.abs(v_h[c_h == row])
    minv_h = np.where(diag > 0, 1.0 / np.where(diag > 0, diag, 1.0), 1.0)
    b_h = np.random.default_rng(4).uniform(-1.0, 1.0, size=rows)
    side = torch.cuda.Stream()
    res = {"matrix": name, "spec": spec, "rows": rows, "stored_entries": nnz, "rounds": rounds, "m": m,
           "library": os.path.basename(capi.LIB_PATH), "families": {}}
    with torch.cuda.stream(side):
        s = side.cuda_stream
        tp, tc, tv = (torch.from_numpy(a).to(dev) for a in (p_h, c_h, v_h))
        tf = torch.zeros(max(1, nnz), dtype=torch.float32, device=dev)
        capi.narrow_values(nnz, tv.data_ptr(), tf.data_ptr(), s)
        plan = capi.C16Plan(rows, cols, p_h, c_h, 0, s)
        P, C = tp.data_ptr(), tc.data_ptr()
        for fam, dtype, vals, scaled, fused in (("c16_f64", torch.float64, tv, plan.spmv_f64_scaled, plan.spmv_f64_scaled_dots),
                                                ("c16_f32xy", torch.float32, tf, plan.spmv_f32xy_scaled, plan.spmv_f32xy_scaled_dots)):
            es = 8 if dtype == torch.float64 else 4
            n = rows
            ldv = (n + 16 // es - 1) // (16 // es) * (16 // es)
            b, minv = torch.from_numpy(b_h).to(dev).to(dtype), torch.from_numpy(minv_h).to(dev).to(dtype)
            basis = torch.zeros(m + 1, ldv, dtype=dtype, device=dev)
            x, vhat = (torch.zeros(n, dtype=dtype, device=dev) for _ in range(2))
            h1, h2 = (torch.zeros(m + 2, dtype=torch.float64, device=dev) for _ in range(2))
            dots, rr, md = (torch.zeros(2, dtype=torch.float64, device=dev) for _ in range(3))
            yd = torch.zeros(m + m % 2, dtype=torch.float64, device=dev)
            state = torch.zeros(capi.gmres_state_doubles(m), dtype=torch.float64, device=dev)
            mbytes, gbytes = plan.dots_workspace_bytes(), capi.gmres_workspace_bytes(n, m)
            mwork = torch.zeros(mbytes // 8, dtype=torch.float64, device=dev)
            gwork = torch.zeros(gbytes // 8, dtype=torch.float64, device=dev)
            A, B = vals.data_ptr(), basis.data_ptr()
            vec = lambda j: B + j * ldv * es
            dt = np.float64 if es == 8 else np.float32

            def restart():
                fused(P, C, A, x.data_ptr(), -1.0, 1.0, b.data_ptr(), vec(0), None, rr.data_ptr(), mwork.data_ptr(), mbytes, s)
                capi.gmres_start(m, rr, state, s)
                capi.gmres_scale(n, state.data_ptr() + 8, vec(0), minv, vhat, s, dtype=dt)

            def begin():
                x.zero_()
                restart()

            def direct():
                for k in range(m):
                    wv = vec(k + 1)
                    fused(P, C, A, vhat.data_ptr(), 1.0, 0.0, None, wv, None, md.data_ptr(), mwork.data_ptr(), mbytes, s)
                    capi.gmres_project(n, k + 1, B, ldv, wv, h1, gwork, gbytes, s, dtype=dt)
                    capi.gmres_update(n, k + 1, B, ldv, h1, wv, dots, gwork, gbytes, s, dtype=dt)
                    capi.gmres_project(n, k + 1, B, ldv, wv, h2, gwork, gbytes, s, dtype=dt)
                    capi.gmres_update(n, k + 1, B, ldv, h2, wv, dots, gwork, gbytes, s, dtype=dt)
                    capi.gmres_column(k, m, h1, h2, dots, state, s)
                    capi.gmres_scale(n, state.data_ptr() + 8, wv, minv, vhat, s, dtype=dt)
                capi.gmres_solve(m, m, state, yd, s)
                capi.gmres_correct(n, m, B, ldv, yd, minv, x, s, dtype=dt)
                restart()

            begin()
            direct()
            side.synchronize()
            final, first = float(rr[0]), float(torch.dot(b.double(), b.double()))
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                direct()

            def composed():
                beta = math.sqrt(float(rr[0]))  # the host read a caller has made before the cycle
                H, gv = np.zeros((m + 1, m)), np.zeros(m + 1)
                gv[0] = beta
                cs, sn = np.zeros(m), np.zeros(m)
                for k in range(m):
                    w = basis[k + 1, :n]
                    Vk = basis[:k + 1, :n]
                    scaled(P, C, A, vhat.data_ptr(), 1.0, 0.0, None, w.data_ptr(), s)
                    ha = torch.mv(Vk, w)
                    w.addmv_(Vk.T, ha, alpha=-1.0)
                    hb = torch.mv(Vk, w)
                    w.addmv_(Vk.T, hb, alpha=-1.0)
                    nrm = math.sqrt(max(torch.dot(w, w).item(), 1e-300))
                    col = (ha + hb).double().cpu().numpy()  # the second host read of the step
                    H[:k + 1, k], H[k + 1, k] = col, nrm
                    for i in range(k):
                        H[i, k], H[i + 1, k] = cs[i] * H[i, k] + sn[i] * H[i + 1, k], cs[i] * H[i + 1, k] - sn[i] * H[i, k]
                    d = math.hypot(H[k, k], nrm)
                    cs[k], sn[k] = H[k, k] / d, nrm / d
                    H[k, k] = d
                    gv[k + 1], gv[k] = -sn[k] * gv[k], cs[k] * gv[k]
                    w.mul_(1.0 / nrm)
                    torch.mul(minv, w, out=vhat)
                try:
                    yh = np.linalg.solve(np.triu(H[:m, :m]), gv[:m])
                except np.linalg.LinAlgError:  # a breakdown on a matrix the cycle is only timed on
                    yh = np.zeros(m)
                u = torch.mv(basis[:m, :n].T, torch.from_numpy(yh).to(dev).to(dtype))
                x.addcmul_(minv, u)
                scaled(P, C, A, x.data_ptr(), -1.0, 1.0, b.data_ptr(), vec(0), s)
                r0 = basis[0, :n]
                r0.mul_(1.0 / math.sqrt(max(torch.dot(r0, r0).item(), 1e-300)))
                torch.mul(minv, r0, out=vhat)

            ways = {"direct": direct, "graph": g.replay, "composed": composed}
            times = {k: [] for k in ways}
            for rnd in range(WARM + rounds):
                for k, run in ways.items():
                    begin()
                    side.synchronize()
                    t0 = time.perf_counter()
                    run()
                    side.synchronize()
                    if rnd >= WARM:
                        times[k].append((time.perf_counter() - t0) * 1e6)
            med = {k: float(np.median(u)) for k, u in times.items()}
            res["families"][fam] = {"per_cycle_us": {k: round(u, 1) for k, u in med.items()},
                                    "direct_over_composed": round(med["direct"] / med["composed"], 3),
                                    "graph_over_composed": round(med["graph"] / med["composed"], 3),
                                    "rr_after_one_cycle_over_rr_of_r0": final / first}
            del g, basis
            torch.cuda.empty_cache()
        plan.close()
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--m", type=int, default=30, help="Arnoldi steps of a cycle")
    ap.add_argument("--only", nargs="*", help="names among: vectors, " + ", ".join(m[0] for m in MATRICES))
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "gmres_ab.log"))
    args = ap.parse_args()
    log = open(args.log, "w")  # a run replaces the log

    def say(text):
        print(text, flush=True)
        log.write(text + "\n")
        log.flush()

    if not args.only or "vectors" in args.only:
        say("project + update against torch.mv + addmv_ + dot, and correct against addmv_; one process, torch events on one stream, "
            "3 warm-up rounds, then %d rounds alternating the ways, medians" % args.rounds)
        res = vectors(args.rounds)
        for k, c in res["cases"].items():
            u = c["pair_us"]
            say("    n %d %-7s pair: torch %8.2f us, fused %8.2f us, ratio %.3f (by bytes %.3f); triad %.1f GB/s, of which fused %.3f, "
                "torch %.3f%s" % (res["n"], k, u["torch"], u["fused"], c["ratio"], c["ratio_by_bytes"], c["triad_GBps"],
                                  c["fused_share_of_triad_bandwidth"], c["torch_share_of_triad_bandwidth"],
                                  ";   correct: torch %8.2f us, fused %8.2f us, ratio %.3f" % (
                                      c["correct_us"]["torch"], c["correct_us"]["fused"], c["correct_ratio"]) if "correct_us" in c else ""))
        say(json.dumps(res))
    first = True
    for name, spec, what in MATRICES:
        if args.only and name not in args.only:
            continue
        if first:
            say("one right-preconditioned GMRES(%d) cycle: enqueue-only calls direct, the cycle captured and replayed, and composed from "
                "the scaled multiply, torch ops and host reads; wall clock per cycle, 3 warm-up rounds, then %d rounds alternating the "
                "ways, medians" % (args.m, args.rounds))
            first = False
        res = cycle(name, spec, args.rounds, args.m)
        say("%-14s %s: %d rows, %d stored entries; %s" % (name, what, res["rows"], res["stored_entries"], res["library"]))
        for k, f in res["families"].items():
            u = f["per_cycle_us"]
            say("    %-9s direct %10.1f us, graph %10.1f us, composed %10.1f us per cycle; direct / composed %.3f, graph / composed %.3f; "
                "r'r after one cycle over that of r0 %.3e" % (k, u["direct"], u["graph"], u["composed"], f["direct_over_composed"],
                                                              f["graph_over_composed"], f["rr_after_one_cycle_over_rr_of_r0"]))
        say(json.dumps(res))
    log.close()


if __name__ == "__main__":
    main()
