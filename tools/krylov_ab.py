#!/usr/bin/env python3
"""The conjugate-gradient updates (include/spmv_hip_krylov.h) against what a caller had to do without them, at Level 2, in ONE
process on one stream, for double and float vectors:

  vectors alone (n = 4096^2: four vectors beyond the Infinity Cache), torch events, with and without minv:
    step        spmv_hip_cg_step_*        against   a = num / den (0-dim), x.addcmul_(p, a), r.addcmul_(q, a, value=-1), torch.dot(r, r)
                                                    [with minv: and z = minv * r, torch.dot(r, z)]           -- no host read in either
    direction   spmv_hip_cg_direction_*   against   b = num / den (0-dim), torch.addcmul(r, p, b, out=p)     [with minv: z = minv * r first]

  one whole preconditioned iteration through a C16Plan (c16_f64 for doubles, c16_f32xy for floats), minv = 1 / |diag|, wall clock
  around --iterations iterations from x0 = 0 with one synchronisation at the end:
    direct      *_scaled_dots(1, 0, w = p), cg_step, cg_direction: three enqueue-only calls, nothing read by the host
    graph       two such iterations captured once, replayed
    composed    the scaled multiply, torch.dot(p, q).item(), x.add_, r.add_, z = minv * r, torch.dot(r, z).item(), p = z + b p

on Poisson 4096^2 and on two matrices whose vectors fit the cache (those two are not positive definite: the iteration is timed on
them, not solved -- r'r grows, which costs the same time).  Three warm-up rounds, then --rounds rounds alternating the
ways, medians.  Everything is reported, nothing gated.  The log goes to stdout and to profiles/krylov_ab.log (--log).

    python tools/krylov_ab.py
    python tools/krylov_ab.py --only vectors poisson --rounds 25
"""
import argparse
import json
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
    ("delaunay_3dof", "delaunay:250000,3,1,rcm", "Delaunay 3-D mesh, 3 unknowns per node, RCM order (6 MB per double vector)"),
    ("mesh_128", "mesh_dofs:128,1", "27-neighbour mesh 128^3 with jittered links, scalar (17 MB per double vector)"),
]
WARM = 3


def vectors(rounds):
    import torch
    from spmv_amd import capi
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    n = 4096 * 4096
    out = {"n": n, "rounds": rounds, "library": os.path.basename(capi.LIB_PATH), "cases": {}}
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    for dtype, name in ((torch.float64, "f64"), (torch.float32, "f32")):
        es = 8 if dtype == torch.float64 else 4
        p, q, x, r = ((torch.rand(n, dtype=torch.float64, device=dev, generator=gen) * 2 - 1).to(dtype) for _ in range(4))
        minv = (torch.rand(n, dtype=torch.float64, device=dev, generator=gen) * 1.5 + 0.5).to(dtype)
        nd = torch.tensor([1e-3, 1.0], dtype=torch.float64, device=dev)
        num, den = nd[0], nd[1]
        dots = torch.zeros(2, dtype=torch.float64, device=dev)
        work = torch.zeros(capi.krylov_workspace_bytes(n) // 8, dtype=torch.float64, device=dev)
        for with_minv in (False, True):
            m = minv if with_minv else None
            got = {}

            def torch_step():
                a = (num / den).to(dtype)
                x.addcmul_(p, a)
                r.addcmul_(q, a, value=-1.0)
                got["rr"] = torch.dot(r, r)
                if with_minv:
                    got["rz"] = torch.dot(r, minv * r)

            def fused_step():
                capi.cg_step(n, nd.data_ptr(), nd.data_ptr() + 8, p, q, x, r, m, dots, work, None, s)

            def torch_direction():
                b = (num / den).to(dtype)
                torch.addcmul(minv * r if with_minv else r, p, b, out=p)

            def fused_direction():
                capi.cg_direction(n, nd.data_ptr(), nd.data_ptr() + 8, r, m, p, s)

            fused_step()
            ref = float(torch.dot(r.double(), r.double()))
            rel = abs(float(dots[0]) - ref) / ref
            st = alternate(torch, {"torch": torch_step, "fused": fused_step}, rounds)
            di = alternate(torch, {"torch": torch_direction, "fused": fused_direction}, rounds)
            # bytes per element: the step reads p, q, x, r (and minv) and writes x, r; torch reads r once more (and r and minv
            # for z, writes z, reads r and z); the direction reads r, p (and minv) and writes p; torch writes and reads z as well
            step_bytes = ((6 + with_minv) * es, (7 + 5 * with_minv) * es)
            dir_bytes = ((3 + with_minv) * es, (3 + 3 * with_minv) * es)
            out["cases"]["%s%s" % (name, "_minv" if with_minv else "")] = {
                "step_us": {k: round(v, 2) for k, v in st.items()}, "step_ratio": round(st["fused"] / st["torch"], 3),
                "step_ratio_by_bytes": round(step_bytes[0] / step_bytes[1], 3),
                "direction_us": {k: round(v, 2) for k, v in di.items()}, "direction_ratio": round(di["fused"] / di["torch"], 3),
                "direction_ratio_by_bytes": round(dir_bytes[0] / dir_bytes[1], 3), "dot_relative_difference_to_torch": rel}
        del p, q, x, r, minv, dots, work
        torch.cuda.empty_cache()
    return out


def iteration(name, spec, rounds, iterations):
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
    res = {"matrix": name, "spec": spec, "rows": rows, "stored_entries": nnz, "rounds": rounds, "iterations": iterations,
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
            b, minv = torch.from_numpy(b_h).to(dev).to(dtype), torch.from_numpy(minv_h).to(dev).to(dtype)
            x, r, p, q = (torch.zeros(rows, dtype=dtype, device=dev) for _ in range(4))
            start = torch.tensor([0.0, 1.0], dtype=torch.float64, device=dev)
            rz = [torch.zeros(2, dtype=torch.float64, device=dev) for _ in range(2)]
            pq = torch.zeros(2, dtype=torch.float64, device=dev)
            mbytes, kbytes = plan.dots_workspace_bytes(), capi.krylov_workspace_bytes(rows)
            mwork = torch.zeros(mbytes // 8, dtype=torch.float64, device=dev)
            kwork = torch.zeros(kbytes // 8, dtype=torch.float64, device=dev)
            A = vals.data_ptr()

            def begin():
                x.zero_()
                r.copy_(b)
                p.zero_()
                q.zero_()
                capi.cg_step(rows, start.data_ptr(), start.data_ptr() + 8, p, q, x, r, minv, rz[0], kwork, kbytes, s)
                capi.cg_direction(rows, start.data_ptr(), start.data_ptr() + 8, r, minv, p, s)

            def one(it):
                old, new = rz[it % 2], rz[1 - it % 2]
                fused(P, C, A, p.data_ptr(), 1.0, 0.0, None, q.data_ptr(), p.data_ptr(), pq.data_ptr(), mwork.data_ptr(), mbytes, s)
                capi.cg_step(rows, old.data_ptr() + 8, pq.data_ptr() + 8, p, q, x, r, minv, new, kwork, kbytes, s)
                capi.cg_direction(rows, new.data_ptr() + 8, old.data_ptr() + 8, r, minv, p, s)

            def direct():
                for it in range(iterations):
                    one(it)

            begin()
            direct()
            side.synchronize()
            final = float(rz[iterations % 2][0])
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                one(0)
                one(1)

            def graph():
                for _ in range(iterations // 2):
                    g.replay()

            def composed():
                rz_old = float(rz[0][1])  # the host read a caller has made before the loop
                for _ in range(iterations):
                    scaled(P, C, A, p.data_ptr(), 1.0, 0.0, None, q.data_ptr(), s)
                    a = rz_old / torch.dot(p, q).item()
                    x.add_(p, alpha=a)
                    r.add_(q, alpha=-a)
                    z = minv * r
                    rz_new = torch.dot(r, z).item()
                    p.mul_(rz_new / rz_old).add_(z)
                    rz_old = rz_new

            ways = {"direct": direct, "graph": graph, "composed": composed}
            times = {k: [] for k in ways}
            for rnd in range(WARM + rounds):
                for k, run in ways.items():
                    begin()
                    side.synchronize()
                    t0 = time.perf_counter()
                    run()
                    side.synchronize()
                    if rnd >= WARM:
                        times[k].append((time.perf_counter() - t0) * 1e6 / iterations)
            med = {k: float(np.median(t)) for k, t in times.items()}
            res["families"][fam] = {"per_iteration_us": {k: round(v, 2) for k, v in med.items()},
                                    "direct_over_composed": round(med["direct"] / med["composed"], 3),
                                    "graph_over_composed": round(med["graph"] / med["composed"], 3),
                                    "rr_after_the_iterations_over_rr_of_r0": final / float(torch.dot(b.double(), b.double()))}
            del g
        plan.close()
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--iterations", type=int, default=8, help="iterations per timed round (even)")
    ap.add_argument("--only", nargs="*", help="names among: vectors, " + ", ".join(m[0] for m in MATRICES))
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "krylov_ab.log"))
    args = ap.parse_args()
    assert args.iterations % 2 == 0
    log = open(args.log, "a")

    def say(text):
        print(text, flush=True)
        log.write(text + "\n")
        log.flush()

    if not args.only or "vectors" in args.only:
        say("the step and the direction against the sync-free torch way; one process, torch events on one stream, 3 warm-up rounds, "
            "then %d rounds alternating the two ways, medians" % args.rounds)
        res = vectors(args.rounds)
        for k, m in res["cases"].items():
            say("    n %d %-9s step: torch %8.2f us, fused %8.2f us, ratio %.3f (by bytes %.3f);   direction: torch %8.2f us, fused %8.2f us, "
                "ratio %.3f (by bytes %.3f);   r'r against torch %.1e" % (
                    res["n"], k, m["step_us"]["torch"], m["step_us"]["fused"], m["step_ratio"], m["step_ratio_by_bytes"], m["direction_us"]["torch"],
                    m["direction_us"]["fused"], m["direction_ratio"], m["direction_ratio_by_bytes"], m["dot_relative_difference_to_torch"]))
        say(json.dumps(res))
    first = True
    for name, spec, what in MATRICES:
        if args.only and name not in args.only:
            continue
        if first:
            say("one preconditioned CG iteration: three enqueue-only calls direct, two iterations captured and replayed, and composed from the "
                "scaled multiply, torch ops and .item(); wall clock per iteration over %d iterations, 3 warm-up rounds, then %d rounds "
                "alternating the ways, medians" % (args.iterations, args.rounds))
            first = False
        res = iteration(name, spec, args.rounds, args.iterations)
        say("%-14s %s: %d rows, %d stored entries; %s" % (name, what, res["rows"], res["stored_entries"], res["library"]))
        for k, m in res["families"].items():
            u = m["per_iteration_us"]
            say("    %-9s direct %9.2f us, graph %9.2f us, composed %9.2f us per iteration; direct / composed %.3f, graph / composed %.3f" % (
                k, u["direct"], u["graph"], u["composed"], m["direct_over_composed"], m["graph_over_composed"]))
        say(json.dumps(res))
    log.close()


if __name__ == "__main__":
    main()
