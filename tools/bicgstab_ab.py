#!/usr/bin/env python3
"""The BiCGStab updates (include/spmv_hip_bicgstab.h) against what a caller had to do without them, at Level 2, in ONE process on
one stream, for double and float vectors:

  vectors alone (n = 4096^2: the vectors of a call beyond the Infinity Cache), torch events, with and without minv -- no host read
  in either way:
    s           spmv_hip_bicgstab_s_*          against   a (0-dim), r.addcmul_(v, a, value=-1)         [with minv: torch.mul(minv, r, out=shat)]
    step        spmv_hip_bicgstab_step_*       against   a, w (0-dim), x.addcmul_(phat, a), x.addcmul_(shat or r, w), r.addcmul_(t, w, value=-1),
                                                         torch.dot(r, r), torch.dot(rhat, r)
    direction   spmv_hip_bicgstab_direction_*  against   w, b (0-dim), p.addcmul_(v, w, value=-1), torch.addcmul(r, p, b, out=p)
                                                                                                       [with minv: torch.mul(minv, p, out=phat)]

  one whole right-preconditioned iteration through a C16Plan (c16_f64 for doubles, c16_f32xy for floats), minv = 1 / |diag|, wall
  clock around --iterations iterations from x0 = 0 with one synchronisation at the end:
    direct      *_scaled_dots(1, 0, x = phat, w = rhat), s, *_scaled_dots(1, 0, x = shat, w = r), step, direction: five enqueue-only
                calls, nothing read by the host
    graph       two such iterations captured once, replayed (reported only)
    composed    the scaled multiply twice, torch ops, and the four .item() reads of rhat'v, t's, t't and rhat'r

on Poisson 4096^2 and on the webbase-like graph, which is nonsymmetric (and on which BiCGStab with this right-hand side need not
converge: the iteration is timed, not solved -- non-finite vectors cost the same time).  Three warm-up rounds, then --rounds
rounds alternating the ways, medians.  Everything is reported, nothing gated.  The log goes to stdout and to
profiles/bicgstab_ab.log (--log).

    python tools/bicgstab_ab.py
    python tools/bicgstab_ab.py --only vectors poisson --rounds 25
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
    ("webbase", "synthetic:webbase", "webbase-1M-like graph, nonsymmetric (8 MB per double vector)"),
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
    gen.manual_seed(6)
    for dtype, name in ((torch.float64, "f64"), (torch.float32, "f32")):
        es = 8 if dtype == torch.float64 else 4
        v, r, phat, t, rhat, x, p = ((torch.rand(n, dtype=torch.float64, device=dev, generator=gen) * 2 - 1).to(dtype) for _ in range(7))
        minv = (torch.rand(n, dtype=torch.float64, device=dev, generator=gen) * 1.5 + 0.5).to(dtype)
        hat = torch.zeros(n, dtype=dtype, device=dev)  # shat, then the direction's phat
        # a = 1e-3, w = -2e-3, the r-quotient 0.5: b = -0.25, and every vector stays bounded over the rounds
        sc = torch.tensor([1e-3, 1.0, -2e-3, 1.0, 0.5, 1.0], dtype=torch.float64, device=dev)
        P = [sc.data_ptr() + 8 * k for k in range(6)]
        dots = torch.zeros(2, dtype=torch.float64, device=dev)
        work = torch.zeros(capi.krylov_workspace_bytes(n) // 8, dtype=torch.float64, device=dev)
        for with_minv in (False, True):
            m, h = (minv, hat) if with_minv else (None, None)
            got = {}

            def torch_s():
                a = (sc[0] / sc[1]).to(dtype)
                r.addcmul_(v, a, value=-1.0)
                if with_minv:
                    torch.mul(minv, r, out=hat)

            def fused_s():
                capi.bicgstab_s(n, P[0], P[1], v, r, m, h, s)

            def torch_step():
                a, w = (sc[0] / sc[1]).to(dtype), (sc[2] / sc[3]).to(dtype)
                x.addcmul_(phat, a)
                x.addcmul_(hat if with_minv else r, w)
                r.addcmul_(t, w, value=-1.0)
                got["rr"] = torch.dot(r, r)
                got["hr"] = torch.dot(rhat, r)

            def fused_step():
                capi.bicgstab_step(n, P[0], P[1], P[2], P[3], phat, h, t, rhat, x, r, dots, work, None, s)

            def torch_direction():
                w = sc[2] / sc[3]
                b = ((sc[4] / sc[5]) * ((sc[0] / sc[1]) / w)).to(dtype)
                p.addcmul_(v, w.to(dtype), value=-1.0)
                torch.addcmul(r, p, b, out=p)
                if with_minv:
                    torch.mul(minv, p, out=hat)

            def fused_direction():
                capi.bicgstab_direction(n, P[4], P[5], P[0], P[1], P[2], P[3], r, v, p, m, h, s)

            fused_step()
            ref = float(torch.dot(r.double(), r.double()))
            rel = abs(float(dots[0]) - ref) / ref
            ss = alternate(torch, {"torch": torch_s, "fused": fused_s}, rounds)
            st = alternate(torch, {"torch": torch_step, "fused": fused_step}, rounds)
            di = alternate(torch, {"torch": torch_direction, "fused": fused_direction}, rounds)
            # bytes per element, fused against torch: s reads v, r (minv) and writes r (shat), torch reads r again for shat; the
            # step reads phat, t, rhat, x, r (shat) and writes x, r, torch's five kernels read 9 and write 3; the direction reads
            # r, v, p (minv) and writes p (phat), torch reads p twice more and writes it once more (and reads it again for phat)
            by = {"s": ((3 + 2 * with_minv) * es, (3 + 3 * with_minv) * es), "step": ((7 + with_minv) * es, 12 * es),
                  "direction": ((4 + 2 * with_minv) * es, (6 + 3 * with_minv) * es)}
            case = {"dot_relative_difference_to_torch": rel}
            for key, med in (("s", ss), ("step", st), ("direction", di)):
                case[key + "_us"] = {k: round(u, 2) for k, u in med.items()}
                case[key + "_ratio"] = round(med["fused"] / med["torch"], 3)
                case[key + "_ratio_by_bytes"] = round(by[key][0] / by[key][1], 3)
            out["cases"]["%s%s" % (name, "_minv" if with_minv else "")] = case
        del v, r, phat, t, rhat, x, p, minv, hat, dots, work
        torch.cuda.empty_cache()
    return out


def _div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


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
            x, r, rhat, p, v, t, phat, shat = (torch.zeros(rows, dtype=dtype, device=dev) for _ in range(8))
            start = torch.tensor([0.0, 1.0], dtype=torch.float64, device=dev)
            Z, O = start.data_ptr(), start.data_ptr() + 8
            rho = [torch.zeros(2, dtype=torch.float64, device=dev) for _ in range(2)]
            vv, ts = (torch.zeros(2, dtype=torch.float64, device=dev) for _ in range(2))
            mbytes, kbytes = plan.dots_workspace_bytes(), capi.krylov_workspace_bytes(rows)
            mwork = torch.zeros(mbytes // 8, dtype=torch.float64, device=dev)
            kwork = torch.zeros(kbytes // 8, dtype=torch.float64, device=dev)
            A = vals.data_ptr()

            def begin():
                for a in (x, p, v, t, phat, shat):
                    a.zero_()
                r.copy_(b)
                rhat.copy_(b)
                capi.bicgstab_step(rows, Z, O, Z, O, phat, shat, t, rhat, x, r, rho[0], kwork, kbytes, s)
                capi.bicgstab_direction(rows, Z, O, O, O, O, O, r, v, p, minv, phat, s)

            def one(it):
                old, new = rho[it % 2].data_ptr(), rho[1 - it % 2].data_ptr()
                V, T = vv.data_ptr(), ts.data_ptr()
                fused(P, C, A, phat.data_ptr(), 1.0, 0.0, None, v.data_ptr(), rhat.data_ptr(), V, mwork.data_ptr(), mbytes, s)
                capi.bicgstab_s(rows, old + 8, V + 8, v, r, minv, shat, s)
                fused(P, C, A, shat.data_ptr(), 1.0, 0.0, None, t.data_ptr(), r.data_ptr(), T, mwork.data_ptr(), mbytes, s)
                capi.bicgstab_step(rows, old + 8, V + 8, T + 8, T, phat, shat, t, rhat, x, r, rho[1 - it % 2], kwork, kbytes, s)
                capi.bicgstab_direction(rows, new + 8, old + 8, old + 8, V + 8, T + 8, T, r, v, p, minv, phat, s)

            def direct():
                for it in range(iterations):
                    one(it)

            begin()
            direct()
            side.synchronize()
            final = float(rho[iterations % 2][0])
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                one(0)
                one(1)

            def graph():
                for _ in range(iterations // 2):
                    g.replay()

            def composed():
                rho_old = float(rho[0][1])  # the host read a caller has made before the loop
                for _ in range(iterations):
                    scaled(P, C, A, phat.data_ptr(), 1.0, 0.0, None, v.data_ptr(), s)
                    a = _div(rho_old, torch.dot(rhat, v).item())
                    r.add_(v, alpha=-a)
                    torch.mul(minv, r, out=shat)
                    scaled(P, C, A, shat.data_ptr(), 1.0, 0.0, None, t.data_ptr(), s)
                    w = _div(torch.dot(t, r).item(), torch.dot(t, t).item())
                    x.add_(phat, alpha=a).add_(shat, alpha=w)
                    r.add_(t, alpha=-w)
                    rho_new = torch.dot(rhat, r).item()
                    beta = _div(rho_new, rho_old) * _div(a, w)
                    p.add_(v, alpha=-w).mul_(beta).add_(r)
                    torch.mul(minv, p, out=phat)
                    rho_old = rho_new

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
            med = {k: float(np.median(u)) for k, u in times.items()}
            res["families"][fam] = {"per_iteration_us": {k: round(u, 2) for k, u in med.items()},
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
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "bicgstab_ab.log"))
    args = ap.parse_args()
    assert args.iterations % 2 == 0
    log = open(args.log, "a")

    def say(text):
        print(text, flush=True)
        log.write(text + "\n")
        log.flush()

    if not args.only or "vectors" in args.only:
        say("s, the step and the direction against the sync-free torch way; one process, torch events on one stream, 3 warm-up rounds, "
            "then %d rounds alternating the two ways, medians" % args.rounds)
        res = vectors(args.rounds)
        for k, m in res["cases"].items():
            say("    n %d %-9s %s;   r'r against torch %.1e" % (res["n"], k, ";   ".join(
                "%s: torch %8.2f us, fused %8.2f us, ratio %.3f (by bytes %.3f)" % (
                    key, m[key + "_us"]["torch"], m[key + "_us"]["fused"], m[key + "_ratio"], m[key + "_ratio_by_bytes"])
                for key in ("s", "step", "direction")), m["dot_relative_difference_to_torch"]))
        say(json.dumps(res))
    first = True
    for name, spec, what in MATRICES:
        if args.only and name not in args.only:
            continue
        if first:
            say("one right-preconditioned BiCGStab iteration: five enqueue-only calls direct, two iterations captured and replayed, and "
                "composed from the scaled multiply, torch ops and .item(); wall clock per iteration over %d iterations, 3 warm-up rounds, "
                "then %d rounds alternating the ways, medians" % (args.iterations, args.rounds))
            first = False
        res = iteration(name, spec, args.rounds, args.iterations)
        say("%-14s %s: %d rows, %d stored entries; %s" % (name, what, res["rows"], res["stored_entries"], res["library"]))
        for k, m in res["families"].items():
            u = m["per_iteration_us"]
            say("    %-9s direct %9.2f us, graph %9.2f us, composed %9.2f us per iteration; direct / composed %.3f, graph / composed %.3f; "
                "r'r after the iterations over that of r0 %.3e" % (k, u["direct"], u["graph"], u["composed"], m["direct_over_composed"],
                                                                     m["graph_over_composed"], m["rr_after_the_iterations_over_rr_of_r0"]))
        say(json.dumps(res))
    log.close()


if __name__ == "__main__":
    main()
