#!/usr/bin/env python3
"""The Chebyshev polynomial preconditioner (include/spmv_hip_cheby.h) against what a caller had to do without it, at Level 2, in
ONE process on one stream, for double and float vectors:

  steps (n = 4096^2; four vectors of doubles are 537 MB, beyond the Infinity Cache), torch events, no host read in any way:
    every mode of spmv_hip_cheby_step_* with minv     against   its torch composition over two 0-dim device scalars:
                                                                d.mul_(c), d.add_((minv * u).mul_(e)), z.add_(d) (+ two torch.dot)
    triad       a = b + s c over three arrays of 2 n elements: the same-process bandwidth the step's passes are a share of

  on Poisson 4096^2 and mesh_dofs(128^3, 1), through a C16Plan (c16_f64 for doubles, c16_f32xy for floats):
    bound       spmv_hip_cheby_bound_* against one multiply (spmv_hip_csr_spmv_*_scaled, alpha 1, beta 0)
    apply       one degree-3 application (three steps, two multiplies) against the same with the steps composed from torch
    pcg         the header's PCG from x0 = 0 to r'r <= 1e-12 r0'r0 (looked at on the host every 25 iterations; at most --cap
                iterations): iterations and wall time with the diagonal alone and with degrees 2, 3, 4 at ratio 30 on the
                Gershgorin bound; on the symmetric positive definite matrix alone (mesh_dofs' values are random: no solve)

Three warm-up rounds, then --rounds rounds alternating the ways, medians.  Everything is reported, nothing gated.  The log goes to
stdout and to profiles/cheby_ab.log (--log).

    python tools/cheby_ab.py
    python tools/cheby_ab.py --only steps poisson_4096 --rounds 25
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
    ("poisson_4096", "synthetic:poisson2d:4096", "5-point Laplacian on a 4096 x 4096 grid", True),
    # (values uniform in (-1, 1) on an unsymmetric pattern: neither symmetric nor definite, so CG does not apply and no solve is run)
    ("mesh_128", "mesh_dofs:128,1", "27-neighbour mesh 128^3 with jittered links, 1 unknown per node", False),
]
# (name, degree, j, dots, vector passes of the fused call with minv)
MODES = (("first", 3, 0, False, 4), ("middle", 3, 1, False, 6), ("last", 3, 2, False, 5), ("last+dots", 3, 2, True, 6), ("sole", 1, 0, False, 3),
         ("sole+dots", 1, 0, True, 4))
RATIO = 30.0


def steps(rounds):
    import torch
    from spmv_amd import capi
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    n = 4096 * 4096
    out = {"n": n, "rounds": rounds, "library": os.path.basename(capi.LIB_PATH), "cases": {}}
    gen = torch.Generator(device=dev)
    gen.manual_seed(22)
    coef = torch.tensor([0.0, 0.5, 0.25, 0.75, 0.125, 0.5], dtype=torch.float64, device=dev)
    for dtype, name in ((torch.float64, "f64"), (torch.float32, "f32")):
        es = 8 if dtype == torch.float64 else 4
        u, minv, r = ((torch.rand(n, dtype=torch.float64, device=dev, generator=gen) * 2 - 1).to(dtype) for _ in range(3))
        d, z, dt, zt = (torch.zeros(n, dtype=dtype, device=dev) for _ in range(4))
        dots = torch.zeros(2, dtype=torch.float64, device=dev)
        work = torch.zeros(capi.krylov_workspace_bytes(n) // 8, dtype=torch.float64, device=dev)
        ta, tb, tc = (torch.zeros(2 * n, dtype=dtype, device=dev) for _ in range(3))
        got = {}

        def triad():
            torch.add(tb, tc, alpha=0.5, out=ta)

        for mode, degree, j, with_dots, passes in MODES:
            c, e = coef[2 * j].to(dtype), coef[2 * j + 1].to(dtype)

            def torch_way():
                if j == 0:
                    torch.mul(minv, u, out=dt)
                    dt.mul_(e)
                    zt.copy_(dt)
                else:
                    dt.mul_(c)
                    dt.add_((minv * u).mul_(e))
                    zt.add_(dt)
                if with_dots:
                    got["rz"], got["zz"] = torch.dot(zt, r), torch.dot(zt, zt)

            def fused():
                capi.cheby_step(n, degree, j, coef, u, minv, d if degree > 1 else None, z, r if with_dots else None, dots if with_dots else None,
                                work if with_dots else None, None, s)

            med = alternate(torch, {"torch": torch_way, "fused": fused, "triad": triad}, rounds)
            triad_bw = 3 * ta.numel() * es / med["triad"]  # bytes per us
            out["cases"]["%s_%s" % (name, mode)] = {
                "us": {k: round(v, 2) for k, v in med.items()}, "fused_over_torch": round(med["fused"] / med["torch"], 3), "passes": passes,
                "triad_GBps": round(triad_bw / 1e3, 1), "fused_GBps": round(passes * n * es / med["fused"] / 1e3, 1),
                "fused_share_of_triad_bandwidth": round(passes * n * es / med["fused"] / triad_bw, 3)}
            d.zero_(), z.zero_(), dt.zero_(), zt.zero_()
        del u, minv, r, d, z, dt, zt, work, ta, tb, tc
        torch.cuda.empty_cache()
    return out


def matrix(name, spec, rounds, cap, spd):
    import torch
    from spmv_amd import capi
    dev = torch.device("cuda:0")
    rows, cols, p_h, c_h, v_h = load(spec)
    assert rows == cols
    nnz = int(p_h[-1])
    row = np.repeat(np.arange(rows), np.diff(p_h))
    diag = np.zeros(rows)
    diag[row[c_h == row]] = np.abs(v_h[c_h == row])
    del row
    minv_h = np.where(diag > 0, 1.0 / np.where(diag > 0, diag, 1.0), 1.0)
    s = torch.cuda.current_stream().cuda_stream
    res = {"matrix": name, "spec": spec, "rows": rows, "stored_entries": nnz, "rounds": rounds, "ratio": RATIO,
           "library": os.path.basename(capi.LIB_PATH), "families": {}}
    tp, tc, tv = (torch.from_numpy(a).to(dev) for a in (p_h, c_h, v_h))
    tf = torch.zeros(max(1, nnz), dtype=torch.float32, device=dev)
    capi.narrow_values(nnz, tv.data_ptr(), tf.data_ptr(), s)
    plan = capi.C16Plan(rows, cols, p_h, c_h, 0, s)
    P, C = tp.data_ptr(), tc.data_ptr()
    rhs_h = np.random.default_rng(9).uniform(-1.0, 1.0, size=rows)
    for fam, dtype, vals, scaled, fused in (("c16_f64", torch.float64, tv, plan.spmv_f64_scaled, plan.spmv_f64_scaled_dots),
                                            ("c16_f32xy", torch.float32, tf, plan.spmv_f32xy_scaled, plan.spmv_f32xy_scaled_dots)):
        n, A = rows, vals.data_ptr()
        minv = torch.from_numpy(minv_h).to(dev).to(dtype)
        rhs = torch.from_numpy(rhs_h).to(dev).to(dtype)
        x, r, pv, q, z, d, u, dt, zt = (torch.zeros(n, dtype=dtype, device=dev) for _ in range(9))
        lam = torch.zeros(1, dtype=torch.float64, device=dev)
        tables = {k: torch.zeros(2 * k, dtype=torch.float64, device=dev) for k in (2, 3, 4)}
        rz, pq, rr = [torch.ones(2, dtype=torch.float64, device=dev) for _ in range(2)], torch.ones(2, dtype=torch.float64, device=dev), \
            torch.ones(2, dtype=torch.float64, device=dev)
        start = torch.tensor([0.0, 1.0], dtype=torch.float64, device=dev)
        mbytes, kbytes = plan.dots_workspace_bytes(), capi.krylov_workspace_bytes(n)
        mwork = torch.zeros(mbytes // 8, dtype=torch.float64, device=dev)
        kwork = torch.zeros(kbytes // 8, dtype=torch.float64, device=dev)

        def bound():
            capi.cheby_bound(n, tp, tv, minv, lam, s)

        def multiply():
            scaled(P, C, A, pv.data_ptr(), 1.0, 0.0, None, q.data_ptr(), s)

        bound()
        for k, t in tables.items():
            capi.cheby_coeffs(k, lam, 1.0, RATIO, t, s)
        torch.cuda.synchronize()
        lam_h = float(lam.cpu()[0])

        def polynomial(degree, src, dots):
            """z = p(M^-1 A) M^-1 src: `degree` steps and the multiplies between them, the last step's dots into `dots`."""
            t = tables[degree]
            for j in range(degree):
                if j > 0:
                    scaled(P, C, A, z.data_ptr(), -1.0, 1.0, src.data_ptr(), u.data_ptr(), s)
                last = j == degree - 1 and dots is not None
                capi.cheby_step(n, degree, j, t, src if j == 0 else u, minv, d, z, src if last else None, dots if last else None,
                                kwork if last else None, None, s)

        def apply_fused():
            polynomial(3, rhs, rz[0])

        c3 = [tables[3][k].to(dtype) for k in range(6)]
        got = {}

        def apply_torch():
            torch.mul(minv, rhs, out=dt)
            dt.mul_(c3[1])
            zt.copy_(dt)
            for j in (1, 2):
                scaled(P, C, A, zt.data_ptr(), -1.0, 1.0, rhs.data_ptr(), u.data_ptr(), s)
                dt.mul_(c3[2 * j])
                dt.add_((minv * u).mul_(c3[2 * j + 1]))
                zt.add_(dt)
            got["rz"], got["zz"] = torch.dot(zt, rhs), torch.dot(zt, zt)

        pv.copy_(rhs)
        med = alternate(torch, {"bound": bound, "multiply": multiply, "apply": apply_fused, "apply_torch": apply_torch}, rounds)

        def pcg(degree):
            """(iterations, seconds, r'r / r0'r0) from x0 = 0; degree 0: the diagonal alone (spmv_hip_krylov.h's loop)."""
            x.zero_()
            r.copy_(rhs)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            k = 1 if degree == 0 else 0  # the element of rz that holds r'z
            if degree == 0:
                capi.cg_step(n, start, start.data_ptr() + 8, pv, q, x, r, minv, rz[0], kwork, None, s)  # a = 0: the dots of r0
                capi.cg_direction(n, start, start.data_ptr() + 8, r, minv, pv, s)
                first = float(rz[0].cpu()[0])
            else:
                polynomial(degree, r, rz[0])
                capi.cg_direction(n, start, start.data_ptr() + 8, z, None, pv, s)
                first = float(torch.dot(r.double(), r.double()))
            it, now = 0, first
            while it < cap and 1e-12 * first < now < 1e6 * first:
                for _ in range(25):
                    old, new = rz[it % 2], rz[1 - it % 2]
                    fused(P, C, A, pv.data_ptr(), 1.0, 0.0, None, q.data_ptr(), pv.data_ptr(), pq.data_ptr(), mwork.data_ptr(), mbytes, s)
                    if degree == 0:
                        capi.cg_step(n, old.data_ptr() + 8, pq.data_ptr() + 8, pv, q, x, r, minv, new, kwork, None, s)
                        capi.cg_direction(n, new.data_ptr() + 8, old.data_ptr() + 8, r, minv, pv, s)
                    else:
                        capi.cg_step(n, old, pq.data_ptr() + 8, pv, q, x, r, None, rr, kwork, None, s)
                        polynomial(degree, r, new)
                        capi.cg_direction(n, new, old, z, None, pv, s)
                    it += 1
                now = float((rz[it % 2] if degree == 0 else rr).cpu()[0])
            torch.cuda.synchronize()
            return it, time.perf_counter() - t0, now / first

        solves = {}
        for degree in (0, 2, 3, 4) if spd else ():
            it, seconds, rel = pcg(degree)
            solves["diagonal" if degree == 0 else "degree_%d" % degree] = {
                "iterations": it, "seconds": round(seconds, 4), "relative_rr": rel, "multiplies": it * max(1, degree), "reached": bool(rel <= 1e-12)}
        res["families"][fam] = {"lambda": lam_h, "us": {k: round(v, 2) for k, v in med.items()},
                                "bound_over_multiply": round(med["bound"] / med["multiply"], 3),
                                "apply_over_torch": round(med["apply"] / med["apply_torch"], 3), "pcg": solves}
        del minv, rhs, x, r, pv, q, z, d, u, dt, zt, mwork, kwork
        torch.cuda.empty_cache()
    plan.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--cap", type=int, default=20000, help="the largest number of PCG iterations")
    ap.add_argument("--only", nargs="*", default=None, help="steps and / or matrix names")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "cheby_ab.log"))
    args = ap.parse_args()
    log = open(args.log, "w")

    def say(text):
        print(text, flush=True)
        log.write(text + "\n")
        log.flush()

    if not args.only or "steps" in args.only:
        say("every mode of the step with minv against its torch composition (mul_, mul, mul_, add_, add_, and two dots where the step forms "
            "them); one process, torch events on one stream, 3 warm-up rounds, then %d rounds alternating the ways, medians" % args.rounds)
        res = steps(args.rounds)
        for k, c in res["cases"].items():
            u = c["us"]
            say("    n %d %-14s torch %8.2f us, fused %7.2f us (%.3f of torch); %d passes at %.1f GB/s, %.3f of the triad's %.1f GB/s" % (
                res["n"], k, u["torch"], u["fused"], c["fused_over_torch"], c["passes"], c["fused_GBps"], c["fused_share_of_triad_bandwidth"],
                c["triad_GBps"]))
        say(json.dumps(res))
    first = True
    for name, spec, what, spd in MATRICES:
        if args.only and name not in args.only:
            continue
        if first:
            say("the bound against one multiply, one degree-3 application against the same with torch's steps, and PCG to r'r <= 1e-12 r0'r0 "
                "with the diagonal alone and with degrees 2, 3, 4 at ratio %g; 3 warm-up rounds, then %d rounds alternating the ways, medians" % (
                    RATIO, args.rounds))
            first = False
        res = matrix(name, spec, args.rounds, args.cap, spd)
        say("%-13s %s: %d rows, %d stored entries; %s" % (name, what, res["rows"], res["stored_entries"], res["library"]))
        for k, f in res["families"].items():
            u = f["us"]
            say("    %-9s lambda %.6f; bound %8.1f us, one multiply %8.1f us (%.3f); one degree-3 application %8.1f us, with torch's steps "
                "%8.1f us (%.3f)" % (k, f["lambda"], u["bound"], u["multiply"], f["bound_over_multiply"], u["apply"], u["apply_torch"],
                                     f["apply_over_torch"]))
            for way, g in f["pcg"].items():
                say("        pcg %-9s %6d iterations, %6d multiplies, %8.4f s, r'r / r0'r0 %.3e%s" % (
                    way, g["iterations"], g["multiplies"], g["seconds"], g["relative_rr"], "" if g["reached"] else " (not reached)"))
            if not f["pcg"]:
                say("        pcg: not measured (the matrix is neither symmetric nor positive definite: conjugate gradients do not apply)")
        say(json.dumps(res))
    log.close()


if __name__ == "__main__":
    main()
