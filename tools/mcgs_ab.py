#!/usr/bin/env python3
"""The multicolour Gauss-Seidel / SSOR preconditioner (include/spmv_hip_mcgs.h) at Level 2, in ONE process on one stream, doubles:

  sweep   a forward sweep (C launches that read the colour-major copy of the matrix once) against ONE multiply of the same CSR
          arrays from plain tiles with 32-bit columns (SPMV_HIP_FLAG_NO_INDEX_COMPRESSION: spmv_hip_tuning.h); both stream 12 bytes
          per stored entry.  Beside the times, the ratio of the streamed bytes computed from the array sizes:
              sweep      12 nnz + rows (4 order + 4 row_ptr + 8 b + 8 minv + 8 x read + 8 x written) + 8 rows (x gathered once)
              multiply   12 nnz + rows (4 row_ptr + 8 y read + 8 y written) + 8 cols (x gathered once)
          and whether the sweep meets that ratio x 1.16 (the spread between boxes README records).  Reported, not gated.
          A matrix whose stored pattern is not symmetric colours with conflicts; its sweep is refused and not measured.
  pcg     on Poisson 4096^2 alone: the header's PCG from x0 = 0 to r'r <= 1e-12 r0'r0 (looked at on the host every 25 iterations;
          at most --cap iterations) through a C16Plan (c16_f64): iterations and wall time with the diagonal, with the degree-3
          Chebyshev polynomial at ratio 30 and with the symmetric sweep at omega = 1.  Reported only.

Three warm-up rounds, then --rounds rounds alternating the ways, medians.  The log goes to stdout and to profiles/mcgs_ab.log
(--log).

    python tools/mcgs_ab.py
    python tools/mcgs_ab.py --only poisson_4096 --rounds 25 --no-pcg
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
    ("mesh_128", "mesh_dofs:128,1", "27-neighbour mesh 128^3 with jittered links, 1 unknown per node", False),
    ("delaunay_1dof", "delaunay:2000000,1,2,rcm", "Delaunay 3-D mesh, scalar, RCM order", False),
]
SPREAD = 1.16
RATIO = 30.0


def matrix(name, spec, rounds, cap, solve):
    import torch
    from spmv_amd import capi
    dev = torch.device("cuda:0")
    rows, cols, p_h, c_h, v_h = load(spec)
    assert rows == cols
    nnz = int(p_h[-1])
    s = torch.cuda.current_stream().cuda_stream
    res = {"matrix": name, "spec": spec, "rows": rows, "stored_entries": nnz, "rounds": rounds, "library": os.path.basename(capi.LIB_PATH)}
    tp, tc, tv = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (p_h, c_h, v_h))
    i32 = dict(dtype=torch.int32, device=dev)
    f64 = dict(dtype=torch.float64, device=dev)
    colour, status = torch.zeros(rows, **i32), torch.zeros(4, **i32)
    work = torch.zeros(capi.mcgs_workspace_bytes(rows) // 8, **f64)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    capi.mcgs_colour(rows, tp, tc, 0, colour, status, work, None, s)
    t1 = time.perf_counter()
    order, pp, pc, pv = torch.zeros(rows, **i32), torch.zeros(rows + 1, **i32), torch.zeros(max(1, nnz), **i32), torch.zeros(max(1, nnz), **f64)
    plan = capi.mcgs_permute(rows, nnz, tp, tc, tv, colour, status, order, pp, pc, pv, work, None, s)
    t2 = time.perf_counter()
    st = status.cpu().numpy().tolist()
    res.update(colours=st[0], rounds_of_colouring=st[1], conflicts=st[2], overflowed=st[3], group=plan.group,
               colour_seconds=round(t1 - t0, 4), permute_seconds=round(t2 - t1, 4))
    minv = torch.zeros(rows, **f64)
    bstatus = torch.zeros(2, **i32)
    capi.bjacobi_setup(rows, 1, tp, tc, tv, minv, bstatus, s)
    gen = torch.Generator(device=dev)
    gen.manual_seed(9)
    rhs = torch.rand(rows, generator=gen, **f64) * 2 - 1
    x, y = torch.zeros(rows, **f64), torch.zeros(rows, **f64)
    sweep_bytes = 12 * nnz + rows * 40 + 8 * rows
    multiply_bytes = 12 * nnz + rows * 20 + 8 * cols
    res.update(sweep_bytes=sweep_bytes, multiply_bytes=multiply_bytes, bytes_ratio=round(sweep_bytes / multiply_bytes, 4))
    plain = capi.CsrPlan(rows, cols, p_h, capi.CSR_AUTO, 0, capi.FLAG_NO_INDEX_COMPRESSION)
    P, C, V = tp.data_ptr(), tc.data_ptr(), tv.data_ptr()

    def multiply():
        plain.spmv(P, C, V, rhs.data_ptr(), y.data_ptr(), s)

    ways = {"multiply": multiply}
    if plan.conflicts == 0 and plan.colours > 0:
        ways["forward_sweep"] = lambda: capi.mcgs_sweep(plan, 0, plan.colours - 1, 1.0, rhs, minv, x, s)
        ways["apply"] = lambda: capi.mcgs_apply(plan, 1.0, rhs, minv, x, None, None, 0, s)
    med = alternate(torch, ways, rounds)
    plain.close()
    res["us"] = {k: round(v, 2) for k, v in med.items()}
    if "forward_sweep" in med:
        ratio = med["forward_sweep"] / med["multiply"]
        res.update(sweep_over_multiply=round(ratio, 3), target=round(SPREAD * sweep_bytes / multiply_bytes, 3),
                   target_met=bool(ratio <= SPREAD * sweep_bytes / multiply_bytes),
                   sweep_GBps=round(sweep_bytes / med["forward_sweep"] / 1e3, 1), multiply_GBps=round(multiply_bytes / med["multiply"] / 1e3, 1))
    if solve and "apply" in med:
        res["pcg"] = pcg(torch, capi, rows, cols, p_h, c_h, tp, tc, tv, minv, rhs, plan, cap, s)
    return res


def pcg(torch, capi, n, cols, p_h, c_h, tp, tc, tv, minv, rhs, mplan, cap, s):
    dev = rhs.device
    f64 = dict(dtype=torch.float64, device=dev)
    c16 = capi.C16Plan(n, cols, p_h, c_h, 0, s)
    P, C, A = tp.data_ptr(), tc.data_ptr(), tv.data_ptr()
    x, r, pv, q, z, d, u = (torch.zeros(n, **f64) for _ in range(7))
    lam, table = torch.zeros(1, **f64), torch.zeros(6, **f64)
    rz, pq, rr = [torch.ones(2, **f64) for _ in range(2)], torch.ones(2, **f64), torch.ones(2, **f64)
    start = torch.tensor([0.0, 1.0], **f64)
    mbytes, kbytes = c16.dots_workspace_bytes(), capi.krylov_workspace_bytes(n)
    mwork, kwork = torch.zeros(mbytes // 8, **f64), torch.zeros(kbytes // 8, **f64)
    capi.cheby_bound(n, tp, tv, minv, lam, s)
    capi.cheby_coeffs(3, lam, 1.0, RATIO, table, s)

    def diagonal(src, dots):
        capi.bjacobi_apply(n, 1, minv, src, z, dots, kwork, None, s)

    def chebyshev(src, dots):
        for j in range(3):
            if j > 0:
                c16.spmv_f64_scaled(P, C, A, z.data_ptr(), -1.0, 1.0, src.data_ptr(), u.data_ptr(), s)
            last = j == 2
            capi.cheby_step(n, 3, j, table, src if j == 0 else u, minv, d, z, src if last else None, dots if last else None,
                            kwork if last else None, None, s)

    def sweeps(src, dots):
        capi.mcgs_apply(mplan, 1.0, src, minv, z, dots, kwork, None, s)

    out = {}
    for way, apply in (("diagonal", diagonal), ("chebyshev_3", chebyshev), ("symmetric_sweep", sweeps)):
        x.zero_()
        r.copy_(rhs)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        apply(r, rz[0])
        capi.cg_direction(n, start, start.data_ptr() + 8, z, None, pv, s)
        first = float(torch.dot(r, r))
        it, now = 0, first
        while it < cap and 1e-12 * first < now < 1e6 * first:
            for _ in range(25):
                old, new = rz[it % 2], rz[1 - it % 2]
                c16.spmv_f64_scaled_dots(P, C, A, pv.data_ptr(), 1.0, 0.0, None, q.data_ptr(), pv.data_ptr(), pq.data_ptr(), mwork.data_ptr(),
                                         mbytes, s)
                capi.cg_step(n, old, pq.data_ptr() + 8, pv, q, x, r, None, rr, kwork, None, s)
                apply(r, new)
                capi.cg_direction(n, new, old, z, None, pv, s)
                it += 1
            now = float(rr.cpu()[0])
        torch.cuda.synchronize()
        out[way] = {"iterations": it, "seconds": round(time.perf_counter() - t0, 4), "relative_rr": now / first, "reached": bool(now <= 1e-12 * first)}
    c16.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--cap", type=int, default=20000, help="the largest number of PCG iterations")
    ap.add_argument("--only", nargs="*", default=None, help="matrix names")
    ap.add_argument("--no-pcg", action="store_true")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "mcgs_ab.log"))
    args = ap.parse_args()
    log = open(args.log, "w")

    def say(text):
        print(text, flush=True)
        log.write(text + "\n")
        log.flush()

    say("a forward sweep (omega 1, doubles) against one multiply of the same CSR arrays from plain tiles with 32-bit columns; one process, torch "
        "events on one stream, 3 warm-up rounds, then %d rounds alternating the ways, medians; the target is the ratio of the streamed bytes x %.2f"
        % (args.rounds, SPREAD))
    for name, spec, what, spd in MATRICES:
        if args.only and name not in args.only:
            continue
        res = matrix(name, spec, args.rounds, args.cap, spd and not args.no_pcg)
        say("%-13s %s: %d rows, %d stored entries; %s" % (name, what, res["rows"], res["stored_entries"], res["library"]))
        say("    %d colours in %d rounds (%.3f s; the plan %.3f s), %d conflicts, %d overflowed rows, group %d" % (
            res["colours"], res["rounds_of_colouring"], res["colour_seconds"], res["permute_seconds"], res["conflicts"], res["overflowed"], res["group"]))
        u = res["us"]
        if "forward_sweep" in u:
            say("    forward sweep %8.1f us (%.1f GB/s), one multiply %8.1f us (%.1f GB/s): ratio %.3f against %.3f by bytes (%d against %d); "
                "target %.3f %s; the symmetric sweep (apply without dots) %8.1f us" % (
                    u["forward_sweep"], res["sweep_GBps"], u["multiply"], res["multiply_GBps"], res["sweep_over_multiply"], res["bytes_ratio"],
                    res["sweep_bytes"], res["multiply_bytes"], res["target"], "met" if res["target_met"] else "MISSED", u["apply"]))
        else:
            say("    one multiply %8.1f us; the sweep: not measured (the stored pattern is not symmetric: %d entries couple rows of one colour, "
                "and such a plan is refused)" % (u["multiply"], res["conflicts"]))
        for way, g in res.get("pcg", {}).items():
            say("        pcg %-16s %6d iterations, %8.4f s, r'r / r0'r0 %.3e%s" % (
                way, g["iterations"], g["seconds"], g["relative_rr"], "" if g["reached"] else " (not reached)"))
        say(json.dumps(res))
    log.close()


if __name__ == "__main__":
    main()
