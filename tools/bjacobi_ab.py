#!/usr/bin/env python3
"""The point-block Jacobi preconditioner (include/spmv_hip_bjacobi.h) against what a caller had to do without it, at Level 2, in
ONE process on one stream, for double and float vectors and b = 1, 2, 3, 4, 6, 8:

  vectors alone (n = 3 * 2^22; the inverse of doubles at b = 3 is 302 MB, beyond the Infinity Cache), torch events, no host read in
  any way:
    apply       spmv_hip_bjacobi_apply_* with dots      against   torch.bmm on the (n / b, b, b) view + torch.dot(r, z)
                                                        and       (inv3 * r3).sum(-1) + torch.dot(r, z): the composition without
                                                                  the batched-GEMM dispatch, with an (n / b, b, b) temporary
    plain, add  the apply without dots and spmv_hip_bjacobi_apply_add_*, reported
    triad       a = b + s c over three arrays of (b + 2) n / 3 elements: the same-process bandwidth that the apply's (b + 2) n
                elements are a share of

  on matrices with 3 unknowns per node (Delaunay 3-dof in RCM order, mesh_dofs(., 3)), through a C16Plan (c16_f64 for doubles,
  c16_f32xy for floats):
    setup       spmv_hip_bjacobi_setup_* at b = 3 against one multiply (spmv_hip_csr_spmv_*_scaled, alpha 1, beta 0)
    pcg         one PCG iteration as the header composes it with 3 x 3 blocks (multiply with dots, step without minv, apply with
                dots, direction over z) against one with the diagonal d_minv (multiply with dots, step, direction); the vectors
                hold what they hold: an iteration is timed, nothing is solved

Three warm-up rounds, then --rounds rounds alternating the ways, medians.  Everything is reported, nothing gated.  The log goes to
stdout and to profiles/bjacobi_ab.log (--log).

    python tools/bjacobi_ab.py
    python tools/bjacobi_ab.py --only vectors delaunay_3dof --rounds 25
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spmv-cache-trace_amd", "python"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from compact_ab import load  # noqa: E402
from scaled_ab import alternate  # noqa: E402

MATRICES = [
    ("delaunay_3dof", "delaunay:250000,3,1,rcm", "Delaunay 3-D mesh, 3 unknowns per node, RCM order"),
    ("mesh_64_3dof", "mesh_dofs:64,3", "27-neighbour mesh 64^3 with jittered links, 3 unknowns per node"),
]
BLOCKS = (1, 2, 3, 4, 6, 8)


def vectors(rounds):
    import torch
    from spmv_amd import capi
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    n = 3 * 2 ** 22
    out = {"n": n, "rounds": rounds, "library": os.path.basename(capi.LIB_PATH), "cases": {}}
    gen = torch.Generator(device=dev)
    gen.manual_seed(12)
    for dtype, name in ((torch.float64, "f64"), (torch.float32, "f32")):
        es = 8 if dtype == torch.float64 else 4
        r, x = ((torch.rand(n, dtype=torch.float64, device=dev, generator=gen) * 2 - 1).to(dtype) for _ in range(2))
        z, zt = (torch.zeros(n, dtype=dtype, device=dev) for _ in range(2))
        dots = torch.zeros(2, dtype=torch.float64, device=dev)
        work = torch.zeros(capi.krylov_workspace_bytes(n) // 8, dtype=torch.float64, device=dev)
        for b in BLOCKS:
            inv = (torch.rand(n * b, dtype=torch.float64, device=dev, generator=gen) * 2 - 1).to(dtype)
            inv3, r3, z3, rrow = inv.view(n // b, b, b), r.view(n // b, b, 1), zt.view(n // b, b, 1), r.view(n // b, 1, b)
            got = {}

            def torch_bmm():
                torch.bmm(inv3, r3, out=z3)
                got["dot"] = torch.dot(r, zt)

            def torch_sum():
                torch.sum(inv3 * rrow, dim=2, out=zt.view(n // b, b))
                got["dot"] = torch.dot(r, zt)

            def fused():
                capi.bjacobi_apply(n, b, inv, r, z, dots, work, None, s)

            def plain():
                capi.bjacobi_apply(n, b, inv, r, z, None, None, 0, s)

            def add():
                capi.bjacobi_apply_add(n, b, inv, r, x, s)

            ta, tb, tc = (torch.zeros((b + 2) * n // 3, dtype=dtype, device=dev) for _ in range(3))

            def triad():
                torch.add(tb, tc, alpha=0.5, out=ta)

            med = alternate(torch, {"bmm": torch_bmm, "sum": torch_sum, "fused": fused, "plain": plain, "add": add, "triad": triad}, rounds)
            triad_bw = 3 * ta.numel() * es / med["triad"]  # bytes per us
            fused_bytes = (b + 2) * n * es
            out["cases"]["%s_b%d" % (name, b)] = {
                "us": {key: round(u, 2) for key, u in med.items()},
                "fused_over_bmm": round(med["fused"] / med["bmm"], 4), "fused_over_sum": round(med["fused"] / med["sum"], 3),
                "ratio_by_bytes": round((b + 2) / (b + 4), 3), "triad_GBps": round(triad_bw / 1e3, 1),
                "fused_GBps": round(fused_bytes / med["fused"] / 1e3, 1),
                "fused_share_of_triad_bandwidth": round(fused_bytes / med["fused"] / triad_bw, 3),
                "plain_share_of_triad_bandwidth": round(fused_bytes / med["plain"] / triad_bw, 3),
                "add_share_of_triad_bandwidth": round((b + 3) * n * es / med["add"] / triad_bw, 3)}
            del inv, inv3, ta, tb, tc
            torch.cuda.empty_cache()
        del r, x, z, zt, work
        torch.cuda.empty_cache()
    return out


def matrix(name, spec, rounds):
    import torch
    from spmv_amd import capi
    dev = torch.device("cuda:0")
    b = 3
    rows, cols, p_h, c_h, v_h = load(spec)
    assert rows == cols and rows % b == 0
    nnz = int(p_h[-1])
    row = np.repeat(np.arange(rows), np.diff(p_h))
    diag = np.zeros(rows)
    diag[row[c_h == row]] = np.abs(v_h[c_h == row])
    minv_h = np.where(diag > 0, 1.0 / np.where(diag > 0, diag, 1.0), 1.0)
    s = torch.cuda.current_stream().cuda_stream
    res = {"matrix": name, "spec": spec, "rows": rows, "stored_entries": nnz, "rounds": rounds, "b": b,
           "library": os.path.basename(capi.LIB_PATH), "families": {}}
    tp, tc, tv = (torch.from_numpy(a).to(dev) for a in (p_h, c_h, v_h))
    tf = torch.zeros(max(1, nnz), dtype=torch.float32, device=dev)
    capi.narrow_values(nnz, tv.data_ptr(), tf.data_ptr(), s)
    plan = capi.C16Plan(rows, cols, p_h, c_h, 0, s)
    P, C = tp.data_ptr(), tc.data_ptr()
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    for fam, dtype, vals, scaled, fused in (("c16_f64", torch.float64, tv, plan.spmv_f64_scaled, plan.spmv_f64_scaled_dots),
                                            ("c16_f32xy", torch.float32, tf, plan.spmv_f32xy_scaled, plan.spmv_f32xy_scaled_dots)):
        n = rows
        A = vals.data_ptr()
        inv = torch.zeros(n * b, dtype=dtype, device=dev)
        minv = torch.from_numpy(minv_h).to(dev).to(dtype)
        x, r, pv, q, z = (torch.from_numpy(np.random.default_rng(k).uniform(-1.0, 1.0, size=n)).to(dev).to(dtype) for k in range(5))
        rz1, pq, rr = (torch.ones(2, dtype=torch.float64, device=dev) for _ in range(3))
        # an iteration is timed, not solved: a = tiny / p'q and b = r'z / huge keep the vectors as they are over the rounds
        tiny, huge = (torch.full((2,), v, dtype=torch.float64, device=dev) for v in (1e-30, 1e30))
        mbytes, kbytes = plan.dots_workspace_bytes(), capi.krylov_workspace_bytes(n)
        mwork = torch.zeros(mbytes // 8, dtype=torch.float64, device=dev)
        kwork = torch.zeros(kbytes // 8, dtype=torch.float64, device=dev)

        def setup():
            capi.bjacobi_setup(n, b, tp, tc, tv, inv, status, s)

        def multiply():
            scaled(P, C, A, pv.data_ptr(), 1.0, 0.0, None, q.data_ptr(), s)

        def pcg_diagonal():
            fused(P, C, A, pv.data_ptr(), 1.0, 0.0, None, q.data_ptr(), pv.data_ptr(), pq.data_ptr(), mwork.data_ptr(), mbytes, s)
            capi.cg_step(n, tiny, pq.data_ptr() + 8, pv, q, x, r, minv, rz1, kwork, None, s)
            capi.cg_direction(n, rz1.data_ptr() + 8, huge, r, minv, pv, s)

        def pcg_blocks():
            fused(P, C, A, pv.data_ptr(), 1.0, 0.0, None, q.data_ptr(), pv.data_ptr(), pq.data_ptr(), mwork.data_ptr(), mbytes, s)
            capi.cg_step(n, tiny, pq.data_ptr() + 8, pv, q, x, r, None, rr, kwork, None, s)
            capi.bjacobi_apply(n, b, inv, r, z, rz1, kwork, None, s)
            capi.cg_direction(n, rz1, huge, z, None, pv, s)

        setup()
        torch.cuda.synchronize()
        st = status.cpu().numpy().tolist()
        med = alternate(torch, {"setup": setup, "multiply": multiply}, rounds)
        medp = alternate(torch, {"diagonal": pcg_diagonal, "blocks": pcg_blocks}, rounds)
        res["families"][fam] = {"singular_blocks": st, "setup_us": round(med["setup"], 2), "multiply_us": round(med["multiply"], 2),
                                "setup_over_multiply": round(med["setup"] / med["multiply"], 3),
                                "pcg_iteration_us": {k: round(u, 2) for k, u in medp.items()},
                                "blocks_over_diagonal": round(medp["blocks"] / medp["diagonal"], 3)}
        assert bool(torch.all(torch.isfinite(x))) and bool(torch.all(torch.isfinite(pv)))
    plan.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--only", nargs="*", default=None, help="vectors and / or matrix names")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "bjacobi_ab.log"))
    args = ap.parse_args()
    log = open(args.log, "w")

    def say(text):
        print(text, flush=True)
        log.write(text + "\n")
        log.flush()

    if not args.only or "vectors" in args.only:
        say("the apply with dots against torch.bmm + dot and against (inv3 * r3).sum(-1) + dot; one process, torch events on one stream, "
            "3 warm-up rounds, then %d rounds alternating the ways, medians" % args.rounds)
        res = vectors(args.rounds)
        for k, c in res["cases"].items():
            u = c["us"]
            say("    n %d %-7s bmm + dot %9.2f us, sum + dot %8.2f us, fused %7.2f us (%.4f of bmm, %.3f of sum; by bytes %.3f), without dots "
                "%7.2f us, apply_add %7.2f us; triad %.1f GB/s, of which fused %.3f, without dots %.3f, apply_add %.3f" % (
                    res["n"], k, u["bmm"], u["sum"], u["fused"], c["fused_over_bmm"], c["fused_over_sum"], c["ratio_by_bytes"], u["plain"],
                    u["add"], c["triad_GBps"], c["fused_share_of_triad_bandwidth"], c["plain_share_of_triad_bandwidth"],
                    c["add_share_of_triad_bandwidth"]))
        say(json.dumps(res))
    first = True
    for name, spec, what in MATRICES:
        if args.only and name not in args.only:
            continue
        if first:
            say("the setup at b = 3 against one multiply, and one PCG iteration with 3 x 3 blocks against one with the diagonal; "
                "3 warm-up rounds, then %d rounds alternating the ways, medians" % args.rounds)
            first = False
        res = matrix(name, spec, args.rounds)
        say("%-14s %s: %d rows, %d stored entries; %s" % (name, what, res["rows"], res["stored_entries"], res["library"]))
        for k, f in res["families"].items():
            u = f["pcg_iteration_us"]
            say("    %-9s setup %8.1f us, one multiply %8.1f us (%.3f); one PCG iteration: diagonal %8.1f us, blocks %8.1f us (%.3f); "
                "singular blocks %s" % (k, f["setup_us"], f["multiply_us"], f["setup_over_multiply"], u["diagonal"], u["blocks"],
                                        f["blocks_over_diagonal"], f["singular_blocks"]))
        say(json.dumps(res))
    log.close()


if __name__ == "__main__":
    main()
