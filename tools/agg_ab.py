#!/usr/bin/env python3
"""The aggregation multigrid level (include/spmv_hip_agg.h) at Level 2, in ONE process on one stream:

  hierarchy  levels down to <= --floor rows by spmv_hip_agg_aggregate (theta 0, seed 0), spmv_hip_agg_plan and the Galerkin product:
             rows and stored entries per level, rounds, the largest aggregate, singletons, the operator complexity (the stored
             entries of all levels over those of the finest) and the seconds of the four setup calls per level.
  transfer   on the finest level, doubles and floats: spmv_hip_agg_restrict against torch.zeros(aggregates).index_add_(0, agg, r),
             spmv_hip_agg_prolong_add against x.add_(e[agg], alpha=w), both beside the triad a = b + s c over `rows` elements of the
             same type in the same process and by counted bytes:
                 restrict   rows (4 member + T r) + aggregates (4 member_ptr + T r_c)
                 prolong    rows (4 agg + 2 T x) + aggregates T e_c
                 triad      rows 3 T
  pcg        on Poisson 4096^2 alone: PCG from x0 = 0 to r'r <= 1e-12 r0'r0 (looked at on the host every --look iterations)
             through C16Plans (c16_f64) with a V-cycle composed from existing calls -- degree-2 Chebyshev smoothing over [lambda / 4,
             lambda] before and behind (spmv_hip_cheby_*), the scaled multiply for the residuals, spmv_hip_agg_restrict_f64 and
             spmv_hip_agg_prolong_add_f64 at omega 1 and 1.5, r'z by torch.dot -- against the diagonal and the degree-3 Chebyshev
             polynomial at ratio 30.  The cycle's levels end at --floor rows or at the first level that the aggregation shrinks by less
             than --stall; the coarsest is solved by its dense inverse in torch where it has at most --dense-limit rows, else a FIXED
             Chebyshev polynomial of --coarse-degree stands for the solve (a fixed symmetric operator: CG stays valid).  Iterations and
             seconds, the set-up of the hierarchy, its plans and its smoothers reported beside them.  Reported only.

--mis2 (include/spmv_hip_agg_mis2.h): the hierarchy by spmv_hip_agg_aggregate_mis2; in `transfer` spmv_hip_agg_restrict_group at
spmv_hip_agg_group(plan) lanes beside spmv_hip_agg_restrict on the same plan, each against the triad by counted bytes with the
target of the counted bytes at the triad's rate x 1.16 ("met" / "missed"); in `pcg` the V-cycle down to <= --floor rows with its
dense coarsest solve and the grouped restriction on every level, at omega 1, 1.5 and 2, and then the distance-1 cycle above built
and run in the same process.  The log goes to profiles/agg_mis2_ab.log.

--coarse library (include/spmv_hip_coarse.h; the default, torch, leaves every recorded figure as it was): the coarsest level of
every matrix is set up by spmv_hip_coarse_setup_f64 and applied by spmv_hip_coarse_apply_f64.  In place of `transfer` the log holds,
for that level, the set-up against torch.linalg.inv of the dense matrix (which the host formed for it) and the apply against torch's
matrix-vector product, alternating; in `pcg` every V-cycle runs with the library's solve and with torch's, alternating, without the
baselines and without the distance-1 cycle.  The log goes to profiles/coarse_ab.log.

--plans device (include/spmv_hip_compact_device.h; the default, host, leaves every recorded figure as it was): every C16Plan of the
cycle by spmv_hip_c16_plan_csr_device from the level's device arrays, no column copied to the host.  --plans both: per level the
host's way (row_ptr and columns copied down, spmv_hip_c16_plan_csr) against the device's, five rounds alternating after one
warm-up, medians (under SPMV_HIP_EXPERIMENTS=1 with the stages of the device call), then `pcg` over the host's plans and once more
over the device's, without the distance-1 cycle.  The log goes to profiles/c16_device_plan_ab.log.

Three warm-up rounds, then --rounds rounds alternating the ways, medians.  The log goes to stdout and to profiles/agg_ab.log
(--log).

    python tools/agg_ab.py
    python tools/agg_ab.py --only poisson_4096 --rounds 25 --no-pcg
    python tools/agg_ab.py --mis2
    python tools/agg_ab.py --mis2 --coarse library
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
RATIO = 30.0
MAX_LEVELS = 20


class Level:
    pass


def hierarchy(torch, capi, rows, tp, tc, tv, floor, s, mis2=False):
    """The levels from the device CSR arrays down to <= floor rows: every level's matrix and, but for the last, its plan.  mis2: the
    aggregates of spmv_hip_agg_aggregate_mis2, and spmv_hip_agg_group(plan) lanes per aggregate in the level's restriction."""
    dev = tp.device
    i32, f64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float64, device=dev)
    levels, n = [], rows
    while True:
        L = Level()
        L.n, L.nnz, L.tp, L.tc, L.tv, L.plan, L.group = n, int(tp[-1]), tp, tc, tv, None, 1
        levels.append(L)
        if n <= floor or len(levels) >= MAX_LEVELS:
            break
        nnz = L.nnz
        work = torch.zeros(max(capi.agg_workspace_bytes(n, nnz), capi.agg_mis2_workspace_bytes(n) if mis2 else 0) // 8, **f64)
        L.agg, status = torch.zeros(n, **i32), torch.zeros(4, **i32)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if mis2:
            capi.agg_aggregate_mis2(n, tp, tc, tv, 0.0, 0, L.agg, status, work, capi.agg_mis2_workspace_bytes(n), s)
        else:
            capi.agg_aggregate(n, tp, tc, tv, 0.0, 0, L.agg, status, work, capi.agg_workspace_bytes(n), s)
        t1 = time.perf_counter()
        st = status.cpu().numpy().tolist()
        aggregates = st[0]
        L.mptr, L.member = torch.zeros(aggregates + 1, **i32), torch.zeros(n, **i32)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        L.plan = capi.agg_plan(n, L.agg, status, L.mptr, L.member, work, capi.agg_workspace_bytes(n), s)
        t3 = time.perf_counter()
        L.group = capi.agg_group(L.plan) if mis2 else 1
        cp, cc, order, eptr = torch.zeros(aggregates + 1, **i32), torch.zeros(max(1, nnz), **i32), torch.zeros(max(1, nnz), **i32), torch.zeros(nnz + 1, **i32)
        cstatus = torch.zeros(1, **i32)
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        capi.agg_galerkin_symbolic(L.plan, nnz, tp, tc, cp, cc, order, eptr, cstatus, work, None, s)
        t5 = time.perf_counter()
        nnz_c = int(cstatus.cpu()[0])
        cv = torch.zeros(max(1, nnz_c), **f64)
        capi.agg_galerkin_numeric(nnz, nnz_c, order, eptr, tv, cv, s)
        torch.cuda.synchronize()
        t6 = time.perf_counter()
        L.status = st
        L.seconds = {"aggregate": round(t1 - t0, 4), "plan": round(t3 - t2, 4), "symbolic": round(t5 - t4, 4), "numeric": round(t6 - t5, 4)}
        del work, order, eptr
        if aggregates >= n:
            break  # no row found a neighbour: nothing below this level
        tp, tc, tv, n = cp, cc[:max(1, nnz_c)], cv, aggregates
    return levels


def transfer(torch, capi, L, rounds, s):
    """Restriction and prolongation on one level against torch and beside the triad, in both types."""
    dev = L.agg.device
    n, na = L.n, L.plan.aggregates
    out = {}
    index = L.agg
    try:  # 32-bit indices where this torch takes them
        torch.zeros(na, dtype=torch.float64, device=dev).index_add_(0, index, torch.zeros(n, dtype=torch.float64, device=dev))
        torch.zeros(n, dtype=torch.float64, device=dev).add_(torch.zeros(na, dtype=torch.float64, device=dev)[index], alpha=1.0)
    except (IndexError, TypeError, RuntimeError):
        index = index.long()
    for name, dtype, size in (("f64", torch.float64, 8), ("f32", torch.float32, 4)):
        gen = torch.Generator(device=dev)
        gen.manual_seed(9)
        r = torch.rand(n, generator=gen, dtype=dtype, device=dev) * 2 - 1
        e = torch.rand(na, generator=gen, dtype=dtype, device=dev) * 2 - 1
        x, rc = torch.zeros(n, dtype=dtype, device=dev), torch.zeros(na, dtype=dtype, device=dev)
        a, b, c = (torch.ones(n, dtype=dtype, device=dev) for _ in range(3))
        kept = {}

        def torch_restrict():
            kept["rc"] = torch.zeros(na, dtype=dtype, device=dev).index_add_(0, index, r)

        ways = {"restrict": lambda: capi.agg_restrict(L.plan, r, rc, s),
                "torch_index_add": torch_restrict,
                "prolong_add": lambda: capi.agg_prolong_add(L.plan, 1e-3, e, x, s),
                "torch_add_gather": lambda: x.add_(e[index], alpha=1e-3),
                "triad": (lambda: capi.triad(n, a.data_ptr(), b.data_ptr(), c.data_ptr(), 3.1, s)) if size == 8 else (lambda: torch.add(b, c, alpha=3.1, out=a))}
        rcg = torch.zeros(na, dtype=dtype, device=dev)
        if L.group > 1:
            ways["restrict_group"] = lambda: capi.agg_restrict_group(L.plan, L.group, r, rcg, s)
        med = alternate(torch, ways, rounds)
        close = float((kept["rc"].double() - rc.double()).abs().max()) if na else 0.0
        bytes_ = {"restrict": n * (4 + size) + na * (4 + size), "prolong_add": n * (4 + 2 * size) + na * size, "triad": 3 * n * size}
        per_byte = med["triad"] / bytes_["triad"]
        out[name] = {"us": {k: round(v, 2) for k, v in med.items()}, "bytes": bytes_,
                     "restrict_over_torch": round(med["restrict"] / med["torch_index_add"], 3),
                     "prolong_over_torch": round(med["prolong_add"] / med["torch_add_gather"], 3),
                     "restrict_over_triad_by_bytes": round(med["restrict"] / bytes_["restrict"] / per_byte, 3),
                     "prolong_over_triad_by_bytes": round(med["prolong_add"] / bytes_["prolong_add"] / per_byte, 3),
                     "restrict_GBps": round(bytes_["restrict"] / med["restrict"] / 1e3, 1),
                     "prolong_GBps": round(bytes_["prolong_add"] / med["prolong_add"] / 1e3, 1),
                     "triad_GBps": round(bytes_["triad"] / med["triad"] / 1e3, 1),
                     "triad_is": "capi.triad" if size == 8 else "torch.add(b, c, alpha=s, out=a)",
                     "index_dtype": str(index.dtype), "restrict_against_index_add_max_abs": close}
        if L.group > 1:
            # the target of DESIGN 3.23: the time of the counted bytes at the triad's rate, times 1.16
            ratio = med["restrict_group"] / bytes_["restrict"] / per_byte
            out[name].update({"group": L.group, "restrict_group_over_restrict": round(med["restrict_group"] / med["restrict"], 3),
                              "restrict_group_over_triad_by_bytes": round(ratio, 3), "restrict_group_GBps": round(bytes_["restrict"] / med["restrict_group"] / 1e3, 1),
                              "restrict_group_target_1.16": "met" if ratio <= 1.16 else "missed",
                              "restrict_target_1.16": "met" if med["restrict"] / bytes_["restrict"] / per_byte <= 1.16 else "missed",
                              "restrict_group_against_restrict_max_abs": float((rcg.double() - rc.double()).abs().max()) if na else 0.0})
    return out


def library_inverse(torch, capi, L, s):
    """(inv, status, work) of spmv_hip_coarse_setup_f64 on the level's device arrays; only enqueued."""
    dev = L.tp.device
    inv = torch.zeros(max(1, L.n * capi.coarse_ld(L.n)), dtype=torch.float64, device=dev)
    status = torch.zeros(3, dtype=torch.int32, device=dev)
    work = torch.zeros(capi.coarse_workspace_bytes(L.n) // 8, dtype=torch.float64, device=dev)
    capi.coarse_setup(L.n, L.tp, L.tc, L.tv, inv, status, work, None, s)
    return inv, status, work


def dense_of(torch, L):
    """The level's matrix as a dense device tensor, formed on the host."""
    import scipy.sparse as sp
    p_h, c_h, v_h = L.tp.cpu().numpy(), L.tc.cpu().numpy()[:L.nnz], L.tv.cpu().numpy()[:L.nnz]
    return torch.from_numpy(sp.csr_matrix((v_h, c_h, p_h), shape=(L.n, L.n)).toarray()).to(L.tp.device)


def coarse_ab(torch, capi, L, rounds, s):
    """The dense solve of the coarsest level by the library and by torch, alternating: the set-up from the level's device CSR arrays
    against torch.linalg.inv of the dense matrix (formed on the host beforehand, outside the timing), the apply against
    torch.matmul(inverse, r, out=z)."""
    n, dev = L.n, L.tp.device
    dense = dense_of(torch, L)
    inv, status, work = library_inverse(torch, capi, L, s)
    gen = torch.Generator(device=dev)
    gen.manual_seed(9)
    r = torch.rand(n, generator=gen, dtype=torch.float64, device=dev) * 2 - 1
    z, zt = torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.float64, device=dev)
    kept = {}

    def torch_inv():
        kept["inverse"] = torch.linalg.inv(dense)

    setup = alternate(torch, {"library": lambda: capi.coarse_setup(n, L.tp, L.tc, L.tv, inv, status, work, None, s), "torch": torch_inv}, rounds)
    apply = alternate(torch, {"library": lambda: capi.coarse_apply(n, inv, r, z, s),
                              "torch": lambda: torch.matmul(kept["inverse"], r, out=zt)}, rounds)
    eye = torch.eye(n, dtype=torch.float64, device=dev)
    mine = inv.view(n, capi.coarse_ld(n))[:, :n]
    return {"rows": n, "launches_of_setup": 2 * n + 3, "status": status.cpu().numpy().tolist(),
            "setup_ms": {k: round(v / 1e3, 4) for k, v in setup.items()}, "apply_us": {k: round(v, 2) for k, v in apply.items()},
            "setup_library_over_torch": round(setup["library"] / setup["torch"], 3), "apply_library_over_torch": round(apply["library"] / apply["torch"], 3),
            "max_abs_AX_minus_I": {"library": float((dense @ mine - eye).abs().max()), "torch": float((dense @ kept["inverse"] - eye).abs().max())},
            "z_max_abs_difference": float((z - zt).abs().max()), "z_max_abs": float(zt.abs().max())}


def plans_ab(torch, capi, levels, s, rounds=5):
    """Per level with a C16Plan in the cycle: what a set-up pays for its plan today -- row_ptr and the columns copied to the host,
    then spmv_hip_c16_plan_csr -- against C16Plan.from_device on the arrays where they are; one warm-up, then `rounds` rounds
    alternating the two, wall clock around a synchronised stream, medians.  The plans are compared by their 20 numbers.  Under
    SPMV_HIP_EXPERIMENTS=1 the library waits between the stages of the device call and reports them."""
    out = []
    for L in levels:
        n = L.n
        times = {"host_copy": [], "host_plan": [], "device": []}
        stages = []
        for rnd in range(rounds + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            p_h, c_h = L.tp.cpu().numpy(), np.ascontiguousarray(L.tc.cpu().numpy()[:L.nnz])
            t1 = time.perf_counter()
            host = capi.C16Plan(n, n, p_h, c_h, 0, s)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            dev = capi.C16Plan.from_device(n, n, L.tp, L.tc, 0, s)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            assert host.info() == dev.info() and dev.verify(L.tc.data_ptr(), s) == 0
            info = dev.info()
            host.close()
            dev.close()
            if rnd > 0:
                times["host_copy"].append(t1 - t0)
                times["host_plan"].append(t2 - t1)
                times["device"].append(t3 - t2)
                st = capi.c16_plan_device_times()
                if st is not None:
                    stages.append(st)
        med = {k: float(np.median(v)) for k, v in times.items()}
        g = {"rows": n, "stored_entries": L.nnz, "tiles": info["tiles"], "wide_tiles": info["wide_tiles"], "ms": {k: round(1e3 * v, 3) for k, v in med.items()},
             "host_ms": round(1e3 * float(np.median(np.array(times["host_copy"]) + np.array(times["host_plan"]))), 3)}
        g["device_over_host"] = round(g["ms"]["device"] / g["host_ms"], 3) if g["host_ms"] > 0 else None
        if stages:
            g["device_stage_ms"] = dict(zip(("row_ptr_copy", "tile_cut", "windows_kernel", "codes_kernel", "rest"),
                                            (round(1e3 * float(v), 3) for v in np.median(np.array(stages), axis=0))))
        out.append(g)
    return out


def prepare_cycle(torch, capi, levels, dense_limit, coarse_degree, s, coarse="torch", plans="host"):
    """Per level: a C16Plan (plans == "device": by C16Plan.from_device, no column copied to the host), minv, the degree-2 table over [lambda / 4, lambda] and the cycle's vectors.  The last level is solved by
    its dense inverse where it has at most dense_limit rows, else by a FIXED Chebyshev polynomial of coarse_degree over [lambda /
    RATIO, lambda] (a fixed symmetric operator, so CG stays valid; not a solve).  coarse == "library": the inverse by
    spmv_hip_coarse_setup_f64 beside torch's (the level has at most SPMV_HIP_COARSE_MAX_N rows, or this raises); L.way says which
    of the two the cycle applies."""
    dev = levels[0].tp.device
    i32, f64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float64, device=dev)
    for k, L in enumerate(levels):
        n = L.n
        L.r, L.z = torch.zeros(n, **f64), torch.zeros(n, **f64)
        L.inverse, L.way = None, "torch"
        if k == len(levels) - 1 and n <= dense_limit:
            L.inverse = torch.linalg.inv(dense_of(torch, L))
            if coarse == "library":
                L.inv, L.inv_status, L.inv_work = library_inverse(torch, capi, L, s)
            continue
        if plans == "device":
            L.c16 = capi.C16Plan.from_device(n, n, L.tp, L.tc, 0, s)
        else:  # whose columns go through the host
            p_h, c_h = L.tp.cpu().numpy(), np.ascontiguousarray(L.tc.cpu().numpy()[:L.nnz])
            L.c16 = capi.C16Plan(n, n, p_h, c_h, 0, s)
        L.P, L.C, L.A = L.tp.data_ptr(), L.tc.data_ptr(), L.tv.data_ptr()
        L.minv, L.ones = torch.zeros(n, **f64), torch.ones(n, **f64)
        L.bstatus = torch.zeros(2, **i32)
        capi.bjacobi_setup(n, 1, L.tp, L.tc, L.tv, L.minv, L.bstatus, s)
        L.lam, L.table, L.coarse_table = torch.zeros(1, **f64), torch.zeros(4, **f64), torch.zeros(2 * coarse_degree, **f64)
        capi.cheby_bound(n, L.tp, L.tv, L.minv, L.lam, s)
        capi.cheby_coeffs(2, L.lam, 1.0, 4.0, L.table, s)
        capi.cheby_coeffs(coarse_degree, L.lam, 1.0, RATIO, L.coarse_table, s)
        L.t, L.u, L.d, L.cz = (torch.zeros(n, **f64) for _ in range(4))
    torch.cuda.synchronize()


def v_cycle(torch, capi, levels, omega, coarse_degree, s):
    """src -> z of the finest level."""

    def polynomial(L, degree, table, rhs, z):
        for j in range(degree):
            if j > 0:
                L.c16.spmv_f64_scaled(L.P, L.C, L.A, z.data_ptr(), -1.0, 1.0, rhs.data_ptr(), L.u.data_ptr(), s)
            capi.cheby_step(L.n, degree, j, table, rhs if j == 0 else L.u, L.minv, L.d, z, None, None, None, None, s)

    def cycle(k, r, z):
        L = levels[k]
        if k == len(levels) - 1:
            if L.way == "library":
                capi.coarse_apply(L.n, L.inv, r, z, s)
            elif L.inverse is not None:
                torch.matmul(L.inverse, r, out=z)
            else:
                polynomial(L, coarse_degree, L.coarse_table, r, z)
            return
        below = levels[k + 1]
        polynomial(L, 2, L.table, r, z)
        L.c16.spmv_f64_scaled(L.P, L.C, L.A, z.data_ptr(), -1.0, 1.0, r.data_ptr(), L.t.data_ptr(), s)
        if L.group > 1:
            capi.agg_restrict_group(L.plan, L.group, L.t, below.r, s)
        else:
            capi.agg_restrict(L.plan, L.t, below.r, s)
        cycle(k + 1, below.r, below.z)
        capi.agg_prolong_add(L.plan, omega, below.z, z, s)
        L.c16.spmv_f64_scaled(L.P, L.C, L.A, z.data_ptr(), -1.0, 1.0, r.data_ptr(), L.t.data_ptr(), s)
        polynomial(L, 2, L.table, L.t, L.cz)
        capi.bjacobi_apply_add(L.n, 1, L.ones, L.cz, z, s)

    return lambda src, z: cycle(0, src, z)


def pcg(torch, capi, levels, rhs, cap, look, coarse_degree, s, omegas=(1.0, 1.5), baselines=True, coarse_ways=("torch",)):
    top = levels[0]
    n, dev = top.n, rhs.device
    f64 = dict(dtype=torch.float64, device=dev)
    c16, P, C, A, minv = top.c16, top.P, top.C, top.A, top.minv
    x, r, pv, q, z, d, u = (torch.zeros(n, **f64) for _ in range(7))
    lam, table = torch.zeros(1, **f64), torch.zeros(6, **f64)
    rz, pq, rr = [torch.ones(2, **f64) for _ in range(2)], torch.ones(2, **f64), torch.ones(2, **f64)
    start = torch.tensor([0.0, 1.0], **f64)
    mbytes, kbytes = c16.dots_workspace_bytes(), capi.krylov_workspace_bytes(n)
    mwork, kwork = torch.zeros(mbytes // 8, **f64), torch.zeros(kbytes // 8, **f64)
    capi.cheby_bound(n, top.tp, top.tv, minv, lam, s)
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

    def cycle_at(omega, way):
        run = v_cycle(torch, capi, levels, omega, coarse_degree, s)

        def apply(src, dots):
            levels[-1].way = way
            run(src, z)
            dots[0:1].copy_(torch.dot(src, z).reshape(1))

        return apply

    out = {}
    ways = ([("diagonal", diagonal), ("chebyshev_3", chebyshev)] if baselines else []) \
        + [("v_cycle_omega_%.1f%s" % (w, "" if coarse_ways == ("torch",) else "_" + way), cycle_at(w, way)) for w in omegas for way in coarse_ways]
    for way, apply in ways:
        x.zero_()
        r.copy_(rhs)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        apply(r, rz[0])
        capi.cg_direction(n, start, start.data_ptr() + 8, z, None, pv, s)
        first = float(torch.dot(r, r))
        it, now = 0, first
        step = look if way.startswith("v_cycle") else 25
        limit = min(cap, 2000) if way.startswith("v_cycle") else cap
        while it < limit and 1e-12 * first < now < 1e6 * first:
            for _ in range(step):
                old, new = rz[it % 2], rz[1 - it % 2]
                c16.spmv_f64_scaled_dots(P, C, A, pv.data_ptr(), 1.0, 0.0, None, q.data_ptr(), pv.data_ptr(), pq.data_ptr(), mwork.data_ptr(),
                                         mbytes, s)
                capi.cg_step(n, old, pq.data_ptr() + 8, pv, q, x, r, None, rr, kwork, None, s)
                apply(r, new)
                capi.cg_direction(n, new, old, z, None, pv, s)
                it += 1
            now = float(rr.cpu()[0])
        torch.cuda.synchronize()
        out[way] = {"iterations": it, "seconds": round(time.perf_counter() - t0, 4), "relative_rr": now / first, "reached": bool(now <= 1e-12 * first),
                    "looked_every": step}
    return out


def solve_with(torch, capi, levels, res, rows, cap, look, floor, stall, dense_limit, coarse_degree, s, omegas=(1.0, 1.5), baselines=True,
               coarse="torch", plans="host"):
    """PCG with the V-cycle over `levels` into res: the cycle's levels, its set-up and res["pcg"]."""
    # the cycle's levels: down to the floor, or to the first level that the aggregation shrinks by less than --stall
    depth = 0
    while depth + 1 < len(levels) and levels[depth].n > floor and levels[depth].n >= stall * levels[depth + 1].n:
        depth += 1
    used = levels[:depth + 1]
    if depth == 0:
        return
    t0 = time.perf_counter()
    prepare_cycle(torch, capi, used, dense_limit, coarse_degree, s, coarse, plans)
    res["plans"] = plans
    res["cycle_setup_seconds"] = round(time.perf_counter() - t0, 4)
    res["cycle_levels"] = [L.n for L in used]
    library = coarse == "library" and used[-1].inverse is not None
    res["coarsest"] = "the library's dense inverse and torch's, alternating" if library else "dense inverse" if used[-1].inverse is not None else "Chebyshev polynomial of degree %d over [lambda / %g, lambda]" % (coarse_degree, RATIO)
    gen = torch.Generator(device=levels[0].tp.device)
    gen.manual_seed(9)
    rhs = torch.rand(rows, generator=gen, dtype=torch.float64, device=levels[0].tp.device) * 2 - 1
    res["pcg"] = pcg(torch, capi, used, rhs, cap, look, coarse_degree, s, omegas, baselines, ("library", "torch") if library else ("torch",))
    for L in used:
        if L.inverse is None:
            L.c16.close()


def matrix(name, spec, rounds, cap, look, floor, stall, dense_limit, coarse_degree, solve, mis2=False, coarse="torch", plans="host"):
    import torch
    from spmv_amd import capi
    dev = torch.device("cuda:0")
    rows, cols, p_h, c_h, v_h = load(spec)
    assert rows == cols
    nnz = int(p_h[-1])
    s = torch.cuda.current_stream().cuda_stream
    res = {"matrix": name, "spec": spec, "rows": rows, "stored_entries": nnz, "rounds": rounds, "library": os.path.basename(capi.LIB_PATH),
           "aggregation": "distance 2" if mis2 else "distance 1"}
    tp, tc, tv = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (p_h, c_h, v_h))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    levels = hierarchy(torch, capi, rows, tp, tc, tv, floor, s, mis2)
    res["hierarchy_seconds"] = round(time.perf_counter() - t0, 4)
    res["levels"] = [{"rows": L.n, "stored_entries": L.nnz, "status": getattr(L, "status", None), "seconds": getattr(L, "seconds", None),
                      "group": L.group} for L in levels]
    res["operator_complexity"] = round(sum(L.nnz for L in levels) / max(1, nnz), 3)
    res["setup_seconds"] = {k: round(sum(L.seconds[k] for L in levels if L.plan is not None), 4) for k in ("aggregate", "plan", "symbolic", "numeric")}
    if coarse == "library":
        res["coarse"] = coarse_ab(torch, capi, levels[-1], rounds, s)
    elif levels[0].plan is not None:
        res["transfer"] = transfer(torch, capi, levels[0], rounds, s)
    if plans == "both":
        res["plans_ab"] = plans_ab(torch, capi, [L for L in levels if L.plan is not None], s)
    if solve and len(levels) > 1:
        omegas = (1.0, 1.5, 2.0) if mis2 else (1.0, 1.5)
        solve_with(torch, capi, levels, res, rows, cap, look, floor, stall, dense_limit, coarse_degree, s, omegas, coarse == "torch", coarse,
                   "device" if plans == "device" else "host")
        if plans == "both":
            # the same cycle once more over plans made on the device: the same bits, so the same iterations; without the baselines
            res["device_plans"] = {}
            solve_with(torch, capi, levels, res["device_plans"], rows, cap, look, floor, stall, dense_limit, coarse_degree, s, omegas, False, coarse,
                       "device")
        if mis2 and coarse == "torch" and plans == "host":
            # the distance-1 cycle of DESIGN 3.24 in the same process, its hierarchy and set-up timed the same way
            del levels
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            levels = hierarchy(torch, capi, rows, tp, tc, tv, floor, s, False)
            one = {"hierarchy_seconds": round(time.perf_counter() - t0, 4)}
            solve_with(torch, capi, levels, one, rows, cap, look, floor, stall, dense_limit, coarse_degree, s, (1.0, 1.5), False)
            res["distance_1"] = one
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--cap", type=int, default=20000, help="the largest number of PCG iterations")
    ap.add_argument("--look", type=int, default=5, help="V-cycle PCG iterations between two looks at r'r on the host")
    ap.add_argument("--floor", type=int, default=1000, help="the hierarchy ends at the first level of at most this many rows")
    ap.add_argument("--stall", type=float, default=1.5, help="the cycle ends at the first level that the aggregation shrinks by less than this")
    ap.add_argument("--dense-limit", type=int, default=12000, help="the largest coarsest level that is solved by its dense inverse")
    ap.add_argument("--coarse-degree", type=int, default=16, help="the degree of the polynomial that stands for the solve on a larger coarsest level")
    ap.add_argument("--only", nargs="*", default=None, help="matrix names")
    ap.add_argument("--no-pcg", action="store_true")
    ap.add_argument("--mis2", action="store_true", help="the distance-2 aggregates and the grouped restriction of spmv_hip_agg_mis2.h; the log "
                    "goes to profiles/agg_mis2_ab.log")
    ap.add_argument("--coarse", choices=("torch", "library"), default="torch", help="who solves the coarsest level: torch.linalg.inv and torch's "
                    "matrix-vector product, or spmv_hip_coarse_setup_f64 and spmv_hip_coarse_apply_f64 beside them; the log goes to profiles/coarse_ab.log")
    ap.add_argument("--plans", choices=("host", "device", "both"), default="host", help="who makes the cycle's C16Plans: spmv_hip_c16_plan_csr from "
                    "arrays copied to the host (the default: every recorded figure as it was), spmv_hip_c16_plan_csr_device from the arrays where they "
                    "are, or both: per level the two set-ups alternating, then the PCG with each kind of plan; the log goes to "
                    "profiles/c16_device_plan_ab.log")
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    log = open(args.log or os.path.join(ROOT, "profiles", "c16_device_plan_ab.log" if args.plans != "host" else "coarse_ab.log" if args.coarse == "library" else "agg_mis2_ab.log" if args.mis2 else "agg_ab.log"), "w")

    def say(text):
        print(text, flush=True)
        log.write(text + "\n")
        log.flush()

    say("plain aggregation (theta 0, seed 0%s) down to <= %d rows; restriction and prolongation against torch and beside the triad; one process, torch "
        "events on one stream, 3 warm-up rounds, then %d rounds alternating the ways, medians" % (
            ", distance-2 roots, spmv_hip_agg_group(plan) lanes per aggregate in the grouped restriction" if args.mis2 else "", args.floor, args.rounds))
    if args.coarse == "library":
        say("--coarse library: the coarsest level by spmv_hip_coarse_setup_f64 and spmv_hip_coarse_apply_f64 against torch.linalg.inv and torch.matmul, "
            "alternating, in place of the transfers; PCG with each, without the baselines and the distance-1 cycle")
    for name, spec, what, spd in MATRICES:
        if args.only and name not in args.only:
            continue
        res = matrix(name, spec, args.rounds, args.cap, args.look, args.floor, args.stall, args.dense_limit, args.coarse_degree, spd and not args.no_pcg,
                     args.mis2, args.coarse, args.plans)
        say("%-13s %s: %d rows, %d stored entries; %s" % (name, what, res["rows"], res["stored_entries"], res["library"]))
        say("    rows per level %s; operator complexity %.3f" % (" -> ".join(str(L["rows"]) for L in res["levels"]), res["operator_complexity"]))
        for k, L in enumerate(res["levels"]):
            if L["status"] is not None:
                st, sec = L["status"], L["seconds"]
                say("    level %2d: %9d rows, %10d entries -> %9d aggregates in %2d rounds, largest %d, %d singletons; aggregate %.4f s, plan %.4f s, "
                    "symbolic %.4f s, numeric %.4f s%s" % (k, L["rows"], L["stored_entries"], st[0], st[1], st[2], st[3], sec["aggregate"], sec["plan"],
                                                           sec["symbolic"], sec["numeric"], "; group %d" % L["group"] if args.mis2 else ""))
        say("    setup, all levels: aggregate %.4f s, plan %.4f s, symbolic %.4f s, numeric %.4f s; the hierarchy with its allocations %.4f s" % (
            res["setup_seconds"]["aggregate"], res["setup_seconds"]["plan"], res["setup_seconds"]["symbolic"], res["setup_seconds"]["numeric"],
            res["hierarchy_seconds"]))
        for t, g in res.get("transfer", {}).items():
            u = g["us"]
            say("    %s: restrict %7.1f us (%.1f GB/s) / index_add_ %7.1f us = %.3f, by bytes beside the triad %.3f; prolong_add %7.1f us (%.1f GB/s) / "
                "add_(e[agg]) %7.1f us = %.3f, by bytes beside the triad %.3f; triad %7.1f us (%.1f GB/s, %s); %s indices" % (
                    t, u["restrict"], g["restrict_GBps"], u["torch_index_add"], g["restrict_over_torch"], g["restrict_over_triad_by_bytes"],
                    u["prolong_add"], g["prolong_GBps"], u["torch_add_gather"], g["prolong_over_torch"], g["prolong_over_triad_by_bytes"], u["triad"],
                    g["triad_GBps"], g["triad_is"], g["index_dtype"]))
            if "group" in g:
                say("    %s: restrict_group at %d lanes %7.1f us (%.1f GB/s) / restrict = %.3f, by bytes beside the triad %.3f (target 1.16: %s; restrict "
                    "%.3f: %s); max |restrict_group - restrict| %.3e" % (
                        t, g["group"], u["restrict_group"], g["restrict_group_GBps"], g["restrict_group_over_restrict"], g["restrict_group_over_triad_by_bytes"],
                        g["restrict_group_target_1.16"], g["restrict_over_triad_by_bytes"], g["restrict_target_1.16"],
                        g["restrict_group_against_restrict_max_abs"]))
        if "coarse" in res:
            g = res["coarse"]
            say("    the coarsest level, %d rows: set-up (%d launches) %.3f ms / torch.linalg.inv %.3f ms = %.3f; apply %.1f us / torch.matmul %.1f us = "
                "%.3f; max |A X - I| %.3e against %.3e; max |z - z_torch| %.3e of max |z| %.3e; status %s" % (
                    g["rows"], g["launches_of_setup"], g["setup_ms"]["library"], g["setup_ms"]["torch"], g["setup_library_over_torch"],
                    g["apply_us"]["library"], g["apply_us"]["torch"], g["apply_library_over_torch"], g["max_abs_AX_minus_I"]["library"],
                    g["max_abs_AX_minus_I"]["torch"], g["z_max_abs_difference"], g["z_max_abs"], g["status"]))
        for k, g in enumerate(res.get("plans_ab", [])):
            say("    plan of level %2d: %9d rows, %10d entries, %7d tiles (%d wide): host %8.3f ms (copies %8.3f + plan %8.3f), device %8.3f ms = %.3f%s" % (
                k, g["rows"], g["stored_entries"], g["tiles"], g["wide_tiles"], g["host_ms"], g["ms"]["host_copy"], g["ms"]["host_plan"], g["ms"]["device"],
                g["device_over_host"], "; device stages, with a wait between them: " + ", ".join("%s %.3f" % kv for kv in g["device_stage_ms"].items())
                if "device_stage_ms" in g else ""))
        dp = res.get("device_plans")
        if dp and "pcg" in dp:
            say("    the same cycle over plans made on the device: its plans, smoothers and tables %.4f s (%.4f s with the host's plans)" % (
                dp["cycle_setup_seconds"], res["cycle_setup_seconds"]))
            setup = res["hierarchy_seconds"] + dp["cycle_setup_seconds"]
            for way, g in dp["pcg"].items():
                say("        pcg device plans %-18s %6d iterations, %8.4f s, with the set-up %8.4f s, r'r / r0'r0 %.3e%s" % (
                    way, g["iterations"], g["seconds"], g["seconds"] + setup, g["relative_rr"], "" if g["reached"] else " (not reached)"))
        if "pcg" in res:
            say("    the cycle's levels %s, the coarsest by %s; its plans, smoothers and tables: %.4f s" % (
                " -> ".join(str(n) for n in res["cycle_levels"]), res["coarsest"], res["cycle_setup_seconds"]))
            setup = res["hierarchy_seconds"] + res["cycle_setup_seconds"]
            for way, g in res["pcg"].items():
                extra = ", with the set-up %8.4f s" % (g["seconds"] + setup) if way.startswith("v_cycle") else ""
                say("        pcg %-18s %6d iterations, %8.4f s%s, r'r / r0'r0 %.3e%s" % (
                    way, g["iterations"], g["seconds"], extra, g["relative_rr"], "" if g["reached"] else " (not reached)"))
        one = res.get("distance_1")
        if one and "pcg" in one:
            say("    the distance-1 cycle in the same process: levels %s, the coarsest by %s; the hierarchy %.4f s, its plans, smoothers and tables "
                "%.4f s" % (" -> ".join(str(n) for n in one["cycle_levels"]), one["coarsest"], one["hierarchy_seconds"], one["cycle_setup_seconds"]))
            setup = one["hierarchy_seconds"] + one["cycle_setup_seconds"]
            for way, g in one["pcg"].items():
                say("        pcg distance-1 %-18s %6d iterations, %8.4f s, with the set-up %8.4f s, r'r / r0'r0 %.3e%s" % (
                    way, g["iterations"], g["seconds"], g["seconds"] + setup, g["relative_rr"], "" if g["reached"] else " (not reached)"))
        say(json.dumps(res))
    log.close()


if __name__ == "__main__":
    main()
