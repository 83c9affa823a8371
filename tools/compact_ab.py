#!/usr/bin/env python3
"""The compact multiply (include/spmv_hip_compact.h: float values, 16-bit column codes, 6 bytes per stored entry) against the
fp32-value multiply (8 bytes) and the library's default fp64 plan, ONE PROCESS PER MATRIX (the parent starts a fresh child for
each), torch tensors, interleaved rounds after a warm-up, each round the median of --reps single launches:

    c16     spmv_hip_csr_spmv_c16
    f32     spmv_hip_csr_spmv_f32 over the same float values and 32-bit columns
    c16_f64 spmv_hip_csr_spmv_c16_f64 (include/spmv_hip_compact_f64.h): the c16 plan object over the fp64 values, 10 bytes per entry
    c16_f32xy spmv_hip_csr_spmv_c16_f32xy (include/spmv_hip_compact_f32xy.h): the c16 plan object and float values over float32 x and y
    fp64    spmv_hip_csr_spmv with the plan spmv_hip_upload_csr builds (tiles, block confirmation, compression, panels, dictionary)

Per matrix: microseconds per multiply (median and min over the rounds), the ratios, the three plans' streamed bytes from their
plan_info, each launch's streamed bytes / time as a share of the STREAM triad timed in the same process, the share of the
stored entries in compact tiles, the windows histogram, the host planning time in ms and whether c16 and f32 gave the same
bits (and c16_f64 the bits of fp64 is NOT expected: the default plan adds a row in another order).  The log goes to stdout and
to profiles/compact_ab.log (--log: the run that added c16_f64 went to profiles/compact_f64_ab.log, the one that added c16_f32xy
to profiles/compact_f32xy_ab.log).

    python tools/compact_ab.py
    python tools/compact_ab.py --only delaunay_1dof mesh_128 --rounds 25
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spmv-cache-trace_amd", "python"))

MATRICES = [
    ("queen", "synthetic:queen", "Queen_4147-like, both triangles (full size)"),
    ("queen_tril", "synthetic:queen:tril", "Queen_4147-like stored triangle"),
    ("kkt", "synthetic:kkt:200", "nlpkkt200-like, both triangles"),
    ("kkt_tril", "synthetic:kkt:200:tril", "nlpkkt200-like stored triangle"),
    ("delaunay_1dof", "delaunay:2000000,1,2,rcm", "Delaunay 3-D mesh, scalar, RCM order: a gate of tests/test_gpu_compact.py"),
    ("delaunay_3dof", "delaunay:250000,3,1,rcm", "Delaunay 3-D mesh, 3 unknowns per node, RCM order"),
    ("poisson", "synthetic:poisson2d:4096", "5-point Poisson 4096^2"),
    ("webbase", "synthetic:webbase", "webbase-1M-like graph"),
    ("mesh_128", "mesh_dofs:128,1", "27-neighbour mesh 128^3 with jittered links, scalar: the other gate"),
]


def load(spec):
    from spmv_amd import hostapi, synth
    if spec.startswith("delaunay:"):
        q = spec[9:].split(",")
        rows, cols, p, c, v = synth.delaunay_mesh(int(q[0]), int(q[1]), seed=int(q[2]), order=q[3])
    elif spec.startswith("mesh_dofs:"):
        q = spec[10:].split(",")
        rows, cols, p, c, v = synth.mesh_dofs((int(q[0]),) * 3, int(q[1]))
    else:
        H = hostapi.load(spec, "csr")
        rows, cols, p, c, v = H.rows, H.cols, np.array(H.row_ptr), np.array(H.column_index), np.array(H.value)
        H.close()
    return rows, cols, np.asarray(p, dtype=np.int32), np.asarray(c, dtype=np.int32), np.asarray(v, dtype=np.float64)


def default_plan(capi, rows, cols, host_p, tp, tc, tv, stream):
    """The plan spmv_hip_upload_csr builds (context.hip)."""
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


def measure(name, spec, rounds, reps):
    import torch
    from spmv_amd import capi, synth
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    triad = triad_gbs(torch, capi, dev, stream)
    t0 = time.time()
    rows, cols, p, c, v = load(spec)
    load_s = time.time() - t0
    nnz = int(p[-1])
    tp, tc, tv = (torch.from_numpy(a).to(dev) for a in (p, c, v))
    tf = torch.zeros(max(1, nnz), dtype=torch.float32, device=dev)
    capi.narrow_values(nnz, tv.data_ptr(), tf.data_ptr(), stream)
    tx = torch.from_numpy(synth.x_vector(cols)).to(dev)
    f32 = capi.F32Plan(rows, cols, p, 0, stream)
    t0 = time.time()
    c16 = capi.C16Plan(rows, cols, p, c, 0, stream)
    plan_ms = (time.time() - t0) * 1e3
    plan = default_plan(capi, rows, cols, p, tp, tc, tv, stream)
    mismatches = c16.verify(tc.data_ptr(), stream)
    torch.cuda.synchronize()

    # one multiply each into y = 0: the same tiles, lanes, products and sums, so the same bits
    ya = torch.zeros(rows, dtype=torch.float64, device=dev)
    yb = torch.zeros(rows, dtype=torch.float64, device=dev)
    c16.spmv(tp.data_ptr(), tc.data_ptr(), tf.data_ptr(), tx.data_ptr(), ya.data_ptr(), stream)
    f32.spmv(tp.data_ptr(), tc.data_ptr(), tf.data_ptr(), tx.data_ptr(), yb.data_ptr(), stream)
    torch.cuda.synchronize()
    same_bits = bool(torch.equal(ya.view(torch.int64), yb.view(torch.int64)))
    del ya, yb

    # float32 x and y of c16_f32xy: x narrowed once, a y of its own (y is the doubles' y: the other ways get its address)
    tx32 = tx.to(torch.float32)
    y32 = torch.zeros(rows, dtype=torch.float32, device=dev)
    ways = {
        "c16": lambda y: c16.spmv(tp.data_ptr(), tc.data_ptr(), tf.data_ptr(), tx.data_ptr(), y, stream),
        "f32": lambda y: f32.spmv(tp.data_ptr(), tc.data_ptr(), tf.data_ptr(), tx.data_ptr(), y, stream),
        "c16_f64": lambda y: c16.spmv_f64(tp.data_ptr(), tc.data_ptr(), tv.data_ptr(), tx.data_ptr(), y, stream),
        "c16_f32xy": lambda y: c16.spmv_f32xy(tp.data_ptr(), tc.data_ptr(), tf.data_ptr(), tx32.data_ptr(), y32.data_ptr(), stream),
        "fp64": lambda y: plan.spmv(tp.data_ptr(), tc.data_ptr(), tv.data_ptr(), tx.data_ptr(), y, stream),
    }
    y = torch.zeros(rows, dtype=torch.float64, device=dev)
    times = {k: [] for k in ways}
    for rnd in range(rounds + 1):  # round 0 warms up
        for k, run in ways.items():
            one = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(y.data_ptr())
                e1.record()
                torch.cuda.synchronize()
                one.append(e0.elapsed_time(e1) * 1e3)
            if rnd > 0:
                times[k].append(float(np.median(one)))
    ci, fi, di = c16.info(), f32.info(), plan.info()
    med = {k: float(np.median(t)) for k, t in times.items()}
    sb = {"c16": ci["streamed_bytes"], "f32": fi["streamed_bytes"], "fp64": di["streamed_bytes"],
          "c16_f64": ci["streamed_bytes"] + 4 * nnz if ci["streamed_bytes"] else 0,
          "c16_f32xy": ci["streamed_bytes"] - 8 * rows - 4 * cols if ci["streamed_bytes"] else 0}
    res = {
        "matrix": name, "spec": spec, "rows": rows, "cols": cols, "stored_entries": nnz, "load_s": round(load_s, 1),
        "library": os.path.basename(capi.LIB_PATH),
        "triad_gbs": round(triad, 1), "plan_ms": round(plan_ms, 1),
        "us": {k: {"median": round(med[k], 2), "min": round(float(np.min(t)), 2)} for k, t in times.items()},
        "ratio_c16_over_f32": round(med["c16"] / med["f32"], 3), "ratio_c16_over_fp64": round(med["c16"] / med["fp64"], 3),
        "ratio_c16_f64_over_fp64": round(med["c16_f64"] / med["fp64"], 3), "byte_ratio_c16_f64_over_fp64": round(sb["c16_f64"] / max(1, sb["fp64"]), 3),
        "ratio_c16_f32xy_over_c16": round(med["c16_f32xy"] / med["c16"], 3), "byte_ratio_c16_f32xy_over_c16": round(sb["c16_f32xy"] / max(1, sb["c16"]), 3),
        "streamed_bytes": {k: sb[k] for k in ways},
        "byte_ratio_c16_over_f32": round(sb["c16"] / max(1, sb["f32"]), 3), "byte_ratio_c16_over_fp64": round(sb["c16"] / max(1, sb["fp64"]), 3),
        "share_of_triad": {k: round(sb[k] / (med[k] * 1e-6) / 1e9 / triad, 3) for k in ways},
        "compact_share": round(ci["compact_entries"] / max(1, nnz), 4), "compact_tiles": ci["compact_tiles"], "wide_tiles": ci["wide_tiles"],
        "windows_1_to_8": [ci["tiles_with_%d_windows" % w] for w in range(1, 9)],
        "verify_mismatches": mismatches, "c16_bits_equal_f32": same_bits,
    }
    c16.close()
    f32.close()
    plan.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", nargs="*", help="names among: " + ", ".join(m[0] for m in MATRICES))
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "compact_ab.log"))
    ap.add_argument("--child", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:  # one matrix in this process: the result as one JSON line
        name, spec, _ = next(m for m in MATRICES if m[0] == args.child)
        print("RESULT " + json.dumps(measure(name, spec, args.rounds, args.reps)), flush=True)
        return

    log = open(args.log, "a")

    def say(text):
        print(text, flush=True)
        log.write(text + "\n")
        log.flush()

    say("c16 = spmv_hip_csr_spmv_c16 (float values, 16-bit column codes); f32 = spmv_hip_csr_spmv_f32; c16_f64 = spmv_hip_csr_spmv_c16_f64 "
        "(fp64 values, the same codes); c16_f32xy = spmv_hip_csr_spmv_c16_f32xy (c16 over float32 x and y); fp64 = spmv_hip_csr_spmv with the default plan; one process per matrix (rounds %d, each the median of %d launches)" % (args.rounds, args.reps))
    for name, spec, what in MATRICES:
        if args.only and name not in args.only:
            continue
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--rounds", str(args.rounds), "--reps", str(args.reps)],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            say("%-14s %s: FAILED (exit status %d)\n%s" % (name, what, r.returncode, r.stderr[-2000:]))
            if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
                say("stopping: nothing more is started on the device after a fault")
                break
            continue
        res = json.loads(line[0][7:])
        us, sb, sh = res["us"], res["streamed_bytes"], res["share_of_triad"]
        say("%-14s %s: %d x %d, %d stored entries; triad %.0f GB/s; %s" % (
            name, what, res["rows"], res["cols"], res["stored_entries"], res["triad_gbs"], res["library"]))
        for k in us:
            say("    %-9s median %9.2f us  min %9.2f us   streams %12d bytes   %.2f of triad" % (k, us[k]["median"], us[k]["min"], sb[k], sh[k]))
        say("    c16_f64 / fp64 (median) %.3f, by bytes %.3f" % (res["ratio_c16_f64_over_fp64"], res["byte_ratio_c16_f64_over_fp64"]))
        say("    c16_f32xy / c16 (median) %.3f, by bytes %.3f" % (res["ratio_c16_f32xy_over_c16"], res["byte_ratio_c16_f32xy_over_c16"]))
        say("    c16 / f32 (median) %.3f, by bytes %.3f;  c16 / fp64 %.3f, by bytes %.3f;  compact tiles hold %.4f of the entries "
            "(%d compact, %d wide; windows 1..8: %r);  planned on the host in %.0f ms;  verify: %d mismatches;  c16 bits == f32 bits: %s" % (
                res["ratio_c16_over_f32"], res["byte_ratio_c16_over_f32"], res["ratio_c16_over_fp64"], res["byte_ratio_c16_over_fp64"],
                res["compact_share"], res["compact_tiles"], res["wide_tiles"], res["windows_1_to_8"], res["plan_ms"],
                res["verify_mismatches"], res["c16_bits_equal_f32"]))
        say(json.dumps(res))
    log.close()


if __name__ == "__main__":
    main()
