#!/usr/bin/env python3
"""The CSR multiply over fp32-stored values (include/spmv_hip_f32values.h) against the library's default fp64 plan, ONE PROCESS
PER MATRIX (the parent starts a fresh child for each), torch tensors, interleaved rounds after a warm-up:

    f32     spmv_hip_csr_spmv_f32 over the float values (8 bytes per stored entry)
    fp64    spmv_hip_csr_spmv with the plan spmv_hip_upload_csr builds (tiles, block confirmation, compression, panels, dictionary)

Per matrix: microseconds per multiply (median and min over the rounds, each round the mean of --reps back-to-back launches),
their ratio, both plans' streamed bytes from their plan_info and the byte ratio, each launch's streamed bytes / time as a share
of the STREAM triad timed in the same process, how many values the narrowing changed and by how much, and the largest
difference against the default plan run on A~ (the values widened back to double) in units of (|A~||x|)_i.  The log goes to
stdout and to profiles/f32values_ab.log.

    python tools/f32values_ab.py
    python tools/f32values_ab.py --only delaunay_1dof --rounds 25 --reps 1
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
    ("delaunay_1dof", "delaunay:2000000,1,2,rcm", "Delaunay 3-D mesh, scalar, RCM order: the gate of tests/test_gpu_f32values.py"),
    ("delaunay_3dof", "delaunay:250000,3,1,rcm", "Delaunay 3-D mesh, 3 unknowns per node, RCM order"),
    ("poisson", "synthetic:poisson2d:4096", "5-point Poisson 4096^2"),
    ("webbase", "synthetic:webbase", "webbase-1M-like graph"),
]


def load(spec):
    from spmv_amd import hostapi, synth
    if spec.startswith("delaunay:"):
        q = spec[9:].split(",")
        rows, cols, p, c, v = synth.delaunay_mesh(int(q[0]), int(q[1]), seed=int(q[2]), order=q[3])
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
    inexact, rel = capi.narrow_values(nnz, tv.data_ptr(), tf.data_ptr(), stream)
    tw = tf[:nnz].double()  # A~'s values: what the default plan multiplies for the comparison of the results
    tx = torch.from_numpy(synth.x_vector(cols)).to(dev)
    f32 = capi.F32Plan(rows, cols, p, 0, stream)
    plan = default_plan(capi, rows, cols, p, tp, tc, tv, stream)
    plan_t = default_plan(capi, rows, cols, p, tp, tc, tw, stream)
    torch.cuda.synchronize()

    # one multiply each into y = 0: f32 against the default plan on A~, scaled by (|A~||x|)_i
    ya = torch.zeros(rows, dtype=torch.float64, device=dev)
    yb = torch.zeros(rows, dtype=torch.float64, device=dev)
    f32.spmv(tp.data_ptr(), tc.data_ptr(), tf.data_ptr(), tx.data_ptr(), ya.data_ptr(), stream)
    plan_t.spmv(tp.data_ptr(), tc.data_ptr(), tw.data_ptr(), tx.data_ptr(), yb.data_ptr(), stream)
    torch.cuda.synchronize()
    lens = (tp[1:] - tp[:-1]).long()
    scale = torch.zeros(rows, dtype=torch.float64, device=dev).index_add_(
        0, torch.repeat_interleave(torch.arange(rows, device=dev), lens), tw.abs() * tx[tc.long()].abs())
    diff = float(torch.max(torch.abs(ya - yb) / torch.clamp(scale, min=1e-300)).item()) if rows and nnz else 0.0
    plan_t.close()
    del ya, yb, scale, tw, lens

    ways = {
        "f32": lambda y: f32.spmv(tp.data_ptr(), tc.data_ptr(), tf.data_ptr(), tx.data_ptr(), y, stream),
        "fp64": lambda y: plan.spmv(tp.data_ptr(), tc.data_ptr(), tv.data_ptr(), tx.data_ptr(), y, stream),
    }
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
    fi, di = f32.info(), plan.info()
    med = {k: float(np.median(t)) for k, t in times.items()}
    res = {
        "matrix": name, "spec": spec, "rows": rows, "cols": cols, "stored_entries": nnz, "load_s": round(load_s, 1),
        "triad_gbs": round(triad, 1),
        "us": {k: {"median": round(med[k], 2), "min": round(float(np.min(t)), 2)} for k, t in times.items()},
        "ratio_f32_over_fp64": round(med["f32"] / med["fp64"], 3),
        "streamed_bytes": {"f32": fi["streamed_bytes"], "fp64": di["streamed_bytes"]},
        "byte_ratio": round(fi["streamed_bytes"] / max(1, di["streamed_bytes"]), 3),
        "share_of_triad": {"f32": round(fi["streamed_bytes"] / (med["f32"] * 1e-6) / 1e9 / triad, 3),
                           "fp64": round(di["streamed_bytes"] / (med["fp64"] * 1e-6) / 1e9 / triad, 3)},
        "values_inexact": inexact, "max_value_rounding": rel,
        "f32_vs_fp64_on_rounded_values_max_scaled_diff": diff,
        "f32_plan": fi,
        "fp64_plan": {k: di[k] for k in ("narrow_tiles", "shifted_tiles", "xwin_tiles", "blockwin_tiles", "panel_tiles", "indexed_values",
                                         "segwin_tiles", "block_tiles", "group_tiles", "masked_block_tiles", "stencil_mask_tiles", "run_tiles")},
    }
    f32.close()
    plan.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", nargs="*", help="names among: " + ", ".join(m[0] for m in MATRICES))
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "f32values_ab.log"))
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

    say("f32 = spmv_hip_csr_spmv_f32 (values stored as floats); fp64 = spmv_hip_csr_spmv with the default plan; one process per "
        "matrix (rounds %d, reps %d)" % (args.rounds, args.reps))
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
        say("%-14s %s: %d x %d, %d stored entries; triad %.0f GB/s" % (name, what, res["rows"], res["cols"], res["stored_entries"], res["triad_gbs"]))
        say("    f32  median %9.2f us  min %9.2f us   streams %12d bytes   %.2f of triad" % (us["f32"]["median"], us["f32"]["min"], sb["f32"], sh["f32"]))
        say("    fp64 median %9.2f us  min %9.2f us   streams %12d bytes   %.2f of triad" % (us["fp64"]["median"], us["fp64"]["min"], sb["fp64"], sh["fp64"]))
        say("    f32 / fp64 (median) %.3f; by bytes %.3f;  %d values inexact as floats (largest relative change %.3g);  "
            "max |f32 - fp64 on rounded values| / (|A~||x|)_i = %.2e" % (
                res["ratio_f32_over_fp64"], res["byte_ratio"], res["values_inexact"], res["max_value_rounding"],
                res["f32_vs_fp64_on_rounded_values_max_scaled_diff"]))
        say(json.dumps(res))
    log.close()


if __name__ == "__main__":
    main()
