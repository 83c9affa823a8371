#!/usr/bin/env python3
"""The scaled multiplies with dots (include/spmv_hip_dots.h) against what a Krylov caller had to do without them, for all four
float-tile multiplies -- f32, c16, c16_f64 and c16_f32xy -- at Level 2, in ONE process, torch events on one stream, on the
matrices of tools/scaled_ab.py:

    q = A p, p' q       the overwrite form (alpha 1, beta 0) + torch.dot(x, y)     against   the fused call with w = x
    r = b - A x, r' r   the residual form (alpha -1, beta 1, y_in = b) + torch.dot(r, r)     against   the fused call with w null

Per matrix and multiply: three warm-up rounds, then --rounds rounds alternating the two ways and the scaled sibling alone; the
medians, fused / two-step, the ratio the byte counts promise, and fused / sibling alone (the price of the epilogue and the
reduction).  y_out of the fused call is compared bit for bit with the sibling's before anything is timed, and its dots with
torch's.  The log goes to stdout and to profiles/dots_ab.log (--log).

    python tools/dots_ab.py
    python tools/dots_ab.py --only poisson webbase --rounds 25
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spmv-cache-trace_amd", "python"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from compact_ab import MATRICES, load  # noqa: E402
from scaled_ab import alternate  # noqa: E402


def measure(name, spec, rounds):
    import torch
    from spmv_amd import capi, synth
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    rows, cols, p, c, v = load(spec)
    nnz = int(p[-1])
    tp, tc, tv = (torch.from_numpy(a).to(dev) for a in (p, c, v))
    tf = torch.zeros(max(1, nnz), dtype=torch.float32, device=dev)
    capi.narrow_values(nnz, tv.data_ptr(), tf.data_ptr(), stream)
    x64 = torch.from_numpy(synth.x_vector(cols)).to(dev)
    b64 = torch.from_numpy(np.random.default_rng(4).uniform(-1.0, 1.0, size=rows)).to(dev)
    f32 = capi.F32Plan(rows, cols, p, 0, stream)
    c16 = capi.C16Plan(rows, cols, p, c, 0, stream)
    ci, fi = c16.info(), f32.info()
    P, C = tp.data_ptr(), tc.data_ptr()
    # per multiply: (scaled call, fused call, its plan, value array, vector dtype, bytes one accumulating launch streams, tiles)
    kinds = {
        "f32": (f32.spmv_scaled, f32.spmv_scaled_dots, f32, tf, torch.float64, fi["streamed_bytes"], fi["tiles"]),
        "c16": (c16.spmv_scaled, c16.spmv_scaled_dots, c16, tf, torch.float64, ci["streamed_bytes"], ci["tiles"]),
        "c16_f64": (c16.spmv_f64_scaled, c16.spmv_f64_scaled_dots, c16, tv, torch.float64,
                    ci["streamed_bytes"] + 4 * nnz if ci["streamed_bytes"] else 0, ci["tiles"]),
        "c16_f32xy": (c16.spmv_f32xy_scaled, c16.spmv_f32xy_scaled_dots, c16, tf, torch.float32,
                      ci["streamed_bytes"] - 8 * rows - 4 * cols if ci["streamed_bytes"] else 0, ci["tiles"]),
    }
    res = {"matrix": name, "spec": spec, "rows": rows, "cols": cols, "stored_entries": nnz, "rounds": rounds,
           "library": os.path.basename(capi.LIB_PATH), "multiplies": {}}
    for k, (scaled, fused, plan, vals, dtype, streamed, tiles) in kinds.items():
        es = 8 if dtype == torch.float64 else 4
        x, b = x64.to(dtype), b64.to(dtype)
        y, r = torch.zeros(rows, dtype=dtype, device=dev), torch.zeros(rows, dtype=dtype, device=dev)
        nbytes = plan.dots_workspace_bytes()
        dots = torch.zeros(2, dtype=torch.float64, device=dev)
        work = torch.zeros(nbytes // 8, dtype=torch.float64, device=dev)
        A, X, Y, B, R, D, W = vals.data_ptr(), x.data_ptr(), y.data_ptr(), b.data_ptr(), r.data_ptr(), dots.data_ptr(), work.data_ptr()
        square = rows == cols
        got = {}

        def q_two_step():
            scaled(P, C, A, X, 1.0, 0.0, None, Y, stream)
            got["q"] = torch.dot(x, y) if square else torch.dot(y, y)

        def q_fused():
            fused(P, C, A, X, 1.0, 0.0, None, Y, X if square else None, D, W, nbytes, stream)

        def r_two_step():
            scaled(P, C, A, X, -1.0, 1.0, B, R, stream)
            got["r"] = torch.dot(r, r)

        def r_fused():
            fused(P, C, A, X, -1.0, 1.0, B, R, None, D, W, nbytes, stream)

        q_two_step()
        want = y.clone()
        y.fill_(float("nan"))
        q_fused()
        torch.cuda.synchronize()
        same = bool(torch.equal(y, want))
        ref = float(torch.dot(x.double(), y.double())) if square else float(torch.dot(y.double(), y.double()))
        rel = abs(float(dots[1 if square else 0]) - ref) / max(abs(ref), 1e-300)
        q = alternate(torch, {"two_step": q_two_step, "fused": q_fused, "scaled_alone": lambda: scaled(P, C, A, X, 1.0, 0.0, None, Y, stream)}, rounds)
        rr = alternate(torch, {"two_step": r_two_step, "fused": r_fused, "scaled_alone": lambda: scaled(P, C, A, X, -1.0, 1.0, B, R, stream)}, rounds)
        slots = 2 * 16 * max(tiles, 1)
        q_bytes, r_bytes = streamed - es * rows, streamed  # the overwrite form does not read y
        res["multiplies"][k] = {
            "streamed_bytes": streamed, "workspace_bytes": nbytes, "y_bits_equal_the_sibling": same, "dot_relative_difference_to_torch": rel,
            "q_us": {a: round(t, 2) for a, t in q.items()}, "q_ratio": round(q["fused"] / q["two_step"], 3),
            "q_ratio_by_bytes": round((q_bytes + (es * rows if square else 0) + slots) / max(1, q_bytes + 2 * es * rows), 3),
            "q_fused_over_scaled_alone": round(q["fused"] / q["scaled_alone"], 3),
            "r_us": {a: round(t, 2) for a, t in rr.items()}, "r_ratio": round(rr["fused"] / rr["two_step"], 3),
            "r_ratio_by_bytes": round((r_bytes + slots) / max(1, r_bytes + es * rows), 3),
            "r_fused_over_scaled_alone": round(rr["fused"] / rr["scaled_alone"], 3),
        }
        del x, b, y, r, want, dots, work
    c16.close()
    f32.close()
    del tp, tc, tv, tf, x64, b64
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--only", nargs="*", help="names among: " + ", ".join(m[0] for m in MATRICES))
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "dots_ab.log"))
    args = ap.parse_args()
    log = open(args.log, "a")

    def say(text):
        print(text, flush=True)
        log.write(text + "\n")
        log.flush()

    say("q = A p with p' q: the overwrite form + torch.dot against the fused call (w = x; y' y where the matrix is not square);  "
        "r = b - A x with r' r: the residual form + torch.dot against the fused call (w null);  one process, torch events on one "
        "stream, 3 warm-up rounds, then %d rounds alternating two-step, fused and the scaled sibling alone, medians" % args.rounds)
    for name, spec, what in MATRICES:
        if args.only and name not in args.only:
            continue
        res = measure(name, spec, args.rounds)
        say("%-14s %s: %d x %d, %d stored entries; %s" % (name, what, res["rows"], res["cols"], res["stored_entries"], res["library"]))
        for k, m in res["multiplies"].items():
            say("    %-9s q: two-step %9.2f us, fused %9.2f us, ratio %.3f (by bytes %.3f), fused / scaled alone %.3f;   "
                "r: two-step %9.2f us, fused %9.2f us, ratio %.3f (by bytes %.3f), fused / scaled alone %.3f;   same y bits: %s, dot "
                "against torch %.1e" % (
                    k, m["q_us"]["two_step"], m["q_us"]["fused"], m["q_ratio"], m["q_ratio_by_bytes"], m["q_fused_over_scaled_alone"],
                    m["r_us"]["two_step"], m["r_us"]["fused"], m["r_ratio"], m["r_ratio_by_bytes"], m["r_fused_over_scaled_alone"],
                    m["y_bits_equal_the_sibling"], m["dot_relative_difference_to_torch"]))
        say(json.dumps(res))
    log.close()


if __name__ == "__main__":
    main()
