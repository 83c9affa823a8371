#!/usr/bin/env python3
"""The scaled multiplies (include/spmv_hip_scaled.h: y_out <- alpha A x + beta y_in) against what a caller had to do without
them, for all four float-tile multiplies -- f32 (spmv_hip_csr_spmv_f32), c16, c16_f64 and c16_f32xy (the C16Plan's three) -- at
Level 2, in ONE process, torch events on one stream, on the matrices of tools/compact_ab.py:

    q = A p        memset of y + the existing multiply (two launches)     against   the overwrite form (alpha 1, beta 0, y_in null)
    r = b - A x    the existing multiply y += A x (the same bytes; what a   against   the residual form (alpha -1, beta 1, y_in = b,
                   caller adds around it -- a copy of b, a negation -- is            y_out = r: out of place)
                   NOT timed)

Per matrix and multiply: three warm-up rounds, then --rounds rounds alternating the two ways, one launch (or memset + launch)
between two events each; the medians, their ratio, and for q = A p the ratio the plan's byte counts promise.  The overwrite form's
result is compared bit for bit with memset + multiply before anything is timed.  The log goes to stdout and to
profiles/scaled_ab.log (--log).

    python tools/scaled_ab.py
    python tools/scaled_ab.py --only poisson webbase --rounds 25
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

WARM = 3


def alternate(torch, ways, rounds):
    times = {k: [] for k in ways}
    for rnd in range(WARM + rounds):
        for k, run in ways.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            e1.synchronize()
            if rnd >= WARM:
                times[k].append(e0.elapsed_time(e1) * 1e3)
    return {k: float(np.median(t)) for k, t in times.items()}


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
    # per multiply: (existing call, scaled call, value array, vector dtype, bytes one existing launch streams)
    kinds = {
        "f32": (f32.spmv, f32.spmv_scaled, tf, torch.float64, fi["streamed_bytes"]),
        "c16": (c16.spmv, c16.spmv_scaled, tf, torch.float64, ci["streamed_bytes"]),
        "c16_f64": (c16.spmv_f64, c16.spmv_f64_scaled, tv, torch.float64, ci["streamed_bytes"] + 4 * nnz if ci["streamed_bytes"] else 0),
        "c16_f32xy": (c16.spmv_f32xy, c16.spmv_f32xy_scaled, tf, torch.float32, ci["streamed_bytes"] - 8 * rows - 4 * cols if ci["streamed_bytes"] else 0),
    }
    res = {"matrix": name, "spec": spec, "rows": rows, "cols": cols, "stored_entries": nnz, "rounds": rounds,
           "library": os.path.basename(capi.LIB_PATH), "compact_share": round(ci["compact_entries"] / max(1, nnz), 4), "multiplies": {}}
    for k, (old, new, vals, dtype, streamed) in kinds.items():
        es = 8 if dtype == torch.float64 else 4
        x, b = x64.to(dtype), b64.to(dtype)
        y, r = torch.zeros(rows, dtype=dtype, device=dev), torch.zeros(rows, dtype=dtype, device=dev)
        A, X, Y, B, R = vals.data_ptr(), x.data_ptr(), y.data_ptr(), b.data_ptr(), r.data_ptr()

        def memset_and_multiply():
            y.zero_()
            old(P, C, A, X, Y, stream)

        def overwrite():
            new(P, C, A, X, 1.0, 0.0, None, Y, stream)

        memset_and_multiply()
        want = y.clone()
        y.fill_(float("nan"))
        overwrite()
        torch.cuda.synchronize()
        same = bool(torch.equal(y, want))
        q = alternate(torch, {"memset_and_multiply": memset_and_multiply, "overwrite": overwrite}, rounds)
        rr = alternate(torch, {"multiply": lambda: old(P, C, A, X, Y, stream),
                               "residual": lambda: new(P, C, A, X, -1.0, 1.0, B, R, stream)}, rounds)
        res["multiplies"][k] = {
            "streamed_bytes": streamed, "overwrite_bits_equal_memset_and_multiply": same,
            "q_us": {a: round(t, 2) for a, t in q.items()}, "q_ratio": round(q["overwrite"] / q["memset_and_multiply"], 3),
            "q_ratio_by_bytes": round((streamed - es * rows) / max(1, streamed + es * rows), 3),
            "r_us": {a: round(t, 2) for a, t in rr.items()}, "r_ratio": round(rr["residual"] / rr["multiply"], 3),
        }
        del x, b, y, r, want
    c16.close()
    f32.close()
    del tp, tc, tv, tf, x64, b64
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--only", nargs="*", help="names among: " + ", ".join(m[0] for m in MATRICES))
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "scaled_ab.log"))
    args = ap.parse_args()
    log = open(args.log, "a")

    def say(text):
        print(text, flush=True)
        log.write(text + "\n")
        log.flush()

    say("q = A p: memset of y + the existing multiply against the overwrite form (alpha 1, beta 0, y_in null);  r = b - A x: the "
        "existing multiply (y += A x) against the residual form (alpha -1, beta 1, out of place);  one process, torch events on one "
        "stream, %d warm-up rounds, then %d rounds alternating the two ways, medians" % (WARM, args.rounds))
    for name, spec, what in MATRICES:
        if args.only and name not in args.only:
            continue
        res = measure(name, spec, args.rounds)
        say("%-14s %s: %d x %d, %d stored entries; compact tiles hold %.4f of them; %s" % (
            name, what, res["rows"], res["cols"], res["stored_entries"], res["compact_share"], res["library"]))
        for k, m in res["multiplies"].items():
            say("    %-9s q = A p: memset + multiply %9.2f us, overwrite %9.2f us, ratio %.3f (by bytes %.3f; same bits: %s);   "
                "r = b - A x: multiply %9.2f us, residual %9.2f us, ratio %.3f;   the multiply streams %d bytes" % (
                    k, m["q_us"]["memset_and_multiply"], m["q_us"]["overwrite"], m["q_ratio"], m["q_ratio_by_bytes"],
                    m["overwrite_bits_equal_memset_and_multiply"], m["r_us"]["multiply"], m["r_us"]["residual"], m["r_ratio"], m["streamed_bytes"]))
        say(json.dumps(res))
    log.close()


if __name__ == "__main__":
    main()
