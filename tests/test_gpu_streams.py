"""Every Level-2 entry point works on the CALLER'S stream: ordered on it, asynchronous where the header says so, usable from two
streams at once, and capturable into a graph -- the scaled forms of the float-tile multiplies (include/spmv_hip_scaled.h)
included; their capture, a linear graph of an overwrite and an alpha == 0 call, is test_gpu_scaled.py's.

The rest of the suite hands the library the null stream, which every blocking stream orders itself against: a kernel, copy or
memset that escaped to another stream could not be seen there.  Here the stream `s` is NON-BLOCKING (asserted through
hipStreamGetFlags), so nothing orders it against the null stream, and every call is made behind a DELAY: D in-place passes of
plain torch work over a 256 MiB tensor, enqueued on `s`, calibrated to about 50 ms -- the host needs tens of microseconds to
enqueue a multiply.  The protocol of a delayed call (stream_helpers.delayed):

  1. every device operand is allocated and filled with contents that are WRONG BUT SAFE: x, the values and y_in NaN, the device
     row_ptr zeros (every row empty), the columns and row indices zeros (in range), y the guard bit pattern;
  2. torch.cuda.synchronize();
  3. on `s`: the delay, the copies that bring the real contents (from staging tensors already on the device), the library call,
     a copy of the result; then `s` is synchronised.

An operation of the library that escapes `s` runs during the delay: it sees an empty all-NaN matrix, or what it writes is
overwritten when the real y0 arrives, and the result is wrong.  Because the wrong contents are in range, an escape can never
fault -- it can only fail an assertion.  Two conditions keep a case from passing vacuously, and a case that cannot meet them
fails: s.query() is False immediately before the call (the delay is still running), and, for the calls documented as
asynchronous, still False when the call returns (which also pins that a multiply does not synchronise).

References: the oracle within the family's own tolerance, and -- where no partial sums meet in atomics (every family but symv,
spmv_t, coo_spmv and the column-panel plan; rows of up to 512 entries: test_gpu_nonfinite.SURE) -- bit for bit the same plan's
result on the null stream with everything synchronised.  y's guards come back bitwise unchanged.

Section 2 puts the DEVICE INPUTS OF THE PLANNING STEPS in place behind the delay.  That can show an operation that escapes
before a step's first own synchronisation of `s`; a race that begins after it (a null-stream read-back of what a kernel on `s`
wrote) is not widened by the delay -- there the code is right by reading: every such read-back is made on `s` (plan_csr.hip:
read_back)."""
import numpy as np
import pytest

import compact_cases as cc
import helpers
import stream_helpers as sh
import test_gpu_nonfinite as nf
from spmv_amd import capi, synth
from stream_helpers import delayed, on_stream, serial
from test_gpu_scaled import restate

pytestmark = pytest.mark.gpu

RUNS = 3


def _torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def side():
    s = sh.Side()
    yield s
    s.report()


def test_the_side_streams_are_non_blocking_and_the_delay_is_calibrated(side):
    assert side.s.cuda_stream != side.s2.cuda_stream
    for s in side.streams:
        assert sh.stream_flags(s) & sh.HIP_STREAM_NON_BLOCKING
    assert side.passes >= 1 and 0.5 * sh.DELAY_MS <= side.delay_ms <= 1.5 * sh.DELAY_CAP_MS, (side.passes, side.pass_ms, side.delay_ms)
    # the null stream does not wait for the side stream: work enqueued on it behind a delay is still pending after a null-stream sync
    t = _torch()
    with t.cuda.stream(side.s):
        side.delay()
    t.cuda.default_stream().synchronize()
    assert not side.s.query()
    side.s.synchronize()


# ---- 1. every multiply, ordered on the caller's stream and asynchronous -------------------------------------------------------------

def _ordered(side, case, runs=1):
    call = case.planner()
    x, y = case.vectors()
    want = serial(call, x, y, runs)  # (the plan's warm-up multiply as well: the first-multiply content check is out of the way)
    (got,), _ = delayed(side, case.mats + [x, y], lambda st: [call(st, x.ptr, y.ptr) for _ in range(runs)], [y], case.what)
    case.check(got, x, y, runs, want, "%s, %d run(s) behind the delay" % (case.what, runs))
    return call, x, y


@pytest.mark.parametrize("name", list(nf.DEFAULT_CASES))
def test_default_plan_spmv_and_spmv_out(oracle, side, name):
    case = sh.default_case(oracle, name)
    _, x, y = _ordered(side, case, RUNS)  # three accumulating runs back to back behind one delay
    # y_out = y_in + A x into a NaN-filled output; y_in comes back as it was
    plan, (P, C, V) = case.plan, (m.ptr for m in case.mats)
    y_in, out = sh.operand(y.host), sh.result(np.full(y.shape, np.nan))
    call = lambda st, xp, yp: plan.spmv_out(P, C, V, xp, y_in.ptr, yp, st)
    want = serial(call, x, out, 1)
    what = case.what + ", spmv_out"
    (got, kept), _ = delayed(side, case.mats + [x, y_in, out], lambda st: call(st, x.ptr, out.ptr), [out, y_in], what)
    helpers.assert_bitexact(kept, y.host, what + ": y_in changed")
    case.check(got, x, y, 1, want, what)
    case.close()


@pytest.mark.parametrize("name", list(nf.SYMV_CASES))
def test_symv(oracle, side, name):
    case = sh.symv_case(oracle, name)
    _ordered(side, case)
    case.close()


@pytest.mark.parametrize("name", list(nf.SPMV_T_CASES))
def test_spmv_t(oracle, side, name):
    case = sh.spmv_t_case(oracle, name)
    _ordered(side, case)
    case.close()


@pytest.mark.parametrize("flags", [0, capi.FLAG_EXACT_ORDER])
@pytest.mark.parametrize("k", [3, 5])
def test_spmm(oracle, side, k, flags):
    case = sh.spmm_case(oracle, k, flags)
    _ordered(side, case)
    case.close()


@pytest.mark.parametrize("family", sh.FLOAT_FAMILIES)
def test_float_value_families(oracle, side, family):
    case = sh.float_family_case(oracle, family)
    _ordered(side, case)
    case.close()


@pytest.mark.parametrize("kind", sh.SCALED_KINDS)
def test_scaled_float_value_families(oracle, side, kind):
    """y_out <- alpha A x + beta y_in (include/spmv_hip_scaled.h), every call behind the delay with every operand -- y_in
    included -- wrong but safe until the copies behind the delay arrive: the residual form out of place (y_in comes back
    unchanged), the overwrite form with y_in null, alpha == 0 (scaled_rows_only_kernel alone) and, on a plan without entries,
    alpha == 1 (that kernel with the alpha * +0.0 term).  Each asynchronous, bit for bit the same plan's serial null-stream
    result, and within the family's rule of the restatement on the oracle's row sums: helpers.assert_close for double vectors;
    the float pair is the bits of spmv_hip_csr_spmv_c16_scaled through the same plan on the widened operands, rounded to float
    once, and that fp64 result is what assert_close judges."""
    t = _torch()
    case = sh.scaled_family_case(oracle, kind)
    case.planner()
    floats = case.xy == np.float32
    x, y = case.vectors()
    y_in, out = sh.operand(y.host), sh.result(np.full(y.shape, np.nan, dtype=case.xy))
    z, absz = case.row_sums(x.host)
    if floats:
        x64, y_in64, out64 = sh.operand(x.host.astype(np.float64)), sh.operand(y.host.astype(np.float64)), sh.result(np.full(y.shape, np.nan))

    def serially(scaled, xa, yi, yo, alpha, beta):
        for a in (xa, yi, yo):
            a.put()
        t.cuda.synchronize()
        scaled(0, xa.ptr, alpha, beta, yi.ptr if beta != 0.0 else 0, yo.ptr)
        t.cuda.synchronize()
        return yo.body(what="serial run")

    for alpha, beta in ((-1.0, 1.0), (1.0, 0.0), (0.0, 0.5)):
        what = "%s, alpha %g, beta %g" % (case.what, alpha, beta)
        want = serially(case.scaled, x, y_in, out, alpha, beta)
        call = lambda st: case.scaled(st, x.ptr, alpha, beta, y_in.ptr if beta != 0.0 else 0, out.ptr)
        (got, kept), _ = delayed(side, case.mats + [x, y_in, out], call, [out, y_in], what)
        sh.assert_rows_bitwise(kept, y.host, None, what + ": y_in changed")
        sh.assert_rows_bitwise(got, want, None, what + " behind the delay")
        y64 = got
        if floats:
            y64 = serially(case.scaled_c16, x64, y_in64, out64, alpha, beta)
            sh.assert_rows_bitwise(got, y64.astype(np.float32), None, what + ": against spmv_hip_csr_spmv_c16_scaled through the same plan, rounded once")
        ref = restate(alpha, beta, z, y.host, np.float64)
        helpers.assert_close(y64, ref, abs(alpha) * absz + abs(beta) * np.abs(y.host.astype(np.float64)), what=what + " against the restatement",
                             nterms=case.nterms)
    case.close()
    # a plan without entries: no tile, the rows-only kernel with its alpha * +0.0 term, behind the delay
    rows, cols, p, c, v = cc.matrix("no_entries")
    plan = capi.F32Plan(rows, cols, p, 0, 0) if kind == "f32" else capi.C16Plan(rows, cols, p, c, 0, 0)
    assert plan.info()["tiles"] == 0
    scaled = {"f32": plan.spmv_scaled, "c16": plan.spmv_scaled, "c16_f64": getattr(plan, "spmv_f64_scaled", None),
              "c16_f32xy": getattr(plan, "spmv_f32xy_scaled", None)}[kind]
    rng = np.random.default_rng(11)
    x0, b = sh.operand(rng.uniform(-1.0, 1.0, size=cols).astype(case.xy)), sh.operand(rng.uniform(-1.0, 1.0, size=rows).astype(case.xy))
    r = sh.result(np.full(rows, np.nan, dtype=case.xy))
    what = "spmv_%s_scaled on no_entries, alpha 1, beta -2.5" % kind
    (got, kept), _ = delayed(side, [x0, b, r], lambda st: scaled(0, 0, 0, x0.ptr, 1.0, -2.5, b.ptr, r.ptr, st), [r, b], what)
    sh.assert_rows_bitwise(kept, b.host, None, what + ": y_in changed")
    sh.assert_rows_bitwise(got, restate(1.0, -2.5, np.zeros(rows), b.host, case.xy), None, what + " against the restatement")
    plan.close()


def _small():
    return cc.matrix("rows_0_to_7_ragged_end")


def test_coo_spmv(oracle, side):
    rows, cols, p, c, v = _small()
    r = np.repeat(np.arange(rows, dtype=np.int32), np.diff(p))
    mats = [sh.index_array(r), sh.index_array(c), sh.value_array(v)]
    case = sh.Case("coo_spmv on rows_0_to_7_ragged_end", oracle, (rows, cols, p, c, v), mats, sure=False)  # atomics
    x, y = case.vectors()
    R, Cc, V = (m.ptr for m in mats)
    (got,), _ = delayed(side, mats + [x, y], lambda st: capi.coo_spmv(rows, len(v), R, Cc, V, x.ptr, y.ptr, st), [y], case.what)
    case.check(got, x, y, 1, None, case.what)


def test_ell_to_column_major_then_ell_spmv(oracle, side):
    rows, cols, p, c, v = _small()
    i, j, a = synth.csr_to_coordinate(rows, p, c, v)
    _, L, ec, ev = oracle.ell_from_coordinate(rows, i, j, a)
    assert L == 7
    what = "ell_to_column_major + ell_spmv on rows_0_to_7_ragged_end"
    rm = [sh.index_array(ec), sh.value_array(ev)]
    cm = [sh.index_array(np.zeros_like(ec)), sh.value_array(np.full(len(ev), np.nan))]  # outputs of the first call, inputs of the second
    x = sh.operand(synth.x_vector(cols, seed=3))
    y = sh.result(np.random.default_rng(7).uniform(-1.0, 1.0, size=rows))

    def both(st):
        capi.ell_to_column_major(rows, L, rm[0].ptr, rm[1].ptr, cm[0].ptr, cm[1].ptr, st)
        capi.ell_spmv(rows, L, cm[0].ptr, cm[1].ptr, x.ptr, y.ptr, st)

    x.put(), y.put()
    both(0)
    _torch().cuda.synchronize()
    want = y.body(what=what)
    (got, col_cm), _ = delayed(side, rm + cm + [x, y], both, [y, cm[0]], what)
    assert np.array_equal(col_cm.reshape(L, rows).T.ravel(), ec), what + ": the column-major copy"
    # rows of up to 16 entries are summed by one lane in the reference's order (helpers.assert_ell): bit for bit the oracle
    helpers.assert_bitexact(got, oracle.ell_spmv(rows, L, ec, ev, x.host, y=y.host), what + " against the oracle")
    helpers.assert_bitexact(got, want, what + " against the serial result")


def test_triad(side):
    n = _small()[0]  # 10007: the pairs' launch and the launch for the odd last element
    assert n % 2 == 1
    rng = np.random.default_rng(n)
    b, c = sh.operand(rng.uniform(-1, 1, n)), sh.operand(rng.uniform(-1, 1, n))
    a = sh.result(np.full(n, 7.0))
    (got,), _ = delayed(side, [a, b, c], lambda st: capi.triad(n, a.ptr, b.ptr, c.ptr, 3.1, st), [a], "triad")
    helpers.assert_bitexact(got, b.host + 3.1 * c.host, "triad behind the delay (multiply, then add)")


# ---- 2. planning steps ordered on the caller's stream -------------------------------------------------------------------------------

PLANNING_CASES = ["stencil run chunks, grid with a hole", "masked stencil tiles, 7-point 60^3 with holes", "constant-row tiles", "block tiles",
                  "group tiles, 2 per node", "segment windows", "column panels"]


@pytest.mark.parametrize("name", PLANNING_CASES)
def test_default_plan_chain_behind_the_delay(oracle, side, name):
    """confirm_blocks, compress, repack, index_values, refresh_values, verify: each with its device inputs arriving behind the
    delay.  Every number of plan_info is that of the same chain on the null stream, the plan reaches its class, and a multiply
    gives that plan's bits."""
    case = sh.default_case(oracle, name)
    (rows, cols, p, c, v), flags, index_values, reached = sh.default_matrix(name)
    P, C, V = (m.ptr for m in case.mats)
    plans = []
    for on_side in (False, True):
        plan = capi.CsrPlan(rows, cols, p, capi.CSR_AUTO, 0, flags)
        case.plans.append(plan)
        plans.append(plan)
        if on_side:
            sh.default_chain(plan, case.mats, index_values,
                             step=lambda step, fn: delayed(side, case.mats, fn, [], "%s, %s" % (case.what, step), asynchronous=False))
        else:
            sh.default_chain(plan, case.mats, index_values)
            _torch().cuda.synchronize()
    want_info, info = plans[0].info(), plans[1].info()
    print("%s: plan_info %s" % (case.what, {k: n for k, n in nf._counts(info).items() if n}))
    assert info == want_info, {k: (info[k], want_info[k]) for k in info if info[k] != want_info[k]}
    assert reached(info), nf._counts(info)
    if info["panel_tiles"] > 0:
        case.sure = None
    x, y = case.vectors()
    results = [serial(lambda st, xp, yp: plan.spmv(P, C, V, xp, yp, st), x, y, RUNS) for plan in plans]
    case.check(results[1], x, y, RUNS, results[0], case.what + ": a multiply of the plan made behind the delay")
    case.close()


@pytest.mark.parametrize("family", ["sym_plan_csr", "tr_plan_csr"])
def test_plans_that_read_the_device_columns_back(oracle, side, family):
    case = sh.symv_case(oracle, next(iter(nf.SYMV_CASES))) if family == "sym_plan_csr" else sh.spmv_t_case(oracle, next(iter(nf.SPMV_T_CASES)))
    case.planner()
    want_info = case.info
    _, call = delayed(side, case.mats, lambda st: case.planner(st), [], case.what + ", the plan behind the delay", asynchronous=False)
    assert case.info == want_info, (case.info, want_info)
    x, y = case.vectors()
    case.check(serial(call, x, y, 1), x, y, 1, None, case.what + ": a multiply of the plan made behind the delay")
    case.close()


def test_c16_plan_verify(oracle, side):
    rows, cols, p, c, v = cc.matrix("mixed_mesh_and_graph")
    col = sh.index_array(c)
    what = "c16_plan_verify on mixed_mesh_and_graph"
    with capi.C16Plan(rows, cols, p, c, 0, 0) as plan0:
        want_info = plan0.info()
        assert plan0.verify(col.ptr, 0) == 0
    _, plan = delayed(side, [col], lambda st: capi.C16Plan(rows, cols, p, c, 0, st), [], what + ", the plan", asynchronous=False)
    assert plan.info() == want_info
    assert want_info["compact_tiles"] > 100
    _, mismatches = delayed(side, [col], lambda st: plan.verify(col.ptr, st), [], what, asynchronous=False)
    assert mismatches == 0, "%s: %d entries decode to another column (verify read the columns before they were in place)" % (what, mismatches)
    plan.close()


def test_coo_sort_by_row(side):
    rows, cols, p, c, v = _small()
    i, j, a = synth.csr_to_coordinate(rows, p, c, v)
    order = np.lexsort((i, j))  # column-major order
    r, cj, vv = (i[order] - 1).astype(np.int32), (j[order] - 1).astype(np.int32), a[order]
    arrays = [sh.index_array(r), sh.index_array(cj), sh.value_array(vv)]
    delayed(side, arrays, lambda st: capi.coo_sort_by_row(rows, len(vv), arrays[0].ptr, arrays[1].ptr, arrays[2].ptr, st), [], "coo_sort_by_row",
            asynchronous=False)
    stable = np.argsort(r, kind="stable")
    sr, sc, sv = (m.body() for m in arrays)
    assert np.array_equal(sr, r[stable]) and np.array_equal(sc, cj[stable]), "coo_sort_by_row behind the delay: the indices"
    helpers.assert_bitexact(sv, vv[stable], "coo_sort_by_row behind the delay: the values")


def test_narrow_values(side):
    v = _small()[4] * (1.0 + 2.0 ** -30)
    f_host, inexact_host, rel_host = capi.narrow_values_host(v)
    assert inexact_host > 0
    src = sh.value_array(v)
    dst = sh.Arr(np.zeros(len(v), dtype=np.float32), sh.nan_bits(np.float32))
    _, (inexact, rel) = delayed(side, [src], lambda st: capi.narrow_values(len(v), src.ptr, dst.ptr, st), [], "narrow_values", asynchronous=False)
    assert (inexact, rel) == (inexact_host, rel_host)
    assert np.array_equal(dst.body().view(np.uint32), f_host.view(np.uint32))


# ---- 3. two streams at once ----------------------------------------------------------------------------------------------------------

def _two_streams(side, case, shared):
    """Three accumulating multiplies per stream, enqueued alternately from this thread behind a delay on either stream, each stream
    with its own x, y0 and y: one plan for both, or a plan each.  Every stream's result is its serial one."""
    t = _torch()
    calls = [case.planner()]
    calls.append(calls[0] if shared else case.planner())
    vecs = [case.vectors(seed=q) for q in (1, 2)]
    want = [serial(call, x, y, RUNS) for call, (x, y) in zip(calls, vecs)]  # (each plan's warm-up as well)
    what = "%s, %s on two streams" % (case.what, "one plan" if shared else "two plans")
    for x, y in vecs:
        x.wrong()
        y.wrong()
    t.cuda.synchronize()
    for q, (s, (x, y)) in enumerate(zip(side.streams, vecs)):
        with t.cuda.stream(s):
            side.delay(q)
            x.put()
            y.put()
    assert not side.s.query() and not side.s2.query(), what + ": a delay was over before the calls"
    for _ in range(RUNS):
        for s, call, (x, y) in zip(side.streams, calls, vecs):
            call(s.cuda_stream, x.ptr, y.ptr)
    assert not side.s.query() and not side.s2.query(), what + ": a call waited for its stream"
    snaps = []
    for s, (x, y) in zip(side.streams, vecs):
        with t.cuda.stream(s):
            snaps.append(y.snap())
    for s in side.streams:
        s.synchronize()
    for q, ((x, y), snap) in enumerate(zip(vecs, snaps)):
        case.check(y.body(snap, what), x, y, RUNS, want[q], "%s, stream %d" % (what, q))
    case.close()


TWO_STREAM_CASES = {
    "default plan, stencil run chunks (the sweep counter)": lambda o: sh.default_case(o, "stencil run chunks, grid with a hole"),
    "default plan, long rows": lambda o: sh.default_case(o, "long rows"),
    "default plan, balanced tiles": lambda o: sh.default_case(o, "balanced tiles"),
    "default plan, constant-row tiles": lambda o: sh.default_case(o, "constant-row tiles"),
    "spmm k=5": lambda o: sh.spmm_case(o, 5),
    "spmv_c16": lambda o: sh.float_family_case(o, "spmv_c16"),
    "symv": lambda o: sh.symv_case(o, next(iter(nf.SYMV_CASES))),
    "spmv_t": lambda o: sh.spmv_t_case(o, next(iter(nf.SPMV_T_CASES))),
}
# the scaled forms: three residual steps y <- y - A x in place per stream
TWO_STREAM_CASES.update({"spmv_%s_scaled" % kind: (lambda o, kind=kind: sh.scaled_family_case(o, kind)) for kind in sh.SCALED_KINDS})


@pytest.mark.parametrize("shared", [False, True], ids=["a plan each", "one plan shared"])
@pytest.mark.parametrize("name", list(TWO_STREAM_CASES))
def test_two_streams_at_once(oracle, side, name, shared):
    _two_streams(side, TWO_STREAM_CASES[name](oracle), shared)


# ---- 4. captured into a graph and replayed ------------------------------------------------------------------------------------------

def _capture(s, call, x, y):
    """One multiply captured on `s`: a linear graph.  A multiply that synchronised or allocated would invalidate the capture."""
    t = _torch()
    g = t.cuda.CUDAGraph()
    with t.cuda.graph(g, stream=s):
        call(s.cuda_stream, x.ptr, y.ptr)
    return g


def _replays(s, g, x, y, runs, what):
    t = _torch()
    with t.cuda.stream(s):
        x.put()
        y.put()
        for _ in range(runs):
            g.replay()
        snap = y.snap()
    s.synchronize()
    return y.body(snap, what)


def _captured(side, case, call=None, x=None, y=None, accumulates=True):
    """Three replays from y0 are three eager multiplies from y0 (the first eager one is the plan's warm-up)."""
    call = call or case.planner()
    if x is None:
        x, y = case.vectors()
    eager = on_stream(side.s, call, x, y, RUNS)
    g = _capture(side.s, call, x, y)
    what = case.what + ", %d replays of the captured multiply" % RUNS
    got = _replays(side.s, g, x, y, RUNS, what)
    case.check(got, x, y, RUNS if accumulates else 1, eager, what)
    del g


@pytest.mark.parametrize("name", ["stencil run chunks, grid with a hole", "stencil run chunks, misaligned triple", "block windows",
                                  "constant-row tiles", "long rows"])
def test_default_plan_spmv_captured(oracle, side, name):
    case = sh.default_case(oracle, name)
    call = case.planner()
    if name.startswith("stencil run chunks"):
        assert case.info["run_variant"] & 4  # the eager runs alternate their sweep, the replays all sweep one way: the same bits
    _captured(side, case, call)
    case.close()


def test_default_plan_spmv_out_with_its_copy_captured(oracle, side):
    """Column panels: y_out = y_in first, a device-to-device copy inside the capture, then the panels accumulate in place."""
    case = sh.default_case(oracle, "column panels")
    case.planner()
    plan, (P, C, V) = case.plan, (m.ptr for m in case.mats)
    x, y = case.vectors()
    y_in, out = sh.operand(y.host), sh.result(np.full(y.shape, np.nan))
    out.host = y.host  # (what check() takes as y0)
    _captured(side, case, lambda st, xp, yp: plan.spmv_out(P, C, V, xp, y_in.ptr, yp, st), x, out, accumulates=False)
    helpers.assert_bitexact(y_in.body(), y.host, "spmv_out captured: y_in changed")
    case.close()


CAPTURED_FAMILIES = {
    "spmm k=5": lambda o: sh.spmm_case(o, 5),
    "spmv_f32": lambda o: sh.float_family_case(o, "spmv_f32"),
    "spmv_c16_f32xy": lambda o: sh.float_family_case(o, "spmv_c16_f32xy"),
    "symv": lambda o: sh.symv_case(o, next(iter(nf.SYMV_CASES))),
    "spmv_t": lambda o: sh.spmv_t_case(o, next(iter(nf.SPMV_T_CASES))),
}


@pytest.mark.parametrize("name", list(CAPTURED_FAMILIES))
def test_family_captured(oracle, side, name):
    case = CAPTURED_FAMILIES[name](oracle)
    _captured(side, case)
    case.close()


def test_the_content_check_is_left_pending_under_capture(oracle, side):
    """A fresh plan after compress, no warm-up: the capture leaves the first multiply's content check pending (it would have to
    synchronise), the replay is right, and the first EAGER multiply makes the check -- on a column array with two entries swapped
    it returns ERR_STATE and launches nothing."""
    name = "plain tiles, ragged ends"
    case = sh.default_case(oracle, name)
    (rows, cols, p, c, v), flags, _, _ = sh.default_matrix(name)
    P, C, V = (m.ptr for m in case.mats)
    plan = capi.CsrPlan(rows, cols, p, capi.CSR_AUTO, 0, flags)
    case.plans.append(plan)
    plan.compress(C, side.s.cuda_stream)
    assert plan.info()["narrow_tiles"] > 0
    call = lambda st, xp, yp: plan.spmv(P, C, V, xp, yp, st)
    x, y = case.vectors()
    g = _capture(side.s, call, x, y)
    got = _replays(side.s, g, x, y, 1, case.what + ", captured before any eager multiply")
    case.check(got, x, y, 1, None, case.what + ", captured before any eager multiply")
    k = int(np.nonzero(c[1:] != c[:-1])[0][0])  # two neighbouring entries with different columns, both in range
    swapped = c.copy()
    swapped[k], swapped[k + 1] = c[k + 1], c[k]
    case.mats[1].set(swapped)
    case.mats[1].put()
    y.put()
    _torch().cuda.synchronize()
    with pytest.raises(capi.SpmvHipError) as e:
        call(side.s.cuda_stream, x.ptr, y.ptr)
    assert e.value.code == capi.ERR_STATE
    side.s.synchronize()
    helpers.assert_bitexact(y.body(), y.host, "the refused multiply launched something")
    del g
    case.close()
