"""The Level-1 context (include/spmv_hip.h and the Level-1 halves of the family headers) held to its contract ACROSS uploads:
one context moved from any of its ten formats to any other with a matrix of another shape, through refused uploads, along a
walk of sixty uploads, on the caller's stream, without the event pair, and behind the multi-GPU front.  Everything goes
through capi.Context.

The reference of a re-used context is a FRESH one: the same upload, set_x, set_y(y0) and three runs in a context created
for it, twice.  Where the two fresh results agree bit for bit -- lifecycle_cases.REPRODUCIBLE says where they must -- the
re-used context owes those bits; elsewhere (atomics: formats 5 and 6, column panels) it is held to the oracle with the
reference and bound of the family's own test file, imported from there.  The fresh result is held to the oracle as well."""
import functools
import os

import numpy as np
import pytest

import helpers
import lifecycle_cases as lc
import oracle_py
import stream_helpers
import test_gpu_compact as fam8
import test_gpu_compact32 as fam10
import test_gpu_f32values as fam7
import test_gpu_multivec as mv
import test_gpu_symmetric as fam5
import test_gpu_transpose as fam6
from spmv_amd import capi, synth

pytestmark = pytest.mark.gpu

RUNS = 3
K = 3  # block vectors of the format-1 contexts
assert RUNS == fam5.RUNS == fam6.RUNS == fam7.RUNS == fam8.RUNS  # their _expected have it built in
INFO_KEYS = ("format", "rows", "cols", "stored", "device_bytes", "streamed_bytes")  # spmv_hip_ctx_info [0..3], [9], [15]


def _bits(got, want, what):
    if np.asarray(want).dtype == np.float32:
        fam10.assert_bits32(got, want, what)
    else:
        helpers.assert_bitexact(got, want, what)


class Case:
    """One (format, matrix): the upload, the vectors of the operator that runs (floats for format 10) and the oracle."""

    def __init__(self, fmt, name):
        self.fmt, self.name, self.what = fmt, name, "format %d on %s" % (fmt, name)
        self.rows, self.cols, self.p, self.c, self.v = lc.matrix(name)
        self.yrows, self.xcols = (self.cols, self.rows) if fmt == 6 else (self.rows, self.cols)
        rng = np.random.default_rng(100 * fmt + len(name))
        self.x = synth.x_vector(self.xcols, seed=7 + fmt)
        self.y0 = rng.uniform(-1.0, 1.0, size=self.yrows)
        if fmt == 10:
            self.x, self.y0 = fam10._f32(self.x), fam10._f32(self.y0)
        self.reproducible = (fmt, name) in lc.REPRODUCIBLE

    def upload(self, ctx):
        rows, cols, p, c, v = self.rows, self.cols, self.p, self.c, self.v
        if self.fmt == 1:
            ctx.upload_csr(rows, cols, p, c, v)
        elif self.fmt == 2:
            i, j, a = synth.csr_to_coordinate(rows, p, c, v)
            ctx.upload_coo(rows, cols, i - 1, j - 1, a)
        elif self.fmt == 3:
            E = lc.converted(self.name, 3)
            ctx.upload_ell(rows, cols, E["row_length"], E["col"], E["val"])
        elif self.fmt == 4:
            E = lc.converted(self.name, 4)
            ctx.upload_hybrid(rows, cols, E["row_length"], E["col"], E["val"], E["coo_row"], E["coo_col"], E["coo_val"])
        elif self.fmt == 5:
            ctx.upload_csr_symmetric(rows, p, c, v, capi.SYMMETRIC)
        elif self.fmt == 6:
            ctx.upload_csr_transposed(rows, cols, p, c, v)
        elif self.fmt == 7:
            ctx.upload_csr_f32values(rows, cols, p, c, v)
        elif self.fmt == 8:
            ctx.upload_csr_compact(rows, cols, p, c, v)
        elif self.fmt == 9:
            ctx.upload_csr_compact_f64(rows, cols, p, c, v)
        else:
            ctx.upload_csr_compact_f32xy(rows, cols, p, c, v)

    def set_x(self, ctx, x=None):
        (ctx.set_x_f32 if self.fmt == 10 else ctx.set_x)(self.x if x is None else x)

    def set_y(self, ctx, y=None):
        (ctx.set_y_f32 if self.fmt == 10 else ctx.set_y)(self.y0 if y is None else y)

    def get_y(self, ctx):
        return (ctx.get_y_f32() if self.fmt == 10 else ctx.get_y()).copy()

    def runs(self, ctx, n=RUNS, start=True):
        """set_x, set_y(y0) (with start) and n runs: y after each."""
        if start:
            self.set_x(ctx)
            self.set_y(ctx)
        out = []
        for _ in range(n):
            ctx.run()
            out.append(self.get_y(ctx))
        return out

    @functools.cached_property
    def expected(self):
        """(y0 + RUNS A x, the scale of its rounding, nterms) as the family's own test file states them."""
        rows, cols, p, c, v, x, y0 = self.rows, self.cols, self.p, self.c, self.v, self.x, self.y0
        if self.fmt == 5:
            return fam5._expected(rows, p, c, v, x, y0, capi.SYMMETRIC) + (4096,)  # scipy's expansion
        if self.fmt == 6:
            return fam6._expected(rows, cols, p, c, v, x, y0)  # the transposed matrix
        if self.fmt == 7:
            return fam7._expected(rows, cols, p, c, fam7._narrow(v)[0], x, y0)  # the rounded values
        if self.fmt == 8:
            return fam8._expected(rows, cols, p, c, fam8._narrow(v)[0], x, y0)
        if len(c) == 0:
            return y0.copy(), np.abs(y0), 4096
        want = oracle_py.Oracle().csr_spmv(rows, p, c, v, x, y=y0, num_threads=4, runs=RUNS)
        return want, RUNS * helpers.abs_products(rows, p, c, v, x) + np.abs(y0), max(4096, int(np.diff(p).max()))

    @functools.cached_property
    def row_sums32(self):
        return fam10._row_sums(self.rows, self.p, self.c, fam10._f32(self.v), self.x)

    def against_the_oracle(self, ys, what):
        """ys: y after each of RUNS runs from y0."""
        assert len(ys) == RUNS
        if self.fmt == 10:
            # the float restatement and its one-run bound, run by run from the y the run started with
            a32, before = fam10._f32(self.v), self.y0
            for k, y in enumerate(ys):
                t, bound = fam10.one_run_bound(self.rows, self.p, self.c, a32, self.x, before, self.row_sums32)
                err = np.abs(y.astype(np.float64) - t)
                assert np.all(err <= bound), "%s, run %d: %d rows outside the bound, worst ratio %.3f" % (
                    what, k + 1, int((err > bound).sum()), float(np.max(err / bound)))
                before = y
            return
        want, scale, nterms = self.expected
        helpers.assert_close(ys[-1], want, scale, what=what, nterms=nterms)


@functools.lru_cache(maxsize=None)
def case(fmt, name):
    return Case(fmt, name)


@functools.lru_cache(maxsize=None)
def fresh(fmt, name):
    """{ys, info}: upload, set_x, set_y(y0) and RUNS runs in a context of its own -- twice; bit for bit the same where
    lc.REPRODUCIBLE says so, and held to the oracle once."""
    cs = case(fmt, name)
    out = []
    for _ in range(2):
        with capi.Context(0) as ctx:
            with pytest.raises(capi.SpmvHipError) as e:
                ctx.last_run_ns()
            assert e.value.code == capi.ERR_STATE
            cs.upload(ctx)
            out.append({"ys": cs.runs(ctx), "info": ctx.info()})
    same = all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(out[0]["ys"], out[1]["ys"]))
    if cs.reproducible:
        assert same, cs.what + ": two fresh contexts differ, where the headers promise rows summed by their owners"
    assert out[0]["info"] == out[1]["info"]
    assert out[0]["info"]["format"] == fmt and out[0]["info"]["rows"] == cs.yrows and out[0]["info"]["cols"] == cs.xcols
    if name == lc.SCATTERED and fmt in (1, 2):
        assert out[0]["info"]["panel_tiles"] > 0, out[0]["info"]  # large and scattered enough for the column panels
    cs.against_the_oracle(out[0]["ys"], cs.what + " (fresh context)")
    return out[0]


def assert_matches_fresh(cs, ys, what):
    want = fresh(cs.fmt, cs.name)["ys"]
    if cs.reproducible:
        for k, (y, w) in enumerate(zip(ys, want)):
            _bits(y, w, "%s, run %d: the bits of a fresh context" % (what, k + 1))
    else:
        cs.against_the_oracle(ys, what)


def assert_info_of_fresh(ctx, cs, what):
    got, want = ctx.info(), fresh(cs.fmt, cs.name)["info"]
    assert {k: got[k] for k in INFO_KEYS} == {k: want[k] for k in INFO_KEYS}, what


def block_inputs(cs):
    return mv._inputs(cs.rows, cs.cols, K)


@functools.lru_cache(maxsize=None)
def block_reference(name):
    """Y0 + RUNS A X by MvPlan on the caller's arrays (Level 2)."""
    cs = case(1, name)
    X, Y0 = block_inputs(cs)
    D = mv.Dev(cs.rows, cs.cols, cs.p, cs.c, cs.v)
    with capi.MvPlan(cs.rows, cs.cols, cs.p, K, 0, D.stream) as plan:
        return D.spmm(plan, X, Y0)


def first_use(ctx, cs):
    """Format a with Ma: the vectors set and one run; for CSR also block vectors and a block run."""
    cs.upload(ctx)
    cs.runs(ctx, 1)
    if cs.fmt == 1:
        X, Y0 = block_inputs(cs)
        ctx.set_block_x(X)
        ctx.set_block_y(Y0)
        ctx.run_block()
        assert ctx.get_block_y(K).shape == (cs.rows, K)


def upload_into_used(ctx, cs, what, n=RUNS):
    """Format b with Mb into a context that held something else: both vectors zero, then the results of a fresh context."""
    cs.upload(ctx)
    y = cs.get_y(ctx)
    assert y.shape == (cs.yrows,) and not y.any(), what + ": y is not zero after the upload"
    ctx.run()
    assert not cs.get_y(ctx).any(), what + ": x is not zero after the upload (a run changed y)"
    ys = cs.runs(ctx, n if cs.reproducible else RUNS)
    assert_matches_fresh(cs, ys, what)
    assert_info_of_fresh(ctx, cs, what)
    return ys


def refused(code, fn, *args):
    with pytest.raises(capi.SpmvHipError) as e:
        fn(*args)
    assert e.value.code == code, e.value


def calls_of_other_formats(ctx, cs):
    """What a context of format b refuses with SPMV_HIP_ERR_STATE (host arrays of the right length, so that only the state
    can be what is wrong)."""
    f32 = lambda n: np.ones(n, dtype=np.float32)
    calls = []
    if cs.fmt <= 6:
        calls.append(("run_scaled", lambda: ctx.run_scaled(0.5, 2.0)))
    if cs.fmt != 10:
        calls += [("set_x_f32", lambda: ctx.set_x_f32(f32(cs.xcols))), ("set_y_f32", lambda: ctx.set_y_f32(f32(cs.yrows))),
                  ("get_y_f32", ctx.get_y_f32)]
    else:
        calls += [("set_x", lambda: ctx.set_x(np.ones(cs.xcols))), ("set_y", lambda: ctx.set_y(np.ones(cs.yrows))), ("get_y", ctx.get_y)]
    if cs.fmt != 1:
        calls += [("set_block_x", lambda: ctx.set_block_x(np.ones((cs.xcols, K)))), ("run_block", ctx.run_block)]
    return calls


# ---- 1: every ordered pair of formats ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("a", lc.FORMATS)
def test_every_format_after_format_a_gives_the_results_of_a_fresh_context(a):
    for b in lc.FORMATS:
        (fa, ma), (fb, mb) = lc.PAIRS[(a, b)]
        with capi.Context(0) as ctx:
            first_use(ctx, case(fa, ma))
            upload_into_used(ctx, case(fb, mb), "format %d on %s after format %d on %s" % (fb, mb, fa, ma))


# ---- 2: what the new state refuses ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("a", lc.FORMATS)
def test_calls_of_other_formats_are_refused_after_format_a_and_leave_y_alone(a):
    for b in lc.FORMATS:
        (fa, ma), (fb, mb) = lc.PAIRS[(a, b)]
        cs = case(fb, mb)
        what = "format %d on %s after format %d on %s" % (fb, mb, fa, ma)
        with capi.Context(0) as ctx:
            first_use(ctx, case(fa, ma))
            cs.upload(ctx)
            before = cs.runs(ctx, 1)[0]
            for name, call in calls_of_other_formats(ctx, cs):
                refused(capi.ERR_STATE, call)
                _bits(cs.get_y(ctx), before, "%s: y after the refused %s" % (what, name))
            if fb == 1:
                # block vectors do not outlive the matrix they were set for
                refused(capi.ERR_STATE, ctx.run_block)
                refused(capi.ERR_STATE, ctx.get_block_y, K)
                _bits(cs.get_y(ctx), before, what + ": y after the refused block calls")
                X, Y0 = block_inputs(cs)
                ctx.set_block_x(X)
                ctx.set_block_y(Y0)
                ctx.run_block(RUNS)
                helpers.assert_bitexact(ctx.get_block_y(K).ravel(), block_reference(mb).ravel(), what + ": block run against MvPlan")
                _bits(cs.get_y(ctx), before, what + ": y after a block run")
            # ... and the context still runs
            ctx.run()
            if cs.reproducible:
                _bits(cs.get_y(ctx), fresh(fb, mb)["ys"][1], what + ": the second run")


def assert_no_memory_lost(one_pass, what):
    """one_pass() creates a context, uses it, destroys it and returns the largest spmv_hip_ctx_info [9] it saw.  The first
    pass warms the runtime's own pools; every later pass may lower the free device memory (torch.cuda.mem_get_info after the
    destroy) by less than that largest context.  The figure is the device's, not the process's: should another process
    have taken memory meanwhile, one more pass is measured -- a leak loses the same amount again, a neighbour does not."""
    import torch
    torch.cuda.synchronize()
    largest, free = 0, []
    for k in range(3):
        largest = max(largest, one_pass())
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
        if k >= 1 and free[-2] - free[-1] < largest:
            break
    print("%s: free device memory after the passes %s; largest context %d bytes" % (what, free, largest))
    lost = min(a - b for a, b in zip(free, free[1:]))
    assert lost < largest, "%s: a pass lost %d bytes of device memory (largest context: %d)" % (what, lost, largest)
    return largest


# ---- 3: one long chain ---------------------------------------------------------------------------------------------------------

def test_a_walk_of_sixty_uploads_in_one_context_twice_without_losing_memory():
    """Every step as in test 1, with one run where the pair is reproducible (the fresh context's first run is on record) and
    three where the oracle judges.  The second pass may lower the free device memory by less than the largest single
    spmv_hip_ctx_info [9] met on the way: one matrix leaked per upload would be sixty times that."""
    steps = lc.walk()

    def one_pass():
        largest = 0
        with capi.Context(0) as ctx:
            first_use(ctx, case(*lc.PAIRS[(1, 1)][0]))
            for k, (fmt, name) in enumerate(steps):
                upload_into_used(ctx, case(fmt, name), "step %d of the walk: format %d on %s" % (k, fmt, name), n=1)
                largest = max(largest, ctx.info()["device_bytes"])
        return largest

    assert_no_memory_lost(one_pass, "a walk of %d uploads" % len(steps))


def test_the_float_and_the_double_vectors_are_freed_with_their_matrix():
    """The walk's cap is the size of a whole matrix; vectors are smaller than that in the pool.  Here they are all there is:
    3 entries per row under an x of 4 000 003 elements (16 MB as floats, 32 MB as doubles), uploaded twelve times as
    format 10 and as format 9 in turn with a small matrix of a third format in between.  The second pass of 36 uploads may
    lower the free device memory by less than the largest spmv_hip_ctx_info [9] on the way (the double x); one x32 left
    behind per format-10 upload would be six times that."""
    f32xy, f64, small = case(10, lc.HOLLOW), case(9, lc.HOLLOW), case(1, "tall")

    def one_pass():
        largest = 0
        with capi.Context(0) as ctx:
            for k in range(12):
                for cs in (f32xy, small, f64):
                    cs.upload(ctx)
                    assert not cs.get_y(ctx).any()
                    ys = cs.runs(ctx, 1)
                    if cs is small:
                        _bits(ys[0], fresh(1, "tall")["ys"][0], "tall between the hollow uploads, round %d" % k)
                    largest = max(largest, ctx.info()["device_bytes"])
            # the last of each against the oracle
            for cs in (f32xy, f64):
                cs.upload(ctx)
                cs.against_the_oracle(cs.runs(ctx), cs.what + " after 36 uploads")
        return largest

    largest = assert_no_memory_lost(one_pass, "36 uploads under a long x")
    assert 8 * f64.cols <= largest < 2 * 8 * f64.cols


# ---- 4: failed uploads ---------------------------------------------------------------------------------------------------------

def _ptr(a):
    return a.ctypes.data


def raw_upload(ctx, fmt, rows, cols, nnz, p, c, v, allow_rounding=1):
    """The C entry point of the format on the context's handle with nnz as given (capi.Context derives it from row_ptr):
    the return code."""
    p, c, v = np.ascontiguousarray(p, dtype=np.int32), np.ascontiguousarray(c, dtype=np.int32), np.ascontiguousarray(v, dtype=np.float64)
    L = ctx.lib
    if fmt == 1:
        return L.spmv_hip_upload_csr(ctx.h, rows, cols, nnz, p, c, v)
    if fmt == 5:
        return L.spmv_hip_upload_csr_symmetric(ctx.h, rows, nnz, _ptr(p), _ptr(c), _ptr(v), capi.SYMMETRIC)
    if fmt == 6:
        return L.spmv_hip_upload_csr_transposed(ctx.h, rows, cols, nnz, _ptr(p), _ptr(c), _ptr(v))
    if fmt == 9:
        return L.spmv_hip_upload_csr_compact_f64(ctx.h, rows, cols, nnz, _ptr(p), _ptr(c), _ptr(v))
    fn = {7: L.spmv_hip_upload_csr_f32values, 8: L.spmv_hip_upload_csr_compact, 10: L.spmv_hip_upload_csr_compact_f32xy}[fmt]
    return fn(ctx.h, rows, cols, nnz, _ptr(p), _ptr(c), _ptr(v), allow_rounding)


def bad_uploads(ctx, cs):
    """[(what, the call that returns the code, the code, the state spmv_hip.h says it leaves: "kept" or "none")]"""
    fmt, rows, cols, p, c, v = cs.fmt, cs.rows, cs.cols, cs.p, cs.c, cs.v
    nnz = len(c)
    mid = nnz // 2
    out = []
    if fmt in (3, 4):
        E = lc.converted(cs.name, fmt)
        L, ec, ev = E["row_length"], E["col"].copy(), E["val"]
        ec[len(ec) // 2] = cols
        if fmt == 3:
            out.append(("a column equal to cols", lambda: ctx.lib.spmv_hip_upload_ell(ctx.h, rows, cols, L, ec, ev), capi.ERR_INVALID, "none"))
            out.append(("a negative row length", lambda: ctx.lib.spmv_hip_upload_ell(ctx.h, rows, cols, -1, ec, ev), capi.ERR_INVALID, "kept"))
        else:
            hybrid = lambda col, cr, cc: ctx.lib.spmv_hip_upload_hybrid(ctx.h, rows, cols, L, col, ev, len(cr), cr, cc, E["coo_val"])
            assert len(E["coo_row"]) > 0
            cr, cc = E["coo_row"].copy(), E["coo_col"].copy()
            cr[len(cr) // 2] = rows
            cc[len(cc) // 2] = cols
            out.append(("a column equal to cols in the ELLPACK part", lambda: hybrid(ec, E["coo_row"], E["coo_col"]), capi.ERR_INVALID, "none"))
            out.append(("a column equal to cols in the remainder", lambda: hybrid(E["col"], E["coo_row"], cc), capi.ERR_INVALID, "none"))
            out.append(("a row equal to rows in the remainder", lambda: hybrid(E["col"], cr, E["coo_col"]), capi.ERR_INVALID, "none"))
        return out
    if fmt == 2:
        i = np.repeat(np.arange(rows, dtype=np.int32), np.diff(p))
        bi, bc = i.copy(), c.copy()
        bi[mid] = rows
        bc[mid] = cols
        coo = lambda ii, cc, n: ctx.lib.spmv_hip_upload_coo(ctx.h, rows, cols, n, ii, cc, v)
        return [("a column equal to cols", lambda: coo(i, bc, nnz), capi.ERR_INVALID, "none"),
                ("a row equal to rows", lambda: coo(bi, c, nnz), capi.ERR_INVALID, "none"),
                ("a negative number of entries", lambda: coo(i, c, -1), capi.ERR_INVALID, "kept")]
    family = fmt >= 5
    bc = c.copy()
    bc[mid] = cols  # (format 6: of A as stored)
    out.append(("a column equal to cols", lambda: raw_upload(ctx, fmt, rows, cols, nnz, p, bc, v), capi.ERR_INVALID, "kept" if family else "none"))
    bp = p.copy()
    r = int(np.nonzero(np.diff(p) > 0)[0][len(p) // 3])
    assert bp[r] > 0 and r + 1 < rows
    bp[r + 1] = bp[r] - 1  # row r ends in front of where it starts
    assert np.any(np.diff(bp) < 0) and bp[0] == 0 and bp[-1] == nnz
    out.append(("a decreasing row_ptr", lambda: raw_upload(ctx, fmt, rows, cols, nnz, bp, c, v), capi.ERR_INVALID, "kept" if family else "none"))
    out.append(("row_ptr[rows] != nnz", lambda: raw_upload(ctx, fmt, rows, cols, nnz - 1, p, c, v), capi.ERR_INVALID, "kept"))
    if fmt in (7, 8, 10):
        big = v.copy()
        big[mid] = 1e300
        out.append(("a value of 1e300", lambda: raw_upload(ctx, fmt, rows, cols, nnz, p, c, big), capi.ERR_OVERFLOW, "kept"))
        assert np.any(v.astype(np.float32).astype(np.float64) != v)
        out.append(("allow_rounding = 0 on values that are not floats", lambda: raw_upload(ctx, fmt, rows, cols, nnz, p, c, v, 0), capi.ERR_INVALID, "kept"))
    if fmt == 5:
        r = int(np.nonzero(np.diff(p) > 0)[0][3])
        up = c.copy()
        up[p[r + 1] - 1] = r + 1  # above the diagonal in a lower triangle
        assert up[p[r + 1] - 1] < rows
        out.append(("an entry in the other triangle", lambda: raw_upload(ctx, fmt, rows, cols, nnz, p, up, v), capi.ERR_INVALID, "kept"))
    return out


@functools.lru_cache(maxsize=None)
def sequence(fmt, name, n):
    """y after each of n runs from y0 in a fresh context of a reproducible pair."""
    cs = case(fmt, name)
    assert cs.reproducible
    with capi.Context(0) as ctx:
        cs.upload(ctx)
        return cs.runs(ctx, n)


@pytest.mark.parametrize("b", lc.FORMATS)
def test_a_refused_upload_leaves_the_old_matrix_or_none_and_never_something_in_between(b):
    old = case(9, "tall") if b == 1 else case(1, "wide")  # another format and another size, run once
    new = case(b, {1: "wide", 4: "bus1138_like", 5: "triangle"}.get(b, "tall"))
    assert new.fmt != old.fmt and lc.differ(lc.operator_shape(old.fmt, old.name), lc.operator_shape(new.fmt, new.name))
    with capi.Context(0) as ctx:
        tries = bad_uploads(ctx, new)
        want = sequence(old.fmt, old.name, len(tries) + 1)
        old.upload(ctx)
        done = len(old.runs(ctx, 1))
        info = ctx.info()
        for what, call, code, leaves in tries:
            what = "format %d refusing %s over format %d" % (b, what, old.fmt)
            rc = call()
            assert rc == code, "%s: returned %d (%s)" % (what, rc, ctx.lib.spmv_hip_last_error().decode())
            state = ctx.info()
            if b >= 5:
                assert leaves == "kept"  # the family headers' promise
            if state["format"] == 0:
                # without a matrix: nothing of the old one answers
                refused(capi.ERR_STATE, ctx.run)
                refused(capi.ERR_STATE, ctx.get_y)
                refused(capi.ERR_STATE, ctx.set_x, old.x)
                refused(capi.ERR_STATE, ctx.last_run_ns)
                assert leaves == "none", what + ": spmv_hip.h says the old matrix is kept"
                old.upload(ctx)
                assert ctx.info() == info
                done = len(old.runs(ctx, 1))
            else:
                # as it was: the next run is the old matrix's next run
                assert state == info, what
                assert leaves == "kept", what + ": spmv_hip.h says the context is left without a matrix"
                ctx.run()
                done += 1
                _bits(old.get_y(ctx), want[done - 1], "%s: run %d of the old matrix" % (what, done))
        # a valid upload afterwards is a fresh context's
        upload_into_used(ctx, new, "format %d on %s after its refused uploads" % (b, new.name))


# ---- 5: streams and events -----------------------------------------------------------------------------------------------------

def _stream_case(fmt):
    return case(fmt, {5: "triangle", 6: "tall"}.get(fmt, "wide"))


@pytest.mark.parametrize("fmt", lc.FORMATS)
def test_the_callers_stream_survives_uploads_and_gives_the_bits_of_the_own_stream(fmt):
    import torch
    cs, other = _stream_case(fmt), case(1 if fmt != 1 else 9, "poisson64")
    side = stream_helpers.nonblocking_stream()
    with capi.Context(0) as ctx:
        cs.upload(ctx)
        refused(capi.ERR_STATE, ctx.last_run_ns)  # nothing has run
        cs.set_x(ctx)
        cs.set_y(ctx)
        ctx.set_stream(side.cuda_stream)
        ys = cs.runs(ctx, 2, start=False)
        ctx.set_stream(None)
        ys += cs.runs(ctx, 1, start=False)
        assert_matches_fresh(cs, ys, cs.what + ": two runs on the caller's stream, one on the own")
        assert ctx.last_run_ns() >= 0
        # re-upload while on the caller's stream: the vectors and the runs of the new matrix go there
        ctx.set_stream(side.cuda_stream)
        first_use(ctx, other)
        assert ctx.last_run_ns() >= 0
        cs.upload(ctx)
        refused(capi.ERR_STATE, ctx.last_run_ns)  # the event pair bracketed a run of the matrix that is gone
        assert not cs.get_y(ctx).any()
        cs.set_x(ctx)
        cs.set_y(ctx)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(side):
            e0.record()
            for _ in range(RUNS):
                ctx.run(sync=False)
            e1.record()
        side.synchronize()  # the caller's own synchronisation is enough: the runs were on its stream
        assert e0.elapsed_time(e1) > 0.0
        y3 = cs.get_y(ctx)
        if cs.reproducible:
            _bits(y3, fresh(cs.fmt, cs.name)["ys"][-1], cs.what + ": after a re-upload on the caller's stream")
        else:
            cs.against_the_oracle([y3] * RUNS, cs.what + ": after a re-upload on the caller's stream")  # (formats 5 and 6: the last y is judged)
        assert_info_of_fresh(ctx, cs, cs.what)
        ctx.set_stream(None)


@pytest.mark.parametrize("fmt", (7, 8, 9, 10, 1))
def test_scaled_and_block_runs_on_the_callers_stream_give_the_bits_of_the_own_stream(fmt):
    cs = _stream_case(fmt)
    side = stream_helpers.nonblocking_stream()

    def three(ctx, between):
        cs.upload(ctx)
        if fmt == 1:
            X, Y0 = block_inputs(cs)
            ctx.set_block_x(X)
            ctx.set_block_y(Y0)
            step, get = ctx.run_block, lambda: ctx.get_block_y(K).ravel().copy()
        else:
            cs.set_x(ctx)
            cs.set_y(ctx)
            step, get = lambda: ctx.run_scaled(-0.75, 0.5), lambda: cs.get_y(ctx)
        between(0)
        step()
        step()
        between(1)
        step()
        return get()

    with capi.Context(0) as ctx:
        want = three(ctx, lambda k: None)
    with capi.Context(0) as ctx:
        got = three(ctx, lambda k: ctx.set_stream(None if k else side.cuda_stream))
        assert ctx.last_run_ns() >= 0
    _bits(got, want, cs.what + (": block runs" if fmt == 1 else ": scaled runs") + " on the caller's stream and on the own")
    if fmt == 1:
        helpers.assert_bitexact(want, block_reference(cs.name).ravel(), cs.what + ": block runs against MvPlan")


@pytest.mark.parametrize("fmt", lc.FORMATS)
def test_without_run_events_there_is_no_time_and_y_has_the_same_bits(fmt):
    cs = _stream_case(fmt)
    with capi.Context(0, capi.FLAG_NO_RUN_EVENTS) as ctx:
        cs.upload(ctx)
        refused(capi.ERR_STATE, ctx.last_run_ns)
        ys = cs.runs(ctx)
        refused(capi.ERR_STATE, ctx.last_run_ns)
        assert_matches_fresh(cs, ys, cs.what + " under SPMV_HIP_FLAG_NO_RUN_EVENTS")
        if fmt >= 7:
            cs.set_y(ctx)
            ctx.run_scaled(-0.75, 0.5)
            refused(capi.ERR_STATE, ctx.last_run_ns)
            got = cs.get_y(ctx)
            with capi.Context(0) as timed:
                cs.upload(timed)
                cs.runs(timed, 0)
                timed.run_scaled(-0.75, 0.5)
                assert timed.last_run_ns() >= 0
                _bits(got, cs.get_y(timed), cs.what + ": run_scaled with and without the event pair")
        if fmt == 1:
            X, Y0 = block_inputs(cs)
            ctx.set_block_x(X)
            ctx.set_block_y(Y0)
            ctx.run_block(RUNS)
            refused(capi.ERR_STATE, ctx.last_run_ns)
            helpers.assert_bitexact(ctx.get_block_y(K).ravel(), block_reference(cs.name).ravel(), cs.what + ": run_block without the event pair")


# ---- 6: the multi-GPU front ----------------------------------------------------------------------------------------------------

_front_ys = {}  # (front, a, b) -> y after each run, for the fronts that owe each other's bits
FRONTS = {"one_device": (1, 0, False), "three_parts_peer_gather": (3, capi.FLAG_PEER_GATHER, True),
          "three_parts_pipelined": (3, capi.FLAG_PEER_GATHER | capi.FLAG_PIPELINE_GATHER, True)}


def _single_device(cs):
    """Three runs of the single-device context for a matrix of the multi-GPU pairs (the two-row matrix is not in the pool)."""
    if cs.name in lc.ACCEPTS[cs.fmt]:
        return fresh(cs.fmt, cs.name)["ys"]
    with capi.Context(0) as ctx:
        cs.upload(ctx)
        ys = cs.runs(ctx)
    cs.against_the_oracle(ys, cs.what + " (single device)")
    return ys


@pytest.mark.parametrize("front", list(FRONTS))
def test_the_multi_gpu_front_moves_between_its_four_formats_and_refuses_the_others(front):
    parts, flags, share = FRONTS[front]
    if share:
        os.environ["SPMV_HIP_SHARE_DEVICES"] = "1"
    try:
        for (a, b), ((fa, ma), (fb, mb)) in lc.MULTI_PAIRS.items():
            csa, cs = case(fa, ma), case(fb, mb)
            what = "%s: format %d on %s after format %d on %s" % (front, fb, mb, fa, ma)
            with capi.Context(num_gpus=parts, flags=flags) as ctx:
                csa.upload(ctx)
                csa.runs(ctx, 1)
                cs.upload(ctx)
                assert not cs.get_y(ctx).any(), what + ": y is not zero after the upload"
                ctx.run()
                assert not cs.get_y(ctx).any(), what + ": x is not zero after the upload"
                ys = cs.runs(ctx)
                single = _single_device(cs)
                want, scale, nterms = cs.expected
                helpers.assert_close(ys[-1], single[-1], scale, what=what + " against the single-device context", nterms=nterms)
                cs.against_the_oracle(ys, what)
                # spmv_hip.h on SPMV_HIP_FLAG_PIPELINE_GATHER: "Same y, bit for bit" as the serial order of the same parts
                _front_ys[(front, a, b)] = ys
                serial = _front_ys.get(("three_parts_peer_gather", a, b))
                if front == "three_parts_pipelined" and serial is not None:
                    for k in range(RUNS):
                        _bits(ys[k], serial[k], "%s, run %d: the bits of the serial gather" % (what, k + 1))
                info = ctx.info()
                assert (info["format"], info["rows"], info["cols"], info["devices"]) == (fb, cs.rows, cs.cols, parts)
                if a == b:
                    # the family uploads are refused and leave the matrix that is there
                    before = cs.get_y(ctx)
                    for f in (5, 6, 7, 8, 9, 10):
                        refused(capi.ERR_STATE, case(f, lc.ACCEPTS[f][0]).upload, ctx)
                        # (capi.Context notes the sizes only after a successful upload)
                        assert ctx.info() == info, what
                    _bits(cs.get_y(ctx), before, what + ": y after the refused uploads")
                    ctx.run()
                    helpers.assert_close(cs.get_y(ctx), before + (single[1] - single[0]), scale, what=what + ": a run after the refused uploads",
                                         nterms=nterms)
    finally:
        if share:
            os.environ.pop("SPMV_HIP_SHARE_DEVICES", None)
