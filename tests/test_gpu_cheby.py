"""The Chebyshev polynomial preconditioner (include/spmv_hip_cheby.h) on the MI355X: spmv_hip_cheby_bound_{f64,f32},
spmv_hip_cheby_coeffs and spmv_hip_cheby_step_{f64,f32}, through capi.cheby_bound / cheby_coeffs / cheby_step.

The bound, the table, d and z are held bit for bit to the numpy restatement of the header (cheby_cases.bound / coeffs / step).
The dots are held (a) bit for bit to sums formed in integers on operands where every order gives the same sum, at every size up to
the one that takes the reduction's second stage, (b) on general operands to n 2^-53 sum |t_i| of math.fsum(t), t_i the rounded
products formed in numpy from the z the GPU returned (test_cheby_cases.py shows without a device that a lost element or a group
taken from the wrong chunk would exceed it tenfold), and (c) with the table {0, 1} at degree 1 in doubles bit for bit to dots[1] of
spmv_hip_cg_step_f64.  Every device array of floating-point numbers lies between NaN guard bands that are checked whenever it is
read back, and the dots and the workspace are NaN when a call starts."""
import math

import numpy as np
import pytest

import bjacobi_cases as bc
import cheby_cases as cb
import dots_cases as dc
import krylov_cases as kc
import stream_helpers as sh
from spmv_amd import capi
from test_gpu_dots import _same_dots
from test_gpu_krylov import Band
from test_gpu_scaled import Dev, _alternate, _bits

pytestmark = pytest.mark.gpu

CASES = [(dtype, with_minv) for dtype in cb.DTYPES for with_minv in (False, True)]
IDS = ["%s-%s" % (np.dtype(dtype).name, "minv" if m else "nominv") for dtype, m in CASES]


class Arrays:
    """The device arrays of one step over host operands (u, minv, d, z, r) and a table."""

    def __init__(self, host, table, dtype, with_minv):
        self.host, self.table_host, self.dtype = host, np.asarray(table, dtype=np.float64), np.dtype(dtype)
        self.n = len(host[0])
        self.u, self.minv, self.d, self.z, self.r = (Band(a, dtype) for a in host)
        self.with_minv = with_minv
        self.table = Band(self.table_host)
        self.bytes = capi.krylov_workspace_bytes(self.n)
        self.dots, self.work = Band(np.full(2, np.nan)), Band(np.full(self.bytes // 8, np.nan))

    def reset(self):
        self.d.set(self.host[2])
        self.z.set(self.host[3])

    def step(self, degree, j, dots, stream=0, d=None, z=None, dots_band=None, work=None, fill=True, no_d=False):
        dd, ww = dots_band or self.dots, work or self.work
        if fill:
            dd.fill()
            ww.fill()
        capi.cheby_step(self.n, degree, j, self.table.ptr, self.u.ptr, self.minv.ptr if self.with_minv else None,
                        None if no_d else (d or self.d).ptr, (z or self.z).ptr, self.r.ptr if dots else None, dd.ptr if dots else None,
                        ww.ptr if dots else None, self.bytes if dots else 0, stream, dtype=self.dtype)

    def read_dots(self, what="", dots=None, work=None):
        (work or self.work).body(what + ", the workspace")
        return (dots or self.dots).body(what + ", the dots")

    def inputs_unchanged(self, what):
        _bits(self.u.body(what), self.host[0], what + ": u changed")
        _bits(self.minv.body(what), self.host[1], what + ": minv changed")
        _bits(self.r.body(what), self.host[4], what + ": r changed")
        _bits(self.table.body(what), self.table_host, what + ": the table changed")


def _within_bound(got, z, r, what):
    for k, t in enumerate(cb.products(z, r)):
        want, b = math.fsum(t), dc.bound(t)
        print("%s: dots[%d] %r, fsum %r, off by %.3e, bound %.3e" % (what, k, got[k], want, abs(got[k] - want), b))
        assert abs(got[k] - want) <= b, "%s: dots[%d] = %r, fsum of the products %r, bound %.3e" % (what, k, got[k], want, b)


# ---- 1: the coefficients, bit for bit the restatement ------------------------------------------------------------------------------

def _table(degree, lam, scale, ratio, stream=0):
    lam_band, out = Band([lam]), Band(np.full(2 * degree, np.nan))
    capi.cheby_coeffs(degree, lam_band.ptr, scale, ratio, out.ptr, stream)
    got = out.body("coeffs")
    assert np.array_equal(lam_band.body("lambda").view(np.uint64), np.array([lam]).view(np.uint64)), "coeffs changed lambda"
    return got


def _same_table(got, want, what):
    """Bit for bit, a NaN being any NaN (IEEE leaves its payload open)."""
    got, want = np.asarray(got), np.asarray(want)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), "%s: %r against %r" % (what, got, want)
    assert np.array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64)), "%s: %r against %r" % (what, got, want)


def test_the_coefficients_are_the_restatement_bit_for_bit():
    for degree in range(1, cb.MAX_DEGREE + 1):
        for lam in (2.0, 2.0000000000000004, 0.7310585786300049e3):
            for ratio in (10.0, 30.0):
                for scale in (1.0, 1.1):
                    _same_table(_table(degree, lam, scale, ratio), cb.coeffs(degree, lam, scale, ratio),
                                "degree %d, lambda %r, scale %r, ratio %r" % (degree, lam, scale, ratio))
    for lam in (0.0, float("nan")):  # what IEEE gives
        got, want = _table(4, lam, 1.0, 30.0), cb.coeffs(4, lam, 1.0, 30.0)
        print("lambda %r: %r" % (lam, got))
        _same_table(got, want, "lambda %r" % lam)
        assert got[0] == 0.0 and not np.signbit(got[0]) and not np.all(np.isfinite(got[1:]))


# ---- 2: the bound, bit for bit the restatement -----------------------------------------------------------------------------------------

def _bound(rows, p, v, minv, dtype, stream=0, lam=None):
    import torch
    tp, tv = torch.from_numpy(np.ascontiguousarray(p, dtype=np.int32)).to("cuda:0"), Band(v)
    m = Band(minv, dtype) if minv is not None else None
    lam = lam or Band([np.nan])
    capi.cheby_bound(rows, tp, tv.ptr, m.ptr if m else None, lam.ptr, stream, dtype=dtype)
    got = lam.body("the bound")
    assert np.array_equal(tp.cpu().numpy(), p), "the bound changed row_ptr"
    assert np.array_equal(tv.body("values").view(np.uint64), np.asarray(v, dtype=np.float64).view(np.uint64)), "the bound changed the values"
    if m:
        _bits(m.body("minv"), np.asarray(minv, dtype=dtype), "the bound changed minv")
    return got


def test_the_bound_is_the_restatement_bit_for_bit():
    rows, cols, p, c, v, b, diag_inv = kc.poisson()
    matrices = [("poisson2D", rows, p, v, diag_inv), ("ragged",) + cb.ragged_matrix()[:2] + (cb.ragged_matrix()[3], None),
                ("last row largest",) + cb.last_row_matrix()[:2] + (cb.last_row_matrix()[3], None)]
    for name, rows, p, v, minv in matrices:
        for dtype in (None,) + cb.DTYPES:
            m = None if dtype is None else (minv.astype(dtype) if minv is not None else cb.bound_minv(rows, dtype))
            got, want = _bound(rows, p, v, m, dtype or np.float64), cb.bound(rows, p, v, m)
            print("%s, minv %s: %r" % (name, "null" if dtype is None else np.dtype(dtype).name, got[0]))
            _same_dots(got, [want], "%s, minv %s: the bound against the restatement" % (name, dtype))
    # a NaN value gives NaN, an Inf gives Inf; no rows give +0.0
    rows, p, c, v = cb.last_row_matrix()
    for value, check in ((np.nan, np.isnan), (np.inf, np.isposinf), (-np.inf, np.isposinf)):
        bad = v.copy()
        bad[p[1234]] = value
        for dtype in (None, np.float32):
            got = _bound(rows, p, bad, None if dtype is None else cb.bound_minv(rows, dtype), dtype or np.float64)
            assert check(got[0]), (value, got)
    _same_dots(_bound(0, np.zeros(1, dtype=np.int32), np.zeros(4), None, np.float64), [0.0], "rows 0")
    _same_dots(_bound(0, np.zeros(1, dtype=np.int32), np.zeros(4), np.zeros(4, dtype=np.float32), np.float32), [0.0], "rows 0, a float minv")


def test_two_calls_of_the_bound_on_two_streams_give_identical_bits():
    import torch
    rows, p, c, v = cb.last_row_matrix()
    want = cb.bound(rows, p, v, cb.bound_minv(rows, np.float64))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    lams = [Band([np.nan]), Band([np.nan])]
    tp, tv, m = torch.from_numpy(p).to("cuda:0"), Band(v), Band(cb.bound_minv(rows, np.float64))
    torch.cuda.synchronize()
    for rnd in range(3):
        for s, lam in zip(streams, lams):
            capi.cheby_bound(rows, tp, tv.ptr, m.ptr, lam.ptr, s.cuda_stream, dtype=np.float64)
    for s in streams:
        s.synchronize()
    for lam in lams:
        _same_dots(lam.body("two streams"), [want], "the bound of two streams at once")


# ---- 3: the step, bit for bit; the dots --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,with_minv", CASES, ids=IDS)
def test_d_and_z_are_the_restatement_bit_for_bit_and_the_dots_are_within_the_bound(dtype, with_minv):
    for n in cb.SIZES:
        general = n <= cb.GENERAL_LIMIT
        host = cb.general_case(n).arrays(dtype) if general else cb.int_case(n).arrays(dtype)
        table = cb.general_table() if general else cb.INT_TABLE
        dev = Arrays(host, table, dtype, with_minv)
        u, m, d0, z0, r = host
        for name, degree, j, dots in cb.MODES:
            tag = "n %d, %s, %s, %s, %s operands" % (n, name, np.dtype(dtype).name, "minv" if with_minv else "no minv", "general" if general else "integer")
            stores_d = j < degree - 1
            dev.reset()
            if j == 0:  # neither d nor z is read
                dev.z.fill()
                dev.d.fill()
            elif not stores_d:
                pass  # the last step reads d and leaves it
            dev.step(degree, j, dots)
            want_d, want_z = cb.step(table, degree, j, u, m if with_minv else None, d0, z0, dtype)
            z = dev.z.body(tag)
            assert z.dtype == dtype
            _bits(z, want_z, tag + ": z against the restatement")
            got_d = dev.d.body(tag)
            if stores_d:
                _bits(got_d, want_d, tag + ": d against the restatement")
            elif j == 0:
                assert np.all(np.isnan(got_d)), tag + ": a step that does not store d wrote it"
            else:
                _bits(got_d, d0, tag + ": the last step changed d")
            got = dev.read_dots(tag)
            if not dots:
                assert np.all(np.isnan(got)), tag + ": a call without dots wrote the dots or the workspace"
            elif general:
                _within_bound(got, z, r, tag)
            else:
                _, zi, s0, s1 = cb.int_case(n).results(degree, j, with_minv)
                assert np.array_equal(z.astype(np.float64), zi), tag + ": z"
                _same_dots(got, [float(s0), float(s1)], tag + ": the dots against the integer sums")
            dev.inputs_unchanged(tag)
        if n == 3:  # at degree 1 d may be null, and u may be r
            dev.z.fill()
            dev.step(1, 0, False, no_d=True)
            _bits(dev.z.body("no d"), cb.step(table, 1, 0, u, m if with_minv else None, None, None, dtype)[1], "degree 1 without d: z")
    # no element: +0.0, +0.0 with dots, nothing without
    dev = Arrays(tuple(np.zeros(0, dtype=dtype) for _ in range(5)), cb.INT_TABLE, dtype, with_minv)
    dev.step(3, 2, True)
    _same_dots(dev.read_dots("n 0"), [0.0, 0.0], "n 0")
    dev.step(3, 1, False)
    dev.step(1, 0, False)


@pytest.mark.parametrize("dtype,with_minv", CASES, ids=IDS)
def test_dots_of_integer_operands_are_the_integer_sums_bit_for_bit(dtype, with_minv):
    for n in cb.SIZES:
        h = cb.int_case(n)
        dev = Arrays(h.arrays(dtype), cb.INT_TABLE, dtype, with_minv)
        for name, degree, j, dots in cb.MODES:
            if not dots:
                continue
            tag = "n %d, %s, %s" % (n, name, np.dtype(dtype).name)
            _, zi, s0, s1 = h.results(degree, j, with_minv)
            dev.reset()
            dev.step(degree, j, True)
            assert np.array_equal(dev.z.body(tag).astype(np.float64), zi), tag + ": z"
            _same_dots(dev.read_dots(tag), [float(s0), float(s1)], tag + ": the dots against the integer sums")


def test_the_table_0_1_at_degree_1_in_doubles_is_the_second_dot_of_the_cg_step_bit_for_bit():
    for n in kc.SIZES[1:] + [65537]:
        rng = np.random.default_rng(n + 5)
        r, minv = rng.uniform(-1.0, 1.0, size=n), rng.uniform(0.5, 2.0, size=n)
        tag = "n %d" % n
        dev = Arrays((r, minv, np.zeros(n), np.zeros(n), r), [0.0, 1.0], np.float64, True)
        dev.step(1, 0, True)
        got = dev.read_dots(tag)
        zero, x, rr, m = (Band(a) for a in (np.zeros(n), np.zeros(n), r, minv))
        nd = Band([0.0, 1.0])
        dots, work = Band(np.full(2, np.nan)), Band(np.full(dev.bytes // 8, np.nan))
        capi.cg_step(n, nd.ptr, nd.ptr + 8, zero.ptr, zero.ptr, x.ptr, rr.ptr, m.ptr, dots.ptr, work.ptr, dev.bytes, 0, dtype=np.float64)
        _bits(rr.body(tag), r, tag + ": a step with a = 0 changed r")
        _same_dots(got[:1], dots.body(tag)[1:], tag + ": r'z of the step against r' M^-1 r of the cg step")
        # ... and u may be r itself
        capi.cheby_step(n, 1, 0, dev.table.ptr, dev.r.ptr, dev.minv.ptr, None, dev.z.ptr, dev.r.ptr, dev.dots.ptr, dev.work.ptr, dev.bytes, 0,
                        dtype=np.float64)
        _same_dots(dev.read_dots(tag), got, tag + ": d_u == d_r")


# ---- 4: identical bits across calls, streams and a captured graph ----------------------------------------------------------------------

class _GridHost:
    """What test_gpu_scaled.Dev reads of a host matrix: a CSR matrix, a right-hand side and 1 / diag."""

    def __init__(self, name, rows, p, c, v, b, minv):
        self.name, self.rows, self.cols, self.p, self.c, self.v, self.b, self.minv = name, rows, rows, p, c, v, b, minv
        self.a32 = v.astype(np.float32)

    def values(self, kind):
        return self.v if kind == "c16_f64" else self.a32

    def vectors(self, kind):
        dtype = np.float32 if kind == "c16_f32xy" else np.float64
        return np.zeros(self.cols, dtype=dtype), np.zeros(self.rows, dtype=dtype), dtype


def _kind(dtype):
    return "c16_f64" if dtype == np.float64 else "c16_f32xy"


def _scaled(mdev, dtype):
    fn = mdev.plan.spmv_f64_scaled if dtype == np.float64 else mdev.plan.spmv_f32xy_scaled
    return lambda x, y_in, y_out, s: fn(mdev.tp.data_ptr(), mdev.ac, mdev.av, x, -1.0, 1.0, y_in, y_out, s)


@pytest.fixture(scope="module")
def side():
    s = sh.Side()
    yield s
    s.report()


@pytest.mark.parametrize("dtype", cb.DTYPES, ids=["float64", "float32"])
def test_two_runs_a_delayed_stream_two_streams_and_a_replayed_graph_give_identical_bits(side, dtype):
    import torch
    rows, p, c, v = cb.poisson_grid(70)  # 4900 unknowns: four chunks and a part
    rhs = np.random.default_rng(70).uniform(-1.0, 1.0, size=rows)
    minv = np.random.default_rng(71).uniform(0.2, 0.25, size=rows)  # (row sums of |M^-1 A| stay below the table's lambda of 2)
    h = _GridHost("poisson_70", rows, p, c, v, rhs, minv)
    mdev = Dev(h, _kind(dtype))
    residual = _scaled(mdev, dtype)
    n, tag = rows, np.dtype(dtype).name
    table = cb.coeffs(cb.DEGREE, 2.0, 1.0, cb.RATIO)
    bytes_ = capi.krylov_workspace_bytes(n)
    r, m, tb = Band(rhs, dtype), Band(minv, dtype), Band(table)

    def application(stream, u, d, z, dots, work):
        """Three steps and the two multiplies between them: one line of five launches and a reduction."""
        capi.cheby_step(n, 3, 0, tb.ptr, r.ptr, m.ptr, d.ptr, z.ptr, None, None, None, 0, stream, dtype=dtype)
        residual(z.ptr, r.ptr, u.ptr, stream)
        capi.cheby_step(n, 3, 1, tb.ptr, u.ptr, m.ptr, d.ptr, z.ptr, None, None, None, 0, stream, dtype=dtype)
        residual(z.ptr, r.ptr, u.ptr, stream)
        capi.cheby_step(n, 3, 2, tb.ptr, u.ptr, m.ptr, d.ptr, z.ptr, r.ptr, dots.ptr, work.ptr, bytes_, stream, dtype=dtype)

    def fresh():
        return (Band(np.full(n, np.nan), dtype), Band(np.full(n, np.nan), dtype), Band(np.full(n, np.nan), dtype), Band(np.full(2, np.nan)),
                Band(np.full(bytes_ // 8, np.nan)))

    first = fresh()
    application(0, *first)
    z, dots = first[2].body(tag), first[3].body(tag)
    first[4].body(tag)
    assert np.all(np.isfinite(z)) and np.all(np.isfinite(dots)) and dots[0] > 0
    again = fresh()
    application(0, *again)
    _bits(again[2].body(tag), z, tag + ": z of a second run")
    _same_dots(again[3].body(tag), dots, tag + ": the dots of a second run")
    # behind the delay on a non-blocking stream: r, minv and the table arrive behind the delay
    ra, ma, ta = sh.operand(rhs.astype(dtype)), sh.operand(minv.astype(dtype)), sh.operand(table)
    ua, da, za = (sh.result(np.zeros(n, dtype=dtype)) for _ in range(3))
    dd, wa = sh.result(np.zeros(2)), sh.result(np.zeros(bytes_ // 8))

    def call(stream):
        capi.cheby_step(n, 3, 0, ta.ptr, ra.ptr, ma.ptr, da.ptr, za.ptr, None, None, None, 0, stream, dtype=dtype)
        residual(za.ptr, ra.ptr, ua.ptr, stream)
        capi.cheby_step(n, 3, 1, ta.ptr, ua.ptr, ma.ptr, da.ptr, za.ptr, None, None, None, 0, stream, dtype=dtype)
        residual(za.ptr, ra.ptr, ua.ptr, stream)
        capi.cheby_step(n, 3, 2, ta.ptr, ua.ptr, ma.ptr, da.ptr, za.ptr, ra.ptr, dd.ptr, wa.ptr, bytes_, stream, dtype=dtype)

    (bz, bd, _), _ = sh.delayed(side, [ra, ma, ta, ua, da, za, dd, wa], call, [za, dd, wa], "one application behind the delay (%s)" % tag)
    _bits(bz, z, tag + ": z behind the delay")
    _same_dots(bd, dots, tag + ": the dots behind the delay")
    # two streams at once: u, d, z, the dots and a workspace each
    own = [fresh() for _ in side.streams]
    torch.cuda.synchronize()
    for rnd in range(3):
        for s, arrays in zip(side.streams, own):
            application(s.cuda_stream, *arrays)
    for s in side.streams:
        s.synchronize()
    for arrays in own:
        _bits(arrays[2].body(tag), z, tag + ": z of two streams at once")
        arrays[4].body(tag)
        _same_dots(arrays[3].body(tag), dots, tag + ": the dots of two streams at once")
    # a captured line of one whole application, replayed twice
    cap = torch.cuda.Stream()
    graph = fresh()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cap):
        application(torch.cuda.current_stream().cuda_stream, *graph)
    for replay in range(2):
        g.replay()
    torch.cuda.synchronize()
    _bits(graph[2].body(tag), z, tag + ": z of the replayed graph")
    graph[4].body(tag)
    _same_dots(graph[3].body(tag), dots, tag + ": the dots of the replayed graph")
    del g
    _bits(r.body(tag), rhs.astype(dtype), tag + ": r changed")
    _bits(m.body(tag), minv.astype(dtype), tag + ": minv changed")
    _bits(tb.body(tag), table, tag + ": the table changed")
    mdev.close()


# ---- 5: eight PCG iterations, call by call ---------------------------------------------------------------------------------------------

def _pcg(dtype, h, inner):
    """Eight PCG iterations as the header composes them at degree 3, every call on a side stream with a snapshot of every array
    behind it; inner: None (the diagonal h.minv inside) or the block size of a point-block Jacobi inside.  Returns r'r of the last r."""
    import torch
    mdev = Dev(h, _kind(dtype))
    plan = mdev.plan
    multiply = plan.spmv_f64_scaled_dots if dtype == np.float64 else plan.spmv_f32xy_scaled_dots
    residual = _scaled(mdev, dtype)
    n, degree = h.rows, cb.DEGREE
    tag = "%s, %s" % (h.name, np.dtype(dtype).name)
    lam, table = Band([np.nan]), Band(np.full(2 * degree, np.nan))
    if inner:
        invh = bc.spd_inverse(inner, dtype)
        inv = Band(invh, dtype)
        dense = np.zeros((n, n))
        dense[np.repeat(np.arange(n), np.diff(h.p)), h.c] = h.v
        blocks = np.zeros((n, n))
        for k in range(n // inner):
            blocks[k * inner:(k + 1) * inner, k * inner:(k + 1) * inner] = invh.reshape(n // inner, inner, inner)[k].astype(np.float64)
        lam_host = float(np.max(np.linalg.eigvals(blocks @ dense).real))  # lambda_max(M^-1 A) of the small matrix, on the host
        lam.set([lam_host])
        scale, minv, mh = 1.05, None, None
    else:
        mh = h.minv.astype(dtype)
        minv = Band(mh, dtype)
        tp, tv = torch.from_numpy(h.p).to("cuda:0"), torch.from_numpy(h.v).to("cuda:0")
        capi.cheby_bound(n, tp, tv, minv.ptr, lam.ptr, 0, dtype=dtype)
        scale = 1.0
    capi.cheby_coeffs(degree, lam.ptr, scale, cb.RATIO, table.ptr, 0)
    lam_got = lam.body(tag)[0]
    coef = table.body(tag)
    if not inner:
        _same_dots([lam_got], [cb.bound(n, h.p, h.v, mh)], tag + ": the bound")
    _same_dots(coef, cb.coeffs(degree, lam_got, scale, cb.RATIO), tag + ": the table")
    print("%s: lambda %r, the table %r" % (tag, lam_got, coef.tolist()))
    x, r, p, q, z, d, u, s = (Band(np.zeros(n), dtype) for _ in range(8))
    r.set(h.b.astype(dtype))
    start = Band([0.0, 1.0])
    rz = [Band(np.full(2, np.nan)), Band(np.full(2, np.nan))]
    rr, pq = Band(np.full(2, np.nan)), Band(np.full(2, np.nan))
    kbytes, mbytes = capi.krylov_workspace_bytes(n), plan.dots_workspace_bytes()
    kwork, mwork = Band(np.full(kbytes // 8, np.nan)), Band(np.full(mbytes // 8, np.nan))
    bands = {"x": x, "r": r, "p": p, "q": q, "z": z, "d": d, "u": u, "s": s, "rz0": rz[0], "rz1": rz[1], "rr": rr, "pq": pq}
    snaps = []

    def snap(name):
        snaps.append((name, {k: v.snap() for k, v in bands.items()}))

    def precondition(st, new, it):
        for j in range(degree):
            src = r
            if j > 0:
                residual(z.ptr, r.ptr, u.ptr, st)
                snap("residual %d %d" % (j, it))
                src = u
            if inner:
                capi.bjacobi_apply(n, inner, inv.ptr, src.ptr, s.ptr, None, None, 0, st, dtype=dtype)
                snap("inner %d %d" % (j, it))
                src = s
            last = j == degree - 1
            capi.cheby_step(n, degree, j, table.ptr, src.ptr, minv.ptr if minv else None, d.ptr, z.ptr, r.ptr if last else None,
                            new.ptr if last else None, kwork.ptr if last else None, kbytes if last else 0, st, dtype=dtype)
            snap("cheby %d %d" % (j, it))

    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        st = stream.cuda_stream
        snap("reset")
        precondition(st, rz[0], -1)
        capi.cg_direction(n, start.ptr, start.ptr + 8, z.ptr, None, p.ptr, st, dtype=dtype)
        snap("begin -1")
        for it in range(cb.ITERATIONS):
            old, new = rz[it % 2], rz[1 - it % 2]
            multiply(mdev.tp.data_ptr(), mdev.ac, mdev.av, p.ptr, 1.0, 0.0, None, q.ptr, p.ptr, pq.ptr, mwork.ptr, mbytes, st)
            snap("multiply %d" % it)
            capi.cg_step(n, old.ptr, pq.ptr + 8, p.ptr, q.ptr, x.ptr, r.ptr, None, rr.ptr, kwork.ptr, kbytes, st, dtype=dtype)
            snap("step %d" % it)
            precondition(st, new, it)
            capi.cg_direction(n, new.ptr, old.ptr, z.ptr, None, p.ptr, st, dtype=dtype)
            snap("direction %d" % it)
    stream.synchronize()
    states = [(name, {k: bands[k].body(tag + ", " + name, sn[k]) for k in bands}) for name, sn in snaps]
    values = h.values(_kind(dtype)).astype(np.float64)
    first_rr = float(np.sum(states[0][1]["r"].astype(np.float64) ** 2))
    starts = h.p[:-1].astype(np.int64)
    cast = (lambda ref: 0.0) if dtype == np.float64 else (lambda ref: 2.0 ** -24 * np.abs(ref) + 2.0 ** -149)
    for (_, before), (name, after) in zip(states, states[1:]):
        what = tag + ", " + name
        words = name.split()
        it = int(words[-1])
        old, new = ("rz%d" % (it % 2), "rz%d" % (1 - it % 2)) if it >= 0 else ("rz1", "rz0")
        j = int(words[1]) if len(words) == 3 else None
        changed = {"multiply": {"q", "pq"}, "step": {"x", "r", "rr"}, "direction": {"p"}, "begin": {"p"}, "residual": {"u"}, "inner": {"s"},
                   "cheby": {"z"} | ({"d"} if j is not None and j < degree - 1 else set()) | ({new} if j == degree - 1 else set())}[words[0]]
        for key in before:
            if key not in changed:
                assert np.array_equal(after[key], before[key], equal_nan=True), what + ": %s changed" % key
        if words[0] in ("multiply", "residual"):
            vec = before["p"] if words[0] == "multiply" else before["z"]
            prod = values * vec.astype(np.float64)[h.c]
            az, scale_ = np.add.reduceat(prod, starts), np.add.reduceat(np.abs(prod), starts)
            if words[0] == "multiply":
                ref, got = az, after["q"]
            else:
                ref, got, scale_ = before["r"].astype(np.float64) - az, after["u"], scale_ + np.abs(before["r"].astype(np.float64))
            err = np.abs(got.astype(np.float64) - ref)
            assert np.all(err <= 2 * 16 * 2.0 ** -53 * scale_ * (1 + 2.0 ** -23) + cast(ref)), what + ": not the product"  # (rows of up to 15 entries)
            if words[0] == "multiply":
                for k, t in enumerate(dc.products(after["q"], before["p"])):
                    assert abs(after["pq"][k] - math.fsum(t)) <= dc.bound(t), what + ": the multiply's dots[%d]" % k
        elif words[0] == "step":
            want_x, want_r = kc.restate_step(before[old][0], before["pq"][1], before["p"], before["q"], before["x"], before["r"], dtype)
            _bits(after["x"], want_x, what + ": x")
            _bits(after["r"], want_r, what + ": r")
        elif words[0] == "inner":
            _bits(after["s"], bc.apply(invh, before["r"] if j == 0 else before["u"], inner, dtype), what + ": s")
        elif words[0] == "cheby":
            src = before["s"] if inner else (before["r"] if j == 0 else before["u"])
            want_d, want_z = cb.step(coef, degree, j, src, mh, before["d"], before["z"], dtype)
            _bits(after["z"], want_z, what + ": z")
            if want_d is not None:
                _bits(after["d"], want_d, what + ": d")
            else:
                _within_bound(after[new], after["z"], after["r"], what)
        elif words[0] == "begin":
            _bits(after["p"], after["z"], what + ": p = z0")
        else:
            _bits(after["p"], kc.restate_direction(before[new][0], before[old][0], before["z"], None, before["p"], dtype), what + ": p")
    last = float(states[-1][1]["rr"][0])
    kwork.body(tag)
    mwork.body(tag)
    mdev.close()
    return first_rr, last


@pytest.mark.parametrize("dtype", cb.DTYPES, ids=["float64", "float32"])
def test_eight_pcg_iterations_on_poisson_at_degree_3_verify_call_by_call(dtype):
    rows, cols, p, c, v, b, minv = kc.poisson()
    first, last = _pcg(dtype, _GridHost("poisson2D", rows, p, c, v, b, minv), None)
    diag = kc.pcg_restated(dtype, True)[-1]
    print("%s: r'r of r0 %.6e, after %d iterations at degree 3, ratio 30 %.6e (the restated diagonal run: %.6e): %.3e of it" % (
        np.dtype(dtype).name, first, cb.ITERATIONS, last, diag, last / diag))
    assert np.isfinite(last) and last < 1e-3 * diag


@pytest.mark.parametrize("dtype", cb.DTYPES, ids=["float64", "float32"])
def test_eight_pcg_iterations_with_3_by_3_blocks_inside_verify_call_by_call(dtype):
    rows, p, c, v, rhs = bc.spd_case()
    first, last = _pcg(dtype, _GridHost("spd_432", rows, p, c, v, rhs, None), 3)
    blocks = bc.pcg_restated(dtype, 3)[-1]
    print("%s: r'r of r0 %.6e, after %d iterations at degree 3 over 3 x 3 blocks %.6e (the restated run with the blocks alone: %.6e)" % (
        np.dtype(dtype).name, first, cb.ITERATIONS, last, blocks))
    assert np.isfinite(last) and last < first


# ---- 6: the gate ---------------------------------------------------------------------------------------------------------------------------

def test_gate_fused_middle_step_is_not_slower_than_its_torch_composition():
    """n = 4096^2 doubles, the middle step with minv, Level 2, one process, torch events on one stream; three warm-up rounds, 25
    rounds alternating the ways, medians.  Asserted: median(spmv_hip_cheby_step_f64) <= 1.00 x median(the torch way), the torch way
    being d.mul_(c), d.add_((minv * t).mul_(e)), z.add_(d) with c and e 0-dim device scalars -- no host read in either.  By bytes
    the fused call moves 6 vector passes (u, minv, d, z read, d, z written: 48 n) where the composition moves at least 9.  The four
    vectors are 537 MB: beyond the 256 MiB Infinity Cache, which is asserted.  A condition, not a measured margin; the ratio and
    the share of the same-process triad bandwidth are printed (tools/cheby_ab.py writes them to profiles/cheby_ab.log).
    Measured: the torch way 284.4 us, the fused step 162.4 us, ratio 0.571 against 0.667 by bytes; the step moves its bytes at
    4.96 TB/s, 0.921 of the same-process triad (tools/cheby_ab.py in another process: 285.1 against 158.4 us, 0.556)."""
    import torch
    n = 4096 * 4096
    assert 4 * n * 8 > 256 * 2 ** 20 and n * 8 < 2 ** 32
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(6)
    t, minv, d0, z0 = (torch.rand(n, dtype=torch.float64, device="cuda:0", generator=gen) * 2 - 1 for _ in range(4))
    coef = torch.tensor([0.0, 0.5, 0.25, 0.75, 0.125, 0.5], dtype=torch.float64, device="cuda:0")
    c, e = coef[2], coef[3]
    d, z, dt, zt = d0.clone(), z0.clone(), d0.clone(), z0.clone()
    s = torch.cuda.current_stream().cuda_stream

    def torch_way():
        dt.mul_(c)
        dt.add_((minv * t).mul_(e))
        zt.add_(dt)

    def fused():
        capi.cheby_step(n, 3, 1, coef, t, minv, d, z, None, None, None, 0, s)

    torch_way()
    fused()
    # (torch may contract c d + e s into a fused multiply-add: a rounding apart at the most)
    assert float((d - dt).abs().max()) <= 2.0 ** -52 and float((z - zt).abs().max()) <= 2.0 ** -51
    ta, tb, tc = (torch.zeros(2 * n, dtype=torch.float64, device="cuda:0") for _ in range(3))

    def triad():
        torch.add(tb, tc, alpha=0.5, out=ta)

    med = _alternate({"torch": torch_way, "fused": fused, "triad": triad})
    triad_bw = 3 * 2 * n * 8 / med["triad"]  # bytes per us
    print("n %d: the torch way (mul_, mul, mul_, add_, add_) median %.1f us, the fused middle step median %.1f us, ratio %.3f against %.3f by "
          "bytes; the fused step moves %.2f TB/s, %.3f of the same-process triad (%.2f TB/s)" % (
              n, med["torch"], med["fused"], med["fused"] / med["torch"], 6.0 / 9.0, 48.0 * n / med["fused"] * 1e-6,
              48.0 * n / med["fused"] / triad_bw, triad_bw * 1e-6))
    assert med["fused"] <= 1.00 * med["torch"], med
