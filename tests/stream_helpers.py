"""What test_gpu_streams.py is made of: a non-blocking side stream with a calibrated delay in front of it, device arrays that
are first filled with contents that are wrong but safe and get their real contents BEHIND the delay, and one `Case` per multiply
family (the device arrays, the call, the oracle's answer and its tolerance, the rows whose sums never meet in atomics) -- the
scaled forms of the float-tile multiplies included (ScaledCase)."""
import ctypes
import functools
import math
import time

import numpy as np

import compact_cases as cc
import helpers
import poison
import test_gpu_nonfinite as nf
from spmv_amd import capi, synth
from test_gpu_multivec import _mixed_lengths
from test_gpu_scaled import restate

HIP_STREAM_NON_BLOCKING = 0x01
SCRATCH_BYTES = 256 << 20   # one pass of the delay reads and writes this much
DELAY_MS, DELAY_CAP_MS = 50.0, 200.0
FRONT, BACK = 4, 6          # guard elements around x and y
SURE = nf.SURE


def torch():
    import torch as t
    return t


# ---- the side stream ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def hip():
    """The HIP runtime the library shares with torch (capi loads torch's copy first)."""
    capi.load()
    lib = ctypes.CDLL(capi.hip_runtime_path or "libamdhip64.so")
    lib.hipStreamGetFlags.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint)]
    lib.hipStreamGetFlags.restype = ctypes.c_int
    lib.hipStreamCreateWithFlags.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint]
    lib.hipStreamCreateWithFlags.restype = ctypes.c_int
    return lib


def stream_flags(s):
    flags = ctypes.c_uint(0xFFFFFFFF)
    rc = hip().hipStreamGetFlags(ctypes.c_void_p(s.cuda_stream), ctypes.byref(flags))
    assert rc == 0, "hipStreamGetFlags: %d" % rc
    return flags.value


def nonblocking_stream():
    """A stream the null stream does not wait for (and that does not wait for the null stream): torch's own where it is one,
    else one made with hipStreamNonBlocking and wrapped."""
    s = torch().cuda.Stream(device=0)
    if not stream_flags(s) & HIP_STREAM_NON_BLOCKING:
        h = ctypes.c_void_p()
        assert hip().hipStreamCreateWithFlags(ctypes.byref(h), HIP_STREAM_NON_BLOCKING) == 0
        s = torch().cuda.ExternalStream(h.value, device=0)
    assert s.cuda_stream != 0
    assert stream_flags(s) & HIP_STREAM_NON_BLOCKING, "the side stream is a blocking one: the null stream would wait for it"
    return s


class Side:
    """Two non-blocking streams, a scratch tensor each, and the number of passes over it that last about DELAY_MS."""

    def __init__(self):
        t = torch()
        self.streams = [nonblocking_stream(), nonblocking_stream()]
        self.s, self.s2 = self.streams
        self.scratch = [t.zeros(SCRATCH_BYTES // 8, dtype=t.float64, device="cuda:0") for _ in self.streams]
        t.cuda.synchronize()
        self.pass_ms = self._time(10) / 10.0
        self.passes = max(1, min(math.ceil(DELAY_MS / self.pass_ms), int(DELAY_CAP_MS / self.pass_ms)))
        self.delay_ms = self._time(self.passes)
        self.calls = 0
        self.longest_async_call = (0.0, "")
        self.started = time.perf_counter()
        print("side streams: one pass over %d MiB takes %.3f ms; D = %d passes give a delay of %.1f ms" % (
            SCRATCH_BYTES >> 20, self.pass_ms, self.passes, self.delay_ms))
        assert self.delay_ms <= 1.5 * DELAY_CAP_MS

    def _time(self, passes):
        t = torch()
        e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        with t.cuda.stream(self.s):
            self.scratch[0].add_(1.0)
            e0.record(self.s)
            for _ in range(passes):
                self.scratch[0].add_(1.0)
            e1.record(self.s)
        self.s.synchronize()
        return e0.elapsed_time(e1)

    def delay(self, which=0):
        """Bounded bandwidth work on the current stream (the caller has made streams[which] current)."""
        for _ in range(self.passes):
            self.scratch[which].add_(1.0)

    def note(self, seconds, what):
        self.calls += 1
        if seconds > self.longest_async_call[0]:
            self.longest_async_call = (seconds, what)

    def report(self):
        print("side streams: D = %d, delay %.1f ms; %d delayed calls; the longest host time of a delayed asynchronous call was "
              "%.0f us (%s); %.1f s since the fixture was made" % (self.passes, self.delay_ms, self.calls, 1e6 * self.longest_async_call[0],
                                                                    self.longest_async_call[1], time.perf_counter() - self.started))


# ---- device arrays with a wrong-but-safe fill ---------------------------------------------------------------------------------------

def bits(value, dtype):
    """The bit pattern of `value` as `dtype`, as the signed integer of that width (what torch's fill_ takes)."""
    dtype = np.dtype(dtype)
    return np.array(value, dtype=dtype).view({4: np.int32, 8: np.int64}[dtype.itemsize]).item()


Y_GUARD = {8: bits(poison.Y_GUARD_BITS, np.uint64), 4: bits(nf.Y_BITS32, np.uint32)}


class Arr:
    """A device array `live` the library is handed, its real contents in `stage` (on the device as well) and a fill that is wrong
    but safe.  With `guard`: FRONT / BACK elements of that bit pattern around the body, checked bitwise by body()."""

    def __init__(self, body, wrong, guard=None):
        t = torch()
        body = np.ascontiguousarray(body)
        assert body.dtype in (np.int32, np.float32, np.float64)
        self.dtype, self.shape, self.n = body.dtype, body.shape, body.size
        self.itype = {4: np.int32, 8: np.int64}[body.dtype.itemsize]
        self.front, self.back = (FRONT, BACK) if guard is not None else (0, 0)
        self.guard, self.wrong_bits = guard, wrong
        self.host = body.copy()
        self.stage = t.from_numpy(self._buffer(body)).to("cuda:0")
        self.live = t.empty_like(self.stage)
        self.ptr = self.live.data_ptr() + self.front * body.dtype.itemsize
        assert self.live.data_ptr() % 256 == 0
        self.put()
        t.cuda.synchronize()

    def _buffer(self, body):
        buf = np.full(self.front + self.n + self.back, self.guard or 0, dtype=self.itype)
        buf[self.front:self.front + self.n] = np.ascontiguousarray(body, dtype=self.dtype).ravel().view(self.itype)
        return buf

    def set(self, body):
        """New real contents (the next put() brings them)."""
        self.host = np.ascontiguousarray(body, dtype=self.dtype).reshape(self.shape).copy()
        self.stage.copy_(torch().from_numpy(self._buffer(self.host)))
        torch().cuda.synchronize()

    def wrong(self):
        self.live.fill_(self.wrong_bits)

    def put(self):
        self.live.copy_(self.stage, non_blocking=True)

    def snap(self):
        return self.live.clone()

    def body(self, snap=None, what=""):
        """The body as a host array; the guards must hold their pattern."""
        raw = (self.live if snap is None else snap).cpu().numpy()
        if self.guard is not None:
            g = np.concatenate([raw[:self.front], raw[self.front + self.n:]])
            assert np.all(g == self.guard), "%s: written outside the array's %d entries" % (what, self.n)
        return raw[self.front:self.front + self.n].view(self.dtype).reshape(self.shape).copy()


def nan_bits(dtype):
    return bits(np.nan, dtype)


def operand(body):
    """x, the values, y_in: NaN until the real contents arrive; NaN guards."""
    body = np.ascontiguousarray(body)
    return Arr(body, nan_bits(body.dtype), guard=nan_bits(body.dtype))


def result(body):
    """y: the guard pattern everywhere until the real contents arrive, and around them afterwards."""
    body = np.ascontiguousarray(body)
    return Arr(body, Y_GUARD[body.dtype.itemsize], guard=Y_GUARD[body.dtype.itemsize])


def index_array(body):
    """row_ptr (every row empty), columns and row indices (column / row 0: in range): zeros."""
    return Arr(np.ascontiguousarray(body, dtype=np.int32), 0)


def value_array(body, dtype=np.float64):
    return Arr(np.ascontiguousarray(np.asarray(body, dtype=np.float64).astype(dtype)), nan_bits(dtype))


def csr_arrays(p, c, v, dtype=np.float64):
    return [index_array(p), index_array(c), value_array(v, dtype)]


# ---- the protocol --------------------------------------------------------------------------------------------------------------------

def delayed(side, operands, call, results, what, asynchronous=True, which=0):
    """The protocol of the module docstring on streams[which]: wrong contents, synchronize, then on the stream the delay, the real
    contents, call(raw stream), a copy of every result; returns the results' bodies (guards checked)."""
    t = torch()
    s = side.streams[which]
    for o in operands:
        o.wrong()
    t.cuda.synchronize()
    with t.cuda.stream(s):
        side.delay(which)
        for o in operands:
            o.put()
        assert not s.query(), what + ": the delay was over before the call: nothing would be proved"
        t0 = time.perf_counter()
        out = call(s.cuda_stream)
        dt = time.perf_counter() - t0
        still_running = not s.query()
        snaps = [r.snap() for r in results]
    s.synchronize()
    if asynchronous:
        assert still_running, what + ": the call returned after the delay had ended (%.1f ms on the host): it waited for the stream" % (1e3 * dt)
        side.note(dt, what)
    bodies = [r.body(snap, what) for r, snap in zip(results, snaps)]
    return bodies, out


def serial(call, x, y, runs):
    """`runs` accumulating multiplies on the null stream, everything synchronised before and after each."""
    t = torch()
    x.put()
    y.put()
    t.cuda.synchronize()
    for _ in range(runs):
        call(0, x.ptr, y.ptr)
        t.cuda.synchronize()
    return y.body(what="serial run")


def on_stream(s, call, x, y, runs):
    """The same on the stream `s`, eagerly."""
    t = torch()
    with t.cuda.stream(s):
        x.put()
        y.put()
        for _ in range(runs):
            call(s.cuda_stream, x.ptr, y.ptr)
        snap = y.snap()
    s.synchronize()
    return y.body(snap, "eager run")


# ---- one multiply family on one matrix -------------------------------------------------------------------------------------------

def assert_rows_bitwise(got, want, only, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    a, b = got.view(u), want.view(u)
    keep = np.ones(got.shape, dtype=bool) if only is None else np.broadcast_to(np.asarray(only, dtype=bool).reshape((-1,) + (1,) * (got.ndim - 1)), got.shape)
    off = (a != b) & keep
    if off.any():
        k = np.argwhere(off)[0]
        raise AssertionError("%s: %d of %d values differ bitwise from the serial result, first at %s: %r vs %r" % (
            what, int(off.sum()), int(keep.sum()), tuple(k), got[tuple(k)], want[tuple(k)]))


class Case:
    """`operator`: the CSR arrays (rows, cols, p, c, v) of the matrix the multiply applies -- the expansion of a stored triangle,
    the transpose -- in fp64; `mats`: the device arrays the library reads; planner() -> call(stream, x address, y address), a
    fresh plan each time; `sure`: whether rows of up to SURE entries are summed without atomics (False: no bitwise claim)."""

    def __init__(self, what, oracle, operator, mats, sure=True, k=1, xy=np.float64):
        self.what, self.oracle, self.operator, self.mats, self.k, self.xy = what, oracle, operator, mats, k, np.dtype(xy)
        rows, cols, p, c, v = operator
        self.lens = np.diff(p.astype(np.int64))
        self.nterms = max(4096, int(self.lens.max()) if rows else 0)
        self.sure = (self.lens <= SURE) if sure else None
        self.plans = []
        self.planner = None

    def vectors(self, seed=0):
        """(x, y): device operands with their own host contents; column q of a block is (q + 1) times column 0."""
        rows, cols = self.operator[:2]
        x = synth.x_vector(cols, seed=3 + 10 * seed)
        y0 = np.random.default_rng(7 + 10 * seed).uniform(-1.0, 1.0, size=rows)
        if self.k > 1:
            x = np.ascontiguousarray(x[:, None] * (np.arange(self.k)[None, :] + 1.0))
            y0 = np.random.default_rng(7 + 10 * seed).uniform(-1.0, 1.0, size=(rows, self.k))
        return operand(x.astype(self.xy)), result(y0.astype(self.xy))

    def reference(self, x, y0, runs):
        """(the oracle's y after `runs` accumulating multiplies, runs (|A||x|) + |y0|), in fp64."""
        rows, cols, p, c, v = self.operator
        x, y0 = np.asarray(x, dtype=np.float64).reshape(cols, -1), np.asarray(y0, dtype=np.float64).reshape(rows, -1)
        ref = np.stack([self.oracle.csr_spmv(rows, p, c, v, np.ascontiguousarray(x[:, q]), y=np.ascontiguousarray(y0[:, q]), num_threads=1, runs=runs)
                        for q in range(x.shape[1])], axis=1)
        scale = np.stack([runs * helpers.abs_products(rows, p, c, v, x[:, q]) for q in range(x.shape[1])], axis=1) + np.abs(y0)
        return ref, scale

    def check(self, got, x, y0, runs, same_as, what):
        """Against the oracle within the family's tolerance; bit for bit `same_as` (the same plan's serial result) where sure."""
        ref, scale = self.reference(x.host, y0.host, runs)
        got2 = np.asarray(got).reshape(ref.shape)
        if self.xy == np.float32:
            self._check_float_pair(got2[:, 0], x.host, y0.host, runs, what)
        else:
            for q in range(ref.shape[1]):
                helpers.assert_close(got2[:, q], ref[:, q], scale[:, q], what="%s, column %d against the oracle" % (what, q), nterms=runs * self.nterms)
        if same_as is not None and self.sure is not None:
            assert np.any(self.sure)
            assert_rows_bitwise(np.asarray(got).reshape(len(self.lens), -1), np.asarray(same_as).reshape(len(self.lens), -1), self.sure, what)

    def _check_float_pair(self, got, x, y0, runs, what):
        """Float x and y: every run is y <- fl32(y + A x) with the sum in fp64.  With T_r = y0 + r (A x) exact and e_r = |y_r - T_r|:
        e_r <= (e_{r-1} + d_r)(1 + 2^-24) + 2^-24 |T_r| + 2^-149, d_r = 2 nterms 2^-53 (r |A||x| + |y0|) the bound on two summation
        orders (helpers.assert_close's second clause).  For one run that is test_gpu_compact32.py's bound."""
        rows, cols, p, c, v = self.operator
        prod = helpers.abs_products(rows, p, c, v, x.astype(np.float64))
        u, e = 2.0 ** -24, np.zeros(rows)
        for r in range(1, runs + 1):
            t_r = self.oracle.csr_spmv(rows, p, c, v, x.astype(np.float64), y=y0.astype(np.float64), num_threads=1, runs=r)
            d_r = 2.0 * self.nterms * 2.0 ** -53 * (r * prod + np.abs(y0.astype(np.float64)))
            e = (e + d_r) * (1.0 + u) + u * np.abs(t_r) + 2.0 ** -149
        err = np.abs(got.astype(np.float64) - t_r)
        assert np.all(np.isfinite(got)) and np.all(err <= e), "%s: %d rows outside the float pair's bound, worst ratio %.3g" % (
            what, int((err > e).sum()), float(np.max(err / e)))

    def close(self):
        for plan in self.plans:
            plan.close()
        self.plans = []


@functools.lru_cache(maxsize=2)
def default_matrix(name):
    make, flags, index_values, reached = nf.DEFAULT_CASES[name]
    return nf._csr(*make()), flags, index_values, reached


def default_chain(plan, mats, index_values, stream=0, step=None):
    """The planning steps of the default plan in order; `step(name, fn)` runs one (default: just calls it on `stream`)."""
    P, C, V = (m.ptr for m in mats)
    steps = [("confirm_blocks", lambda st: plan.confirm_blocks(P, C, None, st)),
             ("compress", lambda st: plan.compress(C, st)),
             ("repack", lambda st: plan.repack(P, C, V, st))]
    if index_values:
        steps.append(("index_values", lambda st: plan.index_values(V, st)))
    steps += [("refresh_values", lambda st: plan.refresh_values(P, C, V, st)),
              ("verify", lambda st: plan.verify(C, st))]
    for name, fn in steps:
        if step is None:
            fn(stream)
        else:
            step(name, fn)


def default_case(oracle, name):
    """The default plan as test_gpu_nonfinite.py builds it (compress, repack, index_values), shown to reach its tile class."""
    A, flags, index_values, reached = default_matrix(name)
    rows, cols, p, c, v = A
    mats = csr_arrays(p, c, v)
    case = Case("default plan, " + name, oracle, A, mats)
    case.flags, case.index_values, case.reached = flags, index_values, reached
    P, C, V = (m.ptr for m in mats)

    def planner():
        plan = capi.CsrPlan(rows, cols, p, capi.CSR_AUTO, 0, flags)
        case.plans.append(plan)
        plan.compress(C, 0)
        plan.repack(P, C, V, 0)
        if index_values:
            plan.index_values(V, 0)
        case.info = plan.info()
        print("%s: plan_info %s" % (case.what, {k: n for k, n in nf._counts(case.info).items() if n}))
        assert reached(case.info), (case.what, nf._counts(case.info))
        if case.info["panel_tiles"] > 0:
            case.sure = None  # column panels: partial sums meet in atomics
        case.plan = plan
        return lambda st, xp, yp: plan.spmv(P, C, V, xp, yp, st)

    case.planner = planner
    return case


def symv_case(oracle, name):
    make, max_windows, window_doubles, info_ok = nf.SYMV_CASES[name]
    T = make()
    rows, _, p, c, v = T
    assert capi.csr_triangle(rows, p, c)[0] == capi.TRIANGLE_LOWER
    mats = csr_arrays(p, c, v)
    case = Case("symv, " + name, oracle, nf._expand(*T), mats, sure=False)
    P, C, V = (m.ptr for m in mats)

    def planner(stream=0):
        plan = capi.SymPlan(rows, p, C, capi.SYMMETRIC, max_windows, window_doubles, stream)
        case.plans.append(plan)
        case.info = plan.info()
        assert info_ok(case.info), (case.what, case.info)
        return lambda st, xp, yp: plan.symv(P, C, V, xp, yp, st)

    case.planner = planner
    return case


def spmv_t_case(oracle, name):
    make, max_windows, window_doubles, info_ok = nf.SPMV_T_CASES[name]
    A = nf._csr(*make())
    rows, cols, p, c, v = A
    mats = csr_arrays(p, c, v)
    case = Case("spmv_t, " + name, oracle, nf._transpose(*A), mats, sure=False)
    P, C, V = (m.ptr for m in mats)

    def planner(stream=0):
        plan = capi.TrPlan(rows, cols, p, C, max_windows, window_doubles, stream)
        case.plans.append(plan)
        case.info = plan.info()
        assert info_ok(case.info), (case.what, case.info)
        return lambda st, xp, yp: plan.spmv_t(P, C, V, xp, yp, st)

    case.planner = planner
    return case


@functools.lru_cache(maxsize=1)
def mixed_lengths():
    return nf._csr(*_mixed_lengths())


def spmm_case(oracle, k, flags=0):
    A = mixed_lengths()
    rows, cols, p, c, v = A
    mats = csr_arrays(p, c, v)
    case = Case("spmm k=%d flags %x on row lengths 1 ... 9000" % (k, flags), oracle, A, mats, k=k)
    P, C, V = (m.ptr for m in mats)

    def planner():
        plan = capi.MvPlan(rows, cols, p, k, flags, 0)
        case.plans.append(plan)
        case.info = plan.info()
        # (the tile kernel and the long-row kernel: rows of more than 4096 entries, none under exact order; k = 5 takes two passes)
        assert case.info["k"] == k and case.info["tiles"] > 0 and case.info["long_rows"] == (0 if flags else int((case.lens > 4096).sum()))
        assert case.info["passes"] == (1 if k == 3 else 2), case.info
        return lambda st, xp, yp: plan.spmm(P, C, V, xp, yp, ldx=k, ldy=k, stream=st)

    case.planner = planner
    return case


FLOAT_FAMILIES = ("spmv_f32", "spmv_c16", "spmv_c16_f64", "spmv_c16_f32xy")


def float_family_case(oracle, family):
    """The four float-value multiplies on mixed_mesh_and_graph: compact and wide tiles in one launch."""
    rows, cols, p, c, v = cc.matrix("mixed_mesh_and_graph")
    a32 = nf._f32(v)
    values = v if family == "spmv_c16_f64" else a32.astype(np.float64)
    mats = csr_arrays(p, c, values, np.float64 if family == "spmv_c16_f64" else np.float32)
    case = Case("%s on mixed_mesh_and_graph" % family, oracle, (rows, cols, p, c, values), mats,
                xy=np.float32 if family == "spmv_c16_f32xy" else np.float64)
    P, C, V = (m.ptr for m in mats)

    def planner():
        if family == "spmv_f32":
            plan = capi.F32Plan(rows, cols, p, 0, 0)
            case.info = plan.info()
            assert case.info["tiles"] > 0
            multiply = plan.spmv
        else:
            plan = capi.C16Plan(rows, cols, p, c, 0, 0)
            case.info = plan.info()
            assert case.info["compact_tiles"] > 100 and case.info["wide_tiles"] > 100, case.info
            multiply = {"spmv_c16": plan.spmv, "spmv_c16_f64": plan.spmv_f64, "spmv_c16_f32xy": plan.spmv_f32xy}[family]
        case.plans.append(plan)
        return lambda st, xp, yp: multiply(P, C, V, xp, yp, st)

    case.planner = planner
    return case


SCALED_KINDS = ("f32", "c16", "c16_f64", "c16_f32xy")


class ScaledCase(Case):
    """y_out <- alpha A x + beta y_in (include/spmv_hip_scaled.h).  planner() plans and returns the in-place residual step
    call(stream, x address, y address), y <- y - A x, for the tests that chain accumulating multiplies; case.scaled(stream, x
    address, alpha, beta, y_in address, y_out address) is the plan's scaled multiply and, for the float pair, case.scaled_c16 the
    double-vector multiply through the SAME plan.  No atomics in this family: every row is claimed bit for bit."""

    def row_sums(self, x):
        """(z, (|A||x|)_i): the oracle's CSR kernel run once from y = +0.0."""
        rows, cols, p, c, v = self.operator
        x = np.asarray(x, dtype=np.float64)
        return self.oracle.csr_spmv(rows, p, c, v, x, num_threads=1, runs=1), helpers.abs_products(rows, p, c, v, x)

    def check(self, got, x, y0, runs, same_as, what):
        """`runs` residual steps in place: bit for bit `same_as`; double vectors within helpers.assert_close of the restatement."""
        assert same_as is not None
        assert_rows_bitwise(np.asarray(got), np.asarray(same_as), None, what)
        if self.xy == np.float64:
            z, absz = self.row_sums(x.host)
            want = y0.host
            for _ in range(runs):
                want = restate(-1.0, 1.0, z, want, np.float64)
            helpers.assert_close(got, want, runs * absz + np.abs(y0.host), what=what + " against the restatement", nterms=runs * self.nterms)


def scaled_family_case(oracle, kind):
    """The four scaled float-tile multiplies on mixed_mesh_and_graph: compact and wide tiles in one launch."""
    rows, cols, p, c, v = cc.matrix("mixed_mesh_and_graph")
    a32 = nf._f32(v)
    values = v if kind == "c16_f64" else a32.astype(np.float64)
    mats = csr_arrays(p, c, values, np.float64 if kind == "c16_f64" else np.float32)
    case = ScaledCase("spmv_%s_scaled on mixed_mesh_and_graph" % kind, oracle, (rows, cols, p, c, values), mats,
                      xy=np.float32 if kind == "c16_f32xy" else np.float64)
    P, C, V = (m.ptr for m in mats)

    def planner():
        if kind == "f32":
            plan = capi.F32Plan(rows, cols, p, 0, 0)
            case.info = plan.info()
            assert case.info["tiles"] > 0
            multiply = plan.spmv_scaled
        else:
            plan = capi.C16Plan(rows, cols, p, c, 0, 0)
            case.info = plan.info()
            assert case.info["compact_tiles"] > 100 and case.info["wide_tiles"] > 100, case.info
            multiply = {"c16": plan.spmv_scaled, "c16_f64": plan.spmv_f64_scaled, "c16_f32xy": plan.spmv_f32xy_scaled}[kind]
            case.scaled_c16 = lambda st, xp, alpha, beta, yi, yo: plan.spmv_scaled(P, C, V, xp, alpha, beta, yi, yo, st)
        case.plans.append(plan)
        case.scaled = lambda st, xp, alpha, beta, yi, yo: multiply(P, C, V, xp, alpha, beta, yi, yo, st)
        return lambda st, xp, yp: multiply(P, C, V, xp, -1.0, 1.0, yp, yp, st)

    case.planner = planner
    return case
