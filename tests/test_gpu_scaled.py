"""y_out <- alpha A x + beta y_in for the four float-tile multiplies (include/spmv_hip_scaled.h) on the MI355X:
spmv_hip_csr_spmv_f32_scaled, _c16_scaled, _c16_f64_scaled and _c16_f32xy_scaled, and spmv_hip_run_scaled on contexts of formats
7 to 10.

With z the row sums of the multiply without a scale, the contract is (T)(fl(alpha z) + fl(beta y_in)), so under
SPMV_HIP_FLAG_EXACT_ORDER every result is compared BIT FOR BIT with a numpy restatement: z from the oracle's CSR kernel run once
on y = +0.0 (the float paths on the narrowed values, f32xy on x widened from float), then alpha * z, beta * y_in and their sum as
separate numpy operations (no product where alpha or beta is 0, as the header says), rounded to float for f32xy.  Level 2 runs
with NaN guard elements around x and y_in, sentinels around y_out, and the column and value arrays as views into larger buffers
whose neighbours hold column 0 and NaN (the guard scheme of test_gpu_compact64.py).

Scale factors that are themselves NaN, +-Inf, -0.0, denormal or large enough to overflow follow the same restatement on clean
operands (-0.0 counts as zero for both), and float vectors are held bit for bit at ties, at FLT_MAX and in the float denormals
(float_edges.py).  Non-finite OPERANDS are test_gpu_nonfinite.py's, the caller's stream test_gpu_streams.py's."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import compact_cases as cc
import float_edges
import helpers
import oracle_py
import poison
from spmv_amd import capi, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "spmv-cache-trace_amd", "spmv-cache-trace-hip")
BUS = os.path.join(ROOT, "tests", "golden", "bus1138_like.mtx")
GUARD = 5   # elements in front of and behind x and every y on the device
PAD = 8     # entries in front of and behind the column and value arrays
SENTINEL = -7.25
CALLS = 3   # chained calls

KINDS = ("f32", "c16", "c16_f64", "c16_f32xy")
PAIRS = [(1.0, 1.0), (1.0, 0.0), (-1.0, 1.0), (0.375, -2.5), (0.0, 0.5), (0.0, 0.0)]
# the matrices that reach all four store sites of the tile (the stream tile with one and with several lanes per row, the
# entry-by-entry tile and empty rows, the long row in both orders, compact and wide tiles in one launch) and the plans without tiles
MATRICES = ["poisson_512", "queen_40_32_24", "rows_0_to_7_ragged_end", "empty_rows", "dense_row_9000_compact", "dense_row_9000_wide",
            "mixed_mesh_and_graph", "one_by_one", "no_rows", "no_cols", "no_entries"]


def _f32(a):
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(np.asarray(a, dtype=np.float64).astype(np.float32))


def _bits(got, want, what):
    """Bit for bit; floats are widened first (exact, and it keeps the sign of a zero)."""
    helpers.assert_bitexact(np.asarray(got).astype(np.float64), np.asarray(want).astype(np.float64), what)


class Host:
    """The host side of one matrix: values that are not floats (for c16_f64), their narrowing, x and y0 as doubles and as floats,
    and per multiply the row sums z of the oracle's CSR kernel from y = +0.0 and (|A||x|)_i."""

    def __init__(self, name):
        self.name = name
        self.rows, self.cols, self.p, self.c, v = cc.matrix(name)
        rng = np.random.default_rng(len(name) + 23)
        if len(v) and np.all(_f32(v).astype(np.float64) == v):  # a stencil's -1 and 4: doubles that no float holds instead
            v = rng.uniform(-1.0, 1.0, size=len(v))
        self.v, self.a32 = v, _f32(v)
        self.x, self.y0 = synth.x_vector(self.cols), rng.uniform(-1.0, 1.0, size=self.rows)
        self.x32, self.y0_32 = _f32(self.x), _f32(self.y0)
        self._z = {}

    def values(self, kind):
        return self.v if kind == "c16_f64" else self.a32

    def vectors(self, kind):
        return (self.x32, self.y0_32, np.float32) if kind == "c16_f32xy" else (self.x, self.y0, np.float64)

    def z(self, kind):
        """(z, (|A||x|)_i) of the multiply `kind`; f32 and c16 are one operator."""
        key = "c16" if kind == "f32" else kind
        if key not in self._z:
            a, x = self.values(kind).astype(np.float64), self.vectors(kind)[0].astype(np.float64)
            if self.rows == 0 or len(self.c) == 0:
                self._z[key] = (np.zeros(self.rows), np.zeros(self.rows))
            else:
                self._z[key] = (oracle_py.Oracle().csr_spmv(self.rows, self.p, self.c, a, x, num_threads=1, runs=1),
                                helpers.abs_products(self.rows, self.p, self.c, a, x))
        return self._z[key]


@functools.lru_cache(maxsize=2)
def host(name):
    return Host(name)


def restate(alpha, beta, z, y_in, dtype):
    """The header's contract in numpy: two products and a sum, each rounded; no product where the factor is 0."""
    y_in = np.asarray(y_in).astype(np.float64)
    if alpha == 0.0:
        r = beta * y_in if beta != 0.0 else np.zeros(len(z))
    elif beta == 0.0:
        r = alpha * z
    else:
        az, by = alpha * z, beta * y_in
        r = az + by
    with np.errstate(over="ignore"):
        return r.astype(dtype)


def _padded(a, dtype, fill):
    import torch
    buf = torch.full((len(a) + 2 * PAD,), fill, dtype=dtype, device="cuda:0")
    if len(a):
        buf[PAD:PAD + len(a)] = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0").to(dtype)
    return buf, buf.data_ptr() + buf.element_size() * PAD


class Vec:
    """n elements on the device between GUARD elements of `guard` (NaN around what is read, the sentinel around what is written)."""

    def __init__(self, a, dtype, guard=float("nan")):
        import torch
        self.n, self.guard = len(a), guard
        self.t = torch.full((self.n + 2 * GUARD,), guard, dtype={np.float64: torch.float64, np.float32: torch.float32}[dtype], device="cuda:0")
        if self.n:
            self.t[GUARD:GUARD + self.n] = torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to("cuda:0")
        self.ptr = self.t.data_ptr() + self.t.element_size() * GUARD

    def body(self, what=""):
        """The n elements, after checking that the guards are what they were."""
        h = self.t.cpu().numpy()
        edge = np.concatenate([h[:GUARD], h[GUARD + self.n:]])
        assert np.all(np.isnan(edge)) if np.isnan(self.guard) else np.all(edge == self.guard), what + ": written outside its elements"
        return h[GUARD:GUARD + self.n].copy()


class Dev:
    """The arrays of one matrix for one multiply on the device, its plan, and scaled calls over them."""

    def __init__(self, h, kind, flags=0):
        import torch
        self.torch, self.h, self.kind, self.flags = torch, h, kind, flags
        self.stream = torch.cuda.current_stream().cuda_stream
        self.tp = torch.from_numpy(np.ascontiguousarray(h.p, dtype=np.int32)).to("cuda:0")
        self.bc, self.ac = _padded(h.c, torch.int32, 0)
        vals = h.values(kind)
        self.bv, self.av = _padded(vals, torch.float64 if kind == "c16_f64" else torch.float32, float("nan"))
        self.xh, self.y0, self.dtype = h.vectors(kind)
        self.x = Vec(self.xh, self.dtype)
        if kind == "f32":
            self.plan = capi.F32Plan(h.rows, h.cols, h.p, flags, self.stream)
        else:
            self.plan = capi.C16Plan(h.rows, h.cols, h.p, h.c, flags, self.stream)
        self.scaled = {"f32": self.plan.spmv_scaled, "c16": self.plan.spmv_scaled, "c16_f64": getattr(self.plan, "spmv_f64_scaled", None),
                       "c16_f32xy": getattr(self.plan, "spmv_f32xy_scaled", None)}[kind]
        self.plain = {"f32": self.plan.spmv, "c16": self.plan.spmv, "c16_f64": getattr(self.plan, "spmv_f64", None),
                      "c16_f32xy": getattr(self.plan, "spmv_f32xy", None)}[kind]

    def close(self):
        self.plan.close()

    def vec(self, a, guard=float("nan")):
        return Vec(a, self.dtype, guard)

    def out(self):
        return Vec(np.full(self.h.rows, np.nan), self.dtype, SENTINEL)

    def call(self, alpha, beta, y_in, y_out, matrix=True, x=True, stream=None):
        """One scaled call; y_in a Vec, an address or None."""
        yi = y_in.ptr if isinstance(y_in, Vec) else y_in
        m = (self.tp.data_ptr(), self.ac, self.av) if matrix else (0, 0, 0)
        self.scaled(m[0], m[1], m[2], self.x.ptr if x else 0, alpha, beta, yi, y_out.ptr, self.stream if stream is None else stream)

    def accumulate(self, y):
        self.plain(self.tp.data_ptr(), self.ac, self.av, self.x.ptr, y.ptr, self.stream)

    def inputs_unchanged(self):
        self.torch.cuda.synchronize()
        assert np.array_equal(self.x.body("x"), self.xh), "x changed"
        assert np.array_equal(self.bc.cpu().numpy()[PAD:PAD + len(self.h.c)], self.h.c), "columns changed"


# ---- exact order: bit for bit against the restatement, three chained calls, in place and out of place ------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", MATRICES)
def test_exact_order_bit_for_bit_against_the_restatement(name, kind):
    h = host(name)
    z, _ = h.z(kind)
    dev = Dev(h, kind, capi.FLAG_EXACT_ORDER)
    for alpha, beta in PAIRS:
        tag = "%s, %s, alpha %g, beta %g" % (name, kind, alpha, beta)
        want = [dev.y0]
        for _ in range(CALLS):
            want.append(restate(alpha, beta, z, want[-1], dev.dtype))
        # in place: y_in == y_out, the sentinels of y_out around it
        y = dev.vec(dev.y0, SENTINEL)
        for _ in range(CALLS):
            dev.call(alpha, beta, y, y)
        got = y.body(tag + ", in place")
        assert np.all(np.isfinite(got)), tag + ": a neighbouring NaN was summed"
        _bits(got, want[-1], tag + ": %d chained calls in place" % CALLS)
        # out of place: y0 -> b1 -> b2 -> b3; every y_in comes back as it was
        chain = [dev.vec(dev.y0)] + [dev.out() for _ in range(CALLS)]
        for k in range(CALLS):
            dev.call(alpha, beta, chain[k], chain[k + 1])
        for k in range(CALLS + 1):
            _bits(chain[k].body(tag + ", out of place"), want[k], tag + ": out of place, the vector after call %d" % k)
    dev.inputs_unchanged()
    if kind != "f32" and h.rows and len(h.c):
        info = dev.plan.info()
        if name == "mixed_mesh_and_graph":
            assert info["compact_tiles"] > 100 and info["wide_tiles"] > 100  # both column sources in one launch
        if name.startswith("dense_row_9000"):
            assert info["long_row_tiles"] == 1
    dev.close()


# ---- default order: the project's tolerance, and (1, 1) in place is the multiply that was there ------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", MATRICES)
def test_default_order_within_the_tolerance_and_1_1_in_place_is_the_existing_multiply(name, kind):
    """helpers.assert_close with scale |alpha| (|A||x|)_i + |beta| |y_in_i| and the helper's own tolerance.  The float vectors of
    c16_f32xy cannot be held to 1e-10 of an fp64 reference, and need not be: its tiles, lanes and order are those of
    spmv_hip_csr_spmv_c16_scaled through the same plan, so its result must be the BITS of that multiply's (on x and y_in
    widened) rounded to float once -- and that multiply's fp64 result is what assert_close judges."""
    h = host(name)
    z, absz = h.z(kind)
    dev = Dev(h, kind)
    wide = Dev(h, "c16") if kind == "c16_f32xy" else None
    if wide:  # the double-vector multiply over the float x and y0, widened
        wide.xh, wide.y0 = dev.xh.astype(np.float64), dev.y0.astype(np.float64)
        wide.x = Vec(wide.xh, np.float64)
    longest = int(np.max(np.diff(h.p))) if h.rows else 0
    for alpha, beta in PAIRS:
        tag = "%s, %s, alpha %g, beta %g (default order)" % (name, kind, alpha, beta)
        y_in, y_out = dev.vec(dev.y0), dev.out()
        dev.call(alpha, beta, y_in, y_out)
        got = y_out.body(tag)
        assert np.all(np.isfinite(got)), tag + ": a neighbouring NaN was summed"
        _bits(y_in.body(tag), dev.y0, tag + ": y_in changed")
        y64 = got
        if wide:
            w_out = wide.out()
            wide.call(alpha, beta, wide.vec(wide.y0), w_out)
            y64 = w_out.body(tag)
            with np.errstate(over="ignore"):
                _bits(got, y64.astype(np.float32), tag + ": against spmv_hip_csr_spmv_c16_scaled through the same plan, rounded once")
        want = restate(alpha, beta, z, dev.y0, np.float64)
        scale = abs(alpha) * absz + abs(beta) * np.abs(dev.y0.astype(np.float64))
        helpers.assert_close(y64, want, scale, what=tag, nterms=max(4096, longest))
        again = dev.out()
        dev.call(alpha, beta, y_in, again)
        _bits(again.body(tag), got, tag + ": two identical calls")
    # alpha = 1, beta = 1, y_in == y_out: the bits of y += A x, in both orders of the two calls
    a, b = dev.vec(dev.y0, SENTINEL), dev.vec(dev.y0, SENTINEL)
    dev.call(1.0, 1.0, a, a)
    dev.accumulate(b)
    dev.accumulate(a)
    dev.call(1.0, 1.0, b, b)
    _bits(a.body(), b.body(), "%s, %s: scaled then existing against existing then scaled" % (name, kind))
    c = dev.vec(dev.y0, SENTINEL)
    dev.accumulate(c)
    dev.accumulate(c)
    _bits(a.body(), c.body(), "%s, %s: (1, 1) in place against the existing multiply" % (name, kind))
    dev.inputs_unchanged()
    dev.close()
    if wide:
        wide.close()


# ---- beta == 0: y_in is not read; alpha == 0: neither the matrix nor x is ---------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("flags", [0, capi.FLAG_EXACT_ORDER])
@pytest.mark.parametrize("name", ["queen_40_32_24", "rows_0_to_7_ragged_end", "dense_row_9000_wide", "no_entries"])
def test_beta_0_never_reads_y_in_and_alpha_0_never_reads_the_matrix_or_x(name, flags, kind):
    h = host(name)
    dev = Dev(h, kind, flags)
    tag = "%s, %s, flags %d" % (name, kind, flags)
    for alpha in (1.0, -0.375, 0.0):
        clean = dev.out()
        dev.call(alpha, 0.0, dev.vec(dev.y0), clean)
        want = clean.body(tag)
        assert np.all(np.isfinite(want))
        for y_in in (dev.vec(np.full(h.rows, np.nan)), None):
            out = dev.out()
            dev.call(alpha, 0.0, y_in, out)
            _bits(out.body(tag), want, "%s, alpha %g, beta 0: y_in %s" % (tag, alpha, "null" if y_in is None else "full of NaN"))
        y = dev.vec(np.full(h.rows, np.inf), SENTINEL)  # in place over Inf
        dev.call(alpha, 0.0, y, y)
        _bits(y.body(tag), want, "%s, alpha %g, beta 0: in place over Inf" % (tag, alpha))
        if alpha == 0.0:
            _bits(want, np.zeros(h.rows), tag + ": alpha 0, beta 0 is +0.0")
    want = restate(0.0, -2.5, np.zeros(h.rows), dev.y0, dev.dtype)
    keep, poisoned = dev.x, dev.vec(np.full(h.cols, np.nan))
    for what, kw in (("x full of NaN", {}), ("null matrix and x pointers", {"matrix": False, "x": False})):
        dev.x = poisoned if not kw else keep
        out = dev.out()
        dev.call(0.0, -2.5, dev.vec(dev.y0), out, **kw)
        _bits(out.body(tag), want, "%s, alpha 0, beta -2.5: %s" % (tag, what))
    dev.x = keep
    dev.inputs_unchanged()
    dev.close()


# ---- refusals: nothing is launched ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_refusals_launch_nothing(kind):
    h = host("queen_40_32_24")
    dev = Dev(h, kind)
    es = 4 if kind == "c16_f32xy" else 8
    tp, ac, av, x = dev.tp.data_ptr(), dev.ac, dev.av, dev.x.ptr
    big = dev.vec(np.concatenate([dev.y0, dev.y0]), SENTINEL)  # room for a partial overlap
    y_in = dev.vec(dev.y0)
    s = dev.stream
    cases = [("y_out == x", (tp, ac, av, x, 1.0, 1.0, y_in.ptr, x), capi.ERR_INVALID),
             ("partial overlap", (tp, ac, av, x, 1.0, 1.0, big.ptr, big.ptr + es * (h.rows // 2)), capi.ERR_INVALID),
             ("overlap by one element", (tp, ac, av, x, 1.0, 1.0, big.ptr + es * (h.rows - 1), big.ptr), capi.ERR_INVALID),
             ("misaligned columns", (tp, ac + 4, av, x, 1.0, 1.0, y_in.ptr, big.ptr), capi.ERR_ALIGN),
             ("misaligned values", (tp, ac, av + 8, x, 1.0, 1.0, y_in.ptr, big.ptr), capi.ERR_ALIGN),
             ("null y_in with beta != 0", (tp, ac, av, x, 1.0, 0.5, 0, big.ptr), capi.ERR_INVALID),
             ("null y_in with beta != 0 and alpha == 0", (0, 0, 0, 0, 0.0, 0.5, 0, big.ptr), capi.ERR_INVALID),
             ("null y_out", (tp, ac, av, x, 1.0, 0.0, 0, 0), capi.ERR_INVALID),
             ("null values", (tp, ac, 0, x, 1.0, 1.0, y_in.ptr, big.ptr), capi.ERR_INVALID),
             ("null x with alpha != 0", (tp, ac, av, 0, 1.0, 1.0, y_in.ptr, big.ptr), capi.ERR_INVALID)]
    if kind == "c16_f32xy":
        cases += [("misaligned float y_out", (tp, ac, av, x, 1.0, 0.0, 0, big.ptr + 2), capi.ERR_ALIGN),
                  ("misaligned float y_in", (tp, ac, av, x, 1.0, 1.0, y_in.ptr + 2, big.ptr), capi.ERR_ALIGN)]
    for what, args, code in cases:
        with pytest.raises(capi.SpmvHipError) as e:
            dev.scaled(*args, s)
        assert e.value.code == code, what
    # y_in == x is valid (both are only read), and adjacent y_in and y_out do not overlap
    assert h.rows == h.cols
    out, ref = dev.out(), dev.out()
    dev.scaled(tp, ac, av, x, 1.0, 1.0, x, out.ptr, s)
    dev.call(1.0, 1.0, dev.vec(dev.xh), ref)
    _bits(out.body(), ref.body(), "y_in == x against y_in a copy of x")
    pair = dev.vec(np.concatenate([dev.y0, dev.y0]), SENTINEL)
    dev.scaled(tp, ac, av, x, 0.0, 1.0, pair.ptr, pair.ptr + es * h.rows, s)
    _bits(pair.body(), np.concatenate([dev.y0, dev.y0]), "adjacent y_in and y_out")
    _bits(big.body("refused calls"), np.concatenate([dev.y0, dev.y0]), "a refused call wrote y")
    _bits(y_in.body("refused calls"), dev.y0, "a refused call wrote y_in")
    dev.inputs_unchanged()
    dev.close()


# ---- Level 1 ---------------------------------------------------------------------------------------------------------------------

UPLOADS = {"f32": ("upload_csr_f32values", 7), "c16": ("upload_csr_compact", 8), "c16_f64": ("upload_csr_compact_f64", 9),
           "c16_f32xy": ("upload_csr_compact_f32xy", 10)}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["queen_40_32_24", "empty_rows", "no_entries"])
def test_run_scaled_is_level_2_bit_for_bit(name, kind):
    h = host(name)
    upload, fmt = UPLOADS[kind]
    f32xy = kind == "c16_f32xy"
    for flags in (0, capi.FLAG_EXACT_ORDER):
        dev = Dev(h, kind, flags)
        with capi.Context(0, flags) as ctx:
            getattr(ctx, upload)(h.rows, h.cols, h.p, h.c, h.v)
            assert ctx.info()["format"] == fmt
            if h.cols:
                (ctx.set_x_f32 if f32xy else ctx.set_x)(dev.xh)
            for alpha, beta in PAIRS:
                (ctx.set_y_f32 if f32xy else ctx.set_y)(dev.y0)
                ctx.run_scaled(alpha, beta, runs=CALLS)
                got = (ctx.get_y_f32 if f32xy else ctx.get_y)()[:h.rows]
                y = dev.vec(dev.y0, SENTINEL)
                for _ in range(CALLS):
                    dev.call(alpha, beta, y, y)
                _bits(got, y.body(), "%s, %s, flags %d, alpha %g, beta %g: level 1 against level 2" % (name, kind, flags, alpha, beta))
                if h.rows and len(h.c):
                    assert ctx.last_run_ns() > 0
        dev.close()


def test_run_scaled_refuses_other_contexts_and_leaves_y_untouched():
    import torch
    h = host("queen_40_32_24")
    with capi.Context(0) as ctx:
        with pytest.raises(capi.SpmvHipError) as e:
            ctx.run_scaled(1.0, 0.0)
        assert e.value.code == capi.ERR_STATE and "format 0" in str(e.value)
        ctx.upload_csr(h.rows, h.cols, h.p, h.c, h.v)
        ctx.set_x(h.x)
        ctx.set_y(h.y0)
        with pytest.raises(capi.SpmvHipError) as e:
            ctx.run_scaled(2.0, 0.0)
        assert e.value.code == capi.ERR_STATE and "format 1" in str(e.value)
        helpers.assert_bitexact(ctx.get_y(), h.y0, "a refused run_scaled changed y")
        # set_stream, sync and last_run_ns as after spmv_hip_run
        ctx.upload_csr_compact_f64(h.rows, h.cols, h.p, h.c, h.v)
        ctx.set_x(h.x)
        ctx.set_y(h.y0)
        side = torch.cuda.Stream()
        assert ctx.lib.spmv_hip_set_stream(ctx.h, side.cuda_stream, 0) == 0
        ctx.run_scaled(-1.0, 1.0, sync=False)
        side.synchronize()
        assert ctx.last_run_ns() > 0
        assert ctx.lib.spmv_hip_set_stream(ctx.h, None, 1) == 0
        got = ctx.get_y()
        dev = Dev(h, "c16_f64")
        y = dev.vec(h.y0, SENTINEL)
        dev.call(-1.0, 1.0, y, y)
        helpers.assert_bitexact(got, y.body(), "run_scaled on a caller's stream")
        dev.close()
    with capi.Context(num_gpus=1) as m:
        m.upload_csr(h.rows, h.cols, h.p, h.c, h.v)
        m.set_y(h.y0)
        with pytest.raises(capi.SpmvHipError) as e:
            m.run_scaled(1.0, 1.0)
        assert e.value.code == capi.ERR_STATE
        helpers.assert_bitexact(m.get_y(), h.y0, "a refused run_scaled changed y of the multi-device context")


# ---- graph capture -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_overwrite_and_alpha_0_calls_captured_and_replayed(kind):
    """One overwrite call (beta == 0, y_in null) and one alpha == 0 call behind it, captured on one stream -- a linear graph, no
    parallel branches -- and replayed twice: the bits of eager execution.  A call that synchronised or allocated would invalidate
    the capture."""
    import torch
    h = host("queen_40_32_24")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        dev = Dev(h, kind)
        q, r = dev.out(), dev.out()

        def calls(stream):
            dev.call(0.375, 0.0, None, q, stream=stream)  # q = 0.375 A x
            dev.call(0.0, -2.5, q, r, matrix=False, x=False, stream=stream)  # r = -2.5 q

        calls(side.cuda_stream)
        side.synchronize()
        eager_q, eager_r = q.body("eager"), r.body("eager")
        assert np.all(np.isfinite(eager_q)) and np.any(eager_q != 0)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            calls(side.cuda_stream)
        for replay in range(2):
            q.t[GUARD:GUARD + q.n] = float("nan")
            r.t[GUARD:GUARD + r.n] = float("nan")
            g.replay()
            side.synchronize()
            _bits(q.body("replay"), eager_q, "%s: replay %d of the captured overwrite call" % (kind, replay))
            _bits(r.body("replay"), eager_r, "%s: replay %d of the captured alpha == 0 call" % (kind, replay))
        del g
        dev.inputs_unchanged()
        dev.close()


# ---- scale factors that are themselves special, on clean operands ------------------------------------------------------------------

NAN, INF, TINY = float("nan"), float("inf"), 2.0 ** -1074  # (the smallest fp64 denormal)
SPECIAL_PAIRS = ([(a, b) for a in (NAN, INF, -INF, -0.0, -1.0, TINY, 1e308) for b in (0.0, 1.0)] +
                 [(a, b) for b in (NAN, INF, -0.0, TINY) for a in (0.0, 1.0)])


def _restate_quietly(alpha, beta, z, y_in, dtype):
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return restate(alpha, beta, z, y_in, dtype)


def judged_rows(h, kind):
    """The rows whose class the restatement fixes in default order as well: rows without entries (z_i is +0.0 in any order), and
    rows whose |z_i| exceeds helpers.assert_close's bound on two summation orders, 2 nterms 2^-53 (|A||x|)_i, so that the sign of
    z_i -- which decides between +Inf, -Inf and NaN under an infinite alpha -- is that of any order.  At most 1 % are left out."""
    z, absz = h.z(kind)
    lens = np.diff(h.p.astype(np.int64))
    nterms = max(4096, int(lens.max()) if h.rows else 0)
    keep = (lens == 0) | (np.abs(z) > 2.0 * nterms * 2.0 ** -53 * absz)
    assert h.rows == 0 or np.mean(~keep) <= 0.01, "%s, %s: %.2f %% of the rows have a sum within the summation bound of zero" % (
        h.name, kind, 100 * np.mean(~keep))
    return keep, lens == 0


def _same_but_nan_payloads(got, want, what):
    """Classes exactly, and every row that is not NaN bit for bit (an infinity's sign is its class)."""
    poison.assert_classes(got, want, what)
    poison.assert_finite_rows_bitwise(got, want, want, what)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("flags", [0, capi.FLAG_EXACT_ORDER])
@pytest.mark.parametrize("name", ["empty_rows", "rows_0_to_7_ragged_end", "dense_row_9000_wide", "no_entries"])
def test_special_scale_factors_follow_the_restatement(name, flags, kind):
    """alpha in NaN, +-Inf, -0.0, -1, 2^-1074, 1e308 with beta in 0, 1; beta in NaN, +Inf, -0.0, 2^-1074 with alpha in 0, 1.
    -0.0 counts as zero for both factors: y_in is not read and may be null under beta = -0.0; no tile runs and the matrix and x
    may be null under alpha = -0.0.  Exact order: classes exactly and every finite row bit for bit the restatement (NaN payloads are
    not compared).  Default order: classes on judged_rows, bits on the rows without entries, helpers.assert_close where both
    factors are finite and at most 1 in magnitude, and two identical calls the same bits.  The float pair in default order is the
    bits of spmv_hip_csr_spmv_c16_scaled through the same plan on the widened operands, rounded once; that fp64 result is judged."""
    h = host(name)
    z, absz = h.z(kind)
    keep, empty = judged_rows(h, kind)
    exact = bool(flags & capi.FLAG_EXACT_ORDER)
    # pinned by the restatement before the GPU is looked at: what a row without entries gives
    if empty.any():
        y0 = h.vectors(kind)[1]
        r = _restate_quietly(-1.0, 0.0, z, y0, np.float64)[empty]
        assert np.all(r == 0) and np.all(np.signbit(r)), "alpha < 0, beta = 0: -0.0 in rows without entries"
        for a in (INF, -INF):
            assert np.all(np.isnan(_restate_quietly(a, 0.0, z, y0, np.float64)[empty])), "alpha = +-Inf: fl(alpha * +0.0) is NaN"
            assert np.all(np.isnan(_restate_quietly(a, 1.0, z, y0, np.float64)[empty]))
    dev = Dev(h, kind, flags)
    wide = Dev(h, "c16", flags) if kind == "c16_f32xy" and not exact else None
    if wide:
        wide.xh, wide.y0 = dev.xh.astype(np.float64), dev.y0.astype(np.float64)
        wide.x = Vec(wide.xh, np.float64)
    longest = int(np.max(np.diff(h.p))) if h.rows else 0
    for alpha, beta in SPECIAL_PAIRS:
        tag = "%s, %s, flags %d, alpha %r, beta %r" % (name, kind, flags, alpha, beta)
        want = _restate_quietly(alpha, beta, z, dev.y0, dev.dtype)
        y_in, out = dev.vec(dev.y0), dev.out()
        dev.call(alpha, beta, y_in, out, matrix=alpha != 0.0, x=alpha != 0.0)  # (alpha = -0.0: null matrix and x)
        got = out.body(tag)
        _bits(y_in.body(tag), dev.y0, tag + ": y_in changed")
        if exact:
            _same_but_nan_payloads(got, want, tag + ": against the restatement")
        else:
            y64, want64 = got, want
            if wide:
                w_out = wide.out()
                wide.call(alpha, beta, wide.vec(wide.y0), w_out, matrix=alpha != 0.0, x=alpha != 0.0)
                y64, want64 = w_out.body(tag), _restate_quietly(alpha, beta, z, dev.y0, np.float64)
                with np.errstate(over="ignore", under="ignore"):
                    _same_but_nan_payloads(got, y64.astype(np.float32), tag + ": against spmv_hip_csr_spmv_c16_scaled through the same plan, rounded once")
            poison.assert_classes(y64[keep], want64[keep], tag + ": rows without entries and rows whose sum is clear of zero")
            _same_but_nan_payloads(got[empty], want[empty], tag + ": rows without entries against the restatement")
            if abs(alpha) <= 1.0 and abs(beta) <= 1.0:
                scale = abs(alpha) * absz + abs(beta) * np.abs(dev.y0.astype(np.float64))
                helpers.assert_close(y64, want64, scale, what=tag, nterms=max(4096, longest))
            again = dev.out()
            dev.call(alpha, beta, y_in, again, matrix=alpha != 0.0, x=alpha != 0.0)
            assert np.array_equal(again.body(tag).view(np.uint8), got.view(np.uint8)), tag + ": two identical calls"
        if beta == 0.0:  # -0.0 included: y_in is not read -- it may be null, and full of NaN it leaves no NaN behind
            for other in (None, dev.vec(np.full(h.rows, np.nan))):
                o = dev.out()
                dev.call(alpha, beta, other, o, matrix=alpha != 0.0, x=alpha != 0.0)
                b = o.body(tag)
                assert np.array_equal(b.view(np.uint8), got.view(np.uint8)), "%s: y_in %s" % (tag, "null" if other is None else "full of NaN")
                if alpha == 0.0:
                    assert not np.any(np.isnan(b)), tag + ": y_in was read"
    dev.inputs_unchanged()
    if name == "dense_row_9000_wide" and kind != "f32":
        assert dev.plan.info()["long_row_tiles"] == 1
    dev.close()
    if wide:
        wide.close()


# ---- float vectors at the edges of the float format ----------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", [0, capi.FLAG_EXACT_ORDER])
def test_float_vectors_at_ties_at_flt_max_and_in_the_denormals(flags):
    """spmv_hip_csr_spmv_c16_f32xy_scaled on float_edges.py's matrix: values and x non-zero small integers, so every row sum is
    one exact integer n_i in any order and BOTH orders must give t.astype(float32) bit for bit, t = alpha n + beta y_in exact in
    fp64.  ties: alpha 2^-24 on y_in cycling through 1.0, 1 + 2^-23, 3.0, -1.0 (a product or a store in float would lose the
    2^-24).  overflow: alpha 2^102 on +-FLT_MAX (n = 1 stays FLT_MAX, n = 2 is the tie and gives Inf).  denormal results: alpha
    2^-150 on y_in = k 2^-149 (the store's conversion must not flush, -0.0 keeps its sign).  denormal x: x = integers 2^-149,
    alpha 2^149, beta 0 gives n_i again (a flushed load gives 0).  The census of row kinds is asserted from numpy alone first."""
    e = float_edges.edges()
    count = e.census()
    print("float_edges: %s" % count)
    calls = e.calls()
    dev = Dev(e, "c16_f32xy", flags)
    info = dev.plan.info()
    assert info["long_row_tiles"] == 1 and info["stored_entries"] % 4 != 0 and info["tiles"] > 1
    x_int = dev.x
    for what, (alpha, beta, x, y_in, t) in calls.items():
        tag = "float_edges, flags %d, %s (alpha %r, beta %r)" % (flags, what, alpha, beta)
        dev.x, dev.xh = (x_int, e.x32) if x is e.x32 else (dev.vec(x), x)
        src = None if y_in is None else dev.vec(y_in)
        want = float_edges.f32(t)
        out = dev.out()
        dev.call(alpha, beta, src, out)
        _bits(out.body(tag), want, tag + ": out of place")
        if src is not None:
            _bits(src.body(tag), y_in, tag + ": y_in changed")
            y = dev.vec(y_in, SENTINEL)
            dev.call(alpha, beta, y, y)
            _bits(y.body(tag), want, tag + ": in place")
        dev.inputs_unchanged()
    dev.close()


# ---- the host program ------------------------------------------------------------------------------------------------------------

def test_cli_compact_f64_residual_steps_check():
    r = subprocess.run([CLI, "--csr", BUS, "--device", "hip", "--compact=f64", "--alpha", "-1", "--beta", "1", "--threads", "1", "--profile", "4",
                        "--check"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    doc = json.loads(r.stdout)  # one JSON document
    assert doc
    text = r.stdout
    assert '"hip-csr-spmv-compact-f64"' in text and '"alpha": -1' in text and '"beta": 1' in text
    assert "scaled runs" in text and '"pass": true' in text, text[-800:]


# ---- the two gates ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def _gate():
    """Poisson 4096^2 through one C16Plan (the matrix of test_gpu_compact32.py's gate): every entry in compact tiles, so the
    32-bit columns are not on the device at all."""
    import torch
    rows, cols, p, c, v = cc._csr(*synth.poisson2d(4096)[:5])
    assert len(c) == 83_869_696
    plan = capi.C16Plan(rows, cols, p, c, 0, torch.cuda.current_stream().cuda_stream)
    info = plan.info()
    assert info["compact_entries"] == info["stored_entries"] == len(c) and info["wide_tiles"] == 0
    dev = {"rows": rows, "cols": cols, "plan": plan, "info": info,
           "p": torch.from_numpy(p).to("cuda:0"),
           "a32": torch.from_numpy(_f32(v)).to("cuda:0"),
           "a64": torch.from_numpy(v).to("cuda:0"),
           "x": torch.from_numpy(synth.x_vector(cols)).to("cuda:0"),
           "b": torch.from_numpy(np.random.default_rng(4).uniform(-1.0, 1.0, size=rows)).to("cuda:0"),
           "y": torch.zeros(rows, dtype=torch.float64, device="cuda:0"),
           "r": torch.zeros(rows, dtype=torch.float64, device="cuda:0")}
    return dev


def _alternate(ways, warm=3, rounds=25):
    """Three warm-up rounds, then 25 rounds alternating the ways; every way between two events on the current stream."""
    import torch
    times = {k: [] for k in ways}
    for rnd in range(warm + rounds):
        for k, run in ways.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            e1.synchronize()
            if rnd >= warm:
                times[k].append(e0.elapsed_time(e1) * 1e3)
    assert all(len(t) == rounds for t in times.values())
    return {k: float(np.median(t)) for k, t in times.items()}


def test_gate_overwrite_is_not_slower_than_memset_and_multiply():
    """Gate (a): q = A p on Poisson 4096^2 through a C16Plan, Level 2, one process, torch events on one stream.  Asserted:
    median(spmv_hip_csr_spmv_c16_scaled, alpha 1, beta 0, y_in null) <= 1.00 x median(memset of y + spmv_hip_csr_spmv_c16): it
    moves strictly fewer bytes in one launch fewer, on the same arrays.  The premise that the streams exceed the 256 MiB Infinity
    Cache is asserted; the ratio the plan's byte counts promise is printed, not asserted.
    Measured: memset + c16 229.0 us, overwrite form 187.3 us, ratio 0.818 against 0.746 by bytes (786.4 MB in one launch against
    920.6 + 134.2 MB in two): faster, by somewhat less than the bytes promise -- Poisson's tiles follow their gathers as much as
    their streams (tools/scaled_ab.py in another process: 225.0 against 184.1 us, 0.818)."""
    import torch
    d = _gate()
    plan, rows, s = d["plan"], d["rows"], torch.cuda.current_stream().cuda_stream
    streamed = d["info"]["streamed_bytes"]
    assert streamed > 256 * 2 ** 20 and streamed - 16 * rows > 256 * 2 ** 20
    P, A, X, Y = d["p"].data_ptr(), d["a32"].data_ptr(), d["x"].data_ptr(), d["y"].data_ptr()
    print("streamed bytes: existing multiply %d + memset %d, overwrite form %d: expected ratio %.3f" % (
        streamed, 8 * rows, streamed - 8 * rows, (streamed - 8 * rows) / (streamed + 8 * rows)))

    def old():
        d["y"].zero_()
        plan.spmv(P, 0, A, X, Y, s)

    old()
    want = d["y"].clone()
    plan.spmv_scaled(P, 0, A, X, 1.0, 0.0, None, Y, s)
    assert torch.equal(d["y"], want)  # the same bits
    med = _alternate({"memset + c16": old, "overwrite": lambda: plan.spmv_scaled(P, 0, A, X, 1.0, 0.0, None, Y, s)})
    print("memset + spmv_hip_csr_spmv_c16 median %.1f us, overwrite form median %.1f us, ratio %.3f" % (
        med["memset + c16"], med["overwrite"], med["overwrite"] / med["memset + c16"]))
    assert med["overwrite"] <= 1.00 * med["memset + c16"], med


def test_gate_residual_out_of_place_is_not_slower_than_the_multiply():
    """Gate (b): r = b - A x (alpha -1, beta 1, y_in = b, y_out = r) through spmv_hip_csr_spmv_c16_f64_scaled against
    spmv_hip_csr_spmv_c16_f64 (y += A x) on the same matrix.  The bytes are the same; y_out is another array, so the bound is the
    project's measured in-process placement spread: median(residual) <= 1.06 x median(existing).
    Measured: c16_f64 242.4 us, residual form 243.5 us, ratio 1.004 (tools/scaled_ab.py in another process: 237.8
    against 241.8 us, 1.017)."""
    import torch
    d = _gate()
    plan, rows, s = d["plan"], d["rows"], torch.cuda.current_stream().cuda_stream
    streamed = d["info"]["streamed_bytes"] + 4 * d["info"]["stored_entries"]
    assert streamed > 256 * 2 ** 20
    P, A, X, Y, B, R = (d[k].data_ptr() for k in ("p", "a64", "x", "y", "b", "r"))
    print("streamed bytes of either way: %d" % streamed)
    med = _alternate({"c16_f64": lambda: plan.spmv_f64(P, 0, A, X, Y, s),
                      "residual": lambda: plan.spmv_f64_scaled(P, 0, A, X, -1.0, 1.0, B, R, s)})
    print("spmv_hip_csr_spmv_c16_f64 median %.1f us, residual form median %.1f us, ratio %.3f" % (
        med["c16_f64"], med["residual"], med["residual"] / med["c16_f64"]))
    assert med["residual"] <= 1.06 * med["c16_f64"], med
