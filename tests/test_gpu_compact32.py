"""The compact multiply over FLOAT x and y, y <- fl32(y + fl32(A) x) with float values and 16-bit column codes
(include/spmv_hip_compact_f32xy.h), on the MI355X.  It is the tile of spmv_hip_csr_spmv_c16 with another vector element type,
through the same plan object: every product and sum in fp64, one rounding to float per row and call.  So under
SPMV_HIP_FLAG_EXACT_ORDER it is compared BIT FOR BIT with a numpy restatement over three accumulating runs, in default order
with a bound derived from the formats, and on small integers -- where every sum is exact in either type -- bit for bit with
spmv_hip_csr_spmv_c16 itself, the two multiplies in turn through one plan.  Level 2 runs with an odd number of float NaN guards
around x and y (both are then 4- but not 8-byte aligned: a paired load or store would be caught), and with the caller's column
and float arrays as views into larger device buffers whose 8 neighbouring entries on each side hold column 0 and value NaN."""
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
from spmv_amd import capi, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "spmv-cache-trace_amd", "spmv-cache-trace-hip")
BUS = os.path.join(ROOT, "tests", "golden", "bus1138_like.mtx")
POISSON_FILE = os.path.join(ROOT, "tests", "golden", "poisson2D.mtx")
RUNS = 3
GUARD = 5   # floats (or doubles) in front of and behind x and y on the device: x and y start at 20 modulo 256 bytes
PAD = 8     # entries in front of and behind the column and value arrays: 32 bytes of columns and of floats
SENTINEL = -7.25


def _f32(a):
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(np.asarray(a, dtype=np.float64).astype(np.float32))


def assert_bits32(got, want, what):
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, what
    same = got.view(np.uint32) == want.view(np.uint32)
    if not same.all():
        k = int(np.nonzero(~same)[0][0])
        raise AssertionError("%s: %d of %d floats differ bitwise, first at %d: %r vs %r" % (
            what, int((~same).sum()), same.size, k, float(got[k]).hex(), float(want[k]).hex()))


def _guarded(a, dtype):
    import torch
    whole = torch.full((len(a) + 2 * GUARD,), float("nan"), dtype=dtype, device="cuda:0")
    if len(a):
        whole[GUARD:GUARD + len(a)] = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0").to(dtype)
    return whole


def _padded(a, dtype, fill):
    """(buffer, address of the view): a behind PAD entries of `fill`, and PAD entries of it behind a."""
    import torch
    buf = torch.full((len(a) + 2 * PAD,), fill, dtype=dtype, device="cuda:0")
    if len(a):
        buf[PAD:PAD + len(a)] = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0").to(dtype)
    return buf, buf.data_ptr() + buf.element_size() * PAD


class Device:
    """The caller's arrays of one matrix on the device -- the float values a32, float x32, and x32 widened for the comparator --
    and multiplies over them through a C16Plan: run(plan) is spmv_hip_csr_spmv_c16_f32xy from the float y0, run64(plan)
    spmv_hip_csr_spmv_c16 from the same y0 widened."""

    def __init__(self, rows, cols, p, c, a32, x32, y0):
        import torch
        self.torch = torch
        self.stream = torch.cuda.current_stream().cuda_stream
        self.rows, self.cols, self.c, self.x32, self.y0 = rows, cols, c, x32, y0
        self.tp = torch.from_numpy(np.ascontiguousarray(p, dtype=np.int32)).to("cuda:0")
        self.bc, self.ac = _padded(c, torch.int32, 0)
        self.bf, self.af = _padded(a32, torch.float32, float("nan"))
        self.xw = _guarded(x32, torch.float32)
        self.xw64 = None
        assert (self.xw.data_ptr() + 4 * GUARD) % 8 == 4  # 4- but not 8-byte aligned

    def _checked(self, yw, xw):
        self.torch.cuda.synchronize()
        yh, xh = yw.cpu().numpy(), xw.cpu().numpy()
        assert np.all(yh[:GUARD] == SENTINEL) and np.all(yh[GUARD + self.rows:] == SENTINEL), "y written outside its rows entries"
        assert np.all(np.isnan(xh[:GUARD])) and np.all(np.isnan(xh[GUARD + self.cols:])) and np.array_equal(xh[GUARD:GUARD + self.cols], self.x32), "x changed"
        assert np.array_equal(self.bc.cpu().numpy()[PAD:PAD + len(self.c)], self.c), "columns changed"
        return yh[GUARD:GUARD + self.rows].copy()

    def run(self, plan, runs=RUNS, columns=True):
        yw = _guarded(self.y0, self.torch.float32)
        yw[:GUARD] = SENTINEL
        yw[GUARD + self.rows:] = SENTINEL
        assert (yw.data_ptr() + 4 * GUARD) % 8 == 4
        for _ in range(runs):
            plan.spmv_f32xy(self.tp.data_ptr(), self.ac if columns else 0, self.af, self.xw.data_ptr() + 4 * GUARD, yw.data_ptr() + 4 * GUARD, self.stream)
        return self._checked(yw, self.xw)

    def run64(self, plan, runs=RUNS):
        if self.xw64 is None:
            self.xw64 = _guarded(self.x32, self.torch.float64)
        yw = _guarded(self.y0, self.torch.float64)
        yw[:GUARD] = SENTINEL
        yw[GUARD + self.rows:] = SENTINEL
        for _ in range(runs):
            plan.spmv(self.tp.data_ptr(), self.ac, self.af, self.xw64.data_ptr() + 8 * GUARD, yw.data_ptr() + 8 * GUARD, self.stream)
        return self._checked(yw, self.xw64)


def _level1(rows, cols, p, c, v, x32, y0, flags=0, runs=RUNS):
    with capi.Context(0, flags) as ctx:
        ctx.upload_csr_compact_f32xy(rows, cols, p, c, v)
        if cols:
            ctx.set_x_f32(x32)
        if rows:
            ctx.set_y_f32(y0)
        ctx.run(runs)
        return ctx.get_y_f32()[:rows], ctx.info(), ctx.last_run_ns()


def _streamed(pinfo):
    return pinfo["streamed_bytes"] - 8 * pinfo["rows"] - 4 * pinfo["cols"] if pinfo["streamed_bytes"] else 0


def _uniform_inputs(name, rows, cols, v):
    """Values (the case's own) and x (uniform doubles) narrowed to float, and a float y0."""
    rng = np.random.default_rng(len(name) + 17)
    return _f32(v), _f32(rng.uniform(-1.0, 1.0, size=cols)), _f32(rng.uniform(-1.0, 1.0, size=rows))


def _row_sums(rows, p, c, a32, x32):
    """s = the oracle's CSR kernel on double(a32), double(x32) from y = 0, one thread: every row left to right from +0.0."""
    if rows == 0:
        return np.zeros(0)
    if len(c) == 0:
        return np.zeros(rows)
    return oracle_py.Oracle().csr_spmv(rows, p, c, a32.astype(np.float64), x32.astype(np.float64), num_threads=1, runs=1)


def restate(y, s):
    """The restatement of one run: y <- float32(float64(y) + s)."""
    return (y.astype(np.float64) + s).astype(np.float32)


def one_run_bound(rows, p, c, a32, x32, y0, s):
    """(t, bound) of the default order, one run: t = double(y0) + s before rounding; the sum of a row in another order is off by
    at most delta_i (helpers.assert_close's a-priori bound on two summation orders), the rounding to float adds 2^-24 of what is
    rounded, which is at most |t| + delta_i, and 2^-149 covers a result in the denormals."""
    t = y0.astype(np.float64) + s
    longest = int(np.max(np.diff(p))) if rows else 0
    nterms = max(4096, longest)
    scale = (helpers.abs_products(rows, p, c, a32.astype(np.float64), x32.astype(np.float64)) if rows and len(c) else np.zeros(rows)) + np.abs(y0.astype(np.float64))
    delta = 2.0 * nterms * 2.0 ** -53 * scale
    return t, 2.0 ** -24 * np.abs(t) + delta * (1.0 + 2.0 ** -24) + 2.0 ** -149


def _check(name):
    rows, cols, p, c, v = cc.matrix(name)
    a32, x32, y0 = _uniform_inputs(name, rows, cols, v)
    s = _row_sums(rows, p, c, a32, x32)
    # the restatement: y <- float32(float64(y) + s), once per run
    want = y0.copy()
    for _ in range(RUNS):
        want = restate(want, s)
    t, bound = one_run_bound(rows, p, c, a32, x32, y0, s)
    dev = Device(rows, cols, p, c, a32, x32, y0)
    info = None
    for flags, order in ((0, "default order"), (capi.FLAG_EXACT_ORDER, "exact order")):
        tag = "%s (%s)" % (name, order)
        with capi.C16Plan(rows, cols, p, c, flags, dev.stream) as plan:
            pinfo = plan.info()
            if flags:
                y = dev.run(plan)
                assert np.all(np.isfinite(y)), tag + ": a neighbouring NaN was summed"
                assert_bits32(y, want, tag + ": against the numpy restatement, %d accumulating runs" % RUNS)
            else:
                y1 = dev.run(plan, runs=1)
                assert np.all(np.isfinite(y1)), tag + ": a neighbouring NaN was summed"
                err = np.abs(y1.astype(np.float64) - t)
                worst = float(np.max(err / bound)) if rows else 0.0
                print("%s: largest |y - t| / bound = %.3f" % (tag, worst))
                assert np.all(err <= bound), "%s: %d rows outside the bound, worst ratio %.3f" % (tag, int((err > bound).sum()), worst)
                y = dev.run(plan)
                assert np.all(np.isfinite(y)), tag
            assert_bits32(dev.run(plan), y, tag + ": a second run from the same y0")
            # the 32-bit columns are read by wide tiles only
            if pinfo["tiles"] and pinfo["wide_tiles"] == 0:
                assert_bits32(dev.run(plan, columns=False), y, tag + ": without the 32-bit columns")
            elif pinfo["tiles"]:
                with pytest.raises(capi.SpmvHipError) as e:
                    dev.run(plan, runs=1, columns=False)
                assert e.value.code == capi.ERR_INVALID and "wide tiles" in str(e.value)
        y1, info1, ns = _level1(rows, cols, p, c, a32.astype(np.float64), x32, y0, flags)
        assert_bits32(y1, y, tag + ": level 1 against level 2")
        assert info1["format"] == 10 and info1["rows"] == rows and info1["cols"] == cols and info1["stored"] == len(c)
        assert info1["streamed_bytes"] == _streamed(pinfo) and info1["workgroups"] == pinfo["workgroups"]
        if rows and cols and len(c):
            assert ns > 0
        info = info or pinfo
    return info


@pytest.mark.parametrize("name", cc.NAMES)
def test_exact_order_bit_for_bit_and_default_order_within_the_derived_bound(name):
    info = _check(name)
    if name == "mixed_mesh_and_graph":
        assert info["compact_tiles"] > 100 and info["wide_tiles"] > 100  # both branches in one launch
    if name == "dense_row_9000_compact":
        assert info["long_row_tiles"] == 1 and info["wide_tiles"] == 0
    if name == "rows_0_to_7_ragged_end":
        assert info["stored_entries"] % 4 != 0


@pytest.mark.parametrize("name", cc.NAMES)
def test_small_integers_give_the_bits_of_the_double_vector_multiply(name):
    """Values integers in [-4, 4], x in [-8, 8], y0 in [-100, 100]: every product, partial sum and y is an integer below 2^24
    in magnitude (longest row 9000: 9000 * 32 * 3 runs + 100 < 2^24), exact in float and in double in any order.  So y32 must
    equal spmv_hip_csr_spmv_c16's y64 through the same plan, converted to float, bit for bit, in both orders."""
    rows, cols, p, c, _ = cc.matrix(name)
    rng = np.random.default_rng(len(name) + 29)
    a32 = rng.integers(-4, 5, size=len(c)).astype(np.float32)
    x32 = rng.integers(-8, 9, size=cols).astype(np.float32)
    y0 = rng.integers(-100, 101, size=rows).astype(np.float32)
    assert (int(np.max(np.diff(p))) if rows else 0) * 32 * RUNS + 100 < 2 ** 24
    dev = Device(rows, cols, p, c, a32, x32, y0)
    for flags, order in ((0, "default order"), (capi.FLAG_EXACT_ORDER, "exact order")):
        tag = "%s, small integers (%s)" % (name, order)
        with capi.C16Plan(rows, cols, p, c, flags, dev.stream) as plan:
            y32 = dev.run(plan)
            y64 = dev.run64(plan)
            assert np.all(np.isfinite(y32)) and np.all(y64 == np.rint(y64)) and (rows == 0 or np.max(np.abs(y64)) < 2 ** 24)
            assert_bits32(y32, y64.astype(np.float32), tag + ": against spmv_hip_csr_spmv_c16 through the same plan")
            # in turn: the float multiply again after the double one, and the double one after that
            assert_bits32(dev.run(plan), y32, tag + ": the float-vector multiply again, after the double-vector one")
            helpers.assert_bitexact(dev.run64(plan), y64, tag + ": the double-vector multiply again, after the float-vector one")


@pytest.mark.parametrize("flags", [0, capi.FLAG_EXACT_ORDER])
def test_sums_are_accumulated_in_fp64_and_rounded_once_to_nearest_even(flags):
    import torch
    stream = torch.cuda.current_stream().cuda_stream

    def once(p, c, a, x, y0):
        rows, cols = len(p) - 1, len(x)
        dev = Device(rows, cols, np.array(p, dtype=np.int32), np.array(c, dtype=np.int32), np.array(a, dtype=np.float32),
                     np.array(x, dtype=np.float32), np.array(y0, dtype=np.float32))
        with capi.C16Plan(rows, cols, dev.tp.cpu().numpy(), np.array(c, dtype=np.int32), flags, stream) as plan:
            return dev.run(plan, runs=1)

    # 1 + 3 * 2^-25 in fp64 rounds to 1 + 2^-23; a float accumulator loses every 2^-25 and gives 1
    y = once([0, 4], [0, 1, 2, 3], [1, 1, 1, 1], [1.0, 2.0 ** -25, 2.0 ** -25, 2.0 ** -25], [0.0])
    assert_bits32(y, np.array([1.0 + 2.0 ** -23], dtype=np.float32), "fp64 accumulation")
    # ties go to even: 1 + 2^-24 -> 1 (even), 1 + 2^-23 + 2^-24 -> 1 + 2^-22 (even)
    y = once([0, 1], [0], [1.0], [2.0 ** -24], [1.0])
    assert_bits32(y, np.array([1.0], dtype=np.float32), "a tie above 1.0")
    y = once([0, 1], [0], [1.0], [2.0 ** -24], [1.0 + 2.0 ** -23])
    assert_bits32(y, np.array([1.0 + 2.0 ** -22], dtype=np.float32), "a tie above 1 + 2^-23")


@pytest.mark.parametrize("flags", [0, capi.FLAG_EXACT_ORDER])
def test_float_denormal_x_and_y_are_neither_flushed_on_the_loads_nor_on_the_store(flags):
    """float_edges.py's matrix (rows of 0 to 7 entries, one compact long row of 9000, nnz % 4 != 0; values and x non-zero small
    integers, so every row sum is one exact integer n_i in any order) with x = the integers times 2^-149 and y0 = k 2^-149, k in
    0 ... 3: y0 + n 2^-149 is a float denormal (or a zero), exact, so both orders give it bit for bit.  A load of x or y0 that
    flushes denormals gives zeros, a store that flushes gives zeros with the sum's sign."""
    e = float_edges.edges()
    e.census()
    t = e.k_den.astype(np.float64) + e.n * float_edges.DEN
    want = float_edges.f32(t)
    assert np.array_equal(want.astype(np.float64), t) and np.all(np.abs(t) < 2.0 ** -126) and np.mean(want != 0) > 0.8
    dev = Device(e.rows, e.cols, e.p, e.c, e.a32, e.x_den, e.k_den)
    with capi.C16Plan(e.rows, e.cols, e.p, e.c, flags, dev.stream) as plan:
        info = plan.info()
        assert info["long_row_tiles"] == 1 and info["stored_entries"] % 4 != 0 and info["wide_tiles"] == 0
        assert_bits32(dev.run(plan, runs=1), want, "float_edges, flags %d: denormal x and y0" % flags)
        # three accumulating runs: y0 + 3 n 2^-149, every intermediate a denormal
        assert_bits32(dev.run(plan), float_edges.f32(t + 2 * e.n * float_edges.DEN), "float_edges, flags %d: three accumulating runs" % flags)


def test_spmv_c16_f32xy_refuses_x_equal_y_and_misaligned_arrays():
    import torch
    rows, cols, p, c, v = cc.matrix("queen_40_32_24")
    a32, x32, y0 = _uniform_inputs("queen_40_32_24", rows, cols, v)
    dev = Device(rows, cols, p, c, a32, x32, y0)
    tp, ac, af = dev.tp.data_ptr(), dev.ac, dev.af
    tx = torch.ones(max(rows, cols) + 2, dtype=torch.float32, device="cuda:0")
    ty = torch.zeros(rows + 2, dtype=torch.float32, device="cuda:0")
    x, y = tx.data_ptr(), ty.data_ptr()
    with capi.C16Plan(rows, cols, p, c) as plan:
        for args, code in [((tp, ac, af, x, x), capi.ERR_INVALID),
                           ((tp, ac + 4, af, x, y), capi.ERR_ALIGN),
                           ((tp, ac, af + 4, x, y), capi.ERR_ALIGN),
                           ((tp, ac, af, x + 1, y), capi.ERR_ALIGN),   # x at an odd byte address
                           ((tp, ac, af, x, y + 1), capi.ERR_ALIGN),
                           ((tp, ac, af, x + 2, y), capi.ERR_ALIGN),
                           ((tp, ac, af, x, y + 2), capi.ERR_ALIGN),
                           ((tp, ac, 0, x, y), capi.ERR_INVALID),
                           ((tp, ac, af, 0, y), capi.ERR_INVALID),
                           ((tp, ac, af, x, 0), capi.ERR_INVALID),
                           ((0, ac, af, x, y), capi.ERR_INVALID)]:
            with pytest.raises(capi.SpmvHipError) as e:
                plan.spmv_f32xy(*args)
            assert e.value.code == code, args
        torch.cuda.synchronize()
        assert float(ty.abs().max()) == 0.0  # nothing was launched
        # 4-byte alignment is enough
        plan.spmv_f32xy(tp, ac, af, x + 4, y + 4)
        torch.cuda.synchronize()
        assert float(ty[1:1 + rows].abs().max()) > 0.0 and float(ty[0]) == 0.0 and float(ty[rows + 1]) == 0.0


def test_level1_refusals_and_state():
    rows, cols, p, c, v = cc.from_lengths(np.full(400, 5), 900, 31)
    a32, x32, y0 = _uniform_inputs("refusals", rows, cols, v)
    v32 = a32.astype(np.float64)
    s = _row_sums(rows, p, c, a32, x32)
    want = y0.copy()
    for _ in range(RUNS):
        want = (want.astype(np.float64) + s).astype(np.float32)
    with capi.Context(num_gpus=1) as m:
        with pytest.raises(capi.SpmvHipError) as e:
            m.upload_csr_compact_f32xy(rows, cols, p, c, v)
        assert e.value.code == capi.ERR_STATE
    with capi.Context(0, capi.FLAG_EXACT_ORDER) as ctx:
        # float setters on any other format are ERR_STATE
        ctx.upload_csr(rows, cols, p, c, v)
        assert ctx.info()["format"] == 1
        for call in (lambda: ctx.set_x_f32(x32), lambda: ctx.set_y_f32(y0), ctx.get_y_f32):
            with pytest.raises(capi.SpmvHipError) as e:
                call()
            assert e.value.code == capi.ERR_STATE
        ctx.upload_csr_compact_f32xy(rows, cols, p, c, v32)
        with pytest.raises(capi.SpmvHipError) as e:
            ctx.upload_csr_compact_f32xy(rows, cols - 500, p, c, v32)  # columns beyond the last one
        assert e.value.code == capi.ERR_INVALID
        bad = p.copy()
        bad[7] = bad[9] + 1  # decreasing
        with pytest.raises(capi.SpmvHipError) as e:
            ctx.upload_csr_compact_f32xy(rows, cols, bad, c, v32)
        assert e.value.code == capi.ERR_INVALID
        assert ctx.lib.spmv_hip_upload_csr_compact_f32xy(ctx.h, rows, cols, len(c) - 1, p.ctypes.data, c.ctypes.data, v32.ctypes.data, 1) == capi.ERR_INVALID
        assert b"row_ptr[rows] must equal nnz" in ctx.lib.spmv_hip_last_error()
        # format 8's narrowing: values that are not floats are refused where rounding is not allowed, a value beyond the floats always
        with pytest.raises(capi.SpmvHipError) as e:
            ctx.upload_csr_compact_f32xy(rows, cols, p, c, v, allow_rounding=False)
        assert e.value.code == capi.ERR_INVALID and "not floats" in str(e.value)
        big = v.copy()
        big[3] = 1e300
        with pytest.raises(capi.SpmvHipError) as e:
            ctx.upload_csr_compact_f32xy(rows, cols, p, c, big)
        assert e.value.code == capi.ERR_OVERFLOW
        # a refused upload leaves the matrix that was there, and the context is usable
        assert ctx.info()["format"] == 10
        # nothing is rounded silently: the double setters are ERR_STATE
        for call in (lambda: ctx.set_x(x32.astype(np.float64)), lambda: ctx.set_y(y0.astype(np.float64)), ctx.get_y):
            with pytest.raises(capi.SpmvHipError) as e:
                call()
            assert e.value.code == capi.ERR_STATE
        ctx.set_x_f32(x32)
        ctx.set_y_f32(y0)
        ctx.run(RUNS)
        # the context's exact order is kept
        assert_bits32(ctx.get_y_f32(), want, "level 1 with SPMV_HIP_FLAG_EXACT_ORDER, after refusals")
        assert ctx.last_run_ns() > 0
        ctx.flush_caches()
        # the columns may be gone: no block runs
        with pytest.raises(capi.SpmvHipError) as e:
            ctx.set_block_x(np.ones((cols, 2)))
        assert e.value.code == capi.ERR_STATE
        with pytest.raises(capi.SpmvHipError) as e:
            ctx.run_block()
        assert e.value.code == capi.ERR_STATE
        # a general upload afterwards is a general multiply with double vectors
        ctx.upload_csr(rows, cols, p, c, v)
        assert ctx.info()["format"] == 1
        ctx.set_x(x32.astype(np.float64))
        ctx.run()
        assert np.all(np.isfinite(ctx.get_y()))


def test_level1_keeps_floats_only_and_no_32bit_columns():
    rows, cols, p, c, v = cc._csr(*synth.poisson2d(1024)[:5])
    nnz = len(c)
    assert nnz > 5_000_000
    pre = capi.c16_plan_preview(rows, cols, p, c, table=False)[0]
    assert pre["wide_tiles"] == 0
    # what spmv_hip_ctx_info [9] counts: row_ptr, the float values, the float vectors (each padded by 64 bytes) and the plan,
    # which holds the codes -- no 4 nnz of columns, no doubles
    base = (4 * (rows + 1) + 64) + (4 * nnz + 64) + (4 * cols + 64) + (4 * rows + 64) + pre["device_bytes"]
    with capi.Context(0) as ctx:
        ctx.upload_csr_compact_f32xy(rows, cols, p, c, v)
        got = ctx.info()["device_bytes"]
    print("ctx_info[9] = %d, base = %d" % (got, base))
    assert base - 4 * 64 <= got <= base + 4 * 64
    assert got < base + 4 * cols + 4 * rows  # less than with double vectors


# ---- the host program ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("matrix", [POISSON_FILE, BUS, "synthetic:kkt:30"])
def test_cli_compact_f32_check(matrix):
    r = subprocess.run([CLI, "--csr", matrix, "--device", "hip", "--compact=f32", "--threads", "1", "--profile", "4", "--check", "--x", "uniform"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    doc = json.loads(r.stdout)  # one JSON document
    assert doc
    text = r.stdout
    assert '"hip-csr-spmv-compact-f32"' in text and '"value_bytes": 4' in text and '"vector_bytes": 4' in text
    for key in ('"values_inexact"', '"max_value_rounding"', '"compact_tiles"', '"wide_tiles"', '"streamed_bytes"', '"tolerance"'):
        assert key in text, key
    assert "values and x rounded to float" in text
    assert '"pass": true' in text, text[-800:]


# ---- the gate ----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def _gate_matrix():
    return cc._csr(*synth.poisson2d(4096)[:5])


def test_not_slower_than_the_compact_multiply_over_double_vectors():
    """Poisson 4096^2 (16.8 M rows, 83 869 696 entries: 503 MB of entries at 6 bytes, larger than the Infinity Cache).  Premises,
    asserted from the preview: compact tiles hold every entry, and this multiply streams <= 0.80 of what the compact multiply
    over double vectors streams (719 257 616 against 920 584 208 bytes, 0.781).  Then, in one process, a format-8 context (the
    parent commit's spmv_hip_csr_spmv_c16, the comparator) and a format-10 context on the same host arrays: three warm-up
    rounds, 25 rounds of one run of each with a sync behind every run, times from last_run_ns.  Asserted:
    median(f32xy) <= 1.06 x median(c16) -- the in-process placement spread the project gates with (the perf floor,
    3.13's gate).  The byte ratio is the expectation, not the condition.
    Measured: c16 206.1 us, f32xy 191.3 us, ratio 0.928 at a byte ratio of 0.781: faster, by about a third of what the bytes
    promise -- Poisson's tiles have two windows 4096 columns apart and the kernel follows its gathers as much as its streams
    (DESIGN 3.14)."""
    rows, cols, p, c, v = _gate_matrix()
    assert len(c) == 83_869_696
    pre = capi.c16_plan_preview(rows, cols, p, c, table=False)[0]
    assert pre["compact_entries"] == pre["stored_entries"] == len(c) and pre["wide_tiles"] == 0
    print("%d entries in %d compact tiles; streamed bytes: c16 %d, f32xy %d (ratio %.3f)" % (
        len(c), pre["compact_tiles"], pre["streamed_bytes"], _streamed(pre), _streamed(pre) / pre["streamed_bytes"]))
    assert _streamed(pre) <= 0.80 * pre["streamed_bytes"]
    x = synth.x_vector(cols)
    with capi.Context(0) as doubles, capi.Context(0) as floats:
        doubles.upload_csr_compact(rows, cols, p, c, v)
        floats.upload_csr_compact_f32xy(rows, cols, p, c, v)
        doubles.set_x(x)
        floats.set_x_f32(_f32(x))
        ways = {"c16": doubles, "f32xy": floats}
        assert doubles.info()["format"] == 8 and floats.info()["format"] == 10
        assert doubles.info()["streamed_bytes"] == pre["streamed_bytes"] and floats.info()["streamed_bytes"] == _streamed(pre)
        times = {k: [] for k in ways}
        for rnd in range(3 + 25):  # three warm-up rounds
            for k, ctx in ways.items():
                ctx.run()  # one run and a sync
                if rnd >= 3:
                    times[k].append(ctx.last_run_ns() / 1e3)
    med = {k: float(np.median(t)) for k, t in times.items()}
    print("%d runs each: c16 median %.1f us, f32xy median %.1f us, ratio %.3f" % (
        len(times["f32xy"]), med["c16"], med["f32xy"], med["f32xy"] / med["c16"]))
    assert len(times["c16"]) == 25 and len(times["f32xy"]) == 25
    assert med["f32xy"] <= 1.06 * med["c16"], med
