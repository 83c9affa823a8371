"""The compact multiply over fp64 values, y += A x with 16-bit column codes beside the caller's doubles
(include/spmv_hip_compact_f64.h), on the MI355X.  It is the tile of spmv_hip_csr_spmv_c16 with another value type, through the
same plan object, so on values that are floats its y is compared BIT FOR BIT with that multiply's; on values that are not it is
the exact operator: bit for bit the oracle's CSR kernel on the unrounded values under SPMV_HIP_FLAG_EXACT_ORDER, within the
project's tolerance in default order, and different from what the float path gives on the narrowed values.  Level 2 runs with
NaN guard elements around x and y, and with the caller's column, double and float arrays as views into larger device buffers
whose 8 neighbouring entries on each side hold column 0 and value NaN (the guard scheme of test_gpu_compact.py)."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import compact_cases as cc
import helpers
import oracle_py
from spmv_amd import capi, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "spmv-cache-trace_amd", "spmv-cache-trace-hip")
BUS = os.path.join(ROOT, "tests", "golden", "bus1138_like.mtx")
POISSON_FILE = os.path.join(ROOT, "tests", "golden", "poisson2D.mtx")
RUNS = 3
GUARD = 5   # doubles in front of and behind x and y on the device
PAD = 8     # entries in front of and behind the column and value arrays: 32 bytes of columns and floats, 64 bytes of doubles
SENTINEL = -7.25


def _narrow(v):
    with np.errstate(over="ignore"):
        f = np.asarray(v, dtype=np.float64).astype(np.float32)
    return f.astype(np.float64), f


def _not_floats(name, v):
    """The case's own values where some of them are not floats (the uniform doubles of compact_cases); a stencil's -1 and 4
    and the like are replaced by uniform doubles, so that every matrix with entries can tell a narrowed value from a whole one."""
    if len(v) == 0 or np.any(_narrow(v)[0] != v):
        return v
    return np.random.default_rng(len(name) + len(v)).uniform(-1.0, 1.0, size=len(v))


def _expected(rows, cols, p, c, v, x, y0):
    if rows == 0 or len(c) == 0:
        return y0.copy(), np.abs(y0), 4096
    want = oracle_py.Oracle().csr_spmv(rows, p, c, v, x, y=y0, num_threads=4, runs=RUNS)
    scale = RUNS * helpers.abs_products(rows, p, c, v, x) + np.abs(y0)
    return want, scale, max(4096, int(np.max(np.diff(p))))


def _guarded(a):
    import torch
    whole = torch.full((len(a) + 2 * GUARD,), float("nan"), dtype=torch.float64, device="cuda:0")
    if len(a):
        whole[GUARD:GUARD + len(a)] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:0")
    return whole


def _padded(a, dtype, fill, shift=0):
    """(buffer, address of the view): a behind PAD + shift entries of `fill`, and PAD entries of it behind a."""
    import torch
    buf = torch.full((len(a) + 2 * PAD + shift,), fill, dtype=dtype, device="cuda:0")
    if len(a):
        buf[PAD + shift:PAD + shift + len(a)] = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0").to(dtype)
    return buf, buf.data_ptr() + buf.element_size() * (PAD + shift)


class Device:
    """The caller's arrays of one matrix on the device -- the doubles `v` and, where given, floats `f` -- and multiplies over them
    through a C16Plan: run(plan) is spmv_hip_csr_spmv_c16_f64, run(plan, floats=True) spmv_hip_csr_spmv_c16."""

    def __init__(self, rows, cols, p, c, v, x, y0, f=None, value_shift=0):
        import torch
        self.torch = torch
        self.stream = torch.cuda.current_stream().cuda_stream
        self.rows, self.cols, self.c, self.v, self.x, self.y0 = rows, cols, c, v, x, y0
        self.tp = torch.from_numpy(np.ascontiguousarray(p, dtype=np.int32)).to("cuda:0")
        self.bc, self.ac = _padded(c, torch.int32, 0)
        self.bv, self.av = _padded(v, torch.float64, float("nan"), value_shift)
        self.bf, self.af = _padded(f, torch.float32, float("nan")) if f is not None else (None, 0)
        self.xw = _guarded(x)

    def run(self, plan, runs=RUNS, columns=True, floats=False):
        yw = _guarded(self.y0)
        yw[:GUARD] = SENTINEL
        yw[GUARD + self.rows:] = SENTINEL
        mul, values = (plan.spmv, self.af) if floats else (plan.spmv_f64, self.av)
        for _ in range(runs):
            mul(self.tp.data_ptr(), self.ac if columns else 0, values, self.xw.data_ptr() + 8 * GUARD, yw.data_ptr() + 8 * GUARD, self.stream)
        self.torch.cuda.synchronize()
        yh, xh = yw.cpu().numpy(), self.xw.cpu().numpy()
        assert np.all(yh[:GUARD] == SENTINEL) and np.all(yh[GUARD + self.rows:] == SENTINEL), "y written outside its rows entries"
        assert np.all(np.isnan(xh[:GUARD])) and np.all(np.isnan(xh[GUARD + self.cols:])) and np.array_equal(xh[GUARD:GUARD + self.cols], self.x), "x changed"
        assert np.array_equal(self.bc.cpu().numpy()[PAD:PAD + len(self.c)], self.c), "columns changed"
        return yh[GUARD:GUARD + self.rows].copy()


def _level1(rows, cols, p, c, v, x, y0, flags=0):
    with capi.Context(0, flags) as ctx:
        ctx.upload_csr_compact_f64(rows, cols, p, c, v)
        if cols:
            ctx.set_x(x)
        if rows:
            ctx.set_y(y0)
        ctx.run(RUNS)
        return ctx.get_y()[:rows], ctx.info(), ctx.last_run_ns()


def _inputs(rows, cols, seed=5):
    rng = np.random.default_rng(seed)
    return synth.x_vector(cols), rng.uniform(-1.0, 1.0, size=rows)


def _f64_streamed(pinfo):
    return pinfo["streamed_bytes"] + 4 * pinfo["stored_entries"] if pinfo["streamed_bytes"] else 0


def _check_floats(rows, cols, p, c, v, what):
    """Values that are floats: the float multiply and the double multiply through ONE plan, in turn, give the same bits."""
    vt, f = _narrow(v)
    x, y0 = _inputs(rows, cols)
    dev = Device(rows, cols, p, c, vt, x, y0, f=f)
    for flags, order in ((0, "default order"), (capi.FLAG_EXACT_ORDER, "exact order")):
        tag = "%s, values that are floats (%s)" % (what, order)
        with capi.C16Plan(rows, cols, p, c, flags, dev.stream) as plan:
            y = dev.run(plan)
            yf = dev.run(plan, floats=True)
            assert np.all(np.isfinite(y)), tag + ": a neighbouring NaN was summed"
            helpers.assert_bitexact(y, yf, tag + ": against spmv_hip_csr_spmv_c16 through the same plan")
            helpers.assert_bitexact(dev.run(plan, floats=True), yf, tag + ": the float multiply again, after the double one")
            helpers.assert_bitexact(dev.run(plan), y, tag + ": the double multiply again, after the float one")


def _check(rows, cols, p, c, v, what, level1=True):
    """Values that are not floats.  Returns the plan's info."""
    vt, f = _narrow(v)
    if len(c):
        assert np.any(vt != v), what + ": the values are floats"
    x, y0 = _inputs(rows, cols)
    want, scale, nterms = _expected(rows, cols, p, c, v, x, y0)
    dev = Device(rows, cols, p, c, v, x, y0, f=f)
    info = None
    for flags, order in ((0, "default order"), (capi.FLAG_EXACT_ORDER, "exact order")):
        tag = "%s (%s)" % (what, order)
        with capi.C16Plan(rows, cols, p, c, flags, dev.stream) as plan:
            y = dev.run(plan)
            assert np.all(np.isfinite(y)), tag + ": a neighbouring NaN was summed"
            if flags:
                helpers.assert_bitexact(y, want, tag + ": against the oracle on the unrounded values")
            else:
                helpers.assert_close(y, want, scale, what=tag + " (level 2)", nterms=nterms)
            if len(c):
                assert np.any(y != dev.run(plan, floats=True)), tag + ": y is the float path's on the narrowed values"
            helpers.assert_bitexact(dev.run(plan), y, tag + ": a second run from the same y0")
            pinfo = plan.info()
            # the 32-bit columns are read by wide tiles only
            if pinfo["tiles"] and pinfo["wide_tiles"] == 0:
                helpers.assert_bitexact(dev.run(plan, columns=False), y, tag + ": without the 32-bit columns")
            elif pinfo["tiles"]:
                with pytest.raises(capi.SpmvHipError) as e:
                    dev.run(plan, runs=1, columns=False)
                assert e.value.code == capi.ERR_INVALID and "wide tiles" in str(e.value)
        if level1:
            y1, info1, ns = _level1(rows, cols, p, c, v, x, y0, flags)
            helpers.assert_bitexact(y1, y, tag + ": level 1 against level 2")
            assert info1["format"] == 9 and info1["rows"] == rows and info1["cols"] == cols and info1["stored"] == len(c)
            assert info1["streamed_bytes"] == _f64_streamed(pinfo) and info1["workgroups"] == pinfo["workgroups"]
            if rows and cols and len(c):
                assert ns > 0
        info = info or pinfo
    return info


@pytest.mark.parametrize("name", cc.NAMES)
def test_values_that_are_floats_give_the_bits_of_the_float_multiply(name):
    rows, cols, p, c, v = cc.matrix(name)
    _check_floats(rows, cols, p, c, v, name)


@pytest.mark.parametrize("name", cc.NAMES)
def test_values_that_are_not_floats_against_the_oracle(name):
    rows, cols, p, c, v = cc.matrix(name)
    info = _check(rows, cols, p, c, _not_floats(name, v), name)
    if name == "mixed_mesh_and_graph":
        assert info["compact_tiles"] > 100 and info["wide_tiles"] > 100  # both branches in one launch
    if name == "dense_row_9000_compact":
        assert info["long_row_tiles"] == 1 and info["wide_tiles"] == 0
    if name == "rows_0_to_7_ragged_end":
        assert info["stored_entries"] % 4 != 0


@pytest.mark.parametrize("name", ["delaunay_60k_1dof_rcm", "rows_0_to_7_ragged_end", "dense_row_9000_wide"])
def test_a_value_array_that_is_16_but_not_32_byte_aligned(name):
    """A quad of four doubles is two 16-byte loads: the array may start at any multiple of 16 bytes."""
    rows, cols, p, c, v = cc.matrix(name)
    x, y0 = _inputs(rows, cols)
    even, odd = Device(rows, cols, p, c, v, x, y0), Device(rows, cols, p, c, v, x, y0, value_shift=2)
    assert even.av % 32 == 0 and odd.av % 32 == 16
    for flags in (0, capi.FLAG_EXACT_ORDER):
        with capi.C16Plan(rows, cols, p, c, flags, even.stream) as plan:
            y = odd.run(plan)
            assert np.all(np.isfinite(y))
            helpers.assert_bitexact(y, even.run(plan), "%s, flags %d: values at 16 modulo 32 bytes" % (name, flags))


def test_spmv_c16_f64_refuses_x_equal_y_and_misaligned_arrays():
    import torch
    rows, cols, p, c, v = cc.matrix("queen_40_32_24")
    dev = Device(rows, cols, p, c, v, *_inputs(rows, cols))
    tp, ac, av = dev.tp.data_ptr(), dev.ac, dev.av
    tx = torch.ones(max(rows, cols), dtype=torch.float64, device="cuda:0")
    ty = torch.zeros(rows, dtype=torch.float64, device="cuda:0")
    with capi.C16Plan(rows, cols, p, c) as plan:
        for args, code in [((tp, ac, av, tx.data_ptr(), tx.data_ptr()), capi.ERR_INVALID),
                           ((tp, ac + 4, av, tx.data_ptr(), ty.data_ptr()), capi.ERR_ALIGN),
                           ((tp, ac, av + 8, tx.data_ptr(), ty.data_ptr()), capi.ERR_ALIGN),
                           ((tp, ac, 0, tx.data_ptr(), ty.data_ptr()), capi.ERR_INVALID),
                           ((0, ac, av, tx.data_ptr(), ty.data_ptr()), capi.ERR_INVALID)]:
            with pytest.raises(capi.SpmvHipError) as e:
                plan.spmv_f64(*args)
            assert e.value.code == code
    torch.cuda.synchronize()
    assert float(ty.abs().max()) == 0.0  # nothing was launched


def test_level1_keeps_the_fp64_values_and_no_32bit_columns():
    rows, cols, p, c, v = cc._csr(*synth.poisson2d(1024)[:5])
    nnz = len(c)
    assert nnz > 5_000_000
    v = np.random.default_rng(71).uniform(-1.0, 1.0, size=nnz)
    pre = capi.c16_plan_preview(rows, cols, p, c, table=False)[0]
    assert pre["wide_tiles"] == 0
    # what spmv_hip_ctx_info [9] counts: row_ptr, the doubles, the vectors (each padded by 64 bytes) and the plan, which holds
    # the codes -- no 4 nnz of columns
    base = (4 * (rows + 1) + 64) + (8 * nnz + 64) + (8 * cols + 64) + (8 * rows + 64) + pre["device_bytes"]
    with capi.Context(0) as ctx:
        ctx.upload_csr_compact_f64(rows, cols, p, c, v)
        got = ctx.info()["device_bytes"]
    print("ctx_info[9] = %d, base = %d (%.3f bytes per stored entry beside row_ptr and the vectors)" % (
        got, base, (got - 4 * (rows + 1) - 8 * cols - 8 * rows) / nnz))
    assert base - 5 * 64 <= got <= base + 5 * 64
    assert got < 10.2 * nnz + 4 * (rows + 1) + 8 * cols + 8 * rows
    # with wide tiles the 32-bit columns stay
    rows, cols, p, c, v = cc.matrix("mixed_mesh_and_graph")
    pre = capi.c16_plan_preview(rows, cols, p, c, table=False)[0]
    with capi.Context(0) as ctx:
        ctx.upload_csr_compact_f64(rows, cols, p, c, v)
        got = ctx.info()["device_bytes"]
    base = (4 * (rows + 1) + 64) + (4 * len(c) + 64) + (8 * len(c) + 64) + (8 * cols + 64) + (8 * rows + 64) + pre["device_bytes"]
    assert base - 5 * 64 <= got <= base + 5 * 64


def test_refusals():
    rows, cols, p, c, v = cc.from_lengths(np.full(400, 5), 900, 31)
    x, y0 = _inputs(rows, cols)
    with capi.Context(num_gpus=1) as m:
        with pytest.raises(capi.SpmvHipError) as e:
            m.upload_csr_compact_f64(rows, cols, p, c, v)
        assert e.value.code == capi.ERR_STATE
    with capi.Context(0) as ctx:
        ctx.upload_csr_compact_f64(rows, cols, p, c, v)
        with pytest.raises(capi.SpmvHipError) as e:
            ctx.upload_csr_compact_f64(rows, cols - 500, p, c, v)  # columns beyond the last one
        assert e.value.code == capi.ERR_INVALID
        bad = p.copy()
        bad[7] = bad[9] + 1  # decreasing
        with pytest.raises(capi.SpmvHipError) as e:
            ctx.upload_csr_compact_f64(rows, cols, bad, c, v)
        assert e.value.code == capi.ERR_INVALID
        assert ctx.lib.spmv_hip_upload_csr_compact_f64(ctx.h, rows, cols, len(c) - 1, p.ctypes.data, c.ctypes.data, v.ctypes.data) == capi.ERR_INVALID
        assert b"row_ptr[rows] must equal nnz" in ctx.lib.spmv_hip_last_error()
        # values that no float holds are values like any other: nothing is rounded, nothing overflows
        big = v.copy()
        big[3] = 1e300
        # a refused upload leaves the matrix that was there, and the context is usable
        assert ctx.info()["format"] == 9
        ctx.set_x(x)
        ctx.set_y(y0)
        ctx.run(RUNS)
        want, scale, nterms = _expected(rows, cols, p, c, v, x, y0)
        helpers.assert_close(ctx.get_y(), want, scale, what="after refusals", nterms=nterms)
        assert ctx.last_run_ns() > 0
        ctx.flush_caches()
        # the columns may be gone: no block runs
        with pytest.raises(capi.SpmvHipError) as e:
            ctx.set_block_x(np.ones((cols, 2)))
        assert e.value.code == capi.ERR_STATE
        with pytest.raises(capi.SpmvHipError) as e:
            ctx.run_block()
        assert e.value.code == capi.ERR_STATE
        ctx.upload_csr_compact_f64(rows, cols, p, c, big)
        ctx.set_x(x)
        ctx.run()
        assert ctx.info()["format"] == 9 and np.all(np.isfinite(ctx.get_y())) and np.max(np.abs(ctx.get_y())) > 1e290
        # a general upload afterwards is a general multiply
        ctx.upload_csr(rows, cols, p, c, v)
        assert ctx.info()["format"] == 1
    # the context's exact order is kept
    with capi.Context(0, capi.FLAG_EXACT_ORDER) as ctx:
        ctx.upload_csr_compact_f64(rows, cols, p, c, v)
        ctx.set_x(x)
        ctx.set_y(y0)
        ctx.run(RUNS)
        helpers.assert_bitexact(ctx.get_y(), want, "level 1 with SPMV_HIP_FLAG_EXACT_ORDER")


# ---- the host program ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("matrix", [POISSON_FILE, BUS, "synthetic:kkt:30"])
def test_cli_compact_f64_check(matrix):
    """(synthetic:kkt:30 has values that are not floats: --compact=exact refuses it, --compact=f64 multiplies it as it is)"""
    r = subprocess.run([CLI, "--csr", matrix, "--device", "hip", "--compact=f64", "--threads", "1", "--profile", "4", "--check", "--x", "uniform"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    doc = json.loads(r.stdout)  # one JSON document
    assert doc
    text = r.stdout
    assert '"hip-csr-spmv-compact-f64"' in text and '"value_bytes": 8' in text
    for key in ('"compact_tiles"', '"wide_tiles"', '"streamed_bytes"'):
        assert key in text, key
    assert '"values_inexact"' not in text and '"max_value_rounding"' not in text
    assert "rounded to float" not in text  # the CPU kernel it is compared with ran on the unrounded values
    assert '"pass": true' in text, text[-800:]


# ---- the gate ----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def _gate_matrix():
    return cc._csr(*synth.delaunay_mesh(2000000, 1, seed=2))


def test_not_slower_than_the_default_plan():
    """delaunay:2000000,1,2,rcm (33 M entries), the scalar unstructured 3-D mesh on which the default plan falls to plain wide
    tiles at 12 bytes per entry.  Premises, asserted: compact tiles hold >= 0.95 of the stored entries (0.9922 by the preview)
    and the format-9 context streams fewer bytes than the default context.  The matrix first passes the correctness check of
    this file.  Then, in one process, a default upload_csr context and an upload_csr_compact_f64 context on the same host
    arrays: three warm-up rounds, 25 rounds of one run of each with a sync behind every run, times from last_run_ns.  Asserted:
    median(c16_f64) <= 1.06 x median(default) -- the in-process placement spread the project has measured (3-6 %, DESIGN §7,
    the perf floor's 1.06).  The expectation, not a condition, was about 0.9 by bytes.
    Measured: default plan 100.0 us, c16_f64 98.8 us, ratio 0.988, at 390.0 against 443.8 MB of streamed bytes (0.879): it is
    not slower, and it does not reach the byte ratio -- the kernel is bound on the gather side as much as by its streams
    (tools/compact_ab.py, medians of ten launches in a row: 91.1 against 96.0 us, 0.949)."""
    rows, cols, p, c, v = _gate_matrix()  # (values U(-1, 1): not floats)
    pre = capi.c16_plan_preview(rows, cols, p, c, table=False)[0]
    share = pre["compact_entries"] / pre["stored_entries"]
    print("%d entries, compact tiles hold %.4f of them (%d compact, %d wide tiles)" % (len(c), share, pre["compact_tiles"], pre["wide_tiles"]))
    assert share >= 0.95
    _check(rows, cols, p, c, v, "delaunay_2m_1dof_rcm")
    x = synth.x_vector(cols)
    with capi.Context(0) as default, capi.Context(0) as compact:
        default.upload_csr(rows, cols, p, c, v)
        compact.upload_csr_compact_f64(rows, cols, p, c, v)
        ways = {"default": default, "c16_f64": compact}
        for ctx in ways.values():
            ctx.set_x(x)
        streamed = {k: ctx.info()["streamed_bytes"] for k, ctx in ways.items()}
        print("streamed bytes: default %d, c16_f64 %d (ratio %.3f); device bytes: default %d, c16_f64 %d" % (
            streamed["default"], streamed["c16_f64"], streamed["c16_f64"] / streamed["default"], default.info()["device_bytes"],
            compact.info()["device_bytes"]))
        assert default.info()["format"] == 1 and compact.info()["format"] == 9
        assert streamed["c16_f64"] == _f64_streamed(pre)
        assert streamed["c16_f64"] < streamed["default"]
        times = {k: [] for k in ways}
        for rnd in range(3 + 25):  # three warm-up rounds
            for k, ctx in ways.items():
                ctx.run()  # one run and a sync
                if rnd >= 3:
                    times[k].append(ctx.last_run_ns() / 1e3)
    med = {k: float(np.median(t)) for k, t in times.items()}
    print("%d runs each: default plan median %.1f us, c16_f64 median %.1f us, ratio %.3f" % (
        len(times["c16_f64"]), med["default"], med["c16_f64"], med["c16_f64"] / med["default"]))
    assert len(times["default"]) == 25 and len(times["c16_f64"]) == 25
    assert med["c16_f64"] <= 1.06 * med["default"], med
