"""The CSR multiply over fp32-stored values, y += fl32(A) x (include/spmv_hip_f32values.h), on the MI355X.  The operator is exactly
the fp64 multiply of the matrix A~ whose values are (double)(float) v, so every case is checked against the oracle's CSR kernel
run on A~ (x = synth.x_vector, a random starting y, three accumulating runs) within the project's tolerance, and bit for bit
under SPMV_HIP_FLAG_EXACT_ORDER.  Level 2 runs with NaN guard elements around x and y, and with the caller's column and float
arrays as views into larger device buffers whose neighbouring entries hold column 0 and value NaN."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import helpers
import oracle_py
from spmv_amd import capi, hostapi, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "spmv-cache-trace_amd", "spmv-cache-trace-hip")
BUS = os.path.join(ROOT, "tests", "golden", "bus1138_like.mtx")
POISSON_FILE = os.path.join(ROOT, "tests", "golden", "poisson2D.mtx")
RUNS = 3
GUARD = 5   # doubles in front of and behind x and y on the device
PAD = 8     # entries in front of and behind the column and float arrays (32 bytes: the views stay 16-byte aligned)
SENTINEL = -7.25


def _narrow(v):
    """(A~'s values as doubles, the float array) by numpy: the reference of the narrowing."""
    with np.errstate(over="ignore"):
        f = np.asarray(v, dtype=np.float64).astype(np.float32)
    return f.astype(np.float64), f


def _expected(rows, cols, p, c, vt, x, y0):
    """(y0 + RUNS A~ x by the oracle's CSR kernel, RUNS (|A~||x|) + |y0|, nterms: the longest row where that exceeds 4096)."""
    if rows == 0:
        return y0.copy(), np.abs(y0), 4096
    if len(c) == 0:
        return y0.copy(), np.abs(y0), 4096
    want = oracle_py.Oracle().csr_spmv(rows, p, c, vt, x, y=y0, num_threads=4, runs=RUNS)
    scale = RUNS * helpers.abs_products(rows, p, c, vt, x) + np.abs(y0)
    return want, scale, max(4096, int(np.max(np.diff(p))))


def _level1(rows, cols, p, c, v, x, y0, flags=0, allow_rounding=True):
    with capi.Context(0, flags) as ctx:
        ctx.upload_csr_f32values(rows, cols, p, c, v, allow_rounding)
        if cols:
            ctx.set_x(x)
        if rows:
            ctx.set_y(y0)
        ctx.run(RUNS)
        y = ctx.get_y()[:rows]
        ns = ctx.last_run_ns()
        return y, ctx.info(), ns


def _guarded(a):
    import torch
    whole = torch.full((len(a) + 2 * GUARD,), float("nan"), dtype=torch.float64, device="cuda:0")
    if len(a):
        whole[GUARD:GUARD + len(a)] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:0")
    return whole, whole[GUARD:GUARD + len(a)]


def _device_csr(p, c, f):
    """row_ptr, and the columns and floats as VIEWS into larger buffers: the PAD entries in front of and behind them hold
    column 0 and value NaN (they may be multiplied, never summed)."""
    import torch
    dev = torch.device("cuda:0")
    n = len(c)
    tp = torch.from_numpy(np.ascontiguousarray(p, dtype=np.int32)).to(dev)
    bc = torch.zeros(n + 2 * PAD, dtype=torch.int32, device=dev)
    bf = torch.full((n + 2 * PAD,), float("nan"), dtype=torch.float32, device=dev)
    if n:
        bc[PAD:PAD + n] = torch.from_numpy(np.ascontiguousarray(c, dtype=np.int32)).to(dev)
        bf[PAD:PAD + n] = torch.from_numpy(np.ascontiguousarray(f, dtype=np.float32)).to(dev)
    return tp, bc, bf, bc.data_ptr() + 4 * PAD, bf.data_ptr() + 4 * PAD


def _level2(rows, cols, p, c, f, x, y0, flags=0, runs=RUNS):
    """`runs` multiplies through an F32Plan over the caller's float array; returns (y, plan info)."""
    import torch
    stream = torch.cuda.current_stream().cuda_stream
    tp, bc, bf, ac, af = _device_csr(p, c, f)
    xw, tx = _guarded(x)
    yw, ty = _guarded(y0)
    yw[:GUARD] = SENTINEL
    yw[GUARD + rows:] = SENTINEL
    with capi.F32Plan(rows, cols, p, flags, stream) as plan:
        for _ in range(runs):
            plan.spmv(tp.data_ptr(), ac, af, xw.data_ptr() + 8 * GUARD, yw.data_ptr() + 8 * GUARD, stream)
        torch.cuda.synchronize()
        info = plan.info()
    yh, xh = yw.cpu().numpy(), xw.cpu().numpy()
    assert np.all(yh[:GUARD] == SENTINEL) and np.all(yh[GUARD + rows:] == SENTINEL), "y written outside its rows entries"
    assert np.all(np.isnan(xh[:GUARD])) and np.all(np.isnan(xh[GUARD + cols:])) and np.array_equal(xh[GUARD:GUARD + cols], x), "x changed"
    assert np.array_equal(bc.cpu().numpy()[PAD:PAD + len(c)], c), "columns changed"
    return yh[GUARD:GUARD + rows].copy(), info


def _inputs(rows, cols, seed=5):
    rng = np.random.default_rng(seed)
    return synth.x_vector(cols), rng.uniform(-1.0, 1.0, size=rows)


def _check(rows, cols, p, c, v, what, lossless=False, exact=True):
    """Level 1, Level 2 (default and exact order) against the oracle on A~ -- on the ORIGINAL values where `lossless`."""
    p, c, v = np.ascontiguousarray(p, dtype=np.int32), np.ascontiguousarray(c, dtype=np.int32), np.ascontiguousarray(v, dtype=np.float64)
    vt, f = _narrow(v)
    inexact = int(np.sum((vt != v) & ~np.isnan(v)))
    if lossless:
        assert inexact == 0, what + ": the case is meant to be float-exact"
        vt = v  # the reference is the oracle on the values as given
    x, y0 = _inputs(rows, cols)
    want, scale, nterms = _expected(rows, cols, p, c, vt, x, y0)
    y2, info2 = _level2(rows, cols, p, c, f, x, y0)
    assert np.all(np.isfinite(y2)), what + ": a neighbouring NaN was summed"
    helpers.assert_close(y2, want, scale, what=what + " (level 2)", nterms=nterms)
    y2b, _ = _level2(rows, cols, p, c, f, x, y0)
    helpers.assert_bitexact(y2b, y2, what + " (a second run from the same y0)")
    y1, info1, ns = _level1(rows, cols, p, c, v, x, y0)
    helpers.assert_bitexact(y1, y2, what + " (level 1 against level 2)")
    assert info1["format"] == 7 and info1["rows"] == rows and info1["cols"] == cols and info1["stored"] == len(c)
    assert info1["streamed_bytes"] == info2["streamed_bytes"] and info1["workgroups"] == info2["workgroups"]
    if rows and cols and len(c):
        assert ns > 0
    pre, _ = capi.f32_plan_preview(rows, cols, p, 0, table=False)
    assert pre == info2  # the host preview and the device plan agree on every number
    if exact:
        ye, infoe = _level2(rows, cols, p, c, f, x, y0, capi.FLAG_EXACT_ORDER)
        helpers.assert_bitexact(ye, want, what + " (exact order, level 2)")
        yeb, _ = _level2(rows, cols, p, c, f, x, y0, capi.FLAG_EXACT_ORDER)
        helpers.assert_bitexact(yeb, ye, what + " (exact order, a second run)")
        ye1, _, _ = _level1(rows, cols, p, c, v, x, y0, capi.FLAG_EXACT_ORDER)
        helpers.assert_bitexact(ye1, want, what + " (exact order, level 1)")
        assert infoe == capi.f32_plan_preview(rows, cols, p, capi.FLAG_EXACT_ORDER, table=False)[0]
    return info2


@functools.lru_cache(maxsize=4)
def _load(spec, expand=False):
    A = hostapi.load(spec, "csr", expand_symmetric=expand)
    out = (A.rows, A.cols, np.array(A.row_ptr), np.array(A.column_index), np.array(A.value))
    A.close()
    return out


def _random(rows, cols, per_row, seed, keep_rows=None, keep_cols=None):
    rng = np.random.default_rng(seed)
    j = np.sort(rng.integers(0, cols, size=(rows, per_row)), axis=1)
    keep = np.ones((rows, per_row), dtype=bool)
    keep[:, 1:] = j[:, 1:] != j[:, :-1]
    if keep_rows is not None:
        keep &= keep_rows[:, None]
    if keep_cols is not None:
        keep &= keep_cols[j]
    p = np.zeros(rows + 1, dtype=np.int32)
    np.cumsum(keep.sum(axis=1), out=p[1:])
    c = j[keep].astype(np.int32)
    return rows, cols, p, c, rng.uniform(-1.0, 1.0, size=len(c))


def _from_lengths(lens, cols, seed):
    rng = np.random.default_rng(seed)
    p = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=p[1:])
    c = np.concatenate([np.sort(rng.choice(cols, size=int(n), replace=False)) for n in lens] or [np.zeros(0, dtype=np.int64)])
    return len(lens), cols, p.astype(np.int32), c.astype(np.int32), rng.uniform(-1, 1, size=len(c))


def _skewed():
    """Row lengths of 1 ... 9000: the edges of the lane choices and of a tile (512 / 513), between runs of short rows."""
    rng = np.random.default_rng(21)
    edges = [1, 2, 15, 16, 17, 31, 32, 33, 64, 65, 128, 129, 255, 256, 257, 508, 509, 511, 512, 513, 1023, 1024, 1025, 2048, 4095, 4096,
             4097, 6000, 8191, 9000]
    lens = []
    for e in edges:
        lens += list(rng.integers(0, 40, size=int(rng.integers(1, 90))))
        lens.append(e)
    lens += [9000, 4097, 1, 0, 4097, 9000]
    return _from_lengths(np.array(lens), 12000, seed=22)


# ---- matrices: against the oracle on A~ ------------------------------------------------------------------------------------------

def test_golden_cases():
    g = helpers.load_golden()
    oracle = oracle_py.Oracle()
    for case in g["cases"]:
        rows, cols, i, j, a, _, _ = helpers.parse_mtx_text(helpers.case_mtx(g, case))
        p, c, v = oracle.csr_from_coordinate(rows, i, j, a, row_alignment=1)
        _check(rows, cols, p, c, v, "golden case %s" % case["name"])
    assert len(g["cases"]) > 0


def test_bus1138_like_expanded():
    rows, cols, p, c, v = _load(BUS, True)
    info = _check(rows, cols, p, c, v, "bus1138_like expanded")
    assert info["tiles"] > 0


def test_poisson_512():
    _check(*synth.poisson2d(512)[:5], "poisson 512^2")


@pytest.mark.parametrize("spec", ["synthetic:queen:40,32,24", "synthetic:queen:40,32,24:tril", "synthetic:kkt:60", "synthetic:kkt:60:tril"])
def test_queen_and_kkt_stand_ins(spec):
    _check(*_load(spec), spec)


@functools.lru_cache(maxsize=2)
def _delaunay(d, order):
    rows, cols, p, c, v = synth.delaunay_mesh(60000, d, seed=3, order=order)
    return rows, cols, np.asarray(p, dtype=np.int32), np.asarray(c, dtype=np.int32), np.asarray(v)


@pytest.mark.parametrize("order", ["rcm", "random"])
@pytest.mark.parametrize("d", [1, 3])
def test_delaunay_60k(d, order):
    _check(*_delaunay(d, order), "delaunay 60k %d-dof %s" % (d, order))


def test_webbase_like_graph():
    rows, cols, p, c, v = _load("synthetic:webbase")
    info = _check(rows, cols, p, c, v, "webbase-like")
    assert info["long_row_tiles"] > 0 and info["longest_row"] > 512


def test_banded():
    _check(*synth.banded(50000, [-40, -3, -1, 0, 1, 2, 57])[:5], "banded")


@pytest.mark.parametrize("rows, cols", [(200000, 5000), (5000, 200000)])
def test_random_rectangles(rows, cols):
    _check(*_random(rows, cols, 8, 21), "random %d x %d" % (rows, cols))


def test_empty_rows_and_columns():
    keep_rows = np.ones(30000, dtype=bool)
    keep_rows[::7] = False
    keep_rows[5000:9000] = False
    keep_cols = np.ones(20000, dtype=bool)
    keep_cols[::5] = False
    keep_cols[12000:16000] = False
    rows, cols, p, c, v = _random(30000, 20000, 6, 3, keep_rows, keep_cols)
    assert np.any(np.diff(p) == 0) and np.any(np.bincount(c, minlength=cols) == 0)
    info = _check(rows, cols, p, c, v, "empty rows and columns")
    assert info["scalar_tiles"] > 0  # tiles of empty rows only


def test_single_dense_row_and_single_dense_column():
    rng = np.random.default_rng(8)
    rows, cols, p, c, v = _random(3000, 20000, 2, 4)
    lens = np.diff(p).copy()
    lens[1717] = cols  # one full row among sparse ones
    r2, c2, p2, j2, v2 = _from_lengths(lens, cols, 9)
    info = _check(r2, c2, p2, j2, v2, "a dense row")
    assert info["long_row_tiles"] == 1 and info["longest_row"] == cols
    rows = 50000  # every row hits column 5
    _check(rows, 64, np.arange(rows + 1, dtype=np.int32), np.full(rows, 5, dtype=np.int32), rng.uniform(-1.0, 1.0, size=rows), "a dense column")


def test_one_row_one_column_and_empty_shapes():
    rng = np.random.default_rng(9)
    n = 3001
    _check(1, n, np.array([0, n], np.int32), np.arange(n, dtype=np.int32), rng.uniform(-1, 1, n), "1 x n")
    _check(n, 1, np.arange(n + 1, dtype=np.int32), np.zeros(n, np.int32), rng.uniform(-1, 1, n), "n x 1")
    _check(1, 1, np.array([0, 1], np.int32), np.array([0], np.int32), np.array([2.5]), "1 x 1")
    _check(0, 7, np.array([0], np.int32), np.zeros(0, np.int32), np.zeros(0), "0 rows")
    _check(7, 0, np.zeros(8, np.int32), np.zeros(0, np.int32), np.zeros(0), "0 cols")
    _check(10, 12, np.zeros(11, np.int32), np.zeros(0, np.int32), np.zeros(0), "no entries")


def test_tiles_that_start_and_end_inside_a_quad():
    """Row lengths 0 .. 7 at random: nnz is not a multiple of 4 and nearly every tile boundary falls inside an aligned quad."""
    rng = np.random.default_rng(13)
    rows, cols = 10007, 9001
    lens = rng.integers(0, 8, size=rows)
    if lens.sum() % 4 == 0:
        lens[-1] += 1
    r, cc, p, c, v = _from_lengths(lens, cols, 14)
    assert int(p[rows]) % 4 != 0
    _, tab = capi.f32_plan_preview(rows, cols, p)
    assert np.any(tab[:, 1] % 4 != 0)
    info = _check(rows, cols, p, c, v, "row lengths 0..7")
    assert info["scalar_tiles"] >= 1  # the last quad of the arrays is not whole


def test_skewed_row_lengths_1_to_9000():
    info = _check(*_skewed(), "row lengths 1 .. 9000")
    assert info["long_row_tiles"] >= 10 and info["longest_row"] == 9000


def test_float_denormal_values():
    """Some values land in the float denormal range (and some below it): they are kept as denormals and widen exactly."""
    rows, cols, p, c, v = _random(20000, 20000, 9, 41)
    rng = np.random.default_rng(42)
    v = v.copy()
    pick = rng.random(len(v)) < 0.3
    v[pick] *= 2.0 ** rng.integers(-160, -120, size=int(pick.sum()))
    vt, f = _narrow(v)
    tiny = np.finfo(np.float32).tiny
    assert np.any((np.abs(f) > 0) & (np.abs(f) < tiny)), "no denormal float among the values"
    x, y0 = _inputs(rows, cols)
    x = x * 2.0 ** 130  # so that the denormal products matter in y
    want, scale, nterms = _expected(rows, cols, p, c, vt, x, y0)
    y2, _ = _level2(rows, cols, p, c, f, x, y0)
    helpers.assert_close(y2, want, scale, what="denormal values (level 2)", nterms=nterms)
    ye, _ = _level2(rows, cols, p, c, f, x, y0, capi.FLAG_EXACT_ORDER)
    helpers.assert_bitexact(ye, want, "denormal values (exact order)")
    y1, _, _ = _level1(rows, cols, p, c, v, x, y0)
    helpers.assert_bitexact(y1, y2, "denormal values (level 1 against level 2)")


# ---- lossless cases: against the oracle on the ORIGINAL values ----------------------------------------------------------------------

def test_lossless_poisson_generated_and_from_the_host_program():
    """The 5-point stencil's -1 and 4 are floats: the oracle on the original values is the reference.  (tests/golden/poisson2D.mtx
    is a finite-element matrix, 2236 of its 2417 values are not floats: it is checked against the oracle on A~ below and among
    the golden cases, and cannot be a lossless case.)"""
    _check(*synth.poisson2d(300)[:5], "poisson 300^2 (lossless)", lossless=True)
    _check(*_load("synthetic:poisson2d:200"), "synthetic:poisson2d:200 (lossless)", lossless=True)
    rows, cols, p, c, v = _load(POISSON_FILE)
    assert int(np.sum(_narrow(v)[0] != v)) > 0
    _check(rows, cols, p, c, v, "poisson2D.mtx")


def test_lossless_pattern_matrix_and_float32_values():
    rows, cols, p, c, v = _random(40000, 30000, 11, 51)
    _check(rows, cols, p, c, np.ones(len(c)), "a pattern matrix (lossless)", lossless=True)
    v32 = np.random.default_rng(52).standard_normal(len(c)).astype(np.float32).astype(np.float64)
    _check(rows, cols, p, c, v32, "values drawn as float32 (lossless)", lossless=True)
    with capi.Context(0) as ctx:  # and Level 1 accepts them with allow_rounding = 0
        ctx.upload_csr_f32values(rows, cols, p, c, v32, allow_rounding=False)


# ---- narrowing on the device ----------------------------------------------------------------------------------------------------------

def _narrow_inputs():
    rng = np.random.default_rng(61)
    fmax = float(np.finfo(np.float32).max)
    floats = rng.standard_normal(5000).astype(np.float32).astype(np.float64)
    lower = np.array([1.0, 1.0 + 2.0 ** -23, 3.0, 2.0 ** -126], dtype=np.float64)  # both parities of the lower neighbour
    ties = np.concatenate([lower + 2.0 ** -24 * np.array([1, 1, 2, 2.0 ** -126]), [1.0 + 3 * 2.0 ** -24]])
    return np.concatenate([
        rng.uniform(-1.0, 1.0, size=200000), rng.uniform(-fmax, fmax, size=50000),
        np.exp(rng.uniform(np.log(1e-50), np.log(fmax * 0.99), size=100000)) * rng.choice([-1.0, 1.0], size=100000),
        floats, ties, 2.0 ** rng.uniform(-152, -124, size=5000), [1.5 * 2.0 ** -149, 2.0 ** -150, 2.0 ** -151],
        [0.0, -0.0, np.inf, -np.inf, np.nan, np.nextafter(2.0 ** 128 - 2.0 ** 103, 0.0)]])


def test_narrow_values_on_the_device_equals_the_host_function():
    import torch
    v = _narrow_inputs()
    f_host, inexact_host, rel_host = capi.narrow_values_host(v)
    tv = torch.from_numpy(v).to("cuda:0")
    tf = torch.zeros(len(v), dtype=torch.float32, device="cuda:0")
    inexact, rel = capi.narrow_values(len(v), tv.data_ptr(), tf.data_ptr(), torch.cuda.current_stream().cuda_stream)
    f_dev = tf.cpu().numpy()
    assert np.array_equal(f_dev.view(np.uint32), f_host.view(np.uint32))
    assert np.array_equal(f_host.view(np.uint32), _narrow(v)[1].view(np.uint32))
    assert inexact == inexact_host and rel == rel_host and inexact > 0
    for bad in (2.0 ** 128 - 2.0 ** 103, 1e300):
        tv[7] = bad
        with pytest.raises(capi.SpmvHipError) as e:
            capi.narrow_values(len(v), tv.data_ptr(), tf.data_ptr())
        assert e.value.code == capi.ERR_OVERFLOW
    assert capi.narrow_values(0, 0, 0) == (0, 0.0)


# ---- Level 1 keeps no fp64 values -------------------------------------------------------------------------------------------------------

def test_level1_keeps_no_fp64_values():
    rows, cols, p, c, v = synth.poisson2d(1024)[:5]
    nnz = len(c)
    assert nnz > 5_000_000
    rng = np.random.default_rng(71)
    v = rng.uniform(-1.0, 1.0, size=nnz)
    pre, _ = capi.f32_plan_preview(rows, cols, p, 0, table=False)
    # what spmv_hip_ctx_info [9] counts for a CSR upload: the arrays (each padded by 64 bytes), the vectors, the plan --
    # with the values priced at 4 bytes per entry
    base = (4 * (rows + 1) + 64) + (4 * nnz + 64) + (4 * nnz + 64) + (8 * cols + 64) + (8 * rows + 64) + pre["device_bytes"]
    with capi.Context(0) as ctx:
        ctx.upload_csr_f32values(rows, cols, p, c, v)
        got = ctx.info()["device_bytes"]
    print("ctx_info[9] = %d, base = %d, base + 2 nnz = %d" % (got, base, base + 2 * nnz))
    assert got < base + 2 * nnz
    assert got >= base - 5 * 64


# ---- refusals ----------------------------------------------------------------------------------------------------------------------

def test_refusals():
    rows, cols, p, c, v = _random(400, 900, 5, 31)
    x, y0 = _inputs(rows, cols)
    with capi.Context(num_gpus=1) as m:
        with pytest.raises(capi.SpmvHipError) as e:
            m.upload_csr_f32values(rows, cols, p, c, v)
        assert e.value.code == capi.ERR_STATE
    inexact = int(np.sum(_narrow(v)[0] != v))
    assert inexact > 0
    with capi.Context(0) as ctx:
        ctx.upload_csr_f32values(rows, cols, p, c, v)
        with pytest.raises(capi.SpmvHipError) as e:
            ctx.upload_csr_f32values(rows, cols, p, c, v, allow_rounding=False)
        assert e.value.code == capi.ERR_INVALID and ("%d value" % inexact) in str(e.value)
        first = int(np.nonzero(_narrow(v)[0] != v)[0][0])
        assert ("entry %d" % first) in str(e.value)
        big = v.copy()
        big[3] = 1e300
        with pytest.raises(capi.SpmvHipError) as e:
            ctx.upload_csr_f32values(rows, cols, p, c, big)
        assert e.value.code == capi.ERR_OVERFLOW
        with pytest.raises(capi.SpmvHipError) as e:
            ctx.upload_csr_f32values(rows, cols - 500, p, c, v)
        assert e.value.code == capi.ERR_INVALID
        # a refused upload leaves the matrix that was there, and the context is usable
        ctx.set_x(x)
        ctx.set_y(y0)
        ctx.run(RUNS)
        want, scale, nterms = _expected(rows, cols, p, c, _narrow(v)[0], x, y0)
        helpers.assert_close(ctx.get_y(), want, scale, what="after refusals", nterms=nterms)
        assert ctx.last_run_ns() > 0
        ctx.flush_caches()
        # there are no fp64 values for the block runs to read
        with pytest.raises(capi.SpmvHipError) as e:
            ctx.set_block_x(np.ones((cols, 2)))
        assert e.value.code == capi.ERR_STATE
        with pytest.raises(capi.SpmvHipError) as e:
            ctx.run_block()
        assert e.value.code == capi.ERR_STATE
        # and a general upload afterwards is a general multiply again
        ctx.upload_csr(rows, cols, p, c, v)
        assert ctx.info()["format"] == 1


def test_spmv_f32_refuses_x_equal_y_and_misaligned_arrays():
    import torch
    rows, cols, p, c, v = _load("synthetic:queen:6,5,4")
    tp, bc, bf, ac, af = _device_csr(p, c, _narrow(v)[1])
    tx = torch.ones(max(rows, cols), dtype=torch.float64, device="cuda:0")
    ty = torch.zeros(rows, dtype=torch.float64, device="cuda:0")
    with capi.F32Plan(rows, cols, p) as plan:
        for args, code in [((tp.data_ptr(), ac, af, tx.data_ptr(), tx.data_ptr()), capi.ERR_INVALID),
                           ((tp.data_ptr(), ac + 4, af, tx.data_ptr(), ty.data_ptr()), capi.ERR_ALIGN),
                           ((tp.data_ptr(), ac, af + 4, tx.data_ptr(), ty.data_ptr()), capi.ERR_ALIGN),
                           ((tp.data_ptr(), ac, 0, tx.data_ptr(), ty.data_ptr()), capi.ERR_INVALID)]:
            with pytest.raises(capi.SpmvHipError) as e:
                plan.spmv(*args)
            assert e.value.code == code
    torch.cuda.synchronize()
    assert float(ty.abs().max()) == 0.0  # nothing was launched


# ---- the host program ------------------------------------------------------------------------------------------------------------

def _cli(matrix, option="--f32-values"):
    return subprocess.run([CLI, "--csr", matrix, "--device", "hip", option, "--threads", "1", "--profile", "4", "--check", "--x", "uniform"],
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)


@pytest.mark.parametrize("matrix", [POISSON_FILE, BUS, "synthetic:kkt:30"])
def test_cli_f32_values_check(matrix):
    r = _cli(matrix)
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout)  # one JSON document
    text = r.stdout
    assert '"hip-csr-spmv-f32values"' in text and '"value_bytes": 4' in text
    assert '"values_inexact"' in text and '"max_value_rounding"' in text
    assert '"pass": true' in text, text[-800:]


def test_cli_f32_values_exact():
    r = _cli("synthetic:poisson2d:200", "--f32-values=exact")  # (the values of tests/golden/poisson2D.mtx are not floats)
    assert r.returncode == 0, r.stderr
    assert '"values_inexact": 0' in r.stdout and '"pass": true' in r.stdout
    r = _cli("synthetic:kkt:30", "--f32-values=exact")
    assert r.returncode == 1 and r.stdout.strip() == "", (r.returncode, r.stdout[:200])
    assert "value" in r.stderr and "not floats" in r.stderr


# ---- the gate ----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def _gate_matrix():
    rows, cols, p, c, v = synth.delaunay_mesh(2000000, 1, seed=2)
    return rows, cols, np.ascontiguousarray(p, dtype=np.int32), np.ascontiguousarray(c, dtype=np.int32), np.ascontiguousarray(v, dtype=np.float64)


@pytest.mark.parametrize("plan_flags", [0, capi.FLAG_NO_INDEX_COMPRESSION], ids=["default_plan", "default_plan_32bit_columns_only"])
def test_not_slower_than_the_default_plan_on_the_scalar_delaunay_mesh(plan_flags):
    """delaunay:2000000,1,2 (33 M entries): the default plan multiplies it in plain wide tiles at 12 bytes per entry; the fp32-value
    multiply does the same gathers, products and row sums on about two thirds of the streamed bytes, so it must not be slower:
    median launch time <= 1.10 x spmv_hip_csr_spmv's with the default plan, both in one process on the same device arrays,
    launches interleaved, 25 each after warm-up.  The premise is read from the default plan's plan_info first (no block, group,
    window, panel, shifted, stencil or dictionary tiles; more streamed bytes than the fp32-value plan); where it does not hold
    the figures are printed and the gate is skipped.  Measured: the default plan gives 3 of this matrix's tiles an x window (and
    9705 of them 16-bit columns), so the premise fails by the letter for plan_flags = 0 (97.3 us against 74.0 us for the
    fp32-value multiply all the same: ratio 0.76, by bytes 0.72); the second case builds the plan as spmv_hip_upload_csr does
    under SPMV_HIP_FLAG_NO_INDEX_COMPRESSION -- nothing derived from the columns, every tile plain with 32-bit columns, 12 bytes
    per entry: the premise as the text states it -- and the same bound holds there by the same reasoning (measured: 89.6 us
    against 73.6 us, ratio 0.82, by bytes 0.71)."""
    import torch
    rows, cols, p, c, v = _gate_matrix()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    tp, tc, tv = (torch.from_numpy(a).to(dev) for a in (p, c, v))
    tf = torch.zeros(len(c), dtype=torch.float32, device=dev)
    inexact, rel = capi.narrow_values(len(c), tv.data_ptr(), tf.data_ptr(), stream)
    tx = torch.from_numpy(synth.x_vector(cols)).to(dev)
    ty = torch.zeros(rows, dtype=torch.float64, device=dev)
    plan = capi.CsrPlan(rows, cols, p, capi.CSR_AUTO, 0, plan_flags)  # the plan spmv_hip_upload_csr builds under these flags:
    if not plan_flags & capi.FLAG_NO_INDEX_COMPRESSION:               # (with that flag it derives nothing from the columns)
        plan.confirm_blocks(tp.data_ptr(), tc.data_ptr(), p, stream)
        plan.compress(tc.data_ptr(), stream)
        plan.repack(tp.data_ptr(), tc.data_ptr(), tv.data_ptr(), stream)
        plan.index_values(tv.data_ptr(), stream)
    with capi.F32Plan(rows, cols, p, 0, stream) as f32:
        d, i = plan.info(), f32.info()
        special = {k: d[k] for k in ("block_tiles", "group_tiles", "xwin_tiles", "blockwin_tiles", "segwin_tiles", "panel_tiles",
                                     "shifted_tiles", "indexed_values", "masked_block_tiles", "stencil_mask_tiles", "run_tiles") if d[k]}
        ways = {
            "fp64": lambda: plan.spmv(tp.data_ptr(), tc.data_ptr(), tv.data_ptr(), tx.data_ptr(), ty.data_ptr(), stream),
            "f32": lambda: f32.spmv(tp.data_ptr(), tc.data_ptr(), tf.data_ptr(), tx.data_ptr(), ty.data_ptr(), stream),
        }
        times = {k: [] for k in ways}
        for rnd in range(3 + 25):  # three warm-up rounds
            for k, run in ways.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run()
                e1.record()
                torch.cuda.synchronize()
                if rnd >= 3:
                    times[k].append(e0.elapsed_time(e1) * 1e3)
    plan.close()
    med = {k: float(np.median(t)) for k, t in times.items()}
    print("delaunay:2000000,1,2, %d entries (%d inexact as floats, largest relative change %.3g), %d launches each: "
          "default fp64 plan (flags %#x) median %.1f us, fp32-value plan median %.1f us, ratio %.3f; streamed bytes %d against %d, ratio %.3f" % (
              len(c), inexact, rel, len(times["f32"]), plan_flags, med["fp64"], med["f32"], med["f32"] / med["fp64"], i["streamed_bytes"],
              d["streamed_bytes"], i["streamed_bytes"] / d["streamed_bytes"]))
    if special or d["streamed_bytes"] <= i["streamed_bytes"]:
        print("gate skipped: the default plan is not plain tiles streaming more bytes: %r, %d against %d bytes" % (
            special, d["streamed_bytes"], i["streamed_bytes"]))
        pytest.skip("the premise (same work on fewer bytes) does not hold for this plan: %r" % (special,))
    assert len(times["fp64"]) >= 20 and len(times["f32"]) >= 20
    assert med["f32"] <= 1.10 * med["fp64"], med
