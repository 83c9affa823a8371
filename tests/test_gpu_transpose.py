"""The transposed multiply y += A' x (include/spmv_hip_transpose.h) on the MI355X, from the CSR arrays of A as they are.  Every
case is checked against the oracle's CSR kernel run on the scipy-transposed arrays (sorted indices) with x = synth.x_vector and
a random starting y over three accumulating runs, within the project's tolerance (the products meet in fp64 atomics: no
bit-exactness is claimed).  Level 2 runs with guard elements around x and y."""
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
GUARD = 5  # doubles in front of and behind x and y on the device
SENTINEL = -7.25


def _sp(rows, cols, p, c, v):
    import scipy.sparse as sp
    return sp.csr_matrix((np.asarray(v, dtype=np.float64), np.asarray(c, dtype=np.int32), np.asarray(p, dtype=np.int32)), shape=(rows, cols))


def _arrays(M):
    M = M.tocsr()
    M.sort_indices()
    return M.shape[0], M.shape[1], M.indptr.astype(np.int32), M.indices.astype(np.int32), M.data.astype(np.float64)


def _expected(rows, cols, p, c, v, x, y0):
    """(y0 + RUNS A' x by the oracle's CSR kernel on the transposed arrays, the scale of the rounding RUNS (|A'| |x|) + |y0|,
    nterms for helpers.assert_close: the longest column of A where that exceeds 4096)."""
    if cols == 0:
        return y0.copy(), np.abs(y0), 4096
    if rows == 0:
        return y0.copy(), np.abs(y0), 4096
    At = _sp(rows, cols, p, c, v).T.tocsr()
    At.sort_indices()
    tp, tc, tv = At.indptr.astype(np.int32), At.indices.astype(np.int32), At.data.astype(np.float64)
    want = oracle_py.Oracle().csr_spmv(cols, tp, tc, tv, x, y=y0, num_threads=4, runs=RUNS)
    scale = RUNS * (abs(At) @ np.abs(x)) + np.abs(y0)
    longest = int(np.max(np.diff(tp))) if cols else 0
    return want, scale, max(4096, longest)


def _level1(rows, cols, p, c, v, x, y0, flags=0):
    with capi.Context(0, flags) as ctx:
        ctx.upload_csr_transposed(rows, cols, p, c, v)
        if rows:
            ctx.set_x(x)
        if cols:
            ctx.set_y(y0)
        ctx.run(RUNS)
        y = ctx.get_y()[:cols]
        ns = ctx.last_run_ns()
        return y, ctx.info(), ns


def _device_csr(p, c, v):
    import torch
    dev = torch.device("cuda:0")
    n = max(1, len(c))
    tp = torch.from_numpy(np.ascontiguousarray(p, dtype=np.int32)).to(dev)
    tc = torch.zeros(n, dtype=torch.int32, device=dev)
    tv = torch.zeros(n, dtype=torch.float64, device=dev)
    if len(c):
        tc[:len(c)] = torch.from_numpy(np.ascontiguousarray(c, dtype=np.int32)).to(dev)
        tv[:len(c)] = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(dev)
    return tp, tc, tv


def _guarded(a):
    """A device vector with GUARD sentinels (NaN: a read of one poisons y) in front and behind; (whole, view of the middle)."""
    import torch
    whole = torch.full((len(a) + 2 * GUARD,), float("nan"), dtype=torch.float64, device="cuda:0")
    if len(a):
        whole[GUARD:GUARD + len(a)] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:0")
    return whole, whole[GUARD:GUARD + len(a)]


def _level2(rows, cols, p, c, v, x, y0, max_windows=0, window_doubles=0, columns_after_plan=None):
    """RUNS multiplies through a TrPlan; x and y sit between guard elements that must come back untouched.
    columns_after_plan: a column array written over the device columns AFTER the plan was made."""
    import torch
    stream = torch.cuda.current_stream().cuda_stream
    tp, tc, tv = _device_csr(p, c, v)
    xw, tx = _guarded(x)
    yw, ty = _guarded(y0)
    yw[:GUARD] = SENTINEL
    yw[GUARD + cols:] = SENTINEL
    with capi.TrPlan(rows, cols, p, tc.data_ptr(), max_windows, window_doubles, stream) as plan:
        if columns_after_plan is not None:
            tc[:len(c)] = torch.from_numpy(np.ascontiguousarray(columns_after_plan, dtype=np.int32)).to("cuda:0")
        for _ in range(RUNS):
            plan.spmv_t(tp.data_ptr(), tc.data_ptr(), tv.data_ptr(), tx.data_ptr() if rows else xw.data_ptr(),
                        ty.data_ptr() if cols else yw.data_ptr(), stream)
        torch.cuda.synchronize()
        info = plan.info()
    yh, xh = yw.cpu().numpy(), xw.cpu().numpy()
    assert np.all(yh[:GUARD] == SENTINEL) and np.all(yh[GUARD + cols:] == SENTINEL), "y written outside its cols entries"
    assert np.all(np.isnan(xh[:GUARD])) and np.all(np.isnan(xh[GUARD + rows:])) and np.array_equal(xh[GUARD:GUARD + rows], x), "x changed"
    return yh[GUARD:GUARD + cols].copy(), info


def _inputs(rows, cols, seed=5):
    rng = np.random.default_rng(seed)
    return synth.x_vector(rows), rng.uniform(-1.0, 1.0, size=cols)


def _check_both(rows, cols, p, c, v, what, **plan_args):
    x, y0 = _inputs(rows, cols)
    want, scale, nterms = _expected(rows, cols, p, c, v, x, y0)
    y1, info1, ns = _level1(rows, cols, p, c, v, x, y0)
    helpers.assert_close(y1, want, scale, what=what + " (level 1)", nterms=nterms)
    assert info1["format"] == 6 and info1["rows"] == cols and info1["cols"] == rows and info1["stored"] == len(c)
    if rows and cols and len(c):
        assert ns > 0
    y2, info2 = _level2(rows, cols, p, c, v, x, y0, **plan_args)
    helpers.assert_close(y2, want, scale, what=what + " (level 2)", nterms=nterms)
    helpers.assert_close(y2, y1, scale, what=what + " (level 1 against level 2)", nterms=nterms)
    assert info2["rows"] == rows and info2["cols"] == cols and info2["stored_entries"] == len(c)
    assert info2["lds_bytes"] <= 80 * 1024
    assert info2["atomic_bytes"] == 8 * (info2["window_slots"] + info2["spilled_entries"])
    # the host preview and the device plan agree on every number
    pre, _ = capi.tr_plan_preview(rows, cols, p, c, plan_args.get("max_windows", 0), plan_args.get("window_doubles", 0), table=False)
    assert pre == info2
    return info2


@functools.lru_cache(maxsize=4)
def _load(spec, expand=False):
    A = hostapi.load(spec, "csr", expand_symmetric=expand)
    out = (A.rows, A.cols, np.array(A.row_ptr), np.array(A.column_index), np.array(A.value))
    A.close()
    return out


def _random(rows, cols, per_row, seed, keep_rows=None, keep_cols=None):
    """per_row uniformly random columns in every row (repeats within a row dropped), values U(-1, 1); keep_rows / keep_cols:
    boolean masks of the rows / columns that keep their entries."""
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


# ---- matrices ------------------------------------------------------------------------------------------------------------------

def test_bus1138_like_expanded():
    _check_both(*_load(BUS, True), "bus1138_like expanded")


def test_poisson2d_file():
    _check_both(*_load(POISSON_FILE), "poisson2D.mtx")


def test_poisson_512():
    info = _check_both(*synth.poisson2d(512), "poisson 512^2")
    assert info["spilled_entries"] == 0  # a range of 2048 rows hits its own four lines and one more on each side: they fit


@pytest.mark.parametrize("spec, expand", [("synthetic:queen:40,32,24", False), ("synthetic:queen:tril", False),
                                          ("synthetic:kkt:60", False), ("synthetic:kkt:125:tril", False)])
def test_queen_and_kkt_stand_ins(spec, expand):
    info = _check_both(*_load(spec, expand), spec)
    if spec == "synthetic:queen:tril":
        assert info["spilled_entries"] == 0  # what the symmetric plan's four windows reach on the same triangle


@functools.lru_cache(maxsize=2)
def _delaunay(order):
    rows, cols, p, c, v = synth.delaunay_mesh(60000, 3, seed=3, order=order)
    return rows, cols, np.asarray(p, dtype=np.int32), np.asarray(c, dtype=np.int32), np.asarray(v)


@pytest.mark.parametrize("order", ["rcm", "random"])
def test_delaunay_3dof_60k(order):
    info = _check_both(*_delaunay(order), "delaunay 60k 3-dof " + order)
    if order == "random":
        assert info["spilled_entries"] > 0  # a randomly numbered mesh does not fit a few windows


def test_webbase_like_graph():
    rows, cols, p, c, v = _load("synthetic:webbase")
    longest_column = int(np.max(np.bincount(c, minlength=cols)))
    assert longest_column > 4096  # hub pages: the summation bound needs the real term count (nterms)
    _check_both(rows, cols, p, c, v, "webbase-like")


def test_banded():
    n = 50000
    rows, cols, p, c, v = synth.banded(n, [-40, -3, -1, 0, 1, 2, 57])[:5]
    _check_both(rows, cols, p, c, v, "banded")


@pytest.mark.parametrize("rows, cols", [(200000, 5000), (5000, 200000)])
def test_random_rectangles(rows, cols):
    _check_both(*_random(rows, cols, 8, 21), "random %d x %d" % (rows, cols))


def test_empty_rows_and_columns():
    keep_rows = np.ones(30000, dtype=bool)
    keep_rows[::7] = False
    keep_rows[5000:9000] = False
    keep_cols = np.ones(20000, dtype=bool)
    keep_cols[::5] = False
    keep_cols[12000:16000] = False
    rows, cols, p, c, v = _random(30000, 20000, 6, 3, keep_rows, keep_cols)
    assert np.any(np.diff(p) == 0) and np.any(np.bincount(c, minlength=cols) == 0)
    _check_both(rows, cols, p, c, v, "empty rows and columns")


def test_single_dense_row_and_single_dense_column():
    import scipy.sparse as sp
    rng = np.random.default_rng(8)
    # one full row among sparse ones
    A = _sp(*_random(3000, 20000, 2, 4)).tolil()
    A[1717, :] = rng.uniform(-1.0, 1.0, size=20000)
    _check_both(*_arrays(A.tocsr()), "a dense row")
    # every row hits column 5: every product lands on one y[j]
    rows = 50000
    p = np.arange(rows + 1, dtype=np.int32)
    c = np.full(rows, 5, dtype=np.int32)
    v = rng.uniform(-1.0, 1.0, size=rows)
    x, y0 = _inputs(rows, 64)
    want, scale, nterms = _expected(rows, 64, p, c, v, x, y0)
    assert nterms == rows
    y2, _ = _level2(rows, 64, p, c, v, x, y0)
    helpers.assert_close(y2, want, scale, what="a dense column (level 2)", nterms=nterms)
    y1, _, _ = _level1(rows, 64, p, c, v, x, y0)
    helpers.assert_close(y1, want, scale, what="a dense column (level 1)", nterms=nterms)


def test_one_row_one_column_and_empty_shapes():
    rng = np.random.default_rng(9)
    n = 3001
    _check_both(1, n, np.array([0, n], np.int32), np.arange(n, dtype=np.int32), rng.uniform(-1, 1, n), "1 x n")
    _check_both(n, 1, np.arange(n + 1, dtype=np.int32), np.zeros(n, np.int32), rng.uniform(-1, 1, n), "n x 1")
    _check_both(1, 1, np.array([0, 1], np.int32), np.array([0], np.int32), np.array([2.5]), "1 x 1")
    _check_both(0, 7, np.array([0], np.int32), np.zeros(0, np.int32), np.zeros(0), "0 rows")
    _check_both(7, 0, np.zeros(8, np.int32), np.zeros(0, np.int32), np.zeros(0), "0 cols")
    _check_both(10, 12, np.zeros(11, np.int32), np.zeros(0, np.int32), np.zeros(0), "no entries")


def _quad_matrix():
    """Row lengths 0 .. 7 at random, nnz no multiple of 4 (test_ranges_that_start_and_end_inside_a_quad)."""
    rng = np.random.default_rng(13)
    rows, cols = 10007, 9001
    lens = rng.integers(0, 8, size=rows)
    if lens.sum() % 4 == 0:
        lens[-1] += 1
    p = np.zeros(rows + 1, dtype=np.int32)
    np.cumsum(lens, out=p[1:])
    nnz = int(p[rows])
    assert nnz % 4 != 0
    c = np.concatenate([np.sort(rng.choice(cols, size=int(p[r + 1] - p[r]), replace=False)) for r in range(rows)]).astype(np.int32)
    v = rng.uniform(-1.0, 1.0, size=nnz)
    return rows, cols, p, c, v


@pytest.mark.parametrize("window_doubles", [0, 100])
def test_ranges_that_start_and_end_inside_a_quad(window_doubles):
    """Row lengths 0 .. 7 at random: nnz is not a multiple of 4 and nearly every range boundary (every 2048 rows, or every 100
    with window_doubles = 100) falls inside an aligned quad of entries."""
    rows, cols, p, c, v = _quad_matrix()
    R = window_doubles or 2048
    assert np.any(p[R:rows:R] % 4 != 0)
    _check_both(rows, cols, p, c, v, "row lengths 0..7, window_doubles=%d" % window_doubles, window_doubles=window_doubles)


# ---- plans -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["poisson512", "tall", "wide"])
def test_forced_spills_agree(name):
    A = {"poisson512": lambda: synth.poisson2d(512), "tall": lambda: _random(200000, 5000, 8, 21),
         "wide": lambda: _random(5000, 200000, 8, 21)}[name]()
    rows, cols, p, c, v = A[:5]
    x, y0 = _inputs(rows, cols)
    want, scale, nterms = _expected(rows, cols, p, c, v, x, y0)
    y_auto, info_auto = _level2(rows, cols, p, c, v, x, y0)
    y_tiny, info_tiny = _level2(rows, cols, p, c, v, x, y0, max_windows=1, window_doubles=32)
    helpers.assert_close(y_auto, want, scale, what=name + " automatic windows", nterms=nterms)
    helpers.assert_close(y_tiny, want, scale, what=name + " max_windows=1, window_doubles=32", nterms=nterms)
    helpers.assert_close(y_tiny, y_auto, scale, what=name + " tiny against automatic", nterms=nterms)
    assert info_tiny["spilled_entries"] > 0
    assert info_tiny["max_windows"] == 1 and info_tiny["rows_per_range"] == 32
    assert info_tiny["spilled_entries"] >= info_auto["spilled_entries"]
    if name == "poisson512":
        assert info_auto["spilled_entries"] == 0
    for mw in (2, 3, 8):  # every kernel instantiation
        y_mw, info_mw = _level2(rows, cols, p, c, v, x, y0, max_windows=mw, window_doubles=64)
        helpers.assert_close(y_mw, want, scale, what=name + " max_windows=%d" % mw, nterms=nterms)
        assert info_mw["max_windows"] == mw


def test_consistent_with_the_symmetric_multiply_of_a_stored_triangle():
    """On a stored triangle T: T x (the general multiply) + T' x (the new one) - diag(T) x is what spmv_hip_csr_symv adds."""
    import torch
    rows, cols, p, c, v = _load("synthetic:queen:30,24,20:tril")
    assert capi.csr_triangle(rows, p, c)[0] == capi.TRIANGLE_LOWER
    x = synth.x_vector(rows)
    with capi.Context(0) as ctx:
        ctx.upload_csr(rows, cols, p, c, v)
        ctx.set_x(x)
        ctx.run()
        y_t = ctx.get_y()
        ctx.upload_csr_transposed(rows, cols, p, c, v)
        ctx.set_x(x)
        ctx.run()
        y_tt = ctx.get_y()
        ctx.upload_csr_symmetric(rows, p, c, v)
        ctx.set_x(x)
        ctx.run()
        y_sym = ctx.get_y()
    T = _sp(rows, cols, p, c, v)
    scale = (abs(T) + abs(T).T) @ np.abs(x)
    helpers.assert_close(y_t + y_tt - T.diagonal() * x, y_sym, scale, what="T x + T' x - D x against symv")


def test_columns_changed_after_planning_give_the_changed_matrix():
    rows, cols, p, c, v = synth.poisson2d(300)[:5]
    rng = np.random.default_rng(17)
    changed = np.array(c, dtype=np.int32)
    pick = rng.choice(len(c), size=len(c) // 3, replace=False)
    changed[pick] = rng.integers(0, cols, size=len(pick))  # anywhere inside [0, cols): mostly outside the planned windows
    x, y0 = _inputs(rows, cols)
    want, scale, nterms = _expected(rows, cols, p, changed, v, x, y0)  # (scipy keeps repeated columns of a row apart)
    y2, info = _level2(rows, cols, p, c, v, x, y0, columns_after_plan=changed)
    helpers.assert_close(y2, want, scale, what="columns changed after planning", nterms=nterms)
    assert info["spilled_entries"] == 0  # the numbers still describe the matrix that was planned


def test_spmv_t_refuses_x_equal_y_and_misaligned_arrays():
    import torch
    rows, cols, p, c, v = _load("synthetic:queen:6,5,4")
    tp, tc, tv = _device_csr(p, c, v)
    tx = torch.ones(rows + 2, dtype=torch.float64, device="cuda:0")
    ty = torch.zeros(cols, dtype=torch.float64, device="cuda:0")
    with capi.TrPlan(rows, cols, p, tc.data_ptr()) as plan:
        with pytest.raises(capi.SpmvHipError) as e:
            plan.spmv_t(tp.data_ptr(), tc.data_ptr(), tv.data_ptr(), tx.data_ptr(), tx.data_ptr())
        assert e.value.code == capi.ERR_INVALID
        with pytest.raises(capi.SpmvHipError) as e:
            plan.spmv_t(tp.data_ptr(), tc.data_ptr() + 4, tv.data_ptr(), tx.data_ptr(), ty.data_ptr())
        assert e.value.code == capi.ERR_ALIGN
        with pytest.raises(capi.SpmvHipError) as e:
            plan.spmv_t(tp.data_ptr(), tc.data_ptr(), 0, tx.data_ptr(), ty.data_ptr())
        assert e.value.code == capi.ERR_INVALID
    torch.cuda.synchronize()
    assert float(ty.abs().max()) == 0.0  # nothing was launched


# ---- refusals --------------------------------------------------------------------------------------------------------------------

def test_refusals():
    rows, cols, p, c, v = _random(400, 900, 5, 31)
    with capi.Context(num_gpus=1) as m:
        with pytest.raises(capi.SpmvHipError) as e:
            m.upload_csr_transposed(rows, cols, p, c, v)
        assert e.value.code == capi.ERR_STATE
    with capi.Context(0, capi.FLAG_EXACT_ORDER) as ctx:
        with pytest.raises(capi.SpmvHipError) as e:
            ctx.upload_csr_transposed(rows, cols, p, c, v)
        assert e.value.code == capi.ERR_INVALID
    import torch
    tc = torch.from_numpy(c).to("cuda:0")
    with pytest.raises(capi.SpmvHipError) as e:
        capi.TrPlan(rows, cols - 500, p, tc.data_ptr())  # columns outside [0, cols)
    assert e.value.code == capi.ERR_INVALID and "out of range" in str(e.value)
    with capi.Context(0) as ctx:
        x, y0 = _inputs(rows, cols)
        ctx.upload_csr_transposed(rows, cols, p, c, v)
        with pytest.raises(capi.SpmvHipError) as e:
            ctx.upload_csr_transposed(rows, cols - 500, p, c, v)
        assert e.value.code == capi.ERR_INVALID
        # a refused upload leaves the matrix that was there, and the context is usable
        ctx.set_x(x)
        ctx.set_y(y0)
        ctx.run(RUNS)
        want, scale, nterms = _expected(rows, cols, p, c, v, x, y0)
        helpers.assert_close(ctx.get_y(), want, scale, what="after refusals", nterms=nterms)
        assert ctx.last_run_ns() > 0
        ctx.flush_caches()
        # and a general upload after a transposed one is a general multiply again
        ctx.upload_csr(rows, cols, p, c, v)
        ctx.set_x(synth.x_vector(cols))
        ctx.run()
        assert ctx.info()["format"] == 1 and len(ctx.get_y()) == rows


# ---- the host program ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("matrix", [POISSON_FILE, "synthetic:queen:20,16,12"])
def test_cli_transpose_check(matrix):
    r = subprocess.run([CLI, "--csr", matrix, "--device", "hip", "--transpose", "--threads", "1", "--profile", "4", "--check", "--x", "uniform"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    doc = json.loads(r.stdout)  # one JSON document
    text = r.stdout
    assert '"hip-csr-spmv-transposed"' in text
    assert '"transposed": true' in text
    assert '"pass": true' in text and "transposed on the host" in text, text[-800:]
    assert doc


# ---- the gate ----------------------------------------------------------------------------------------------------------------------

def test_not_slower_than_the_symmetric_multiply_on_the_queen_triangle():
    """On a stored lower triangle the transposed multiply does a subset of what spmv_hip_csr_symv does on the same arrays (the
    same streams, the same scatter adds, no row sums), so it must not be slower: median launch time <= 1.10 x the symmetric
    multiply's, both plans in one process on the same device arrays, launches interleaved, 25 each after warm-up."""
    import torch
    rows, cols, p, c, v = _load("synthetic:queen:tril")
    stream = torch.cuda.current_stream().cuda_stream
    tp, tc, tv = _device_csr(p, c, v)
    tx = torch.from_numpy(synth.x_vector(rows)).to("cuda:0")
    ty = torch.zeros(rows, dtype=torch.float64, device="cuda:0")
    with capi.SymPlan(rows, p, tc.data_ptr(), capi.SYMMETRIC, 0, 0, stream) as sym, capi.TrPlan(rows, cols, p, tc.data_ptr(), 0, 0, stream) as tr:
        ways = {
            "symv": lambda: sym.symv(tp.data_ptr(), tc.data_ptr(), tv.data_ptr(), tx.data_ptr(), ty.data_ptr(), stream),
            "spmv_t": lambda: tr.spmv_t(tp.data_ptr(), tc.data_ptr(), tv.data_ptr(), tx.data_ptr(), ty.data_ptr(), stream),
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
        info = tr.info()
    med = {k: float(np.median(t)) for k, t in times.items()}
    print("queen:tril, %d launches each: spmv_hip_csr_symv median %.1f us, spmv_hip_csr_spmv_t median %.1f us, ratio %.3f; "
          "transposed plan: %d windows in %d ranges, %d spilled, %.1f MB of atomic adds" % (
              len(times["symv"]), med["symv"], med["spmv_t"], med["spmv_t"] / med["symv"], info["windows"], info["ranges"],
              info["spilled_entries"], info["atomic_bytes"] / 1e6))
    assert len(times["symv"]) >= 20 and len(times["spmv_t"]) >= 20
    assert med["spmv_t"] <= 1.10 * med["symv"], med
