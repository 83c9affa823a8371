"""The symmetric multiply of a stored triangle (include/spmv_hip_symmetric.h) on the MI355X: y += (T + T' - diag(T)) x, or
(T - T') x for a skew-symmetric matrix, from the triangle T alone.  Every case is checked against scipy's T + T' - D (T - T')
with x = synth.x_vector and a random starting y over three accumulating runs, within the project's tolerance (the partial sums
meet in fp64 atomics: no bit-exactness is claimed)."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import helpers
from spmv_amd import capi, hostapi, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "spmv-cache-trace_amd", "spmv-cache-trace-hip")
BUS = os.path.join(ROOT, "tests", "golden", "bus1138_like.mtx")
RUNS = 3


def _sp(rows, p, c, v):
    import scipy.sparse as sp
    return sp.csr_matrix((np.asarray(v, dtype=np.float64), np.asarray(c, dtype=np.int64), np.asarray(p, dtype=np.int64)), shape=(rows, rows))


def _csr(T):
    T = T.tocsr()
    T.sort_indices()
    return T.shape[0], T.indptr.astype(np.int32), T.indices.astype(np.int32), T.data.astype(np.float64)


def _tril(rows, p, c, v, k=0):
    import scipy.sparse as sp
    return _csr(sp.tril(_sp(rows, p, c, v), k=k, format="csr"))


def _upper(rows, p, c, v):
    return _csr(_sp(rows, p, c, v).T)


def _expected(rows, p, c, v, x, y0, kind):
    """y0 + RUNS (E x) with E = T + T' - D (symmetric) or T - T' (skew) built by scipy, and the scale of the rounding:
    RUNS (|E| |x|) + |y0|."""
    import scipy.sparse as sp
    if rows == 0:
        return y0.copy(), np.abs(y0)
    T = _sp(rows, p, c, v)
    if kind == capi.SYMMETRIC:
        E = (T + T.T - sp.diags(T.diagonal())).tocsr()
    else:
        E = (T - T.T).tocsr()
    want = y0 + RUNS * (E @ x)
    scale = RUNS * (abs(E) @ np.abs(x)) + np.abs(y0)
    return want, scale


def _expected_operator(rows, p, c, v, x, y0):
    """The same for matrices too large to expand in memory here: T x + T' x - D x without forming T + T'."""
    T = _sp(rows, p, c, v)
    d = T.diagonal()
    want = y0 + RUNS * (T @ x + T.T @ x - d * x)
    A = abs(T)
    scale = RUNS * (A @ np.abs(x) + A.T @ np.abs(x)) + np.abs(y0)
    return want, scale


def _level1(rows, p, c, v, x, y0, kind=capi.SYMMETRIC, flags=0):
    with capi.Context(0, flags) as ctx:
        ctx.upload_csr_symmetric(rows, p, c, v, kind)
        if rows:
            ctx.set_x(x)
            ctx.set_y(y0)
        ctx.run(RUNS)
        return ctx.get_y(), ctx.info()


def _level2(rows, p, c, v, x, y0, kind=capi.SYMMETRIC, max_windows=0, window_doubles=0):
    import torch
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    n = max(1, len(c))
    tp = torch.from_numpy(np.ascontiguousarray(p, dtype=np.int32)).to(dev)
    tc = torch.zeros(n, dtype=torch.int32, device=dev)
    tv = torch.zeros(n, dtype=torch.float64, device=dev)
    if len(c):
        tc[:len(c)] = torch.from_numpy(np.ascontiguousarray(c, dtype=np.int32)).to(dev)
        tv[:len(c)] = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(dev)
    tx = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev) if rows else torch.zeros(1, dtype=torch.float64, device=dev)
    ty = torch.from_numpy(np.ascontiguousarray(y0, dtype=np.float64)).to(dev) if rows else torch.zeros(1, dtype=torch.float64, device=dev)
    with capi.SymPlan(rows, p, tc.data_ptr(), kind, max_windows, window_doubles, stream) as plan:
        for _ in range(RUNS):
            plan.symv(tp.data_ptr(), tc.data_ptr(), tv.data_ptr(), tx.data_ptr(), ty.data_ptr(), stream)
        torch.cuda.synchronize()
        return ty.cpu().numpy()[:rows], plan.info()


def _inputs(rows, seed=5):
    rng = np.random.default_rng(seed)
    return synth.x_vector(rows), rng.uniform(-1.0, 1.0, size=rows)


def _check_both(rows, p, c, v, what, kind=capi.SYMMETRIC, operator=False, level2=True):
    x, y0 = _inputs(rows)
    want, scale = (_expected_operator(rows, p, c, v, x, y0) if operator else _expected(rows, p, c, v, x, y0, kind))
    y1, info1 = _level1(rows, p, c, v, x, y0, kind)
    helpers.assert_close(y1, want, scale, what=what + " (level 1)")
    assert info1["format"] == 5
    if level2:
        y2, info2 = _level2(rows, p, c, v, x, y0, kind)
        helpers.assert_close(y2, want, scale, what=what + " (level 2)")
        helpers.assert_close(y2, y1, scale, what=what + " (level 1 against level 2)")
        return info2
    return None


def _load(spec):
    A = hostapi.load(spec, "csr")
    out = (A.rows, np.array(A.row_ptr), np.array(A.column_index), np.array(A.value))
    A.close()
    return out


# ---- matrices ------------------------------------------------------------------------------------------------------------------

def test_bus1138_like_file():
    rows, p, c, v = _load(BUS)
    t, d = capi.csr_triangle(rows, p, c)
    assert t in (capi.TRIANGLE_LOWER, capi.TRIANGLE_UPPER) and d > 0
    info = _check_both(rows, p, c, v, "bus1138_like")
    assert info["stored_entries"] == len(c) and info["diagonal_entries"] == d


def test_bus1138_like_upper():
    rows, p, c, v = _upper(*_load(BUS))
    assert capi.csr_triangle(rows, p, c)[0] == capi.TRIANGLE_UPPER
    _check_both(rows, p, c, v, "bus1138_like, upper")


@pytest.mark.parametrize("upper", [False, True])
def test_poisson_512_triangle(upper):
    rows, cols, p, c, v = synth.poisson2d(512)
    T = _tril(rows, p, c, v)
    if upper:
        T = _upper(*T)
    info = _check_both(*T, "poisson 512^2 " + ("upper" if upper else "lower"))
    assert info["triangle"] == (capi.TRIANGLE_UPPER if upper else capi.TRIANGLE_LOWER)


@pytest.mark.parametrize("upper", [False, True])
def test_queen_small_tril(upper):
    T = _load("synthetic:queen:30,24,20:tril")
    if upper:
        T = _upper(*T)
    _check_both(*T, "queen:30,24,20:tril" + (" upper" if upper else ""))


def test_queen_full_size_tril():
    rows, p, c, v = _load("synthetic:queen:tril")
    info = _check_both(rows, p, c, v, "queen:tril (full size)", operator=True)
    # a mesh in natural order: the previous line and plane fit the windows, almost nothing is spilled
    assert info["spilled_entries"] < 0.01 * len(c), info
    assert info["multiplied_entries"] == 2 * len(c) - info["diagonal_entries"]


def test_kkt_125_tril():
    rows, p, c, v = _load("synthetic:kkt:125:tril")
    _check_both(rows, p, c, v, "kkt:125:tril", operator=True)


@functools.lru_cache(maxsize=2)
def _delaunay_tril(order):
    rows, cols, p, c, v = synth.delaunay_mesh(60000, 3, seed=3, order=order)
    return _tril(rows, p, c, v)


@pytest.mark.parametrize("order", ["rcm", "random"])
@pytest.mark.parametrize("upper", [False, True])
def test_delaunay_3dof_60k(order, upper):
    T = _delaunay_tril(order)
    if upper:
        T = _upper(*T)
    info = _check_both(*T, "delaunay 60k 3-dof %s%s" % (order, " upper" if upper else ""))
    if order == "random":
        assert info["spilled_entries"] > 0  # a randomly numbered mesh does not fit a few windows


def test_skew_symmetric_random():
    rows = 20000
    rng = np.random.default_rng(11)
    import scipy.sparse as sp
    R = sp.random(rows, rows, density=8.0 / rows, random_state=12, format="csr")
    R.data = rng.uniform(-1.0, 1.0, size=len(R.data))
    T = _csr(sp.tril(R, k=-1))
    assert capi.csr_triangle(*T[:3])[1] == 0
    _check_both(*T, "skew random", kind=capi.SKEW_SYMMETRIC)
    _check_both(*_upper(*T), "skew random, upper", kind=capi.SKEW_SYMMETRIC)


def test_empty_rows_diagonal_only_and_tiny():
    # rows without entries between full ones
    rows, cols, p, c, v = synth.poisson2d(64)
    T = _tril(rows, p, c, v)
    keep = np.ones(rows, dtype=bool)
    keep[::7] = False
    keep[100:400] = False
    import scipy.sparse as sp
    M = _sp(*T).tolil()
    for r in np.nonzero(~keep)[0]:
        M.rows[r] = []
        M.data[r] = []
    _check_both(*_csr(M.tocsr()), "empty rows")
    # diagonal only
    n = 5000
    d = np.random.default_rng(2).uniform(-1, 1, n)
    _check_both(n, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), d, "diagonal only")
    # one row, zero rows, a matrix without entries
    _check_both(1, np.array([0, 1], np.int32), np.array([0], np.int32), np.array([2.5]), "1 row")
    _check_both(0, np.array([0], np.int32), np.zeros(0, np.int32), np.zeros(0), "0 rows")
    _check_both(10, np.zeros(11, np.int32), np.zeros(0, np.int32), np.zeros(0), "no entries")


# ---- plans -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spec", ["queen", "delaunay"])
def test_forced_tiny_windows_spill_and_agree(spec):
    if spec == "queen":
        T = _load("synthetic:queen:30,24,20:tril")
    else:
        rows, cols, p, c, v = synth.delaunay_mesh(20000, 3, seed=4, order="rcm")
        T = _tril(rows, p, c, v)
    rows = T[0]
    x, y0 = _inputs(rows)
    want, scale = _expected(*T, x, y0, capi.SYMMETRIC)
    y_auto, info_auto = _level2(*T, x, y0)
    y_tiny, info_tiny = _level2(*T, x, y0, max_windows=1, window_doubles=64)
    helpers.assert_close(y_auto, want, scale, what=spec + " automatic windows")
    helpers.assert_close(y_tiny, want, scale, what=spec + " max_windows=1, window_doubles=64")
    helpers.assert_close(y_tiny, y_auto, scale, what=spec + " tiny against automatic")
    assert info_tiny["spilled_entries"] > info_auto["spilled_entries"]
    assert info_tiny["max_windows"] == 1 and info_tiny["rows_per_range"] == 64
    assert info_auto["windows"] > info_auto["ranges"]  # the automatic plan uses windows beside the own rows
    # two windows of 64 doubles: fewer spills than one, more than automatic
    y_two, info_two = _level2(*T, x, y0, max_windows=2, window_doubles=64)
    helpers.assert_close(y_two, want, scale, what=spec + " max_windows=2")
    assert info_two["spilled_entries"] <= info_tiny["spilled_entries"]


def test_plan_info_accounting():
    T = _load("synthetic:queen:30,24,20:tril")
    rows = T[0]
    x, y0 = _inputs(rows)
    _, info = _level2(*T, x, y0)
    assert info["rows"] == rows and info["ranges"] == -(-rows // info["rows_per_range"])
    assert info["atomic_bytes"] == 8 * (info["window_slots"] + info["spilled_entries"])
    assert 0 < info["lds_bytes"] <= 160 * 1024
    assert info["device_bytes"] > 0 and info["kind"] == capi.SYMMETRIC


def test_symv_refuses_x_equal_y():
    import torch
    T = _load("synthetic:queen:6,5,4:tril")
    rows, p, c, v = T
    dev = torch.device("cuda:0")
    tp, tc, tv = (torch.from_numpy(a).to(dev) for a in (p, c, v))
    tx = torch.ones(rows, dtype=torch.float64, device=dev)
    with capi.SymPlan(rows, p, tc.data_ptr()) as plan:
        with pytest.raises(capi.SpmvHipError) as e:
            plan.symv(tp.data_ptr(), tc.data_ptr(), tv.data_ptr(), tx.data_ptr(), tx.data_ptr())
        assert e.value.code == capi.ERR_INVALID


# ---- refusals --------------------------------------------------------------------------------------------------------------------

def test_refusals():
    rows, p, c, v = _load("synthetic:queen:6,5,4:tril")
    with capi.Context(num_gpus=1) as m:
        with pytest.raises(capi.SpmvHipError) as e:
            m.upload_csr_symmetric(rows, p, c, v)
        assert e.value.code == capi.ERR_STATE
    with capi.Context(0, capi.FLAG_EXACT_ORDER) as ctx:
        with pytest.raises(capi.SpmvHipError) as e:
            ctx.upload_csr_symmetric(rows, p, c, v)
        assert e.value.code == capi.ERR_INVALID
    full = _load("synthetic:queen:6,5,4")  # both triangles
    with capi.Context(0) as ctx:
        with pytest.raises(capi.SpmvHipError) as e:
            ctx.upload_csr_symmetric(*full)
        assert e.value.code == capi.ERR_INVALID and "both sides" in str(e.value)
        with pytest.raises(capi.SpmvHipError) as e:
            ctx.upload_csr_symmetric(rows, p, c, v, capi.SKEW_SYMMETRIC)  # it has a diagonal
        assert e.value.code == capi.ERR_INVALID
        # the context is usable afterwards
        ctx.upload_csr_symmetric(rows, p, c, v)
        x, y0 = _inputs(rows)
        ctx.set_x(x)
        ctx.set_y(y0)
        ctx.run(RUNS)
        want, scale = _expected(rows, p, c, v, x, y0, capi.SYMMETRIC)
        helpers.assert_close(ctx.get_y(), want, scale, what="after refusals")
        assert ctx.last_run_ns() > 0
    import torch
    tc = torch.from_numpy(full[2]).to("cuda:0")
    with pytest.raises(capi.SpmvHipError) as e:
        capi.SymPlan(full[0], full[1], tc.data_ptr())
    assert e.value.code == capi.ERR_INVALID


# ---- the host program ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("matrix", [BUS, "synthetic:queen:20,16,12:tril"])
def test_cli_symmetric_check(matrix):
    r = subprocess.run([CLI, "--csr", matrix, "--device", "hip", "--symmetric", "--threads", "1", "--profile", "4", "--check", "--x", "uniform"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    json.loads(r.stdout)  # one JSON document
    text = r.stdout
    assert '"hip-csr-spmv-symmetric"' in text
    assert '"pass": true' in text and "expanded" in text, text[-800:]
    assert '"symmetry": "symmetric"' in text and '"stored_triangle": "lower"' in text
