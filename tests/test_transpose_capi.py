"""The C ABI of the transposed multiply (include/spmv_hip_transpose.h) without a GPU: the symbols are exported and bound, the
header is plain C99 on its own, arguments are validated before any device is touched, and the plan's host part
(spmv_hip_tr_plan_preview) is recounted in numpy from the window table it returns."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from spmv_amd import capi, synth

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spmv_hip_transpose.h")
NEW = ["spmv_hip_upload_csr_transposed", "spmv_hip_tr_plan_preview", "spmv_hip_tr_plan_csr", "spmv_hip_csr_spmv_t",
       "spmv_hip_tr_plan_info", "spmv_hip_tr_plan_destroy"]
LDS_LIMIT = 80 * 1024


def _csr(rows, cols, entries):
    """CSR (row_ptr, column_index) of (i, j) pairs."""
    p = np.zeros(rows + 1, dtype=np.int32)
    entries = sorted(entries)
    for i, _ in entries:
        p[i + 1] += 1
    p = np.cumsum(p).astype(np.int32)
    c = np.array([j for _, j in entries], dtype=np.int32)
    return p, c


def _random(rows, cols, per_row, seed):
    import scipy.sparse as sp
    A = sp.random(rows, cols, density=per_row / cols, random_state=seed, format="csr")
    A.sort_indices()
    return A.indptr.astype(np.int32), A.indices.astype(np.int32)


def test_symbols_exported_declared_and_bound():
    lib = C.CDLL(capi.LIB_PATH)
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(spmv_hip_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(NEW)
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in capi.SIGNATURES, s
    assert HEADER in [os.path.abspath(h) for h in capi.HEADER_PATHS]
    assert hasattr(capi.Context, "upload_csr_transposed") and hasattr(capi, "TrPlan") and hasattr(capi, "tr_plan_preview")
    assert capi.load().spmv_hip_version() == 130  # callers detect the feature by the symbols


def test_header_is_c99_on_its_own_and_keeps_the_small_one_small():
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.dirname(HEADER), "-fsyntax-only", "-x", "c", "-"],
                       input='#include "spmv_hip_transpose.h"\nint main(void) { return SPMV_HIP_TR_MAX_WINDOWS + SPMV_HIP_TR_INFO; }\n',
                       text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout
    defines = dict(re.findall(r"#define (SPMV_HIP_[A-Z_]+) (\d+)", open(HEADER).read()))
    assert defines["SPMV_HIP_TR_MAX_WINDOWS"] == "8" and int(defines["SPMV_HIP_TR_INFO"]) == len(capi.TR_INFO_KEYS)
    small = re.sub(r"/\*.*?\*/", "", open(capi.HEADER_PATH).read(), flags=re.S)
    assert "transpos" not in small and "spmv_hip_tr_" not in small


def test_argument_validation_needs_no_device():
    lib = capi.load()
    p, c = _csr(3, 4, [(0, 0), (1, 3), (2, 2)])
    v = np.ones(3)
    h = C.c_void_p()
    out = np.zeros(14, dtype=np.int64)
    tab = np.zeros(64, dtype=np.int32)
    P, Cc, O, T = p.ctypes.data, c.ctypes.data, out.ctypes.data, tab.ctypes.data
    # null ctx / plan / out
    assert lib.spmv_hip_upload_csr_transposed(None, 3, 4, 3, P, Cc, v.ctypes.data) == capi.ERR_INVALID
    assert lib.spmv_hip_tr_plan_csr(None, 3, 4, P, None, 0, 0, None) == capi.ERR_INVALID
    assert lib.spmv_hip_csr_spmv_t(None, None, None, None, None, None, None) == capi.ERR_INVALID
    assert lib.spmv_hip_tr_plan_info(None, out, 14) == capi.ERR_INVALID
    lib.spmv_hip_tr_plan_destroy(None)  # a no-op
    assert lib.spmv_hip_tr_plan_preview(3, 4, P, Cc, 0, 0, None, 14, None, 0) == capi.ERR_INVALID
    assert lib.spmv_hip_tr_plan_preview(3, 4, None, Cc, 0, 0, O, 14, None, 0) == capi.ERR_INVALID
    assert lib.spmv_hip_tr_plan_preview(3, 4, P, None, 0, 0, O, 14, None, 0) == capi.ERR_INVALID
    assert b"column_index is null" in lib.spmv_hip_last_error()
    # negative sizes, a bad row_ptr, bad window arguments, a column outside [0, cols): preview and plan alike
    bad = np.array([0, 2, 1, 3], dtype=np.int32)  # decreasing
    for rows, cols, rp, mw, wd, text in [(-1, 4, P, 0, 0, b"rows < 0"), (3, -1, P, 0, 0, b"cols < 0"),
                                        (3, 4, bad.ctypes.data, 0, 0, b"non-decreasing"), (3, 4, P, -1, 0, b"max_windows"),
                                        (3, 4, P, 9, 0, b"max_windows"), (3, 4, P, 0, -1, b"window_doubles")]:
        assert lib.spmv_hip_tr_plan_preview(rows, cols, rp, Cc, mw, wd, O, 14, None, 0) == capi.ERR_INVALID
        assert text in lib.spmv_hip_last_error(), (text, lib.spmv_hip_last_error())
        assert lib.spmv_hip_tr_plan_csr(C.byref(h), rows, cols, rp, 0x1000, mw, wd, None) == capi.ERR_INVALID
        assert text in lib.spmv_hip_last_error(), (text, lib.spmv_hip_last_error())
    nonzero_start = np.array([1, 1, 2, 3], dtype=np.int32)
    assert lib.spmv_hip_tr_plan_preview(3, 4, nonzero_start.ctypes.data, Cc, 0, 0, O, 14, None, 0) == capi.ERR_INVALID
    for cols in (3, 2):  # column 3 is outside [0, 3)
        assert lib.spmv_hip_tr_plan_preview(3, cols, P, Cc, 0, 0, O, 14, None, 0) == capi.ERR_INVALID
        assert b"out of range" in lib.spmv_hip_last_error()
    neg = np.array([0, -1, 2], dtype=np.int32)
    assert lib.spmv_hip_tr_plan_preview(3, 4, P, neg.ctypes.data, 0, 0, O, 14, None, 0) == capi.ERR_INVALID
    assert lib.spmv_hip_tr_plan_csr(C.byref(h), 3, 4, P, None, 0, 0, None) == capi.ERR_INVALID  # entries but no columns
    assert not h.value
    # a window table with too little room
    assert lib.spmv_hip_tr_plan_preview(3, 4, P, Cc, 0, 0, O, 14, T, 1) == capi.ERR_INVALID
    assert lib.spmv_hip_tr_plan_preview(3, 4, P, Cc, 0, 0, O, 14, T, -1) == capi.ERR_INVALID
    assert lib.spmv_hip_tr_plan_preview(3, 4, P, Cc, 0, 0, O, 14, T, 64) == capi.OK


def test_no_gpu_means_failure_not_fallback():
    if capi.device_count() > 0:
        pytest.skip("a GPU is present; this test covers the no-device behaviour")
    p, c = _csr(3, 4, [(0, 0), (1, 3), (2, 2)])
    with pytest.raises(capi.SpmvHipError) as e:
        capi.TrPlan(3, 4, p, 0x1000)  # the columns cannot be read back without a device
    assert e.value.code == capi.ERR_NO_DEVICE
    with pytest.raises(capi.SpmvHipError) as e:
        capi.Context(0)  # Level 1 starts with a context: there is none to upload into
    assert e.value.code == capi.ERR_NO_DEVICE


# ---- the plan's host part against a numpy recount ---------------------------------------------------------------------------------

def _matrices():
    out = {}
    n = 3000
    ent = [(i, j) for i in range(n) for j in range(max(0, i - 3), min(n, i + 4))]
    out["banded"] = (n, n) + _csr(n, n, ent)
    rows, cols, p, c, _ = synth.poisson2d(64)
    out["poisson64"] = (rows, cols, np.asarray(p, dtype=np.int32), np.asarray(c, dtype=np.int32))
    out["wide_300x1000"] = (300, 1000) + _random(300, 1000, 12, 1)
    out["tall_1000x300"] = (1000, 300) + _random(1000, 300, 12, 2)
    # rows 10 .. 59 and every seventh row empty; columns 100 .. 399 and every fifth column never hit
    ent = [(i, j) for i in range(500) if i % 7 and not 10 <= i < 60 for j in ((i * 13) % 900, (i * 29 + 5) % 900, 899 - i)
           if j % 5 and not 100 <= j < 400]
    out["empty_rows_and_columns"] = (500, 900) + _csr(500, 900, sorted(set(ent)))
    out["no_entries"] = (40, 50, np.zeros(41, dtype=np.int32), np.zeros(0, dtype=np.int32))
    out["no_rows"] = (0, 50, np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32))
    out["no_cols"] = (40, 0, np.zeros(41, dtype=np.int32), np.zeros(0, dtype=np.int32))
    return out


MATRICES = _matrices()
SETTINGS = [(0, 0), (1, 32), (2, 64), (8, 0), (3, 100), (8, 32)]


def _recount(rows, cols, p, c, info, win):
    """Every claim of the preview that can be recounted from the window table."""
    nnz = int(p[rows])
    R, ranges, mw = info["rows_per_range"], info["ranges"], info["max_windows"]
    assert info["rows"] == rows and info["cols"] == cols and info["stored_entries"] == nnz
    assert ranges == (-(-rows // R) if rows and cols and nnz else 0)
    assert win.shape == (ranges, mw, 2)
    assert info["lds_bytes"] <= LDS_LIMIT
    assert info["streamed_bytes"] == 12 * nnz + 4 * (rows + 1) + 8 * rows
    assert info["device_bytes"] == 8 * ranges * mw
    spilled = used = slots = most = widest = 0
    for b in range(ranges):
        r0, r1 = b * R, min(rows, (b + 1) * R)
        cc = c[p[r0]:p[r1]].astype(np.int64)
        most = max(most, len(cc))
        covered = np.zeros(len(cc), dtype=np.int64)
        spans = []
        for first, length in win[b]:
            if length == 0:
                continue
            assert 0 <= first and first + length <= cols, (b, first, length)
            spans.append((int(first), int(first + length)))
            covered += (cc >= first) & (cc < first + length)
        spans.sort()
        for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
            assert a1 <= b0, "windows of range %d overlap: %r" % (b, spans)
        assert covered.max(initial=0) <= 1
        spilled += int((covered == 0).sum())
        used += len(spans)
        width = sum(e - s for s, e in spans)
        slots += width
        widest = max(widest, width)
    assert info["spilled_entries"] == spilled
    assert info["windows"] == used and info["window_slots"] == slots
    assert info["atomic_bytes"] == 8 * (slots + spilled)
    assert info["most_entries_in_a_range"] == most
    assert info["lds_bytes"] == (8 * widest + 4 * (R + 1) if ranges else 0)


@pytest.mark.parametrize("name", sorted(MATRICES))
@pytest.mark.parametrize("max_windows, window_doubles", SETTINGS)
def test_preview_against_a_recount(name, max_windows, window_doubles):
    rows, cols, p, c = MATRICES[name]
    info, win = capi.tr_plan_preview(rows, cols, p, c, max_windows, window_doubles)
    assert info["max_windows"] == (max_windows or 4)
    assert info["rows_per_range"] == (min(2048, window_doubles) if window_doubles else 2048)
    _recount(rows, cols, p, c, info, win)
    for first, length in win.reshape(-1, 2):
        if window_doubles:
            assert length <= window_doubles


@pytest.mark.parametrize("name", ["wide_300x1000", "tall_1000x300"])
def test_one_window_of_32_columns_spills_on_the_random_rectangles(name):
    """One window of 32 columns cannot cover 300 or 1000 random ones: the spill path is planned, not silently avoided."""
    rows, cols, p, c = MATRICES[name]
    info, win = capi.tr_plan_preview(rows, cols, p, c, 1, 32)
    assert info["spilled_entries"] > 0
    assert info["windows"] <= info["ranges"]
    _recount(rows, cols, p, c, info, win)


def test_automatic_windows_cover_a_mesh_and_an_empty_matrix_is_a_no_op():
    rows, cols, p, c = MATRICES["poisson64"]
    info, _ = capi.tr_plan_preview(rows, cols, p, c)
    assert info["spilled_entries"] == 0 and info["ranges"] == 2
    for name in ("no_entries", "no_rows", "no_cols"):
        info, win = capi.tr_plan_preview(*MATRICES[name])
        assert info["ranges"] == 0 and info["spilled_entries"] == 0 and info["atomic_bytes"] == 0 and win.size == 0
