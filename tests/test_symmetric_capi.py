"""The C ABI of the symmetric multiply (include/spmv_hip_symmetric.h) without a GPU: the symbols are exported and bound, the
triangle of a CSR matrix is classified on the host, arguments are validated before any device is touched, and the header is
plain C99 on its own."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from spmv_amd import capi

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spmv_hip_symmetric.h")
NEW = ["spmv_hip_csr_triangle", "spmv_hip_upload_csr_symmetric", "spmv_hip_sym_plan_csr", "spmv_hip_csr_symv",
       "spmv_hip_sym_plan_info", "spmv_hip_sym_plan_destroy"]


def _csr(rows, entries):
    """CSR of (i, j) pairs, values 1."""
    p = np.zeros(rows + 1, dtype=np.int32)
    entries = sorted(entries)
    for i, _ in entries:
        p[i + 1] += 1
    p = np.cumsum(p).astype(np.int32)
    c = np.array([j for _, j in entries], dtype=np.int32)
    return p, c


def test_symbols_exported_declared_and_bound():
    lib = C.CDLL(capi.LIB_PATH)
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(spmv_hip_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(NEW)
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in capi.SIGNATURES, s
    assert HEADER in [os.path.abspath(h) for h in capi.HEADER_PATHS]
    assert hasattr(capi.Context, "upload_csr_symmetric") and hasattr(capi, "SymPlan")


def test_header_is_c99_on_its_own_and_keeps_the_small_one_small():
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.dirname(HEADER), "-fsyntax-only", "-x", "c", "-"],
                       input='#include "spmv_hip_symmetric.h"\nint main(void) { return SPMV_HIP_SYMMETRIC + SPMV_HIP_SKEW_SYMMETRIC; }\n',
                       text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout
    defines = dict(re.findall(r"#define (SPMV_HIP_[A-Z_]+) (\d+)", open(HEADER).read()))
    assert defines["SPMV_HIP_SYMMETRIC"] == "1" and defines["SPMV_HIP_SKEW_SYMMETRIC"] == "2"
    small = open(capi.HEADER_PATH).read()
    assert "symmetric" not in re.sub(r"/\*.*?\*/", "", small, flags=re.S)


@pytest.mark.parametrize("case, want, diag", [
    ("lower", capi.TRIANGLE_LOWER, 3),
    ("upper", capi.TRIANGLE_UPPER, 3),
    ("diagonal", capi.TRIANGLE_DIAGONAL, 4),
    ("mixed", capi.TRIANGLE_MIXED, 2),
    ("strict_lower", capi.TRIANGLE_LOWER, 0),
    ("empty", capi.TRIANGLE_DIAGONAL, 0),
    ("no_rows", capi.TRIANGLE_DIAGONAL, 0),
])
def test_triangle_classification(case, want, diag):
    entries = {
        "lower": [(0, 0), (1, 0), (1, 1), (3, 1), (3, 3)],
        "upper": [(0, 0), (0, 1), (1, 1), (1, 3), (3, 3)],
        "diagonal": [(0, 0), (1, 1), (2, 2), (3, 3)],
        "mixed": [(0, 0), (0, 2), (2, 1), (3, 3)],
        "strict_lower": [(1, 0), (2, 0), (3, 2)],
        "empty": [],
        "no_rows": [],
    }[case]
    rows = 0 if case == "no_rows" else 4
    p, c = _csr(rows, entries)
    assert capi.csr_triangle(rows, p, c) == (want, diag)


def test_triangle_of_a_real_file_and_its_transpose():
    from spmv_amd import hostapi
    A = hostapi.load(os.path.join(os.path.dirname(HEADER), "..", "tests", "golden", "bus1138_like.mtx"), "csr")
    p, c = np.array(A.row_ptr), np.array(A.column_index)
    rows = A.rows
    A.close()
    t, d = capi.csr_triangle(rows, p, c)
    assert t == capi.TRIANGLE_LOWER and 0 < d <= rows
    r = np.repeat(np.arange(rows), np.diff(p))
    order = np.lexsort((r, c))  # the transpose: rows become columns
    pt = np.zeros(rows + 1, dtype=np.int32)
    np.cumsum(np.bincount(c, minlength=rows), out=pt[1:])
    assert capi.csr_triangle(rows, pt, r[order].astype(np.int32)) == (capi.TRIANGLE_UPPER, d)


def test_triangle_validation():
    lib = capi.load()
    t, d = C.c_int(-7), C.c_int64(-7)
    p, c = _csr(3, [(0, 0), (1, 0), (2, 2)])
    assert lib.spmv_hip_csr_triangle(3, p.ctypes.data, c.ctypes.data, None, C.byref(d)) == capi.ERR_INVALID
    assert lib.spmv_hip_csr_triangle(3, None, c.ctypes.data, C.byref(t), C.byref(d)) == capi.ERR_INVALID
    assert lib.spmv_hip_csr_triangle(-1, p.ctypes.data, c.ctypes.data, C.byref(t), C.byref(d)) == capi.ERR_INVALID
    bad = np.array([0, 2, 1, 3], dtype=np.int32)  # decreasing
    assert lib.spmv_hip_csr_triangle(3, bad.ctypes.data, c.ctypes.data, C.byref(t), C.byref(d)) == capi.ERR_INVALID
    assert b"non-decreasing" in lib.spmv_hip_last_error()
    out_of_range = np.array([0, 3, 2], dtype=np.int32)
    assert lib.spmv_hip_csr_triangle(3, p.ctypes.data, out_of_range.ctypes.data, C.byref(t), C.byref(d)) == capi.ERR_INVALID
    assert b"out of range" in lib.spmv_hip_last_error()
    with pytest.raises(capi.SpmvHipError):
        capi.csr_triangle(3, p, np.array([0, -1, 2], dtype=np.int32))


def test_argument_validation_needs_no_device():
    lib = capi.load()
    p, c = _csr(3, [(0, 0), (1, 0), (2, 2)])
    v = np.ones(3)
    h = C.c_void_p()
    # null ctx / plan
    assert lib.spmv_hip_upload_csr_symmetric(None, 3, 3, p.ctypes.data, c.ctypes.data, v.ctypes.data, capi.SYMMETRIC) == capi.ERR_INVALID
    assert lib.spmv_hip_sym_plan_csr(None, 3, p.ctypes.data, None, capi.SYMMETRIC, 0, 0, None) == capi.ERR_INVALID
    assert lib.spmv_hip_csr_symv(None, None, None, None, None, None, None) == capi.ERR_INVALID
    out = np.zeros(16, dtype=np.int64)
    assert lib.spmv_hip_sym_plan_info(None, out, 16) == capi.ERR_INVALID
    lib.spmv_hip_sym_plan_destroy(None)  # a no-op
    # a decreasing row_ptr, a bad kind, bad window arguments: refused before anything is read from a device
    bad = np.array([0, 2, 1, 3], dtype=np.int32)
    assert lib.spmv_hip_sym_plan_csr(C.byref(h), 3, bad.ctypes.data, None, capi.SYMMETRIC, 0, 0, None) == capi.ERR_INVALID
    assert b"non-decreasing" in lib.spmv_hip_last_error()
    for kind in (0, 3, -1):
        assert lib.spmv_hip_sym_plan_csr(C.byref(h), 3, p.ctypes.data, None, kind, 0, 0, None) == capi.ERR_INVALID
        assert b"kind" in lib.spmv_hip_last_error()
    assert lib.spmv_hip_sym_plan_csr(C.byref(h), -1, p.ctypes.data, None, capi.SYMMETRIC, 0, 0, None) == capi.ERR_INVALID
    assert lib.spmv_hip_sym_plan_csr(C.byref(h), 3, p.ctypes.data, None, capi.SYMMETRIC, 0, 0, None) == capi.ERR_INVALID  # no columns
    assert not h.value


def test_no_gpu_means_failure_not_fallback():
    if capi.device_count() > 0:
        pytest.skip("a GPU is present; this test covers the no-device behaviour")
    p, c = _csr(3, [(0, 0), (1, 0), (2, 2)])
    with pytest.raises(capi.SpmvHipError):
        capi.SymPlan(3, p, 0x1000)  # the columns cannot be read back without a device
