"""The C ABI of the compact multiply over float x and y (include/spmv_hip_compact_f32xy.h) without a GPU: the five functions are
declared, exported and bound, they refuse a null plan / context before any device is touched, the plan's info keeps its 20
numbers, and the bytes one multiply streams -- spmv_hip_c16_plan_info [19] - 8 * [0] - 4 * [1] -- are recounted from row_ptr, the
columns and the tile table: 6 per stored entry of a compact tile, 8 per stored entry of a wide one, 8 per row of y, 4 per
column of x."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import compact_cases as cc
from spmv_amd import capi

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
HEADER = os.path.join(INCLUDE, "spmv_hip_compact_f32xy.h")
NEW = ["spmv_hip_csr_spmv_c16_f32xy", "spmv_hip_upload_csr_compact_f32xy", "spmv_hip_set_x_f32", "spmv_hip_set_y_f32", "spmv_hip_get_y_f32"]


def test_symbols_exported_declared_and_bound():
    lib = C.CDLL(capi.LIB_PATH)
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(spmv_hip_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(NEW)
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in capi.SIGNATURES, s
    assert HEADER in [os.path.abspath(h) for h in capi.HEADER_PATHS]
    for method in ("upload_csr_compact_f32xy", "set_x_f32", "set_y_f32", "get_y_f32"):
        assert hasattr(capi.Context, method), method
    assert hasattr(capi.C16Plan, "spmv_f32xy")
    # float values AND float vectors, through the plan type of spmv_hip_compact.h
    assert re.search(r"spmv_hip_csr_spmv_c16_f32xy\(const spmv_hip_c16_plan \*plan,[^;]*const float \*d_value,\s*const float \*d_x,\s*float \*d_y,", text)
    assert '#include "spmv_hip_compact.h"' in text


def test_header_is_c99_on_its_own_and_the_info_keeps_its_size():
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INCLUDE, "-fsyntax-only", "-x", "c", "-"],
                       input='#include "spmv_hip_compact_f32xy.h"\nint main(void) { return SPMV_HIP_C16_INFO; }\n',
                       text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout
    defines = dict(re.findall(r"#define (SPMV_HIP_[A-Z0-9_]+) (\d+)", open(os.path.join(INCLUDE, "spmv_hip_compact.h")).read()))
    assert int(defines["SPMV_HIP_C16_INFO"]) == len(capi.C16_INFO_KEYS) == 20
    assert not re.findall(r"#define SPMV_HIP_C16_INFO", open(HEADER).read())


def test_argument_validation_needs_no_device():
    lib = capi.load()
    p = np.array([0, 1, 2, 3], dtype=np.int32)
    c = np.array([0, 3, 2], dtype=np.int32)
    v = np.ones(3)
    f = np.ones(4, dtype=np.float32)
    assert lib.spmv_hip_csr_spmv_c16_f32xy(None, None, None, None, None, None, None) == capi.ERR_INVALID
    assert b"plan is null" in lib.spmv_hip_last_error()
    assert lib.spmv_hip_csr_spmv_c16_f32xy(None, p.ctypes.data, c.ctypes.data, f.ctypes.data, f.ctypes.data, f.ctypes.data, None) == capi.ERR_INVALID
    assert lib.spmv_hip_upload_csr_compact_f32xy(None, 3, 4, 3, p.ctypes.data, c.ctypes.data, v.ctypes.data, 1) == capi.ERR_INVALID
    assert b"ctx is null" in lib.spmv_hip_last_error()
    for fn in (lib.spmv_hip_set_x_f32, lib.spmv_hip_set_y_f32, lib.spmv_hip_get_y_f32):
        assert fn(None, f.ctypes.data) == capi.ERR_INVALID
        assert b"null" in lib.spmv_hip_last_error()


@pytest.mark.parametrize("flags", [0, capi.FLAG_EXACT_ORDER])
@pytest.mark.parametrize("name", cc.NAMES)
def test_streamed_bytes_against_a_recount(name, flags):
    rows, cols, p, c, _ = cc.matrix(name)
    info, tab, _ = capi.c16_plan_preview(rows, cols, p, c, flags)
    nnz = len(c)
    assert info["stored_entries"] == nnz and info["rows"] == rows and info["cols"] == cols
    streamed = info["streamed_bytes"] - 8 * info["rows"] - 4 * info["cols"] if info["streamed_bytes"] else 0  # the documented formula
    if rows == 0 or cols == 0 or nnz == 0:
        assert info["tiles"] == 0 and streamed == 0
        return
    nt = info["tiles"]
    p64 = p.astype(np.int64)
    r0, k0, nr = (tab[:, i].astype(np.int64) for i in range(3))
    k1 = p64[r0 + nr]
    is_compact = tab[:, 4] > 0
    compact_entries = int((k1 - k0)[is_compact].sum())
    wide_entries = int((k1 - k0)[~is_compact].sum())
    assert compact_entries + wide_entries == nnz
    # row_ptr is read by every tile that is not a long row and not a stream tile of equally long rows (compact_cases.recount)
    lens = np.diff(p64)
    row_ptr_bytes = 0
    for w in range(nt):
        if nr[w] == 1 and k1[w] - (k0[w] & ~3) > cc.TILE:
            continue
        tl = lens[r0[w]:r0[w] + nr[w]]
        fast = k1[w] > k0[w] and ((k1[w] - 1) & ~3) + 4 <= nnz
        if not (fast and tl.min() == tl.max()):
            row_ptr_bytes += 4 * (int(nr[w]) + 1)
    # y is read and written as floats (8 per row), x is read once as floats (4 per column)
    assert streamed == 6 * compact_entries + 8 * wide_entries + row_ptr_bytes + 8 * rows + 4 * cols + 16 * (nt + 1) + 32 * nt
    assert streamed > 0
