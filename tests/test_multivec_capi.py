"""The C ABI of the multi-vector multiply (include/spmv_hip_multivec.h) without a GPU: the symbols are exported and bound, the
header is plain C99 on its own, arguments are refused with the right codes before any device is needed, and without a device
the compute entry points fail instead of running anything in their place."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from spmv_amd import capi

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spmv_hip_multivec.h")
NEW = ["spmv_hip_mv_plan_csr", "spmv_hip_csr_spmm", "spmv_hip_mv_plan_info", "spmv_hip_mv_plan_destroy",
       "spmv_hip_set_block_x", "spmv_hip_set_block_y", "spmv_hip_get_block_y", "spmv_hip_run_block"]
FAKE = 0x10000  # a 16-byte aligned address that is never dereferenced (every call below fails or returns before a launch)


def test_symbols_exported_declared_and_bound():
    lib = C.CDLL(capi.LIB_PATH)
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(spmv_hip_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(NEW)
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in capi.SIGNATURES, s
    assert HEADER in [os.path.abspath(h) for h in capi.HEADER_PATHS]
    for m in ("set_block_x", "set_block_y", "get_block_y", "run_block"):
        assert hasattr(capi.Context, m), m
    assert hasattr(capi, "MvPlan") and hasattr(capi.MvPlan, "spmm") and hasattr(capi.MvPlan, "info")


def test_header_is_c99_on_its_own():
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.dirname(HEADER), "-fsyntax-only", "-x", "c", "-"],
                       input='#include "spmv_hip_multivec.h"\nint main(void) { spmv_hip_mv_plan *p = 0; (void) p; return SPMV_HIP_MV_MAX_VECTORS; }\n',
                       text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout
    small = re.sub(r"/\*.*?\*/", "", open(capi.HEADER_PATH).read(), flags=re.S)
    assert "block" not in small and "spmm" not in small  # spmv_hip.h is not touched


def _empty_plan(k, rows=0, cols=4):
    """A plan of a matrix without rows: made on the host alone (nothing to copy to a device)."""
    lib = capi.load()
    h = C.c_void_p()
    p = np.zeros(rows + 1, dtype=np.int32)
    assert lib.spmv_hip_mv_plan_csr(C.byref(h), rows, cols, p.ctypes.data, k, 0, None) == capi.OK, lib.spmv_hip_last_error()
    return h


def test_plan_arguments_refused_before_any_device():
    lib = capi.load()
    h = C.c_void_p()
    p = np.array([0, 1, 2, 2], dtype=np.int32)
    for k in (0, 17, -1, 100):
        assert lib.spmv_hip_mv_plan_csr(C.byref(h), 3, 3, p.ctypes.data, k, 0, None) == capi.ERR_INVALID
        assert b"k must be" in lib.spmv_hip_last_error()
    for flags in (0x1, 0x4, 0x10, 0x80000, 0x2 | 0x8):
        assert lib.spmv_hip_mv_plan_csr(C.byref(h), 3, 3, p.ctypes.data, 4, flags, None) == capi.ERR_INVALID
        assert b"flags" in lib.spmv_hip_last_error()
    assert lib.spmv_hip_mv_plan_csr(None, 3, 3, p.ctypes.data, 4, 0, None) == capi.ERR_INVALID
    assert lib.spmv_hip_mv_plan_csr(C.byref(h), 3, 3, None, 4, 0, None) == capi.ERR_INVALID
    assert lib.spmv_hip_mv_plan_csr(C.byref(h), -1, 3, p.ctypes.data, 4, 0, None) == capi.ERR_INVALID
    bad = np.array([0, 2, 1, 3], dtype=np.int32)
    assert lib.spmv_hip_mv_plan_csr(C.byref(h), 3, 3, bad.ctypes.data, 4, 0, None) == capi.ERR_INVALID
    assert b"non-decreasing" in lib.spmv_hip_last_error()
    assert not h.value
    out = np.zeros(11, dtype=np.int64)
    assert lib.spmv_hip_mv_plan_info(None, out, 11) == capi.ERR_INVALID
    lib.spmv_hip_mv_plan_destroy(None)  # a no-op


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6, 7, 8, 9, 13, 16])
def test_empty_plan_reports_its_passes(k):
    lib = capi.load()
    h = _empty_plan(k)
    out = np.zeros(11, dtype=np.int64)
    assert lib.spmv_hip_mv_plan_info(h, out, 11) == capi.OK
    info = dict(zip(capi.MvPlan.INFO_KEYS, out.tolist()))
    assert info["k"] == k and info["rows"] == 0 and info["cols"] == 4 and info["tiles"] == 0 and info["long_rows"] == 0
    # k = 1, 2, 3, 4, 6 and 8 take one pass over the matrix
    assert (info["passes"] == 1) == (k in (1, 2, 3, 4, 6, 8))
    assert info["widest_pass"] == max(w for w in (8, 6, 4, 3, 2, 1) if w <= k)
    assert info["streamed_bytes"] == info["passes"] * 4 + 8 * k * 4
    lib.spmv_hip_mv_plan_destroy(h)


def test_spmm_arguments_refused_before_any_device():
    lib = capi.load()
    k = 3
    h = _empty_plan(k)
    assert lib.spmv_hip_csr_spmm(None, FAKE, FAKE, FAKE, FAKE, k, FAKE + 4096, k, None) == capi.ERR_INVALID
    for ldx, ldy in ((2, 3), (3, 2), (0, 3), (-5, 7)):
        assert lib.spmv_hip_csr_spmm(h, FAKE, FAKE, FAKE, FAKE, ldx, FAKE + 4096, ldy, None) == capi.ERR_INVALID
        assert b"ld" in lib.spmv_hip_last_error()
    assert lib.spmv_hip_csr_spmm(h, FAKE, FAKE, FAKE, FAKE, k, FAKE, k, None) == capi.ERR_INVALID  # X == Y
    assert b"different" in lib.spmv_hip_last_error()
    for i in range(5):
        args = [FAKE, FAKE, FAKE, FAKE, FAKE + 4096]
        args[i] = None
        assert lib.spmv_hip_csr_spmm(h, args[0], args[1], args[2], args[3], k, args[4], k, None) == capi.ERR_INVALID
    assert lib.spmv_hip_csr_spmm(h, FAKE, FAKE + 4, FAKE, FAKE, k, FAKE + 4096, k, None) == capi.ERR_ALIGN
    assert lib.spmv_hip_csr_spmm(h, FAKE, FAKE, FAKE, FAKE + 4, k, FAKE + 4096, k, None) == capi.ERR_ALIGN
    # a column slice of a wider tensor: 8-byte aligned X and Y, odd leading dimensions
    assert lib.spmv_hip_csr_spmm(h, FAKE, FAKE, FAKE, FAKE + 8, 5, FAKE + 4104, 7, None) == capi.OK
    lib.spmv_hip_mv_plan_destroy(h)


def test_level1_arguments_refused_before_any_device():
    lib = capi.load()
    X = np.zeros(16)
    for k in (0, 17):
        assert lib.spmv_hip_set_block_x(None, k, X.ctypes.data) == capi.ERR_INVALID
    for fn in (lib.spmv_hip_set_block_x, lib.spmv_hip_set_block_y, lib.spmv_hip_get_block_y):
        assert fn(None, 2, X.ctypes.data) == capi.ERR_INVALID
    assert lib.spmv_hip_run_block(None) == capi.ERR_INVALID


def test_no_gpu_means_failure_not_fallback():
    if capi.device_count() > 0:
        pytest.skip("a GPU is present; this test covers the no-device behaviour")
    p = np.array([0, 1, 2, 3], dtype=np.int32)
    with pytest.raises(capi.SpmvHipError):
        capi.MvPlan(3, 3, p, 4)  # the tile list cannot be copied to a device
    with pytest.raises(capi.SpmvHipError) as e:
        capi.Context(0)
    assert e.value.code == capi.ERR_NO_DEVICE
