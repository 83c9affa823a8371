"""The C ABI of the scaled multiplies with dots (include/spmv_hip_dots.h) without a GPU: the eight functions are declared,
exported and bound, the header is C99 on its own, include/spmv_hip.h is still the 19-function boundary, and a null plan or context
is refused before any device is touched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from spmv_amd import capi

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
HEADER = os.path.join(INCLUDE, "spmv_hip_dots.h")
LEVEL2 = ["spmv_hip_csr_spmv_f32_scaled_dots", "spmv_hip_csr_spmv_c16_scaled_dots", "spmv_hip_csr_spmv_c16_f64_scaled_dots",
          "spmv_hip_csr_spmv_c16_f32xy_scaled_dots"]
WORKSPACE = ["spmv_hip_f32_dots_workspace", "spmv_hip_c16_dots_workspace"]
NEW = LEVEL2 + WORKSPACE + ["spmv_hip_run_scaled_dots", "spmv_hip_get_dots"]


def _code(path):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def test_symbols_exported_declared_and_bound():
    lib = C.CDLL(capi.LIB_PATH)
    text = _code(HEADER)
    declared = sorted(set(re.findall(r"\b(spmv_hip_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(NEW) and len(NEW) == 8
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in capi.SIGNATURES, s
    assert HEADER in [os.path.abspath(h) for h in capi.HEADER_PATHS]
    assert '#include "spmv_hip_scaled.h"' in open(HEADER).read()
    for m in ("spmv_scaled_dots", "dots_workspace_bytes"):
        assert hasattr(capi.F32Plan, m) and hasattr(capi.C16Plan, m), m
    for m in ("spmv_f64_scaled_dots", "spmv_f32xy_scaled_dots"):
        assert hasattr(capi.C16Plan, m), m
    assert hasattr(capi.Context, "run_scaled_dots") and hasattr(capi.Context, "get_dots")
    # the sibling's arguments up to d_y_out, then w, dots, the workspace and its size, the stream
    for s, plan, value, vec in (("f32", "f32", "float", "double"), ("c16", "c16", "float", "double"), ("c16_f64", "c16", "double", "double"),
                                ("c16_f32xy", "c16", "float", "float")):
        pattern = (r"int spmv_hip_csr_spmv_%s_scaled_dots\(const spmv_hip_%s_plan \*plan,[^;]*const %s \*d_value, const %s \*d_x, double alpha,\s*"
                   r"double beta,\s*const %s \*d_y_in,\s*%s \*d_y_out,\s*const %s \*d_w,\s*double \*d_dots,\s*void \*d_work,\s*size_t work_bytes,\s*"
                   r"void \*stream\);" % (s, plan, value, vec, vec, vec, vec))
        assert re.search(pattern, text), s
    assert re.search(r"int spmv_hip_run_scaled_dots\(spmv_hip_ctx \*ctx, double alpha, double beta\);", text)
    assert re.search(r"int spmv_hip_get_dots\(spmv_hip_ctx \*ctx, double dots\[2\]\);", text)
    for s in LEVEL2:
        args = capi.SIGNATURES[s][1]
        assert args[5:7] == [C.c_double, C.c_double] and len(args) == 14 and args[12] == C.c_size_t
    assert capi.SIGNATURES["spmv_hip_run_scaled_dots"][1][1:] == [C.c_double, C.c_double]


def test_header_is_c99_on_its_own_and_the_boundary_header_keeps_its_19_functions():
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INCLUDE, "-fsyntax-only", "-x", "c", "-"],
                       input='#include "spmv_hip_dots.h"\nint main(void) { return SPMV_HIP_VERSION; }\n',
                       text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout
    small = _code(capi.HEADER_PATH)
    assert len(set(re.findall(r"\b(spmv_hip_[a-z0-9_]+)\s*\(", small))) == 19
    assert "dots" not in small
    assert not re.findall(r"#define SPMV_HIP_VERSION", open(HEADER).read())
    assert capi.load().spmv_hip_version() == 130


def test_a_null_plan_or_context_fails_cleanly_without_a_device():
    lib = capi.load()
    v = np.ones(4)
    ptr = v.ctypes.data
    n = C.c_size_t(7)
    for s in WORKSPACE:
        assert getattr(lib, s)(None, C.byref(n)) == capi.ERR_INVALID, s
        assert b"plan is null" in lib.spmv_hip_last_error()
    assert n.value == 7
    for s in LEVEL2:
        fn = getattr(lib, s)
        assert fn(None, None, None, None, None, 1.0, 1.0, None, None, None, None, None, 0, None) == capi.ERR_INVALID, s
        assert b"plan is null" in lib.spmv_hip_last_error()
        assert fn(None, ptr, ptr, ptr, ptr, 0.0, 0.0, None, ptr, None, ptr, ptr, 64, None) == capi.ERR_INVALID, s
    assert np.all(v == 1.0)
    assert lib.spmv_hip_run_scaled_dots(None, 1.0, 1.0) == capi.ERR_INVALID
    assert b"ctx is null" in lib.spmv_hip_last_error()
    d = np.full(2, 5.0)
    assert lib.spmv_hip_get_dots(None, d.ctypes.data) == capi.ERR_INVALID
    assert np.all(d == 5.0)
