"""The C ABI of the scaled multiplies (include/spmv_hip_scaled.h) without a GPU: the five functions are declared, exported and
bound, the header is C99 on its own, include/spmv_hip.h is still the 19-function boundary, and the arguments that need no device
to be refused are refused."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from spmv_amd import capi

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
HEADER = os.path.join(INCLUDE, "spmv_hip_scaled.h")
LEVEL2 = ["spmv_hip_csr_spmv_f32_scaled", "spmv_hip_csr_spmv_c16_scaled", "spmv_hip_csr_spmv_c16_f64_scaled",
          "spmv_hip_csr_spmv_c16_f32xy_scaled"]
NEW = LEVEL2 + ["spmv_hip_run_scaled"]


def _code(path):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def test_symbols_exported_declared_and_bound():
    lib = C.CDLL(capi.LIB_PATH)
    text = _code(HEADER)
    declared = sorted(set(re.findall(r"\b(spmv_hip_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(NEW)
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in capi.SIGNATURES, s
    assert HEADER in [os.path.abspath(h) for h in capi.HEADER_PATHS]
    assert hasattr(capi.F32Plan, "spmv_scaled") and hasattr(capi.Context, "run_scaled")
    for m in ("spmv_scaled", "spmv_f64_scaled", "spmv_f32xy_scaled"):
        assert hasattr(capi.C16Plan, m), m
    # alpha and beta are doubles for every element type, between x and y_in; the plan types are the siblings'
    for s, plan, value, vec in (("f32", "f32", "float", "double"), ("c16", "c16", "float", "double"), ("c16_f64", "c16", "double", "double"),
                                ("c16_f32xy", "c16", "float", "float")):
        pattern = (r"int spmv_hip_csr_spmv_%s_scaled\(const spmv_hip_%s_plan \*plan,[^;]*const %s \*d_value, const %s \*d_x, double alpha, "
                   r"double beta,\s*const %s \*d_y_in,\s*%s \*d_y_out, void \*stream\);" % (s, plan, value, vec, vec, vec))
        assert re.search(pattern, text), s
    assert re.search(r"int spmv_hip_run_scaled\(spmv_hip_ctx \*ctx, double alpha, double beta\);", text)
    for s in LEVEL2:
        assert capi.SIGNATURES[s][1][5:7] == [C.c_double, C.c_double] and len(capi.SIGNATURES[s][1]) == 10
    assert capi.SIGNATURES["spmv_hip_run_scaled"][1][1:] == [C.c_double, C.c_double]


def test_header_is_c99_on_its_own_and_the_boundary_header_keeps_its_19_functions():
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INCLUDE, "-fsyntax-only", "-x", "c", "-"],
                       input='#include "spmv_hip_scaled.h"\nint main(void) { return SPMV_HIP_VERSION; }\n',
                       text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout
    small = _code(capi.HEADER_PATH)
    assert len(set(re.findall(r"\b(spmv_hip_[a-z0-9_]+)\s*\(", small))) == 19
    assert "scaled" not in small and "alpha" not in small
    assert not re.findall(r"#define SPMV_HIP_VERSION", open(HEADER).read())
    assert capi.load().spmv_hip_version() == 130


def test_argument_validation_needs_no_device():
    lib = capi.load()
    v = np.ones(4)
    ptr = v.ctypes.data
    for s in LEVEL2:
        fn = getattr(lib, s)
        assert fn(None, None, None, None, None, 1.0, 1.0, None, None, None) == capi.ERR_INVALID, s
        assert b"plan is null" in lib.spmv_hip_last_error()
        assert fn(None, ptr, ptr, ptr, ptr, 0.0, 0.0, None, ptr, None) == capi.ERR_INVALID, s  # a null plan also where nothing would be read
    assert lib.spmv_hip_run_scaled(None, 1.0, 1.0) == capi.ERR_INVALID
    assert b"ctx is null" in lib.spmv_hip_last_error()
