"""The C ABI of the Chebyshev polynomial preconditioner (include/spmv_hip_cheby.h) without a GPU: the five functions are declared,
exported and bound, the header is C99 on its own, and every refusal of the header is given through capi with made-up addresses
-- the refusals precede the first HIP call, so nothing is dereferenced and no device is needed.  A workspace one byte too small
is looked at with everything else valid, so such a call is shown to pass every other check by being refused for that alone."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from spmv_amd import capi

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
HEADER = os.path.join(INCLUDE, "spmv_hip_cheby.h")
NEW = ["spmv_hip_cheby_bound_f64", "spmv_hip_cheby_bound_f32", "spmv_hip_cheby_coeffs", "spmv_hip_cheby_step_f64", "spmv_hip_cheby_step_f32"]
INV, ALI = capi.ERR_INVALID, capi.ERR_ALIGN
DTYPES = [np.float64, np.float32]


def test_symbols_exported_declared_and_bound():
    lib = C.CDLL(capi.LIB_PATH)
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(spmv_hip_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(NEW) and len(NEW) == 5
    for s in NEW:
        assert hasattr(lib, s) and s in capi.SIGNATURES, s
    assert HEADER in [os.path.abspath(h) for h in capi.HEADER_PATHS]
    for m in ("bound", "coeffs", "step"):
        assert callable(getattr(capi, "cheby_" + m)), m
    assert '#include "spmv_hip_krylov.h"' in text and "#define SPMV_HIP_CHEBY_MAX_DEGREE 16" in text and capi.CHEBY_MAX_DEGREE == 16


def test_header_is_c99_on_its_own_and_the_version_is_unchanged():
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INCLUDE, "-fsyntax-only", "-x", "c", "-"],
                       input='#include "spmv_hip_cheby.h"\nint main(void) { return SPMV_HIP_VERSION + SPMV_HIP_CHEBY_MAX_DEGREE; }\n',
                       text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout
    assert not re.findall(r"#define SPMV_HIP_VERSION", open(HEADER).read())
    assert capi.load().spmv_hip_version() == 130


# made-up addresses, 16-byte aligned and far apart
N, DEGREE = 6030, 3
A = {"coef": 0x10000000, "u": 0x20000000, "minv": 0x30000000, "d": 0x40000000, "z": 0x50000000, "r": 0x60000000, "dots": 0x70000000,
     "work": 0x80000000, "p": 0x90000000, "v": 0xa0000000, "lam": 0xb0000000}


def _refused(code, fn, *args, **kw):
    with pytest.raises(capi.SpmvHipError) as e:
        fn(*args, **kw)
    assert e.value.code == code, (e.value, args, kw)
    assert capi.load().spmv_hip_last_error()


def _calls(dtype):
    base = dict(A, n=N, degree=DEGREE, j=DEGREE - 1, work_bytes=capi.krylov_workspace_bytes(N), scale=1.0, ratio=30.0)

    def step(**o):
        a = dict(base, **o)
        capi.cheby_step(a["n"], a["degree"], a["j"], a["coef"], a["u"], a["minv"], a["d"], a["z"], a["r"], a["dots"], a["work"], a["work_bytes"],
                        dtype=dtype)

    def bound(**o):
        a = dict(base, **o)
        capi.cheby_bound(a["n"], a["p"], a["v"], a["minv"], a["lam"], dtype=dtype)

    def coeffs(**o):
        a = dict(base, **o)
        capi.cheby_coeffs(a["degree"], a["lam"], a["scale"], a["ratio"], a["coef"])

    return {"step": step, "bound": bound, "coeffs": coeffs}


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_every_refusal_with_made_up_addresses(dtype):
    calls = _calls(dtype)
    step, bound, coeffs = calls["step"], calls["bound"], calls["coeffs"]
    es = np.dtype(dtype).itemsize
    vec, need = N * es, capi.krylov_workspace_bytes(N)
    sizes = {"coef": 16 * DEGREE, "u": vec, "minv": vec, "d": vec, "z": vec, "r": vec, "dots": 16, "work": need, "p": 4 * (N + 1), "v": 8, "lam": 8}
    align = {"coef": 8, "u": 16, "minv": 16, "d": 16, "z": 16, "r": 16, "dots": 16, "work": 16, "p": 4, "v": 8, "lam": 8}
    uses = {"step": ("coef", "u", "minv", "d", "z", "r", "dots", "work"), "bound": ("p", "v", "minv", "lam"), "coeffs": ("lam", "coef")}
    required = {"step": ("coef", "u", "d", "z"), "bound": ("p", "v", "lam"), "coeffs": ("lam", "coef")}
    nodots = dict(r=None, dots=None, work=None, work_bytes=0)
    # n, the degree and j
    _refused(INV, step, n=-1)
    _refused(INV, bound, n=-1)
    for degree in (0, -1, 17, 64):
        _refused(INV, step, degree=degree, j=0)
        _refused(INV, coeffs, degree=degree)
    for degree, j in ((3, -1), (3, 3), (1, 1), (16, 16)):
        _refused(INV, step, degree=degree, j=j, **nodots)
    # scale and ratio: finite, scale > 0, ratio > 1
    for scale in (0.0, -1.0, float("inf"), float("nan")):
        _refused(INV, coeffs, scale=scale)
    for ratio in (1.0, 0.5, -30.0, float("inf"), float("nan")):
        _refused(INV, coeffs, ratio=ratio)
    # a null required pointer, also where n == 0; alignment
    for name, call in calls.items():
        for p in required[name]:
            _refused(INV, call, **{p: None})
            _refused(INV, call, n=0, **{p: None})
        for p in uses[name]:
            _refused(ALI, call, **{p: A[p] + align[p] // 2})
    _refused(INV, step, j=0, d=None, **nodots)  # d is required wherever degree > 1
    # the dots: all three or none, and at the last step alone
    for missing in ("r", "dots", "work"):
        _refused(INV, step, **{missing: None})
        _refused(INV, step, **dict(nodots, **{missing: A[missing]}))
    for j in (0, 1):
        _refused(INV, step, j=j)
        with pytest.raises(capi.SpmvHipError, match="last step"):
            step(j=j)
    # 4 GiB
    big = 2 ** 32 // es
    _refused(INV, step, n=big, work_bytes=capi.krylov_workspace_bytes(big))
    with pytest.raises(capi.SpmvHipError, match="4 GiB"):
        step(n=big, work_bytes=capi.krylov_workspace_bytes(big))
    with pytest.raises(capi.SpmvHipError, match="4 GiB"):
        bound(n=big)
    # a written array overlapping any other array of the call, from either end
    written = {("step", 2): ("z", "dots", "work"), ("step", 1): ("d", "z"), ("step", 0): ("d", "z"), ("bound", 2): ("lam",), ("coeffs", 2): ("coef",)}
    for (name, j), ws in written.items():
        over = {} if j == DEGREE - 1 else dict(nodots, j=j)
        call = calls[name]
        for wname in ws:
            for other in uses[name]:
                if other == wname or (over and other in nodots):
                    continue
                _refused(INV, call, **dict(over, **{other: A[wname] + (sizes[wname] // 16) * 16 - (16 if sizes[wname] >= 16 else 0)}))
                if sizes[other] > 16:
                    _refused(INV, call, **dict(over, **{wname: A[other] + (sizes[other] // 16) * 16 - 16}))
    _refused(INV, step, z=A["u"])
    _refused(INV, step, j=1, d=A["u"], **nodots)
    _refused(INV, step, coef=A["z"] + 64)                      # the table inside a written array
    _refused(INV, step, coef=A["work"] + 16)
    _refused(INV, step, j=0, coef=A["d"] + vec - 16 * DEGREE - (vec % 8), **nodots)
    _refused(INV, coeffs, lam=A["coef"] + 16 * DEGREE - 8)     # lambda in the table's last double
    # the workspace's size last: refused for that alone
    _refused(INV, step, work_bytes=0)
    for degree in (1, 2, 16):
        with pytest.raises(capi.SpmvHipError, match="work_bytes"):
            step(degree=degree, j=degree - 1, coef=0x10000000, work_bytes=need - 1)
    with pytest.raises(capi.SpmvHipError, match="work_bytes"):
        step(r=A["u"], work_bytes=need - 1)                    # d_u == d_r is valid: both are only read
    with pytest.raises(capi.SpmvHipError, match="work_bytes"):
        step(d=A["u"], work_bytes=need - 1)                    # the last step only reads d: it may be u
    with pytest.raises(capi.SpmvHipError, match="work_bytes"):
        step(minv=None, work_bytes=need - 1)
    with pytest.raises(capi.SpmvHipError, match="work_bytes"):
        step(degree=1, j=0, d=None, work_bytes=need - 1)       # at degree 1 d may be null ...
    with pytest.raises(capi.SpmvHipError, match="work_bytes"):
        step(degree=1, j=0, d=A["z"] + 8, work_bytes=need - 1)  # ... and is not looked at
    # n == 0 without dots launches nothing: accepted without a device
    step(n=0, **nodots)
    step(n=0, j=0, **nodots)
    step(n=0, degree=1, j=0, d=None, minv=None, **nodots)
    with pytest.raises(TypeError):
        capi.cheby_step(N, DEGREE, 0, A["coef"], A["u"], None, A["d"], A["z"])  # raw addresses need dtype=
