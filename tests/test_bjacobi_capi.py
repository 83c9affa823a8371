"""The C ABI of the point-block Jacobi preconditioner (include/spmv_hip_bjacobi.h) without a GPU: the six functions are declared,
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
HEADER = os.path.join(INCLUDE, "spmv_hip_bjacobi.h")
NEW = ["spmv_hip_bjacobi_%s_%s" % (c, s) for c in ("setup", "apply", "apply_add") for s in ("f64", "f32")]
INV, ALI = capi.ERR_INVALID, capi.ERR_ALIGN
DTYPES = [np.float64, np.float32]


def test_symbols_exported_declared_and_bound():
    lib = C.CDLL(capi.LIB_PATH)
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(spmv_hip_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(NEW) and len(NEW) == 6
    for s in NEW:
        assert hasattr(lib, s) and s in capi.SIGNATURES, s
    assert HEADER in [os.path.abspath(h) for h in capi.HEADER_PATHS]
    for m in ("setup", "apply", "apply_add"):
        assert callable(getattr(capi, "bjacobi_" + m)), m
    assert '#include "spmv_hip_krylov.h"' in text and "#define SPMV_HIP_BJACOBI_MAX_BLOCK 8" in text and capi.BJACOBI_MAX_BLOCK == 8


def test_header_is_c99_on_its_own_and_the_version_is_unchanged():
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INCLUDE, "-fsyntax-only", "-x", "c", "-"],
                       input='#include "spmv_hip_bjacobi.h"\nint main(void) { return SPMV_HIP_VERSION + SPMV_HIP_BJACOBI_MAX_BLOCK; }\n',
                       text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout
    assert not re.findall(r"#define SPMV_HIP_VERSION", open(HEADER).read())
    assert capi.load().spmv_hip_version() == 130


# made-up addresses, 16-byte aligned and far apart
N, B = 6030, 3
A = {"inv": 0x10000000, "r": 0x20000000, "z": 0x30000000, "dots": 0x40000000, "work": 0x50000000, "p": 0x60000000, "c": 0x70000000,
     "v": 0x80000000, "status": 0x90000000}


def _refused(code, fn, *args, **kw):
    with pytest.raises(capi.SpmvHipError) as e:
        fn(*args, **kw)
    assert e.value.code == code, (e.value, args, kw)
    assert capi.load().spmv_hip_last_error()


def _calls(dtype):
    base = dict(A, n=N, b=B, work_bytes=capi.krylov_workspace_bytes(N))

    def apply(**o):
        a = dict(base, **o)
        capi.bjacobi_apply(a["n"], a["b"], a["inv"], a["r"], a["z"], a["dots"], a["work"], a["work_bytes"], dtype=dtype)

    def apply_add(**o):
        a = dict(base, **o)
        capi.bjacobi_apply_add(a["n"], a["b"], a["inv"], a["r"], a["z"], dtype=dtype)

    def setup(**o):
        a = dict(base, **o)
        capi.bjacobi_setup(a["n"], a["b"], a["p"], a["c"], a["v"], a["inv"], a["status"], dtype=dtype)

    return {"apply": apply, "apply_add": apply_add, "setup": setup}


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_every_refusal_with_made_up_addresses(dtype):
    calls = _calls(dtype)
    es = np.dtype(dtype).itemsize
    vec, inv_bytes = N * es, N * B * es
    required = {"apply": ("inv", "r", "z"), "apply_add": ("inv", "r", "z"), "setup": ("p", "c", "v", "inv", "status")}
    written = {"apply": ("z", "dots", "work"), "apply_add": ("z",), "setup": ("inv", "status")}
    uses = {"apply": ("inv", "r", "z", "dots", "work"), "apply_add": ("inv", "r", "z"), "setup": ("p", "c", "v", "inv", "status")}
    sizes = {"inv": inv_bytes, "r": vec, "z": vec, "dots": 16, "work": capi.krylov_workspace_bytes(N), "p": 4 * (N + 1), "c": 4, "v": 8, "status": 8}
    align = {"inv": 16, "r": 16, "z": 16, "dots": 16, "work": 16, "p": 4, "c": 4, "v": 8, "status": 4}
    for name, call in calls.items():
        _refused(INV, call, n=-B)
        for b in (0, -1, 9, 64):
            _refused(INV, call, b=b)                     # b outside 1 ... 8
        for b in (4, 7, 8):
            _refused(INV, call, b=b)                     # 6030 is a multiple of 1, 2, 3, 5, 6 only
        for p in required[name]:
            _refused(INV, call, **{p: None})             # a null required pointer
            _refused(INV, call, n=0, **{p: None})        # ... also where n == 0
        for p in uses[name]:
            _refused(ALI, call, **{p: A[p] + align[p] // 2})
        big = 2 ** 32 // es                              # a vector of 4 GiB: a multiple of 1, 2, 4, 8 only
        _refused(INV, call, n=big, b=2, work_bytes=capi.krylov_workspace_bytes(big))
        with pytest.raises(capi.SpmvHipError, match="4 GiB"):
            call(n=big, b=2, work_bytes=capi.krylov_workspace_bytes(big))
        # a written array overlapping any other array of the call, from either end
        for wname in written[name]:
            for other in uses[name]:
                if other == wname:
                    continue
                _refused(INV, call, **{other: A[wname] + (sizes[wname] // 16) * 16 - (16 if sizes[wname] >= 16 else 0)})
                if sizes[other] > 16:
                    _refused(INV, call, **{wname: A[other] + (sizes[other] // 16) * 16 - 16})
        if name == "setup":
            _refused(INV, call, inv=A["p"])
        else:
            _refused(INV, call, z=A["r"])
    # the dots and the workspace: together or not at all, and the workspace's size last
    _refused(INV, calls["apply"], dots=None)
    _refused(INV, calls["apply"], work=None)
    need = capi.krylov_workspace_bytes(N)
    _refused(INV, calls["apply"], work_bytes=0)
    with pytest.raises(capi.SpmvHipError, match="work_bytes"):
        calls["apply"](work_bytes=need - 1)
    for b in (1, 2, 3, 5, 6):  # every valid b at this n passes every other check
        with pytest.raises(capi.SpmvHipError, match="work_bytes"):
            calls["apply"](b=b, work_bytes=need - 1)
    # the inverse may exceed 4 GiB: refused for the workspace alone
    n8 = 2 ** 26 + 8
    with pytest.raises(capi.SpmvHipError, match="work_bytes"):
        calls["apply"](n=n8, b=8, z=0x300000000, r=0x400000000, dots=0x500000000, work=0x600000000, work_bytes=15)
    _refused(INV, calls["apply"], n=n8, b=8, z=A["inv"] + n8 * 8 * es - 16, r=0x400000000, dots=0x500000000, work=0x600000000,
             work_bytes=capi.krylov_workspace_bytes(n8))  # z in the last bytes of such an inverse
    # n == 0 without dots launches nothing: accepted without a device
    calls["apply"](n=0, dots=None, work=None, work_bytes=0)
    calls["apply_add"](n=0)
    with pytest.raises(TypeError):
        capi.bjacobi_apply(N, B, A["inv"], A["r"], A["z"])  # raw addresses need dtype=
