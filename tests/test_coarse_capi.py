"""The C ABI of the dense coarsest-level solve (include/spmv_hip_coarse.h) without a GPU: the six functions are declared, exported
and bound, the header is C99 on its own, spmv_hip_coarse_ld and the workspace rule are what the header says, and every refusal of
the header is given through capi with made-up addresses -- the refusals precede the first HIP call, so nothing is dereferenced
and no device is needed.  A workspace one byte too small is looked at with everything else valid, so such a call is shown to pass
every other check by being refused for that alone."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import coarse_cases as cc
from spmv_amd import capi

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
HEADER = os.path.join(INCLUDE, "spmv_hip_coarse.h")
NEW = ["spmv_hip_coarse_ld", "spmv_hip_coarse_workspace"] + ["spmv_hip_coarse_%s_%s" % (c, s) for c in ("setup", "apply") for s in ("f64", "f32")]
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
    for m in ("ld", "workspace_bytes", "setup", "apply"):
        assert callable(getattr(capi, "coarse_" + m)), m
    assert "#define SPMV_HIP_COARSE_MAX_N 2048" in text and capi.COARSE_MAX_N == cc.MAX_N == 2048


def test_header_is_c99_on_its_own_and_the_version_is_unchanged():
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INCLUDE, "-fsyntax-only", "-x", "c", "-"],
                       input='#include "spmv_hip_coarse.h"\nint main(void) { return SPMV_HIP_VERSION + SPMV_HIP_COARSE_MAX_N; }\n',
                       text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout
    assert not re.findall(r"#define SPMV_HIP_VERSION", open(HEADER).read())
    assert capi.load().spmv_hip_version() == 130


def test_ld_is_n_rounded_up_to_a_multiple_of_four():
    assert [capi.coarse_ld(n) for n in (-2 ** 31, -1, 0, 1, 2, 3, 4, 5, 225, 2047, 2048)] == [0, 0, 0, 4, 4, 4, 4, 8, 228, 2048, 2048]
    for n in range(0, 2049):
        assert capi.coarse_ld(n) == cc.ld_of(n)


def test_the_workspace_is_pinned_at_the_shipped_sizes():
    """[B | I] as n rows of 2 ld doubles and one column of ld doubles."""
    assert [capi.coarse_workspace_bytes(n) for n in (0, 1, 225, 2048)] == [16, 96, 822624, 67125248]
    for n in cc.SIZES + (2047,):
        b = capi.coarse_workspace_bytes(n)
        assert b == cc.workspace_of(n) and b >= 16 and b % 16 == 0
    for n in (-1, 2049, 2 ** 31 - 1):
        with pytest.raises(capi.SpmvHipError) as e:
            capi.coarse_workspace_bytes(n)
        assert e.value.code == INV
    assert capi.load().spmv_hip_coarse_workspace(4, None) == INV


# made-up addresses, 16-byte aligned and far apart (the workspace of 2048 rows is 64 MiB)
N = 225
A = {"inv": 0x10000000, "r": 0x20000000, "z": 0x30000000, "work": 0x50000000, "p": 0x60000000, "c": 0x70000000, "v": 0x80000000,
     "status": 0x90000000}


def _refused(code, fn, *args, **kw):
    with pytest.raises(capi.SpmvHipError) as e:
        fn(*args, **kw)
    assert e.value.code == code, (e.value, args, kw)
    assert capi.load().spmv_hip_last_error()


def _calls(dtype):
    base = dict(A, n=N, work_bytes=capi.coarse_workspace_bytes(N))

    def apply(**o):
        a = dict(base, **o)
        capi.coarse_apply(a["n"], a["inv"], a["r"], a["z"], dtype=dtype)

    def setup(**o):
        a = dict(base, **o)
        capi.coarse_setup(a["n"], a["p"], a["c"], a["v"], a["inv"], a["status"], a["work"], a["work_bytes"], dtype=dtype)

    return {"apply": apply, "setup": setup}


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_every_refusal_with_made_up_addresses(dtype):
    calls = _calls(dtype)
    es = np.dtype(dtype).itemsize
    vec, inv_bytes = N * es, N * cc.ld_of(N) * es
    required = {"apply": ("inv", "r", "z"), "setup": ("p", "c", "v", "inv", "status", "work")}
    written = {"apply": ("z",), "setup": ("inv", "status", "work")}
    sizes = {"inv": inv_bytes, "r": vec, "z": vec, "work": capi.coarse_workspace_bytes(N), "p": 4 * (N + 1), "c": 4, "v": 8, "status": 12}
    align = {"inv": 16, "r": 16, "z": 16, "work": 16, "p": 4, "c": 4, "v": 8, "status": 4}
    for name, call in calls.items():
        for n in (-1, -N, 2049, 2 ** 31 - 1):
            _refused(INV, call, n=n, work_bytes=2 ** 40)     # n < 0, n above SPMV_HIP_COARSE_MAX_N
        for p in required[name]:
            _refused(INV, call, **{p: None})                 # a null required pointer
            _refused(INV, call, n=0, **{p: None})            # ... also where n == 0
        for p in required[name]:
            _refused(ALI, call, **{p: A[p] + align[p] // 2})
        # a written array overlapping any other array of the call, from either end
        for wname in written[name]:
            for other in required[name]:
                if other == wname:
                    continue
                last = (sizes[wname] - 1) // align[other] * align[other]  # the last aligned address inside the written array
                _refused(INV, call, **{other: A[wname] + last})
                if sizes[other] > 16:
                    _refused(INV, call, **{wname: A[other] + (sizes[other] - 1) // 16 * 16})
        _refused(INV, call, **({"inv": A["p"]} if name == "setup" else {"z": A["r"]}))
    # the status is three ints: its third counts too
    _refused(INV, calls["setup"], c=A["status"] + 8)
    # the workspace's size, looked at last
    need = capi.coarse_workspace_bytes(N)
    _refused(INV, calls["setup"], work_bytes=0)
    with pytest.raises(capi.SpmvHipError, match="work_bytes"):
        calls["setup"](work_bytes=need - 1)
    for n in (0, 1, 2048):
        with pytest.raises(capi.SpmvHipError, match="work_bytes"):
            calls["setup"](n=n, work_bytes=capi.coarse_workspace_bytes(n) - 1)
    # n == 0 launches nothing in the apply: accepted without a device
    calls["apply"](n=0)
    with pytest.raises(TypeError):
        capi.coarse_apply(N, A["inv"], A["r"], A["z"])  # raw addresses need dtype=
