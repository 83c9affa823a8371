"""The C ABI of the GMRES updates (include/spmv_hip_gmres.h) without a GPU: the thirteen functions are declared, exported and bound,
the header is C99 on its own, and every refusal of the header is given through capi with made-up addresses -- the refusals
precede the first HIP call, so nothing is dereferenced and no device is needed.  A workspace one byte too small is looked at
last: such a call has passed every other check, so the placements the header accepts (w right behind the basis, d_scale inside
the state) are shown to pass by being refused for that alone.  The workspace and state-size rules."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import gmres_cases as gc
from spmv_amd import capi

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
HEADER = os.path.join(INCLUDE, "spmv_hip_gmres.h")
TYPED = ["spmv_hip_gmres_%s_%s" % (c, s) for c in ("project", "update", "scale", "correct") for s in ("f64", "f32")]
NEW = TYPED + ["spmv_hip_gmres_" + c for c in ("workspace", "state_doubles", "start", "column", "solve")]
INV, ALI = capi.ERR_INVALID, capi.ERR_ALIGN
DTYPES = [np.float64, np.float32]


def test_symbols_exported_declared_and_bound():
    lib = C.CDLL(capi.LIB_PATH)
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(spmv_hip_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(NEW) and len(NEW) == 13
    for s in NEW:
        assert hasattr(lib, s) and s in capi.SIGNATURES, s
    assert HEADER in [os.path.abspath(h) for h in capi.HEADER_PATHS]
    for m in ("project", "update", "scale", "correct", "start", "column", "solve", "workspace_bytes", "state_doubles"):
        assert callable(getattr(capi, "gmres_" + m)), m
    assert '#include "spmv_hip_krylov.h"' in text and "#define SPMV_HIP_GMRES_MAX_BASIS 32" in text and capi.GMRES_MAX_BASIS == 32
    assert "SPMV_HIP_KRYLOV_CHUNK (1024)" in open(HEADER).read()


def test_header_is_c99_on_its_own_and_the_version_is_unchanged():
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INCLUDE, "-fsyntax-only", "-x", "c", "-"],
                       input='#include "spmv_hip_gmres.h"\nint main(void) { return SPMV_HIP_VERSION + SPMV_HIP_GMRES_MAX_BASIS; }\n',
                       text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout
    assert not re.findall(r"#define SPMV_HIP_VERSION", open(HEADER).read())
    assert capi.load().spmv_hip_version() == 130


def test_workspace_and_state_rules():
    sizes = sorted(set(gc.SIZES + gc.BIG_SIZES + [2 ** 22, 2 ** 31 - 1]))
    table = [[capi.gmres_workspace_bytes(n, k) for k in range(33)] for n in sizes]
    for row, n in zip(table, sizes):
        assert all(b >= 16 and b % 16 == 0 for b in row)
        assert all(a <= b for a, b in zip(row, row[1:])), "decreasing in k_max at n %d" % n
        assert row[0] >= capi.krylov_workspace_bytes(n)  # the update's slots are a step's
        assert row[32] == 17 * capi.krylov_workspace_bytes(n)  # a pair of sums per 16-byte slot
    for lo, hi in zip(table, table[1:]):
        assert all(a <= b for a, b in zip(lo, hi)), "decreasing in n"
    assert [capi.gmres_workspace_bytes(n, 5) for n in sizes] == [capi.gmres_workspace_bytes(n, 5) for n in sizes]
    for bad in ((-1, 0), (0, -1), (0, 33)):
        with pytest.raises(capi.SpmvHipError) as e:
            capi.gmres_workspace_bytes(*bad)
        assert e.value.code == INV
    assert capi.load().spmv_hip_gmres_workspace(8, 8, None) == INV
    counts = [capi.gmres_state_doubles(m) for m in range(1, 33)]
    assert counts == [gc.state_doubles(m) for m in range(1, 33)]
    assert all(c % 2 == 0 for c in counts) and all(a < b for a, b in zip(counts, counts[1:]))
    for m, c in zip(range(1, 33), counts):
        lay = capi.gmres_state_layout(m)
        assert (lay["g"], lay["c"] - lay["g"], lay["s"] - lay["c"], lay["r"] - lay["s"]) == (2, m + 1, m, m)
        assert lay["r"] + m * (m + 1) // 2 <= c
    for m in (0, -1, 33):
        with pytest.raises(capi.SpmvHipError) as e:
            capi.gmres_state_doubles(m)
        assert e.value.code == INV


# made-up addresses, 16-byte aligned and far apart
N, K = 5000, 5
A = {"V": 0x10000000, "w": 0x20000000, "h": 0x30000000, "work": 0x40000000, "dots": 0x50000000, "scale": 0x60000000, "v": 0x70000000,
     "minv": 0x80000000, "vhat": 0x90000000, "y": 0xa0000000, "x": 0xb0000000, "state": 0xc0000000, "nrm2": 0xd0000000, "h1": 0xe0000000,
     "h2": 0xe8000000}


def _refused(code, fn, *args, **kw):
    with pytest.raises(capi.SpmvHipError) as e:
        fn(*args, **kw)
    assert e.value.code == code, (e.value, args)
    assert capi.load().spmv_hip_last_error()


def _calls(dtype):
    """{name: function of overrides} for the four streaming calls with valid made-up arguments."""
    es = np.dtype(dtype).itemsize
    ldv = gc.ldv_of(N, dtype)
    base = dict(A, n=N, k=K, ldv=ldv, work_bytes=capi.gmres_workspace_bytes(N, K))

    def project(**o):
        a = dict(base, **o)
        capi.gmres_project(a["n"], a["k"], a["V"], a["ldv"], a["w"], a["h"], a["work"], a["work_bytes"], dtype=dtype)

    def update(**o):
        a = dict(base, **o)
        capi.gmres_update(a["n"], a["k"], a["V"], a["ldv"], a["h"], a["w"], a["dots"], a["work"], a["work_bytes"], dtype=dtype)

    def scale(**o):
        a = dict(base, **o)
        capi.gmres_scale(a["n"], a["scale"], a["v"], a["minv"], a["vhat"], dtype=dtype)

    def correct(**o):
        a = dict(base, **o)
        capi.gmres_correct(a["n"], a["k"], a["V"], a["ldv"], a["y"], a["minv"], a["x"], dtype=dtype)

    return {"project": project, "update": update, "scale": scale, "correct": correct}, es, ldv


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_refusals_of_the_streaming_calls(dtype):
    calls, es, ldv = _calls(dtype)
    vec, basis = N * es, ((K - 1) * ldv + N) * es
    required = {"project": ("V", "w", "h", "work"), "update": ("V", "h", "w", "dots", "work"), "scale": ("scale", "v"), "correct": ("V", "y", "x")}
    written = {"project": ("h", "work"), "update": ("w", "dots", "work"), "scale": ("v", "vhat"), "correct": ("x",)}
    sizes = {"V": basis, "w": vec, "v": vec, "minv": vec, "vhat": vec, "x": vec, "h": 8 * K, "y": 8 * K, "dots": 16, "scale": 8,
             "work": capi.gmres_workspace_bytes(N, K)}
    uses = {"project": ("V", "w", "h", "work"), "update": ("V", "h", "w", "dots", "work"), "scale": ("scale", "v", "minv", "vhat"),
            "correct": ("V", "y", "minv", "x")}
    for name, call in calls.items():
        _refused(INV, call, n=-1)
        for p in required[name]:
            _refused(INV, call, **{p: None})            # a null required pointer
            _refused(INV, call, n=0, **{p: None})       # ... also where n == 0
            if p != "scale":
                _refused(ALI, call, **{p: A[p] + 8})    # off 16 bytes (the scalar: below)
        if name != "scale":
            for k in (-1, 33):
                _refused(INV, call, k=k)
            _refused(INV, call, ldv=ldv + 1)            # ldv sizeof(T) no multiple of 16
            _refused(INV, call, n=N, ldv=N - 16 // es)  # ldv < n
        # one vector of 4 GiB or more
        big = 2 ** 32 // es
        _refused(INV, call, n=big, ldv=big + 16 // es, work_bytes=capi.gmres_workspace_bytes(big, K))
        # a written array overlapping any other array of the call, from either end
        sizes["work"] = capi.gmres_workspace_bytes(N, K if name == "project" else 0)  # what the call uses of it
        for wname in written[name]:
            for other in uses[name]:
                if other == wname:
                    continue
                _refused(INV, call, **{other: A[wname] + (sizes[wname] // 16) * 16 - 16})
                if sizes[other] > 16:
                    _refused(INV, call, **{wname: A[other] + (sizes[other] // 16) * 16 - 16})
    # scale: the scalar off 8 bytes, and minv and vhat both or neither
    _refused(ALI, calls["scale"], scale=A["scale"] + 4)
    _refused(INV, calls["scale"], minv=None)
    _refused(INV, calls["scale"], vhat=None)
    calls["scale"](n=0, minv=None, vhat=None)  # nothing to launch: accepted without a device
    calls["correct"](n=0)
    calls["correct"](k=0, V=None)              # k == 0 leaves x as it is: nothing to launch
    _refused(ALI, calls["correct"], minv=A["minv"] + 4)
    # the workspace one byte too small: refused last, so everything else about the call is accepted
    for name in ("project", "update"):
        need = capi.gmres_workspace_bytes(N, K) if name == "project" else capi.gmres_workspace_bytes(N, 0)
        _refused(INV, calls[name], work_bytes=need - 1)
        _refused(INV, calls[name], work_bytes=0)
        # w directly behind the k vectors that are read is accepted (refused for the workspace alone) ...
        with pytest.raises(capi.SpmvHipError, match="work_bytes"):
            calls[name](w=A["V"] + K * ldv * es, work_bytes=need - 1)
        # ... and k == 0 without a basis
        with pytest.raises(capi.SpmvHipError, match="work_bytes"):
            calls[name](k=0, V=None, work_bytes=15)
    # the update's w inside the vectors that are read, and h inside w
    _refused(INV, calls["update"], w=A["V"] + (K - 1) * ldv * es)
    _refused(INV, calls["update"], h=A["w"] + 16)
    _refused(INV, calls["correct"], y=A["x"] + 16)
    _refused(INV, calls["scale"], scale=A["v"] + 8)
    with pytest.raises(TypeError):
        capi.gmres_scale(N, A["scale"], A["v"], None, None)  # raw addresses need dtype=


def test_refusals_of_the_small_calls():
    m, k = 8, 3
    state_bytes = 8 * capi.gmres_state_doubles(m)
    base = dict(A, m=m, k=k)
    start = lambda **o: capi.gmres_start(*[dict(base, **o)[x] for x in ("m", "nrm2", "state")])
    column = lambda **o: capi.gmres_column(*[dict(base, **o)[x] for x in ("k", "m", "h1", "h2", "nrm2", "state")])
    solve = lambda **o: capi.gmres_solve(*[dict(base, **o)[x] for x in ("k", "m", "state", "y")])
    for call in (start, column, solve):
        for bad in (0, -1, 33):
            _refused(INV, call, m=bad)
        _refused(INV, call, state=None)
        _refused(ALI, call, state=A["state"] + 8)
    for call in (start, column):
        _refused(INV, call, nrm2=None)
        _refused(ALI, call, nrm2=A["nrm2"] + 4)
        _refused(INV, call, nrm2=A["state"] + 8)                 # a scalar inside a written array
        _refused(INV, call, nrm2=A["state"] + state_bytes - 8)
    for bad in (-1, m, m + 1):
        _refused(INV, column, k=bad)                              # column's k >= m included
    for bad in (-1, m + 1):
        _refused(INV, solve, k=bad)
    for p in ("h1", "h2"):
        _refused(INV, column, **{p: None})
        _refused(ALI, column, **{p: A[p] + 8})
        _refused(INV, column, **{p: A["state"] + 16})
    _refused(INV, solve, y=None)
    _refused(ALI, solve, y=A["y"] + 8)
    _refused(INV, solve, y=A["state"] + 16)
    _refused(INV, solve, state=A["y"])
    solve(k=0)  # nothing to solve: accepted without a device
