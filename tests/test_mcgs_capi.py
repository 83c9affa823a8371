"""The C ABI of the multicolour Gauss-Seidel / SSOR preconditioner (include/spmv_hip_mcgs.h) without a GPU: the seven functions
are declared, exported and bound, the header is C99 on its own, the plan struct has the header's layout, and every refusal of
the header is given through capi with made-up addresses -- the refusals precede the first HIP call, so nothing is dereferenced
and no device is needed.  A workspace one byte too small is looked at with everything else valid, so such a call is shown to
pass every other check by being refused for that alone."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from spmv_amd import capi

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
HEADER = os.path.join(INCLUDE, "spmv_hip_mcgs.h")
NEW = ["spmv_hip_mcgs_workspace", "spmv_hip_mcgs_colour", "spmv_hip_mcgs_permute"] + \
      ["spmv_hip_mcgs_%s_%s" % (c, s) for c in ("sweep", "apply") for s in ("f64", "f32")]
INV, ALI = capi.ERR_INVALID, capi.ERR_ALIGN
DTYPES = [np.float64, np.float32]


def test_symbols_exported_declared_and_bound():
    lib = C.CDLL(capi.LIB_PATH)
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(spmv_hip_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(NEW) and len(NEW) == 7
    for s in NEW:
        assert hasattr(lib, s) and s in capi.SIGNATURES, s
    assert HEADER in [os.path.abspath(h) for h in capi.HEADER_PATHS]
    for m in ("workspace_bytes", "colour", "permute", "sweep", "apply"):
        assert callable(getattr(capi, "mcgs_" + m)), m
    assert '#include "spmv_hip_krylov.h"' in text and "#define SPMV_HIP_MCGS_MAX_COLOURS 64" in text and capi.MCGS_MAX_COLOURS == 64


def test_header_is_c99_on_its_own_the_plan_has_its_layout_and_the_version_is_unchanged(tmp_path):
    src = '#include <stdio.h>\n#include "spmv_hip_mcgs.h"\nint main(void) { spmv_hip_mcgs_plan p; ' \
          'printf("%d %d %d %d %d\\n", (int) sizeof p, (int) ((char *) p.colour_ptr - (char *) &p), (int) ((char *) &p.d_order - (char *) &p), ' \
          '(int) ((char *) &p.d_value - (char *) &p), SPMV_HIP_VERSION + SPMV_HIP_MCGS_MAX_COLOURS); return 0; }\n'
    exe = str(tmp_path / "layout")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INCLUDE, "-x", "c", "-", "-o", exe],
                       input=src, text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout
    got = [int(t) for t in subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    P = capi.McgsPlan
    assert got == [C.sizeof(P), P.colour_ptr.offset, P.d_order.offset, P.d_value.offset, 130 + 64], got
    assert not re.findall(r"#define SPMV_HIP_VERSION", open(HEADER).read())
    assert capi.load().spmv_hip_version() == 130


def test_the_workspace_is_a_function_of_rows_alone():
    sizes = [capi.mcgs_workspace_bytes(n) for n in (0, 1, 1024, 1025, 4099, 2 ** 24)]
    assert sizes[0] >= 16 and all(s % 16 == 0 for s in sizes) and sizes == sorted(sizes) and sizes[-1] >= 2 ** 24
    assert sizes[-1] < 2 * 2 ** 24  # a byte per row and a quarter of one per row for the sort's histograms
    with pytest.raises(capi.SpmvHipError):
        capi.mcgs_workspace_bytes(-1)
    assert capi.load().spmv_hip_mcgs_workspace(5, None) == INV


# made-up addresses, 16-byte aligned and far apart
N, NNZ, COLOURS = 6030, 30000, 5
A = {"p": 0x10000000, "c": 0x20000000, "v": 0x30000000, "colour": 0x40000000, "status": 0x50000000, "order": 0x60000000,
     "pp": 0x70000000, "pc": 0x80000000, "pv": 0x90000000, "work": 0xA0000000, "b": 0xB0000000, "minv": 0xC0000000, "x": 0xD0000000,
     "dots": 0xE0000000}


def _refused(code, fn, *args, **kw):
    with pytest.raises(capi.SpmvHipError) as e:
        fn(*args, **kw)
    assert e.value.code == code, (e.value, args, kw)
    assert capi.load().spmv_hip_last_error()


def _plan(**o):
    a = dict(A, rows=N, colours=COLOURS, conflicts=0, group=8)
    a.update(o)
    plan = capi.McgsPlan()
    plan.rows, plan.colours, plan.conflicts, plan.group = a["rows"], a["colours"], a["conflicts"], a["group"]
    ptr = a.get("colour_ptr")
    if ptr is None:
        ptr = [min(a["rows"], k * (a["rows"] // max(1, a["colours"]))) for k in range(max(0, min(64, a["colours"])))] + [a["rows"]] * 66
    for k in range(65):
        plan.colour_ptr[k] = ptr[k]
    plan.d_order, plan.d_row_ptr, plan.d_column_index, plan.d_value = a["order"], a["pp"], a["pc"], a["pv"]
    return plan


PLAN_KEYS = ("rows", "colours", "conflicts", "group", "colour_ptr", "order", "pp", "pc", "pv")


def _calls(dtype):
    base = dict(A, first=0, last=COLOURS - 1, omega=1.0, work_bytes=capi.krylov_workspace_bytes(N), plan=True)

    def split(o):
        a = dict(base, **{k: w for k, w in o.items() if k not in PLAN_KEYS})
        plan = _plan(**{k: w for k, w in o.items() if k in PLAN_KEYS}) if a["plan"] else None
        return a, plan

    def sweep(**o):
        a, plan = split(o)
        capi.mcgs_sweep(plan, a["first"], a["last"], a["omega"], a["b"], a["minv"], a["x"], dtype=dtype)

    def apply(**o):
        a, plan = split(o)
        capi.mcgs_apply(plan, a["omega"], a["b"], a["minv"], a["x"], a["dots"], a["work"], a["work_bytes"], dtype=dtype)

    return {"sweep": sweep, "apply": apply}


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_every_refusal_of_sweep_and_apply_with_made_up_addresses(dtype):
    calls = _calls(dtype)
    es = np.dtype(dtype).itemsize
    vec = N * es
    sizes = {"b": vec, "minv": vec, "x": vec, "dots": 16, "work": capi.krylov_workspace_bytes(N), "order": 4 * N, "pp": 4 * N + 4, "pc": 4, "pv": 8}
    align = {"b": 16, "minv": 16, "x": 16, "dots": 16, "work": 16, "order": 4, "pp": 4, "pc": 4, "pv": 8}
    uses = {"sweep": ("order", "pp", "pc", "pv", "b", "minv", "x"), "apply": ("order", "pp", "pc", "pv", "b", "minv", "x", "dots", "work")}
    written = {"sweep": ("x",), "apply": ("x", "dots", "work")}
    for name, call in calls.items():
        _refused(INV, call, plan=False)                        # a null plan
        _refused(INV, call, rows=-1)
        for p in ("order", "pp", "pc", "pv", "b", "minv", "x"):
            _refused(INV, call, **{p: None})                   # a null required pointer
            _refused(INV, call, rows=0, colours=0, **{p: None})    # ... also where rows == 0
        for omega in (0.0, 2.0, -0.5, 2.5, float("nan"), float("inf"), -float("inf")):
            _refused(INV, call, omega=omega)
        for group in (0, -1, 3, 6, 12, 65, 128):
            _refused(INV, call, group=group)
        for colours in (-1, 65):
            _refused(INV, call, colours=colours)
        _refused(INV, call, conflicts=1)
        _refused(INV, call, conflicts=-1)
        with pytest.raises(capi.SpmvHipError, match="conflicts"):
            call(conflicts=3)
        good = [0, 1000, 2000, 3000, 4000] + [N] * 61
        for bad in ([1] + good[1:], good[:2] + [999] + good[3:], good[:5] + [N - 1] * 61, good[:5] + [N + 1] * 61):
            _refused(INV, call, colour_ptr=bad)
        for p in uses[name]:
            _refused(ALI, call, **{p: A[p] + align[p] // 2})
        big = 2 ** 32 // es
        _refused(INV, call, rows=big, work_bytes=capi.krylov_workspace_bytes(big))
        with pytest.raises(capi.SpmvHipError, match="4 GiB"):
            call(rows=big, work_bytes=capi.krylov_workspace_bytes(big))
        # a written array overlapping any other array of the call, from either end
        for wname in written[name]:
            for other in uses[name]:
                if other == wname:
                    continue
                _refused(INV, call, **{other: A[wname] + (sizes[wname] // 16) * 16 - (16 if sizes[wname] >= 16 else 0)})
                if sizes[other] > 16:
                    _refused(INV, call, **{wname: A[other] + (sizes[other] // 16) * 16 - 16})
        _refused(INV, call, x=A["b"])
        _refused(INV, call, x=A["minv"])
    # a colour index outside the plan
    for first, last in ((-1, 0), (0, -1), (COLOURS, 0), (0, COLOURS), (64, 64)):
        _refused(INV, calls["sweep"], first=first, last=last)
    _refused(INV, calls["sweep"], rows=0, colours=0, first=1, last=0)
    # every group the header allows passes the checks: refused for the workspace alone
    need = capi.krylov_workspace_bytes(N)
    for group in (1, 2, 4, 8, 16, 32, 64):
        with pytest.raises(capi.SpmvHipError, match="work_bytes"):
            calls["apply"](group=group, work_bytes=need - 1)
    _refused(INV, calls["apply"], work_bytes=0)
    _refused(INV, calls["apply"], dots=None)
    _refused(INV, calls["apply"], work=None)
    # rows == 0 without dots launches nothing: accepted without a device
    calls["apply"](rows=0, colours=0, dots=None, work=None, work_bytes=0)
    calls["sweep"](rows=0, colours=0, first=0, last=0)
    with pytest.raises(TypeError):
        capi.mcgs_sweep(_plan(), 0, 0, 1.0, A["b"], A["minv"], A["x"])  # raw addresses need dtype=


def test_every_refusal_of_colour_and_permute_with_made_up_addresses():
    need = capi.mcgs_workspace_bytes(N)
    base = dict(A, rows=N, nnz=NNZ, seed=0, work_bytes=need, plan=True)

    def colour(**o):
        a = dict(base, **o)
        capi.mcgs_colour(a["rows"], a["p"], a["c"], a["seed"], a["colour"], a["status"], a["work"], a["work_bytes"])

    def permute(**o):
        a = dict(base, **o)
        capi.mcgs_permute(a["rows"], a["nnz"], a["p"], a["c"], a["v"], a["colour"], a["status"], a["order"], a["pp"], a["pc"], a["pv"], a["work"],
                          a["work_bytes"])

    sizes = {"p": 4 * N + 4, "c": 4 * NNZ, "v": 8 * NNZ, "colour": 4 * N, "status": 16, "order": 4 * N, "pp": 4 * N + 4, "pc": 4 * NNZ,
             "pv": 8 * NNZ, "work": need}
    align = {"p": 4, "c": 4, "v": 8, "colour": 4, "status": 4, "order": 4, "pp": 4, "pc": 4, "pv": 8, "work": 16}
    uses = {colour: ("p", "c", "colour", "status", "work"), permute: ("p", "c", "v", "colour", "status", "order", "pp", "pc", "pv", "work")}
    written = {colour: ("colour", "status", "work"), permute: ("order", "pp", "pc", "pv", "work")}
    for call in (colour, permute):
        _refused(INV, call, rows=-1)
        for p in uses[call]:
            _refused(INV, call, **{p: None})
            _refused(INV, call, rows=0, **{p: None})
            _refused(ALI, call, **{p: A[p] + align[p] // 2})
        _refused(INV, call, work_bytes=0)
        with pytest.raises(capi.SpmvHipError, match="work_bytes"):
            call(work_bytes=need - 1)
        for wname in written[call]:
            for other in uses[call]:
                if other == wname:
                    continue
                known = sizes[other] if call is permute or other not in ("c",) else 4  # colour does not know the columns' length
                _refused(INV, call, **{other: A[wname] + (sizes[wname] // 16) * 16 - 16})
                if known > 16:
                    _refused(INV, call, **{wname: A[other] + (known // 16) * 16 - 16})
    _refused(INV, permute, nnz=-1)
    lib = capi.load()
    assert lib.spmv_hip_mcgs_permute(N, NNZ, A["p"], A["c"], A["v"], A["colour"], A["status"], A["order"], A["pp"], A["pc"], A["pv"], None,
                                     A["work"], need, None) == INV  # a null plan
