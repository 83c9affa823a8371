"""The C ABI of the aggregation multigrid level (include/spmv_hip_agg.h) without a GPU: the nine functions are declared, exported
and bound, the header is C99 on its own, the plan struct has the header's layout, and every refusal of the header is given
through capi with made-up addresses -- the refusals precede the first HIP call, so nothing is dereferenced and no device is
needed.  A workspace one byte too small is looked at with everything else valid, so such a call is shown to pass every other
check by being refused for that alone."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from spmv_amd import capi

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
HEADER = os.path.join(INCLUDE, "spmv_hip_agg.h")
NEW = ["spmv_hip_agg_workspace", "spmv_hip_agg_aggregate", "spmv_hip_agg_plan", "spmv_hip_agg_galerkin_symbolic", "spmv_hip_agg_galerkin_numeric"] + \
      ["spmv_hip_agg_%s_%s" % (c, s) for c in ("restrict", "prolong_add") for s in ("f64", "f32")]
INV, ALI = capi.ERR_INVALID, capi.ERR_ALIGN
DTYPES = [np.float64, np.float32]


def test_symbols_exported_declared_and_bound():
    lib = capi.load()  # (not ctypes.CDLL on its own: this file runs first, and the library is to share the HIP runtime torch loads)
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(spmv_hip_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(NEW) and len(NEW) == 9
    for s in NEW:
        assert hasattr(lib, s) and s in capi.SIGNATURES, s
    assert HEADER in [os.path.abspath(h) for h in capi.HEADER_PATHS]
    for m in ("workspace_bytes", "aggregate", "plan", "galerkin_symbolic", "galerkin_numeric", "restrict", "prolong_add"):
        assert callable(getattr(capi, "agg_" + m)), m
    assert '#include "spmv_hip_krylov.h"' in text


def test_header_is_c99_on_its_own_the_plan_has_its_layout_and_the_version_is_unchanged(tmp_path):
    P = capi.AggPlan
    text = subprocess.run(["gcc", "-std=c99", "-I", INCLUDE, "-x", "c", "-", "-E", "-dM"], input='#include "spmv_hip_agg.h"\n', text=True,
                          stdout=subprocess.PIPE, check=True).stdout
    version = int(re.search(r"#define SPMV_HIP_VERSION (\d+)", text).group(1))
    assert version == 130 and capi.load().spmv_hip_version() == 130
    assert not re.findall(r"#define SPMV_HIP_VERSION", open(HEADER).read())
    # the layout, from the compiler's own offsetof through a program that is only compiled
    src2 = '#include <stddef.h>\n#include "spmv_hip_agg.h"\n' + "".join(
        "typedef char check_%s[offsetof(struct spmv_hip_agg_plan, %s) == %d ? 1 : -1];\n" % (f, f, getattr(P, f).offset)
        for f in ("rows", "aggregates", "largest", "d_agg", "d_member_ptr", "d_member")) + \
        "typedef char check_size[sizeof(struct spmv_hip_agg_plan) == %d ? 1 : -1];\n" % C.sizeof(P) + \
        "int (*const the_call)(int32_t, const int32_t *, const int32_t *, int32_t *, int32_t *, struct spmv_hip_agg_plan *, void *, size_t, void *) " \
        "= spmv_hip_agg_plan;\n"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INCLUDE, "-x", "c", "-", "-c", "-o", str(tmp_path / "o.o")],
                       input=src2, text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout


def test_the_workspace_is_a_function_of_rows_and_nnz_alone():
    sizes = [capi.agg_workspace_bytes(n) for n in (0, 1, 1024, 1025, 4099, 2 ** 24)]
    assert sizes[0] >= 16 and all(s % 16 == 0 for s in sizes) and sizes == sorted(sizes)
    assert 25 * 2 ** 24 <= sizes[-1] < 26 * 2 ** 24  # a mark, four ints and a double per row
    with_nnz = [capi.agg_workspace_bytes(4099, nnz) for nnz in (0, 1, 20000, 2 ** 26)]
    assert with_nnz == sorted(with_nnz) and with_nnz[0] == sizes[4] and all(s % 16 == 0 for s in with_nnz)
    assert 20 * 2 ** 26 <= with_nnz[-1] - with_nnz[0] < 20 * 2 ** 26 + 64  # two 8-byte keys and a position per entry
    for bad in ((-1, 0), (0, -1)):
        with pytest.raises(capi.SpmvHipError):
            capi.agg_workspace_bytes(*bad)
    assert capi.load().spmv_hip_agg_workspace(5, 5, None) == INV


# made-up addresses, 16-byte aligned and far apart
N, NNZ, AGGS, NNZ_C = 6030, 30000, 2100, 11000
A = {"p": 0x10000000, "c": 0x20000000, "v": 0x30000000, "agg": 0x40000000, "status": 0x50000000, "mptr": 0x60000000, "member": 0x70000000,
     "cp": 0x80000000, "cc": 0x90000000, "order": 0xA0000000, "eptr": 0xB0000000, "work": 0xC0000000, "fine": 0xD0000000, "coarse": 0xE0000000,
     "cv": 0xF0000000}


def _refused(code, fn, *args, **kw):
    with pytest.raises(capi.SpmvHipError) as e:
        fn(*args, **kw)
    assert e.value.code == code, (e.value, args, kw)
    assert capi.load().spmv_hip_last_error()


def _plan(**o):
    a = dict(A, rows=N, aggregates=AGGS, largest=5)
    a.update(o)
    plan = capi.AggPlan()
    plan.rows, plan.aggregates, plan.largest = a["rows"], a["aggregates"], a["largest"]
    plan.d_agg, plan.d_member_ptr, plan.d_member = a["agg"], a["mptr"], a["member"]
    return plan


PLAN_KEYS = ("rows", "aggregates", "largest", "agg", "mptr", "member")


def _split(base, o):
    a = dict(base, **{k: w for k, w in o.items() if k not in PLAN_KEYS})
    plan = _plan(**{k: w for k, w in o.items() if k in PLAN_KEYS}) if a["plan"] else None
    return a, plan


def _overlaps(call, uses, written, sizes):
    """A written array overlapping any other array of the call, from either end."""
    for wname in written:
        for other in uses:
            if other == wname:
                continue
            _refused(INV, call, **{other: A[wname] + (sizes[wname] // 16) * 16 - (16 if sizes[wname] >= 16 else 0)})
            if sizes[other] > 16:
                _refused(INV, call, **{wname: A[other] + (sizes[other] // 16) * 16 - 16})


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_every_refusal_of_restrict_and_prolong_add_with_made_up_addresses(dtype):
    base = dict(A, omega=1.0, plan=True)

    def restrict(**o):
        a, plan = _split(base, o)
        capi.agg_restrict(plan, a["fine"], a["coarse"], dtype=dtype)

    def prolong(**o):
        a, plan = _split(base, o)
        capi.agg_prolong_add(plan, a["omega"], a["coarse"], a["fine"], dtype=dtype)

    es = np.dtype(dtype).itemsize
    sizes = {"agg": 4 * N, "mptr": 4 * AGGS + 4, "member": 4 * N, "fine": N * es, "coarse": AGGS * es}
    align = {"agg": 4, "mptr": 4, "member": 4, "fine": 16, "coarse": 16}
    for call, written in ((restrict, "coarse"), (prolong, "fine")):
        _refused(INV, call, plan=False)
        _refused(INV, call, rows=-1)
        for p in sizes:
            _refused(INV, call, **{p: None})
            _refused(INV, call, rows=0, aggregates=0, **{p: None})
            _refused(ALI, call, **{p: A[p] + align[p] // 2})
        for aggregates in (-1, N + 1, 0):
            _refused(INV, call, aggregates=aggregates)
        _refused(INV, call, rows=0, aggregates=1)
        big = 2 ** 32 // es
        _refused(INV, call, rows=big)
        with pytest.raises(capi.SpmvHipError, match="4 GiB"):
            call(rows=big)
        _overlaps(call, tuple(sizes), (written,), sizes)
        call(rows=0, aggregates=0)  # nothing is launched: accepted without a device
    for omega in (float("nan"), float("inf"), -float("inf")):
        _refused(INV, prolong, omega=omega)
    with pytest.raises(TypeError):
        capi.agg_restrict(_plan(), A["fine"], A["coarse"])  # raw addresses need dtype=


def test_every_refusal_of_the_setup_calls_with_made_up_addresses():
    need0, need = capi.agg_workspace_bytes(N), capi.agg_workspace_bytes(N, NNZ)
    base = dict(A, n=N, nnz=NNZ, nnz_c=NNZ_C, theta=0.25, seed=0, work_bytes=need, plan=True)

    def aggregate(**o):
        a = dict(base, **o)
        capi.agg_aggregate(a["n"], a["p"], a["c"], a["v"], a["theta"], a["seed"], a["agg"], a["status"], a["work"], a["work_bytes"])

    def plan(**o):
        a = dict(base, **o)
        capi.agg_plan(a["n"], a["agg"], a["status"], a["mptr"], a["member"], a["work"], a["work_bytes"])

    def symbolic(**o):
        a, pl = _split(base, o)
        capi.agg_galerkin_symbolic(pl, a["nnz"], a["p"], a["c"], a["cp"], a["cc"], a["order"], a["eptr"], a["status"], a["work"], a["work_bytes"])

    def numeric(**o):
        a = dict(base, **o)
        capi.agg_galerkin_numeric(a["nnz"], a["nnz_c"], a["order"], a["eptr"], a["v"], a["cv"])

    align = {"p": 4, "c": 4, "v": 8, "agg": 4, "status": 4, "mptr": 4, "member": 4, "cp": 4, "cc": 4, "order": 4, "eptr": 4, "work": 16, "cv": 8}
    # aggregate: the columns' and the values' length is not known to it
    sizes = {"p": 4 * N + 4, "c": 4, "v": 8, "agg": 4 * N, "status": 16, "work": need0}
    _refused(INV, aggregate, n=-1)
    for p in sizes:
        if p != "v":
            _refused(INV, aggregate, **{p: None})
            _refused(INV, aggregate, n=0, **{p: None})
        _refused(ALI, aggregate, **{p: A[p] + align[p] // 2})
    for theta in (-0.25, 1.5, float("nan"), float("inf"), -float("inf")):
        _refused(INV, aggregate, theta=theta)
    _refused(INV, aggregate, work_bytes=0)
    with pytest.raises(capi.SpmvHipError, match="work_bytes"):
        aggregate(work_bytes=need0 - 1, v=None, theta=1.0)
    with pytest.raises(capi.SpmvHipError, match="work_bytes"):
        aggregate(work_bytes=need0 - 1, theta=0.0)
    _overlaps(aggregate, tuple(sizes), ("agg", "status", "work"), sizes)
    # plan: d_member_ptr is as long as the status says, which is read on the device: its first element is known
    sizes = {"agg": 4 * N, "status": 16, "mptr": 4, "member": 4 * N, "work": need0}
    _refused(INV, plan, n=-1)
    for p in sizes:
        _refused(INV, plan, **{p: None})
        _refused(INV, plan, n=0, **{p: None})
        _refused(ALI, plan, **{p: A[p] + align[p] // 2})
    with pytest.raises(capi.SpmvHipError, match="work_bytes"):
        plan(work_bytes=need0 - 1)
    _overlaps(plan, tuple(sizes), ("mptr", "member", "work"), sizes)
    assert capi.load().spmv_hip_agg_plan(N, A["agg"], A["status"], A["mptr"], A["member"], None, A["work"], need0, None) == INV  # a null plan
    # symbolic
    sizes = {"agg": 4 * N, "p": 4 * N + 4, "c": 4 * NNZ, "cp": 4 * AGGS + 4, "cc": 4 * NNZ, "order": 4 * NNZ, "eptr": 4 * NNZ + 4, "status": 4,
             "work": need}
    _refused(INV, symbolic, plan=False)
    _refused(INV, symbolic, rows=-1)
    _refused(INV, symbolic, nnz=-1)
    for aggregates in (-1, N + 1, 0):
        _refused(INV, symbolic, aggregates=aggregates)
    for p in tuple(sizes) + ("mptr", "member"):  # (the member lists are not read here: a plan without them is refused all the same)
        _refused(INV, symbolic, **{p: None})
        _refused(INV, symbolic, rows=0, aggregates=0, **{p: None})
        if p in sizes:
            _refused(ALI, symbolic, **{p: A[p] + align[p] // 2})
    _refused(INV, symbolic, work_bytes=need0)
    with pytest.raises(capi.SpmvHipError, match="work_bytes"):
        symbolic(work_bytes=need - 1)
    _overlaps(symbolic, tuple(sizes), ("cp", "cc", "order", "eptr", "status", "work"), sizes)
    # numeric
    sizes = {"order": 4 * NNZ, "eptr": 4 * NNZ_C + 4, "v": 8 * NNZ, "cv": 8 * NNZ_C}
    for bad in (dict(nnz=-1), dict(nnz_c=-1), dict(nnz_c=NNZ + 1)):
        _refused(INV, numeric, **bad)
    for p in sizes:
        _refused(INV, numeric, **{p: None})
        _refused(INV, numeric, nnz=0, nnz_c=0, **{p: None})
        _refused(ALI, numeric, **{p: A[p] + align[p] // 2})
    _overlaps(numeric, tuple(sizes), ("cv",), sizes)
    numeric(nnz_c=0)  # nothing is launched: accepted without a device
