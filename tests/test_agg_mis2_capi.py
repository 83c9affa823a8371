"""The C ABI of include/spmv_hip_agg_mis2.h without a GPU: the five functions are declared, exported and bound, the header is C99
on its own and leaves spmv_hip_agg.h and the version as they were, the workspace is a function of rows alone, the recommended
group is host arithmetic, and every refusal of the header is given through capi with made-up addresses -- the refusals precede
the first HIP call, so nothing is dereferenced and no device is needed.  A workspace one byte too small is looked at with
everything else valid, so such a call is shown to pass every other check by being refused for that alone."""
import os
import re
import subprocess

import numpy as np
import pytest

from spmv_amd import capi
from test_agg_capi import A, AGGS, ALI, DTYPES, INCLUDE, INV, N, _overlaps, _plan, _refused, _split

HEADER = os.path.join(INCLUDE, "spmv_hip_agg_mis2.h")
NEW = ["spmv_hip_agg_mis2_workspace", "spmv_hip_agg_aggregate_mis2", "spmv_hip_agg_restrict_group_f64", "spmv_hip_agg_restrict_group_f32",
       "spmv_hip_agg_group"]
GROUPS = (1, 2, 4, 8, 16, 32, 64)


def test_symbols_exported_declared_and_bound():
    lib = capi.load()
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(spmv_hip_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(NEW)
    for s in NEW:
        assert hasattr(lib, s) and s in capi.SIGNATURES, s
    assert HEADER in [os.path.abspath(h) for h in capi.HEADER_PATHS]
    for m in ("aggregate_mis2", "mis2_workspace_bytes", "restrict_group", "group"):
        assert callable(getattr(capi, "agg_" + m)), m
    assert '#include "spmv_hip_agg.h"' in text


def test_header_is_c99_on_its_own_and_the_version_is_unchanged(tmp_path):
    src = '#include "spmv_hip_agg_mis2.h"\n' \
          "int (*const the_call)(const struct spmv_hip_agg_plan *, int32_t, const float *, float *, void *) = spmv_hip_agg_restrict_group_f32;\n" \
          "int32_t (*const the_group)(const struct spmv_hip_agg_plan *) = spmv_hip_agg_group;\n" \
          "int (*const the_rule)(int32_t, size_t *) = spmv_hip_agg_mis2_workspace;\n"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INCLUDE, "-x", "c", "-", "-c", "-o", str(tmp_path / "o.o")],
                       input=src, text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout
    assert capi.load().spmv_hip_version() == 130 and not re.findall(r"#define SPMV_HIP_VERSION", open(HEADER).read())


def test_the_workspace_is_a_function_of_rows_alone():
    sizes = [capi.agg_mis2_workspace_bytes(n) for n in (0, 1, 1024, 1025, 4099, 2 ** 24)]
    assert sizes[0] >= 16 and all(s % 16 == 0 for s in sizes) and sizes == sorted(sizes)
    assert 26 * 2 ** 24 <= sizes[-1] < 27 * 2 ** 24  # two marks, four ints and a double per row
    assert capi.agg_workspace_bytes(2 ** 24) < sizes[-1], "the rule of spmv_hip_agg_workspace is another one"
    with pytest.raises(capi.SpmvHipError):
        capi.agg_mis2_workspace_bytes(-1)
    assert capi.load().spmv_hip_agg_mis2_workspace(5, None) == INV


def test_the_recommended_group_is_host_arithmetic_on_the_two_counts():
    for rows, aggregates, want in ((262144, 36783, 8), (110592, 10145, 16), (5001, 1, 64), (10, 10, 1), (10, 5, 2), (11, 5, 4), (64, 1, 64),
                                   (2 ** 31 - 1, 1, 64), (2 ** 31 - 1, 2 ** 30, 2), (0, 0, 1), (7, 0, 1), (-3, 1, 1)):
        assert capi.agg_group(_plan(rows=rows, aggregates=aggregates)) == want, (rows, aggregates)
    assert capi.agg_group(None) == 1
    assert capi.agg_group(_plan(agg=None, mptr=None, member=None)) == 4  # no array is looked at


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_every_refusal_of_restrict_group_with_made_up_addresses(dtype):
    base = dict(A, plan=True, group=8)

    def restrict(**o):
        a, plan = _split(base, o)
        capi.agg_restrict_group(plan, a["group"], a["fine"], a["coarse"], dtype=dtype)

    es = np.dtype(dtype).itemsize
    sizes = {"agg": 4 * N, "mptr": 4 * AGGS + 4, "member": 4 * N, "fine": N * es, "coarse": AGGS * es}
    align = {"agg": 4, "mptr": 4, "member": 4, "fine": 16, "coarse": 16}
    for group in list(range(-2, 1)) + [g for g in range(1, 70) if g not in GROUPS] + [128, 256, 2 ** 30, -2 ** 31, -8, -64]:
        _refused(INV, restrict, group=group)
        with pytest.raises(capi.SpmvHipError, match="power of two"):
            restrict(group=group)
    for group in GROUPS:  # every group that is instantiated, the one that is the plain restriction among them
        _refused(INV, restrict, plan=False, group=group)
        _refused(INV, restrict, rows=-1, group=group)
        for p in sizes:
            _refused(INV, restrict, group=group, **{p: None})
            _refused(INV, restrict, rows=0, aggregates=0, group=group, **{p: None})
            _refused(ALI, restrict, group=group, **{p: A[p] + align[p] // 2})
        for aggregates in (-1, N + 1, 0):
            _refused(INV, restrict, aggregates=aggregates, group=group)
        _refused(INV, restrict, rows=0, aggregates=1, group=group)
        big = 2 ** 32 // es
        _refused(INV, restrict, rows=big, group=group)
        with pytest.raises(capi.SpmvHipError, match="4 GiB"):
            restrict(rows=big, group=group)
        restrict(rows=0, aggregates=0, group=group)  # nothing is launched: accepted without a device
    _overlaps(restrict, tuple(sizes), ("coarse",), sizes)
    _refused(INV, restrict, rows=0, aggregates=0, group=3)  # the group is looked at before anything is skipped
    with pytest.raises(TypeError):
        capi.agg_restrict_group(_plan(), 8, A["fine"], A["coarse"])  # raw addresses need dtype=


def test_every_refusal_of_aggregate_mis2_with_made_up_addresses():
    need = capi.agg_mis2_workspace_bytes(N)
    base = dict(A, n=N, theta=0.25, seed=0, work_bytes=need)

    def aggregate(**o):
        a = dict(base, **o)
        capi.agg_aggregate_mis2(a["n"], a["p"], a["c"], a["v"], a["theta"], a["seed"], a["agg"], a["status"], a["work"], a["work_bytes"])

    align = {"p": 4, "c": 4, "v": 8, "agg": 4, "status": 4, "work": 16}
    sizes = {"p": 4 * N + 4, "c": 4, "v": 8, "agg": 4 * N, "status": 16, "work": need}  # the columns' and the values' length is not known to it
    _refused(INV, aggregate, n=-1)
    for p in sizes:
        if p != "v":
            _refused(INV, aggregate, **{p: None})
            _refused(INV, aggregate, n=0, **{p: None})
        _refused(ALI, aggregate, **{p: A[p] + align[p] // 2})
    for theta in (-0.25, 1.5, float("nan"), float("inf"), -float("inf")):
        _refused(INV, aggregate, theta=theta)
    _refused(INV, aggregate, work_bytes=0)
    _refused(INV, aggregate, work_bytes=capi.agg_workspace_bytes(N))  # the rule of the distance-1 call is too small
    with pytest.raises(capi.SpmvHipError, match="work_bytes"):
        aggregate(work_bytes=need - 1, v=None, theta=1.0)
    with pytest.raises(capi.SpmvHipError, match="work_bytes"):
        aggregate(work_bytes=need - 1, theta=0.0)
    with pytest.raises(capi.SpmvHipError, match="spmv_hip_agg_mis2_workspace"):
        aggregate(work_bytes=need - 1)
    _overlaps(aggregate, tuple(sizes), ("agg", "status", "work"), sizes)
