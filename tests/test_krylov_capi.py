"""The C ABI of the conjugate-gradient updates (include/spmv_hip_krylov.h) without a GPU: the five functions are declared, exported
and bound, the header is C99 on its own, include/spmv_hip.h is still the 19-function boundary, the workspace is a monotone
function of n, and every refusal of the header is given with made-up addresses -- the refusals precede the first HIP call, so
nothing is dereferenced and no device is needed."""
import ctypes as C
import os
import re
import subprocess

import pytest

from spmv_amd import capi
from spmv_amd.capi import cg_direction, cg_step, krylov_workspace_bytes  # noqa: F401

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
HEADER = os.path.join(INCLUDE, "spmv_hip_krylov.h")
STEPS = ["spmv_hip_cg_step_f64", "spmv_hip_cg_step_f32"]
DIRECTIONS = ["spmv_hip_cg_direction_f64", "spmv_hip_cg_direction_f32"]
NEW = ["spmv_hip_krylov_workspace"] + STEPS + DIRECTIONS
INV, ALI = capi.ERR_INVALID, capi.ERR_ALIGN


def _code(path):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def test_symbols_exported_declared_and_bound():
    lib = C.CDLL(capi.LIB_PATH)
    text = _code(HEADER)
    declared = sorted(set(re.findall(r"\b(spmv_hip_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(NEW) and len(NEW) == 5
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in capi.SIGNATURES, s
    assert HEADER in [os.path.abspath(h) for h in capi.HEADER_PATHS]
    for m in ("krylov_workspace_bytes", "cg_step", "cg_direction"):
        assert callable(getattr(capi, m)), m
    assert re.search(r"int spmv_hip_krylov_workspace\(int32_t n, size_t \*bytes\);", text)
    for suffix, t in (("f64", "double"), ("f32", "float")):
        assert re.search(r"int spmv_hip_cg_step_%s\(int32_t n, const double \*d_num, const double \*d_den, const %s \*d_p, const %s \*d_q, "
                         r"%s \*d_x,\s*%s \*d_r, const %s \*d_minv, double \*d_dots, void \*d_work, size_t work_bytes, void \*stream\);"
                         % (suffix, t, t, t, t, t), text), suffix
        assert re.search(r"int spmv_hip_cg_direction_%s\(int32_t n, const double \*d_num, const double \*d_den, const %s \*d_r, "
                         r"const %s \*d_minv,\s*%s \*d_p, void \*stream\);" % (suffix, t, t, t), text), suffix
    for s in STEPS:
        args = capi.SIGNATURES[s][1]
        assert len(args) == 12 and args[0] == C.c_int32 and args[10] == C.c_size_t
    for s in DIRECTIONS:
        assert len(capi.SIGNATURES[s][1]) == 7 and capi.SIGNATURES[s][1][0] == C.c_int32
    # the chunk is written in the header
    assert re.search(r"#define SPMV_HIP_KRYLOV_CHUNK 1024\b", text) and "SPMV_HIP_KRYLOV_CHUNK (1024)" in open(HEADER).read()


def test_header_is_c99_on_its_own_and_the_boundary_header_keeps_its_19_functions():
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INCLUDE, "-fsyntax-only", "-x", "c", "-"],
                       input='#include "spmv_hip_krylov.h"\nint main(void) { return SPMV_HIP_VERSION + SPMV_HIP_KRYLOV_CHUNK; }\n',
                       text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout
    small = _code(capi.HEADER_PATH)
    assert len(set(re.findall(r"\b(spmv_hip_[a-z0-9_]+)\s*\(", small))) == 19
    assert "krylov" not in small and "cg_step" not in small
    assert not re.findall(r"#define SPMV_HIP_VERSION", open(HEADER).read())
    assert capi.load().spmv_hip_version() == 130


def test_the_workspace_is_a_monotone_function_of_n_and_at_least_16():
    lib = capi.load()
    sizes = list(range(0, 70)) + [1023, 1024, 1025, 4095, 4096, 4097, 2 ** 20, 2 ** 21 - 1, 2 ** 21, 2 ** 21 + 1, 2 ** 24, 2 ** 29, 2 ** 31 - 1]
    got = [capi.krylov_workspace_bytes(n) for n in sizes]
    assert got[0] == 16 and all(b >= 16 and b % 16 == 0 for b in got)
    assert all(a <= b for a, b in zip(got, got[1:]))
    assert got == [capi.krylov_workspace_bytes(n) for n in sizes]  # of n alone
    # a slot per 1024 elements, and one per 2048 slots
    assert capi.krylov_workspace_bytes(1024) == 32 and capi.krylov_workspace_bytes(1025) == 48
    n = C.c_size_t(7)
    assert lib.spmv_hip_krylov_workspace(-1, C.byref(n)) == INV and n.value == 7
    assert lib.spmv_hip_krylov_workspace(5, None) == INV


# made-up addresses, 16-byte aligned and far apart; the step's arguments by name
N = 5000
BASE = {"num": 0x10000, "den": 0x10008, "p": 0x100000, "q": 0x200000, "x": 0x300000, "r": 0x400000, "minv": 0x500000, "dots": 0x600000,
        "work": 0x700000}


def _step(lib, suffix, n=N, work_bytes=None, **over):
    a = dict(BASE, **over)
    if work_bytes is None:
        work_bytes = capi.krylov_workspace_bytes(n) if n >= 0 else 1 << 20
    return getattr(lib, "spmv_hip_cg_step_" + suffix)(n, a["num"], a["den"], a["p"], a["q"], a["x"], a["r"], a["minv"], a["dots"], a["work"],
                                                       work_bytes, None)


def _direction(lib, suffix, n=N, **over):
    a = dict(BASE, **over)
    return getattr(lib, "spmv_hip_cg_direction_" + suffix)(n, a["num"], a["den"], a["r"], a["minv"], a["p"], None)


@pytest.mark.parametrize("suffix,es", [("f64", 8), ("f32", 4)])
def test_every_refusal_of_the_step_precedes_the_first_hip_call(suffix, es):
    lib = capi.load()
    need = capi.krylov_workspace_bytes(N)
    vec = N * es
    last = lambda base: base + ((vec - 1) & ~15)  # the last 16 bytes of a vector at base
    cases = [("n < 0", dict(n=-1), INV)]
    cases += [("null " + k, {k: None}, INV) for k in ("num", "den", "p", "q", "x", "r", "dots", "work")]
    cases += [("null %s with n == 0" % k, {"n": 0, k: None}, INV) for k in ("num", "den", "p", "q", "x", "r", "dots", "work")]
    cases += [("work_bytes one byte short", dict(work_bytes=need - 1), INV), ("work_bytes 0", dict(work_bytes=0), INV),
              ("work_bytes 15 with n == 0", dict(n=0, work_bytes=15), INV),
              ("vectors of 4 GiB", dict(n=2 ** 32 // es, work_bytes=1 << 40, p=1 << 40, q=2 << 40, x=3 << 40, r=4 << 40, minv=5 << 40), INV),
              ("vectors of more than 4 GiB", dict(n=2 ** 31 - 1, work_bytes=1 << 40, p=1 << 40, q=2 << 40, x=3 << 40, r=4 << 40, minv=5 << 40), INV)]
    # a written array overlapping any other array of the call
    pairs = [("x", "p"), ("x", "q"), ("x", "r"), ("x", "minv"), ("r", "p"), ("r", "q"), ("r", "minv")]
    cases += [("%s == %s" % (w, o), {o: BASE[w]}, INV) for w, o in pairs]
    cases += [("%s begins in the last bytes of %s" % (o, w), {o: last(BASE[w])}, INV) for w, o in pairs]
    cases += [("%s ends in the first bytes of %s" % (o, w), {o: BASE[w] - ((vec - 1) & ~15)}, INV) for w, o in pairs]
    for k in ("p", "q", "x", "r", "minv"):
        cases += [("dots inside " + k, {"dots": BASE[k] + 64}, INV), ("dots in the last bytes of " + k, {"dots": last(BASE[k])}, INV),
                  ("the workspace inside " + k, {"work": BASE[k] + 64}, INV), ("the workspace ending inside " + k, {"work": BASE[k] - need + 16}, INV)]
    cases += [("dots inside the workspace", {"dots": BASE["work"] + need - 16}, INV), ("dots == the workspace", {"dots": BASE["work"]}, INV),
              ("the workspace ending inside dots", {"work": BASE["dots"] - need + 16}, INV)]
    for s in ("num", "den"):
        cases += [("%s inside %s" % (s, k), {s: BASE[k] + 8}, INV) for k in ("dots", "work", "x", "r")]
        cases += [("%s the last double of %s" % (s, k), {s: BASE[k] + ((vec - 8) & ~7)}, INV) for k in ("x", "r")]
        cases += [("%s the last double of the workspace" % s, {s: BASE["work"] + need - 8}, INV), ("%s == dots + 8" % s, {s: BASE["dots"] + 8}, INV)]
    cases += [("num == den inside dots", {"num": BASE["dots"], "den": BASE["dots"]}, INV)]
    # alignment
    cases += [("%s off 16-byte alignment" % k, {k: BASE[k] + off}, ALI) for k in ("p", "q", "x", "r", "minv", "dots", "work") for off in (es, 8)]
    cases += [("%s off 8-byte alignment" % k, {k: BASE[k] + 4}, ALI) for k in ("num", "den")]
    for what, over, code in cases:
        rc = _step(lib, suffix, **over)
        assert rc == code, "%s: %d (%s)" % (what, rc, lib.spmv_hip_last_error())
        assert lib.spmv_hip_last_error(), what


@pytest.mark.parametrize("suffix,es", [("f64", 8), ("f32", 4)])
def test_every_refusal_of_the_direction_precedes_the_first_hip_call(suffix, es):
    lib = capi.load()
    vec = N * es
    last = lambda base: base + ((vec - 1) & ~15)
    cases = [("n < 0", dict(n=-1), INV)]
    cases += [("null " + k, {k: None}, INV) for k in ("num", "den", "r", "p")]
    cases += [("null %s with n == 0" % k, {"n": 0, k: None}, INV) for k in ("num", "den", "r", "p")]
    cases += [("vectors of 4 GiB", dict(n=2 ** 32 // es, p=1 << 40, r=4 << 40, minv=5 << 40), INV),
              ("vectors of more than 4 GiB", dict(n=2 ** 31 - 1, p=1 << 40, r=4 << 40, minv=5 << 40), INV)]
    for o in ("r", "minv"):
        cases += [("p == " + o, {o: BASE["p"]}, INV), ("%s begins in the last bytes of p" % o, {o: last(BASE["p"])}, INV),
                  ("%s ends in the first bytes of p" % o, {o: BASE["p"] - ((vec - 1) & ~15)}, INV)]
    for s in ("num", "den"):
        cases += [("%s inside p" % s, {s: BASE["p"] + 8}, INV), ("%s the last double of p" % s, {s: BASE["p"] + ((vec - 8) & ~7)}, INV)]
    cases += [("%s off 16-byte alignment" % k, {k: BASE[k] + off}, ALI) for k in ("r", "minv", "p") for off in (es, 8)]
    cases += [("%s off 8-byte alignment" % k, {k: BASE[k] + 4}, ALI) for k in ("num", "den")]
    for what, over, code in cases:
        rc = _direction(lib, suffix, **over)
        assert rc == code, "%s: %d (%s)" % (what, rc, lib.spmv_hip_last_error())


def test_the_binding_dispatches_on_the_dtype_and_refuses_mixed_or_unknown_ones():
    import numpy as np
    import torch
    # raw addresses need dtype=; the refusal that follows shows which entry point was reached: 2^29 doubles span 4 GiB and are
    # refused for that, 2^29 floats are not, and are refused for the overlap that is looked at next
    with pytest.raises(TypeError):
        capi.cg_direction(4, BASE["num"], BASE["den"], BASE["r"], None, BASE["p"])
    with pytest.raises(TypeError):
        capi.cg_direction(4, BASE["num"], BASE["den"], BASE["r"], None, BASE["p"], dtype=np.int32)
    with pytest.raises(TypeError):
        capi.cg_direction(4, BASE["num"], BASE["den"], torch.zeros(4, dtype=torch.float64), None, torch.zeros(4, dtype=torch.float32))
    big = dict(p=1 << 40, r=4 << 40)
    with pytest.raises(capi.SpmvHipError) as e:
        capi.cg_direction(2 ** 29, BASE["num"], BASE["den"], big["r"], None, big["p"], dtype=np.float64)
    assert e.value.code == INV and "4 GiB" in str(e.value)
    with pytest.raises(capi.SpmvHipError) as e:
        capi.cg_direction(2 ** 29, BASE["num"], BASE["den"], big["p"] + 1024, None, big["p"], dtype=np.float32)
    assert e.value.code == INV and "overlap" in str(e.value)
    with pytest.raises(capi.SpmvHipError) as e:
        capi.cg_step(2 ** 29, BASE["num"], BASE["den"], 1 << 40, 2 << 40, 3 << 40, 4 << 40, None, BASE["dots"], BASE["work"], 1 << 40, dtype="float64")
    assert e.value.code == INV and "4 GiB" in str(e.value)
    # host tensors carry their dtype (nothing runs: n < 0)
    t64, t32 = torch.zeros(4, dtype=torch.float64), torch.zeros(4, dtype=torch.float32)
    for t in (t64, t32):
        with pytest.raises(capi.SpmvHipError) as e:
            capi.cg_step(-1, t64, t64, t, t, t, t, None, t64, t64)
        assert e.value.code == INV and "n < 0" in str(e.value)
