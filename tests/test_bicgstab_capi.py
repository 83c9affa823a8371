"""The C ABI of the BiCGStab updates (include/spmv_hip_bicgstab.h) without a GPU: the six functions are declared, exported and
bound, the header is C99 on its own, include/spmv_hip.h is still the 19-function boundary and the version 130, and every refusal
of the header is given with made-up addresses -- the refusals precede the first HIP call, so nothing is dereferenced and no device
is needed.  The aliasings the header accepts pass the argument check: a workspace one byte too small stops the step before its
launch, and behind the check of its arrays."""
import ctypes as C
import os
import re
import subprocess

import pytest

import bicgstab_cases  # noqa: F401  (no feature, no tests)
from spmv_amd import capi

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
HEADER = os.path.join(INCLUDE, "spmv_hip_bicgstab.h")
S = ["spmv_hip_bicgstab_s_f64", "spmv_hip_bicgstab_s_f32"]
STEPS = ["spmv_hip_bicgstab_step_f64", "spmv_hip_bicgstab_step_f32"]
DIRECTIONS = ["spmv_hip_bicgstab_direction_f64", "spmv_hip_bicgstab_direction_f32"]
NEW = S + STEPS + DIRECTIONS
INV, ALI = capi.ERR_INVALID, capi.ERR_ALIGN


def _code(path):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def test_symbols_exported_declared_and_bound():
    lib = C.CDLL(capi.LIB_PATH)
    text = _code(HEADER)
    declared = sorted(set(re.findall(r"\b(spmv_hip_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(NEW) and len(NEW) == 6
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in capi.SIGNATURES, s
    assert HEADER in [os.path.abspath(h) for h in capi.HEADER_PATHS]
    for m in ("bicgstab_s", "bicgstab_step", "bicgstab_direction"):
        assert callable(getattr(capi, m)), m
    flat = re.sub(r"\s+", " ", text)
    for suffix, t in (("f64", "double"), ("f32", "float")):
        d = {"T": t, "s": suffix}
        assert ("int spmv_hip_bicgstab_s_%(s)s(int32_t n, const double *d_num, const double *d_den, const %(T)s *d_v, %(T)s *d_r, "
                "const %(T)s *d_minv, %(T)s *d_shat, void *stream);" % d) in flat, suffix
        assert ("int spmv_hip_bicgstab_step_%(s)s(int32_t n, const double *d_num_a, const double *d_den_a, const double *d_num_w, "
                "const double *d_den_w, const %(T)s *d_phat, const %(T)s *d_shat, const %(T)s *d_t, const %(T)s *d_rhat, %(T)s *d_x, %(T)s *d_r, "
                "double *d_dots, void *d_work, size_t work_bytes, void *stream);" % d) in flat, suffix
        assert ("int spmv_hip_bicgstab_direction_%(s)s(int32_t n, const double *d_num_r, const double *d_den_r, const double *d_num_a, "
                "const double *d_den_a, const double *d_num_w, const double *d_den_w, const %(T)s *d_r, const %(T)s *d_v, %(T)s *d_p, "
                "const %(T)s *d_minv, %(T)s *d_phat, void *stream);" % d) in flat, suffix
    for s, count, size_at in ((S, 8, None), (STEPS, 15, 13), (DIRECTIONS, 13, None)):
        for name in s:
            args = capi.SIGNATURES[name][1]
            assert len(args) == count and args[0] == C.c_int32 and capi.SIGNATURES[name][0] == C.c_int
            assert [i for i, a in enumerate(args) if a == C.c_size_t] == ([size_at] if size_at else [])
    # the header includes the CG header (the chunk, the workspace query) and defines neither again
    assert '#include "spmv_hip_krylov.h"' in text and "#define SPMV_HIP_KRYLOV_CHUNK" not in text
    assert "SPMV_HIP_KRYLOV_CHUNK (1024)" in open(HEADER).read()


def test_header_is_c99_on_its_own_and_the_boundary_header_keeps_its_19_functions():
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INCLUDE, "-fsyntax-only", "-x", "c", "-"],
                       input='#include "spmv_hip_bicgstab.h"\nint main(void) { return SPMV_HIP_VERSION + SPMV_HIP_KRYLOV_CHUNK; }\n',
                       text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout
    small = _code(capi.HEADER_PATH)
    assert len(set(re.findall(r"\b(spmv_hip_[a-z0-9_]+)\s*\(", small))) == 19
    assert "bicgstab" not in small and "bicgstab" not in _code(os.path.join(INCLUDE, "spmv_hip_krylov.h"))
    assert not re.findall(r"#define SPMV_HIP_VERSION", open(HEADER).read())
    assert capi.load().spmv_hip_version() == 130


# made-up addresses, 16-byte aligned and far apart; the arguments of the three calls by name
N = 5000
SCALARS = ("num_a", "den_a", "num_w", "den_w", "num_r", "den_r")
BASE = {"num_a": 0x10000, "den_a": 0x10008, "num_w": 0x10010, "den_w": 0x10018, "num_r": 0x10020, "den_r": 0x10028,
        "v": 0x100000, "r": 0x200000, "minv": 0x300000, "shat": 0x400000, "phat": 0x500000, "t": 0x600000, "rhat": 0x700000, "x": 0x800000,
        "p": 0x900000, "dots": 0xa00000, "work": 0xb00000}
S_ARGS = ("num_a", "den_a", "v", "r", "minv", "shat")
STEP_ARGS = ("num_a", "den_a", "num_w", "den_w", "phat", "shat", "t", "rhat", "x", "r", "dots", "work")
DIRECTION_ARGS = SCALARS[4:] + SCALARS[:4] + ("r", "v", "p", "minv", "phat")


def _s(lib, suffix, n=N, **over):
    a = dict(BASE, **over)
    return getattr(lib, "spmv_hip_bicgstab_s_" + suffix)(n, *[a[k] for k in S_ARGS], None)


def _step(lib, suffix, n=N, work_bytes=None, **over):
    a = dict(BASE, **over)
    if work_bytes is None:
        work_bytes = capi.krylov_workspace_bytes(n) if n >= 0 else 1 << 20
    return getattr(lib, "spmv_hip_bicgstab_step_" + suffix)(n, *[a[k] for k in STEP_ARGS], work_bytes, None)


def _direction(lib, suffix, n=N, **over):
    a = dict(BASE, **over)
    return getattr(lib, "spmv_hip_bicgstab_direction_" + suffix)(n, *[a[k] for k in DIRECTION_ARGS], None)


def _run(call, lib, suffix, cases):
    for what, over, code in cases:
        rc = call(lib, suffix, **over)
        assert rc == code, "%s: %d (%s)" % (what, rc, lib.spmv_hip_last_error())
        assert lib.spmv_hip_last_error(), what


def _vector_cases(es, scalars, vectors, written, optional, work=False):
    """The refusals every call shares over its scalars, vectors (all of them) and written vectors."""
    vec = N * es
    last = lambda base: base + ((vec - 1) & ~15)  # the last 16 bytes of a vector at base
    far = {k: (i + 1) << 40 for i, k in enumerate(vectors)}
    cases = [("n < 0", dict(n=-1), INV)]
    required = [k for k in scalars + vectors if k not in optional]
    cases += [("null " + k, {k: None}, INV) for k in required]
    cases += [("null %s with n == 0" % k, {"n": 0, k: None}, INV) for k in required]
    big = dict(far, work_bytes=1 << 40) if work else far
    cases += [("vectors of 4 GiB", dict(big, n=2 ** 32 // es), INV), ("vectors of more than 4 GiB", dict(big, n=2 ** 31 - 1), INV)]
    pairs = [(w, o) for w in written for o in vectors if o != w and (o not in written or o > w)]
    cases += [("%s == %s" % (w, o), {o: BASE[w]}, INV) for w, o in pairs]
    cases += [("%s begins in the last bytes of %s" % (o, w), {o: last(BASE[w])}, INV) for w, o in pairs]
    cases += [("%s ends in the first bytes of %s" % (o, w), {o: BASE[w] - ((vec - 1) & ~15)}, INV) for w, o in pairs]
    for s in scalars:
        cases += [("%s inside %s" % (s, k), {s: BASE[k] + 8}, INV) for k in written]
        cases += [("%s the last double of %s" % (s, k), {s: BASE[k] + ((vec - 8) & ~7)}, INV) for k in written]
        cases += [("%s off 8-byte alignment" % s, {s: BASE[s] + 4}, ALI)]
    cases += [("%s off 16-byte alignment" % k, {k: BASE[k] + off}, ALI) for k in vectors for off in (es, 8)]
    return cases


@pytest.mark.parametrize("suffix,es", [("f64", 8), ("f32", 4)])
def test_every_refusal_of_s_precedes_the_first_hip_call(suffix, es):
    lib = capi.load()
    cases = _vector_cases(es, ("num_a", "den_a"), ("v", "r", "minv", "shat"), ("r", "shat"), ("minv", "shat"))
    cases += [("minv without shat", dict(shat=None), INV), ("shat without minv", dict(minv=None), INV),
              ("minv without shat, n == 0", dict(n=0, shat=None), INV)]
    _run(_s, lib, suffix, cases)


@pytest.mark.parametrize("suffix,es", [("f64", 8), ("f32", 4)])
def test_every_refusal_of_the_step_precedes_the_first_hip_call(suffix, es):
    lib = capi.load()
    need = capi.krylov_workspace_bytes(N)
    vec = N * es
    vectors = ("phat", "shat", "t", "rhat", "x", "r")
    cases = _vector_cases(es, SCALARS[:4], vectors, ("x", "r"), ("shat",), work=True)
    cases += [("null dots", dict(dots=None), INV), ("null work", dict(work=None), INV), ("null dots with n == 0", dict(n=0, dots=None), INV),
              ("work_bytes one byte short", dict(work_bytes=need - 1), INV), ("work_bytes 0", dict(work_bytes=0), INV),
              ("work_bytes 15 with n == 0", dict(n=0, work_bytes=15), INV)]
    for k in vectors:
        cases += [("dots inside " + k, {"dots": BASE[k] + 64}, INV), ("dots in the last bytes of " + k, {"dots": BASE[k] + ((vec - 1) & ~15)}, INV),
                  ("the workspace inside " + k, {"work": BASE[k] + 64}, INV), ("the workspace ending inside " + k, {"work": BASE[k] - need + 16}, INV)]
    cases += [("dots inside the workspace", {"dots": BASE["work"] + need - 16}, INV), ("dots == the workspace", {"dots": BASE["work"]}, INV),
              ("the workspace ending inside dots", {"work": BASE["dots"] - need + 16}, INV)]
    for s in SCALARS[:4]:
        cases += [("%s inside dots" % s, {s: BASE["dots"]}, INV), ("%s == dots + 8" % s, {s: BASE["dots"] + 8}, INV),
                  ("%s inside the workspace" % s, {s: BASE["work"] + 8}, INV),
                  ("%s the last double of the workspace" % s, {s: BASE["work"] + need - 8}, INV)]
    cases += [("all four scalars inside dots", {s: BASE["dots"] for s in SCALARS[:4]}, INV)]
    cases += [("%s off 16-byte alignment" % k, {k: BASE[k] + 8}, ALI) for k in ("dots", "work")]
    _run(_step, lib, suffix, cases)


@pytest.mark.parametrize("suffix,es", [("f64", 8), ("f32", 4)])
def test_every_refusal_of_the_direction_precedes_the_first_hip_call(suffix, es):
    lib = capi.load()
    cases = _vector_cases(es, SCALARS, ("r", "v", "p", "minv", "phat"), ("p", "phat"), ("minv", "phat"))
    cases += [("minv without phat", dict(phat=None), INV), ("phat without minv", dict(minv=None), INV),
              ("minv without phat, n == 0", dict(n=0, phat=None), INV)]
    _run(_direction, lib, suffix, cases)


def _text(lib):
    e = lib.spmv_hip_last_error()
    return e.decode() if isinstance(e, bytes) else str(e)


@pytest.mark.parametrize("suffix,es", [("f64", 8), ("f32", 4)])
def test_the_accepted_aliasings_pass_the_argument_check(suffix, es):
    """The step looks at the size of its workspace LAST: with an accepted aliasing and a workspace one byte short, the refusal
    names work_bytes, so the aliasing passed the check of the arrays, and nothing was launched.  s and the direction have no
    workspace: equal scalars are shown at n == 0, where they launch nothing and return 0 (a scalar's eight bytes do not depend on
    n), and equal read-only vectors by ONE refused overlap that the table reaches after the aliased pair (it is walked in the
    order of the arguments): the message names that later pair."""
    lib = capi.load()
    need = capi.krylov_workspace_bytes(N)
    one = {s: BASE["num_a"] for s in SCALARS}
    four = {k: one[k] for k in SCALARS[:4]}
    for over in (four, {"num_w": BASE["num_a"], "den_w": BASE["den_a"]}, {"rhat": BASE["phat"]}, {"t": BASE["phat"], "rhat": BASE["phat"]},
                 {"shat": None}, {"shat": BASE["phat"]}, {"shat": BASE["t"], "rhat": BASE["t"]}, dict(four, rhat=BASE["phat"], shat=None)):
        rc = _step(lib, suffix, work_bytes=need - 1, **over)
        assert rc == INV and "work_bytes" in _text(lib), "%s: %d (%s)" % (over, rc, _text(lib))
    # (the same workspace with an aliasing that is NOT accepted names the arrays, not work_bytes)
    assert _step(lib, suffix, work_bytes=need - 1, rhat=BASE["x"]) == INV and "overlap" in _text(lib)
    assert _s(lib, suffix, n=0, den_a=BASE["num_a"]) == 0 and _s(lib, suffix, n=0, den_a=BASE["num_a"], minv=None, shat=None) == 0
    assert _direction(lib, suffix, n=0, **one) == 0 and _direction(lib, suffix, n=0, minv=None, phat=None, **one) == 0
    for call, over, then, names in ((_s, {"minv": BASE["v"]}, {"den_a": BASE["shat"] + 8}, ("d_shat", "d_den")),
                                    (_direction, {"v": BASE["r"]}, {"den_w": BASE["phat"] + 8}, ("d_phat", "d_den_w")),
                                    (_direction, {"v": BASE["r"], "minv": BASE["r"]}, {"den_w": BASE["phat"] + 8}, ("d_phat", "d_den_w")),
                                    (_direction, {"v": BASE["r"], "minv": None, "phat": None}, {"den_w": BASE["p"] + 8}, ("d_p", "d_den_w"))):
        rc = call(lib, suffix, **dict(over, **then))
        assert rc == INV and "overlap" in _text(lib) and all(k in _text(lib) for k in names), "%s: %d (%s)" % (over, rc, _text(lib))


def test_the_binding_dispatches_on_the_dtype_and_refuses_mixed_or_unknown_ones():
    import numpy as np
    import torch
    B = BASE
    sc = [B[k] for k in SCALARS]
    # raw addresses need dtype=; the refusal that follows shows which entry point was reached: 2^29 doubles span 4 GiB and are
    # refused for that, 2^29 floats are not, and are refused for the overlap that is looked at next
    with pytest.raises(TypeError):
        capi.bicgstab_s(4, sc[0], sc[1], B["v"], B["r"], None, None)
    with pytest.raises(TypeError):
        capi.bicgstab_s(4, sc[0], sc[1], B["v"], B["r"], None, None, dtype=np.int32)
    with pytest.raises(TypeError):
        capi.bicgstab_direction(4, *sc, torch.zeros(4, dtype=torch.float64), B["v"], torch.zeros(4, dtype=torch.float32), None, None)
    with pytest.raises(TypeError):
        capi.bicgstab_step(4, *sc[:4], B["phat"], None, B["t"], B["rhat"], B["x"], B["r"], B["dots"], B["work"], 64)
    big = {k: (i + 1) << 40 for i, k in enumerate(("v", "r", "phat", "t", "rhat", "x", "p"))}
    for dtype, word in ((np.float64, "4 GiB"), (np.float32, "overlap")):
        with pytest.raises(capi.SpmvHipError) as e:
            capi.bicgstab_s(2 ** 29, sc[0], sc[1], big["r"] + 1024, big["r"], None, None, dtype=dtype)
        assert e.value.code == INV and word in str(e.value), dtype
        with pytest.raises(capi.SpmvHipError) as e:
            capi.bicgstab_step(2 ** 29, *sc[:4], big["phat"], None, big["t"], big["x"] + 1024, big["x"], big["r"], B["dots"], B["work"], 1 << 40,
                               dtype=dtype)
        assert e.value.code == INV and word in str(e.value), dtype
        with pytest.raises(capi.SpmvHipError) as e:
            capi.bicgstab_direction(2 ** 29, *sc, big["r"], big["p"] + 1024, big["p"], None, None, dtype=dtype)
        assert e.value.code == INV and word in str(e.value), dtype
    # host tensors carry their dtype (nothing runs: n < 0), and work_bytes defaults to the workspace tensor's size
    t64, t32 = torch.zeros(4, dtype=torch.float64), torch.zeros(4, dtype=torch.float32)
    for t in (t64, t32):
        for call in (lambda: capi.bicgstab_s(-1, t64, t64, t, t, t, t), lambda: capi.bicgstab_step(-1, t64, t64, t64, t64, t, t, t, t, t, t, t64, t64),
                     lambda: capi.bicgstab_direction(-1, t64, t64, t64, t64, t64, t64, t, t, t, t, t)):
            with pytest.raises(capi.SpmvHipError) as e:
                call()
            assert e.value.code == INV and "n < 0" in str(e.value)
