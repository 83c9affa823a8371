"""The GMRES updates (include/spmv_hip_gmres.h) on the MI355X, through capi.gmres_*.

The vectors are held bit for bit to the numpy restatement of the header (gmres_cases.restate_*: every product and sum rounded in
fp64, one cast to float last, vhat from the value as stored).  h and dots[0] are held (a) bit for bit to sums formed in integers
on operands where every order gives the same sum, up to the two sizes around the reduction's second stage, (b) on general
operands to n 2^-53 sum |t_i| of math.fsum(t), and (c) bit for bit to each other across k, the position in the basis and
spmv_hip_cg_step_*: the order is a function of n alone.  The small calls are held to the restatement within the bounds of
gmres_cases.column_bound / solve_residual_and_bound.  Every device array, the padding between the basis vectors, the scalars, d_h,
the dots, the state and the workspace lie between or hold NaN guards that are checked whenever an array is read back."""
import functools
import math

import numpy as np
import pytest

import gmres_cases as gc
import stream_helpers as sh
from spmv_amd import capi
from test_gpu_bicgstab import _ChainHost
from test_gpu_dots import _same_dots
from test_gpu_krylov import CASES, IDS, Band, _torch_dtype
from test_gpu_scaled import Dev, _alternate, _bits

pytestmark = pytest.mark.gpu
DTYPES = [np.float64, np.float32]
DIDS = ["f64", "f32"]


class Arrays:
    """One case on the device: the basis with w behind it in ONE band (the padding NaN), h (k + 1), the coefficients of the
    update and of the correction (k each), dots, the workspace, a scale, x, minv and vhat."""

    def __init__(self, case, with_minv=True, k_max=None):
        self.c, self.n, self.k, self.dtype, self.ldv = case, case.n, case.k, case.dtype, case.ldv
        self.es = self.dtype.itemsize
        self.basis = Band(case.basis, self.dtype)
        self.h = Band(np.full(self.k + 1, np.nan))
        self.coef, self.y = Band(case.h), Band(case.y)
        self.bytes = capi.gmres_workspace_bytes(self.n, self.k if k_max is None else k_max)
        self.dots, self.work = Band(np.full(2, np.nan)), Band(np.full(self.bytes // 8, np.nan))
        self.scale = Band([0.625])
        self.x = Band(case.x, self.dtype)
        self.minv = Band(case.minv, self.dtype) if with_minv else None
        self.vhat = Band(np.full(self.n, np.nan), self.dtype) if with_minv else None

    @property
    def V(self):
        return self.basis.ptr if self.k else None

    @property
    def w(self):
        return self.basis.ptr + self.k * self.ldv * self.es

    def vec(self, j):
        return self.basis.ptr + j * self.ldv * self.es

    def reset(self):
        self.basis.set(self.c.basis)
        self.x.set(self.c.x)

    def project(self, stream=0, fill=True, **o):
        if fill:
            self.h.fill()
            self.work.fill()
        a = dict(n=self.n, k=self.k, V=self.V, w=self.w, h=self.h.ptr, work=self.work.ptr, work_bytes=self.bytes, ldv=self.ldv)
        a.update(o)
        capi.gmres_project(a["n"], a["k"], a["V"], a["ldv"], a["w"], a["h"], a["work"], a["work_bytes"], stream, dtype=self.dtype)

    def update(self, stream=0, fill=True, **o):
        if fill:
            self.dots.fill()
            self.work.fill()
        a = dict(n=self.n, k=self.k, V=self.V, w=self.w, h=self.coef.ptr, dots=self.dots.ptr, work=self.work.ptr, work_bytes=self.bytes,
                 ldv=self.ldv)
        a.update(o)
        capi.gmres_update(a["n"], a["k"], a["V"], a["ldv"], a["h"], a["w"], a["dots"], a["work"], a["work_bytes"], stream, dtype=self.dtype)

    def scale_w(self, stream=0, **o):
        if self.vhat:
            self.vhat.fill()
        a = dict(n=self.n, scale=self.scale.ptr, v=self.w, minv=self.minv.ptr if self.minv else None, vhat=self.vhat.ptr if self.vhat else None)
        a.update(o)
        capi.gmres_scale(a["n"], a["scale"], a["v"], a["minv"], a["vhat"], stream, dtype=self.dtype)

    def correct(self, stream=0, **o):
        a = dict(n=self.n, k=self.k, V=self.V, y=self.y.ptr, minv=self.minv.ptr if self.minv else None, x=self.x.ptr, ldv=self.ldv)
        a.update(o)
        capi.gmres_correct(a["n"], a["k"], a["V"], a["ldv"], a["y"], a["minv"], a["x"], stream, dtype=self.dtype)

    def get_basis(self, what):
        """(the k vectors, w) as stored; the padding between them must still be NaN."""
        b = self.basis.body(what + ", the basis").reshape(self.k + 1, self.ldv)
        assert np.all(np.isnan(b[:, self.n:])), what + ": the padding between the vectors was written"
        return [b[j, :self.n].copy() for j in range(self.k)], b[self.k, :self.n].copy()

    def read(self, band, what):
        self.work.body(what + ", the workspace")
        return band.body(what)

    def all_four(self, what):
        """project, update, scale, correct on the null stream, each read back behind its call."""
        out = {}
        self.project()
        out["h"] = self.read(self.h, what + ", h")
        V, w = self.get_basis(what + ", behind project")
        for j in range(self.k):
            _same(V[j], self.c.V[j], what + ": project changed vector %d" % j)
        _same(w, self.c.w, what + ": project changed w")
        self.update()
        out["dots"] = self.read(self.dots, what + ", dots")
        V, out["w"] = self.get_basis(what + ", behind update")
        for j in range(self.k):
            _same(V[j], self.c.V[j], what + ": update changed vector %d" % j)
        self.scale_w()
        out["v"] = self.get_basis(what + ", behind scale")[1]
        out["vhat"] = self.vhat.body(what + ", vhat") if self.vhat else None
        self.correct()
        out["x"] = self.x.body(what + ", x")
        _same(self.coef.body(what), self.c.h, what + ": the update's coefficients changed")
        _same_dots(self.y.body(what), self.c.y, what + ": y changed")
        if self.minv:
            _same(self.minv.body(what), self.c.minv, what + ": minv changed")
        return out


def _same(got, want, what):
    """NaN where the restatement has NaN (a NaN's sign and payload are the unit's own), every other element bit for bit."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what + ": NaN elsewhere than the restatement has it"
    assert got[~nan].tobytes() == want[~nan].tobytes(), what + ": not bit for bit"


def _ulp(got, want, what):
    """sqrt is allowed 1 ulp, and the quotient behind it one rounding of its own."""
    assert abs(got - want) <= 2.0 ** -52 * abs(want), "%s: %r against %r" % (what, got, want)


def _within(got, t, what):
    want, b = math.fsum(t), gc.bound(t)
    assert abs(got - want) <= b, "%s: %r, fsum of the products %r, bound %.3e" % (what, got, want, b)


# ---- 1 and 3: general operands: the vectors bit for bit, h and dots within the bound ----------------------------------------------------

@functools.lru_cache(maxsize=None)
def _general_runs(dtype, with_minv):
    runs = []
    for n, k in gc.small_cases():
        case = gc.general_case(n, k, dtype)
        tag = "n %d, k %d, %s, minv %s" % (n, k, np.dtype(dtype).name, with_minv)
        runs.append((tag, case, Arrays(case, with_minv).all_four(tag)))
    return runs


@pytest.mark.parametrize("dtype,with_minv", CASES, ids=IDS)
def test_w_v_vhat_and_x_are_the_restatement_bit_for_bit(dtype, with_minv):
    for tag, case, out in _general_runs(dtype, with_minv):
        assert out["w"].dtype == dtype and out["x"].dtype == dtype
        _bits(out["w"], gc.restate_update(case.V, case.h, case.w, dtype), tag + ": w")
        v, vhat = gc.restate_scale(0.625, out["w"], case.minv if with_minv else None, dtype)
        _bits(out["v"], v, tag + ": v")
        assert (vhat is None) == (out["vhat"] is None)
        if with_minv:
            _bits(out["vhat"], vhat, tag + ": vhat")
        _bits(out["x"], gc.restate_correct(case.V, case.y, case.minv if with_minv else None, case.x, dtype), tag + ": x")


@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
def test_h_and_dots_of_general_operands_are_within_the_bound(dtype):
    for tag, case, out in _general_runs(dtype, True):
        for j, t in enumerate(gc.project_products(case.V, case.w)):
            _within(out["h"][j], t, "%s: h[%d]" % (tag, j))
        wd = out["w"].astype(np.float64)
        _within(out["dots"][0], wd * wd, tag + ": dots[0]")
        assert out["dots"][1] == 0.0 and not np.signbit(out["dots"][1]), tag + ": dots[1] is not +0.0"


# ---- 2: integer operands: the integer sums bit for bit -----------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
@pytest.mark.parametrize("cases", [gc.small_cases(), [(gc.BIG_SIZES[0], gc.BIG_K)], [(gc.BIG_SIZES[1], gc.BIG_K)]],
                         ids=["small", "one_stage", "two_stages"])
def test_h_and_dots_of_integer_operands_are_the_integer_sums_bit_for_bit(cases, dtype):
    for n, k in cases:
        ops = gc.int_case(n, k)
        h, w4, d0 = ops.sums()
        dev = Arrays(ops.case(dtype), False)
        tag = "n %d, k %d, %s" % (n, k, np.dtype(dtype).name)
        dev.project()
        _same_dots(dev.read(dev.h, tag), h, tag + ": h")
        dev.update()
        got = dev.read(dev.dots, tag)
        assert np.array_equal(dev.get_basis(tag)[1].astype(np.float64) * 4, w4), tag + ": w"
        _same_dots(got, [d0, 0.0], tag + ": dots")


# ---- 4: the order is a function of n alone -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
def test_h_does_not_depend_on_k_or_the_position_and_equals_the_cg_steps_dots(dtype):
    # 17 vectors and w are cut into register blocks of 6, 6, 6; 7 and w into one of 8; 32 and w into 7, 7, 7, 6, 6; V_j alone
    # shares a block of 2 with w
    cases = [(n, 2 * gc.BLOCK + 1) for n in [s for s in gc.SIZES if s] + [8 * gc.CHUNK + 3]]
    cases += [(n, k) for n in (gc.CHUNK + 1, 2 * gc.CHUNK + 7) for k in (gc.BLOCK - 1, gc.GMRES_MAX_BASIS)]
    for n, k in cases:
        case = gc.general_case(n, k, dtype) if n <= 4 * gc.CHUNK + 1 else gc.Case(
            n, k, dtype, *[np.random.default_rng(n).standard_normal(s) for s in ((k, n), n, k, k, n)], np.ones(n))
        dev = Arrays(case, False)
        tag = "n %d, k %d, %s" % (n, k, np.dtype(dtype).name)
        dev.project()
        h = dev.read(dev.h, tag)
        for j in range(k):  # V_j alone, as the only vector of a call
            dev.project(k=1, V=dev.vec(j))
            one = dev.read(dev.h, tag)
            assert one[0].tobytes() == h[j].tobytes(), "%s: h[%d] over %d vectors %r, over V_%d alone %r" % (tag, j, k, h[j], j, one[0])
            assert one[1].tobytes() == h[k].tobytes(), tag + ": w' w depends on k"
        # the CG step's r' r of the same vector: num -> 0.0, den -> 1.0 over zeroed p and q
        zero, x, nd, dots = Band(np.zeros(n), dtype), Band(np.zeros(n), dtype), Band([0.0, 1.0]), Band(np.full(2, np.nan))
        kwork = Band(np.full(capi.krylov_workspace_bytes(n) // 8, np.nan))
        capi.cg_step(n, nd.ptr, nd.ptr + 8, zero.ptr, zero.ptr, x.ptr, dev.w, None, dots.ptr, kwork.ptr, kwork.nbytes, 0, dtype=dtype)
        step = dots.body(tag)
        assert step[0].tobytes() == h[k].tobytes(), "%s: h[k] %r, the CG step's dots[0] %r" % (tag, h[k], step[0])
        dev.update(k=0, V=None)  # leaves w as it is
        assert dev.read(dev.dots, tag)[0].tobytes() == step[0].tobytes(), tag + ": the update's dots[0] is not the CG step's"
        _bits(dev.get_basis(tag)[1], case.w, tag + ": an update over no vector changed w")


# ---- 5: two runs, a delayed non-blocking stream, two streams at once -----------------------------------------------------------------------

@pytest.fixture(scope="module")
def side():
    s = sh.Side()
    yield s
    s.report()


N_STREAMS, K_STREAMS = 3 * gc.CHUNK + 7, gc.BLOCK + 3


def _pass(n, k, ldv, es, basis, h, dots, work, bytes_, scale, minv, vhat, y, x, stream, dtype):
    """project, update with what it stored, scale, correct: one chained pass over one set of addresses."""
    V, w = basis, basis + k * ldv * es
    capi.gmres_project(n, k, V, ldv, w, h, work, bytes_, stream, dtype=dtype)
    capi.gmres_update(n, k, V, ldv, h, w, dots, work, bytes_, stream, dtype=dtype)
    capi.gmres_scale(n, scale, w, minv, vhat, stream, dtype=dtype)
    capi.gmres_correct(n, k, V, ldv, y, minv, x, stream, dtype=dtype)


@pytest.mark.parametrize("dtype,with_minv", CASES, ids=IDS)
def test_two_runs_a_delayed_stream_and_two_streams_at_once_give_identical_bits(side, dtype, with_minv):
    import torch
    n, k = N_STREAMS, K_STREAMS
    rng = np.random.default_rng(91)
    case = gc.Case(n, k, dtype, rng.standard_normal((k, n)), rng.standard_normal(n), np.zeros(k), rng.standard_normal(k),
                   rng.standard_normal(n), rng.uniform(0.5, 2.0, size=n))
    tag = "%s, minv %s" % (np.dtype(dtype).name, with_minv)
    es, ldv = case.dtype.itemsize, case.ldv

    def run(dev, stream=0):
        _pass(n, k, ldv, es, dev.basis.ptr, dev.h.ptr, dev.dots.ptr, dev.work.ptr, dev.bytes, dev.scale.ptr, dev.minv.ptr if dev.minv else None,
              dev.vhat.ptr if dev.vhat else None, dev.y.ptr, dev.x.ptr, stream, dtype)

    def state(dev, what):
        out = {"basis": dev.basis.body(what), "h": dev.h.body(what), "dots": dev.dots.body(what), "x": dev.x.body(what)}
        if dev.vhat:
            out["vhat"] = dev.vhat.body(what)
        dev.work.body(what)
        return out

    def same(got, want, what):
        for key in want:
            _same(got[key], want[key], "%s: %s" % (what, key))

    dev = Arrays(case, with_minv)
    run(dev)
    first = state(dev, tag)
    V, w = [first["basis"].reshape(k + 1, ldv)[j, :n] for j in range(k)], first["basis"].reshape(k + 1, ldv)[k, :n]
    for j, t in enumerate(gc.project_products(case.V, case.w)):
        _within(first["h"][j], t, "%s: h[%d]" % (tag, j))
    updated = gc.restate_update(case.V, first["h"][:k], case.w, dtype)
    v, vhat = gc.restate_scale(0.625, updated, case.minv if with_minv else None, dtype)
    _bits(w, v, tag + ": the chained pass, w")
    _bits(first["x"], gc.restate_correct(V, case.y, case.minv if with_minv else None, case.x, dtype), tag + ": the chained pass, x")
    dev.reset()
    dev.h.fill()
    dev.dots.fill()
    dev.work.fill()
    run(dev)
    same(state(dev, tag), first, tag + ": a second run")
    # behind the delay on a non-blocking stream
    ro = {"scale": sh.operand(np.array([0.625])), "y": sh.operand(case.y)}
    if with_minv:
        ro["minv"] = sh.operand(case.minv)
    rw = {"basis": sh.result(np.nan_to_num(case.basis, nan=0.0)), "h": sh.result(np.zeros(k + 1)), "dots": sh.result(np.zeros(2)),
          "work": sh.result(np.zeros(dev.bytes // 8)), "x": sh.result(case.x)}
    if with_minv:
        rw["vhat"] = sh.result(np.zeros(n, dtype=dtype))
    for a in list(ro.values()) + list(rw.values()):
        assert a.ptr % 16 == 0

    def call(stream):
        _pass(n, k, ldv, es, rw["basis"].ptr, rw["h"].ptr, rw["dots"].ptr, rw["work"].ptr, dev.bytes, ro["scale"].ptr,
              ro["minv"].ptr if with_minv else None, rw["vhat"].ptr if with_minv else None, ro["y"].ptr, rw["x"].ptr, stream, dtype)

    keys = [key for key in ("basis", "h", "dots", "x", "vhat") if key in rw]
    bodies, _ = sh.delayed(side, list(ro.values()) + list(rw.values()), call, [rw[key] for key in keys], "a GMRES pass behind the delay (%s)" % tag)
    got = dict(zip(keys, bodies))
    pad = np.isnan(case.basis)
    assert np.all(got["basis"][pad] == 0.0), tag + ": the padding was written behind the delay"
    got["basis"][pad] = np.nan
    same(got, first, tag + ": behind the delay")
    # two streams at once, a workspace (and every written array) each
    own = [Arrays(case, with_minv) for _ in side.streams]
    torch.cuda.synchronize()
    for s, d in zip(side.streams, own):
        run(d, s.cuda_stream)
    for s in side.streams:
        s.synchronize()
    for d in own:
        same(state(d, tag + ", two streams"), first, tag + ": two streams at once")


# ---- 6: NaN and +-Inf stay where numpy has them ---------------------------------------------------------------------------------------------

def _classes(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what + ": NaN elsewhere than numpy has it"
    assert np.array_equal(np.isposinf(got), np.isposinf(want)) and np.array_equal(np.isneginf(got), np.isneginf(want)), what + ": Inf"
    fin = np.isfinite(want)
    assert np.array_equal(got[fin], want[fin]), what + ": a finite element changed"


@pytest.mark.parametrize("dtype,with_minv", CASES, ids=IDS)
def test_nan_and_inf_in_one_element_stay_in_their_sum_or_their_element(dtype, with_minv):
    n, k = gc.CHUNK + 1, gc.BLOCK + 1
    base = gc.general_case(n, k, dtype)
    mh = (lambda c: c.minv) if with_minv else (lambda c: None)
    for bad in (np.nan, np.inf, -np.inf):
        for where, j, i in (("V", 2, 5), ("V", k - 1, n - 1), ("w", None, 700), ("minv", None, n - 1), ("h", 3, None)):
            V, w, minv, h = [v.copy() for v in base.V], base.w.copy(), base.minv.copy(), base.h.copy()
            if where == "V":
                V[j][i] = bad
            elif where == "w":
                w[i] = bad
            elif where == "minv":
                minv[i] = bad
            else:
                h[j] = bad
            case = gc.Case(n, k, dtype, V, w, h, base.y, base.x, minv)
            tag = "%r in %s[%s][%s], %s, minv %s" % (bad, where, j, i, np.dtype(dtype).name, with_minv)
            out = Arrays(case, with_minv).all_four(tag)
            with np.errstate(invalid="ignore", over="ignore"):
                sums = [float(np.sum(t)) for t in gc.project_products(case.V, case.w)]
            finite = np.isfinite(sums)
            _classes(np.where(finite, 0.0, out["h"]), np.where(finite, 0.0, sums), tag + ": h")  # confined to that vector's h[j]
            assert np.all(np.isfinite(out["h"][finite])), tag + ": a non-finite h[j] of a finite vector"
            want_w = gc.restate_update(case.V, case.h, case.w, dtype)
            _same(out["w"], want_w, tag + ": w")
            v, vhat = gc.restate_scale(0.625, out["w"], mh(case), dtype)
            _same(out["v"], v, tag + ": v")
            if with_minv:
                _same(out["vhat"], vhat, tag + ": vhat")
            _same(out["x"], gc.restate_correct(case.V, case.y, mh(case), case.x, dtype), tag + ": x")
            expected_bad = {"V": 1, "w": 1, "minv": 0, "h": n}[where]
            assert int(np.sum(~np.isfinite(out["w"].astype(np.float64)))) == expected_bad, tag + ": not confined to its element"
    # state[1] = 1 / 0 goes through scale as IEEE has it: +-Inf, and NaN where the element is zero
    case = gc.general_case(n, 0, dtype)
    dev = Arrays(case, with_minv)
    zeroed = case.w.copy()
    zeroed[[0, n - 1]] = 0.0
    dev.basis.set(np.concatenate([zeroed, case.basis[n:]]))
    state = Band(np.full(gc.state_doubles(4), np.nan))
    nrm2 = Band([0.0])
    capi.gmres_start(4, nrm2.ptr, state.ptr)
    assert state.body("start of a zero norm")[1] == np.inf
    dev.scale_w(scale=state.ptr + 8)
    got = dev.get_basis("1 / 0")[1].astype(np.float64)
    with np.errstate(invalid="ignore"):
        _classes(got, zeroed.astype(np.float64) * np.inf, "v scaled by 1 / 0")


# ---- 7: refusals write nothing; the accepted placements run ----------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
def test_refusals_on_device_arrays_write_nothing(dtype):
    n, k = 2 * gc.CHUNK + 7, 5
    case = gc.general_case(n, k, dtype)
    dev = Arrays(case, True)
    es = dev.es
    for b in (dev.h, dev.dots, dev.work, dev.vhat):
        b.fill()
    bands = [dev.basis, dev.h, dev.coef, dev.y, dev.dots, dev.work, dev.scale, dev.x, dev.minv, dev.vhat]
    before = [b.snap() for b in bands]
    INV, ALI = capi.ERR_INVALID, capi.ERR_ALIGN
    refusals = [(dev.project, dict(n=-1), INV), (dev.project, dict(k=33), INV), (dev.project, dict(w=None), INV),
                (dev.project, dict(ldv=n - 16 // es), INV), (dev.project, dict(ldv=dev.ldv + 1), INV), (dev.project, dict(work_bytes=dev.bytes - 1), INV),
                (dev.project, dict(h=dev.h.ptr + 8), ALI), (dev.project, dict(h=dev.w + 16), INV), (dev.project, dict(work=dev.basis.ptr), INV),
                (dev.update, dict(w=dev.vec(k - 1)), INV), (dev.update, dict(w=dev.w + es), ALI), (dev.update, dict(h=dev.w + 32), INV),
                (dev.update, dict(dots=dev.w), INV), (dev.update, dict(work_bytes=15), INV), (dev.update, dict(V=None), INV),
                (dev.scale_w, dict(minv=None), INV), (dev.scale_w, dict(vhat=None), INV), (dev.scale_w, dict(scale=dev.w + 8), INV),
                (dev.scale_w, dict(scale=dev.scale.ptr + 4), ALI), (dev.scale_w, dict(vhat=dev.w), INV),
                (dev.correct, dict(x=dev.vec(1)), INV), (dev.correct, dict(y=dev.x.ptr + 16), INV), (dev.correct, dict(k=-1), INV),
                (dev.correct, dict(minv=dev.x.ptr), INV)]
    for call, over, code in refusals:
        with pytest.raises(capi.SpmvHipError) as e:
            call(fill=False, **over) if call in (dev.project, dev.update) else call(**over)
        assert e.value.code == code, (over, e.value)
    for b, snap in zip(bands, before):
        assert np.array_equal(b.snap().cpu().numpy().view(np.uint8), snap.cpu().numpy().view(np.uint8)), "a refused call wrote"
    # w directly behind the basis is what every test here runs; a w elsewhere gives the same bits
    out = dev.all_four("w behind the basis")
    apart = Band(case.w, dtype)
    dev.reset()
    dev.project(w=apart.ptr)
    _same_dots(dev.read(dev.h, "w apart"), out["h"], "h with w apart from the basis")
    dev.update(w=apart.ptr)
    _bits(apart.body("w apart"), out["w"], "w apart from the basis")
    _same_dots(dev.read(dev.dots, "w apart"), out["dots"], "dots with w apart")


# ---- 8: one vector pair 4 GiB apart ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
def test_two_vectors_more_than_4_gib_apart(dtype):
    import torch
    n, k = gc.CHUNK + 1, 2
    es = np.dtype(dtype).itemsize
    ldv = (2 ** 32 + 16) // es
    assert ldv * es == 2 ** 32 + 16
    guard = 64
    try:
        big = torch.empty(ldv + n + 2 * guard, dtype=_torch_dtype(dtype), device="cuda:0")
    except RuntimeError as e:  # the allocation, nothing else
        pytest.skip("no room for a basis of %.1f GiB: %s" % ((ldv + n) * es / 2.0 ** 30, str(e)[:80]))
    case = gc.general_case(n, k, dtype)
    for j in range(k):  # only the used parts, NaN around each
        at = guard + j * ldv
        big[at - guard:at + n + guard] = float("nan")
        big[at:at + n] = torch.from_numpy(case.V[j]).to("cuda:0")
    V = big.data_ptr() + guard * es
    assert V % 16 == 0
    w, x, h, coef, y = Band(case.w, dtype), Band(case.x, dtype), Band(np.full(k + 1, np.nan)), Band(case.h), Band(case.y)
    bytes_ = capi.gmres_workspace_bytes(n, k)
    work, dots = Band(np.full(bytes_ // 8, np.nan)), Band(np.full(2, np.nan))
    capi.gmres_project(n, k, V, ldv, w.ptr, h.ptr, work.ptr, bytes_, dtype=dtype)
    got = h.body("4 GiB apart")
    for j, t in enumerate(gc.project_products(case.V, case.w)):
        _within(got[j], t, "4 GiB apart: h[%d]" % j)
    small = Arrays(case, False)
    small.project()
    _same_dots(got, small.read(small.h, "the same vectors side by side"), "h of vectors 4 GiB apart against the same side by side")
    capi.gmres_update(n, k, V, ldv, coef.ptr, w.ptr, dots.ptr, work.ptr, bytes_, dtype=dtype)
    _bits(w.body("4 GiB apart"), gc.restate_update(case.V, case.h, case.w, dtype), "4 GiB apart: w")
    capi.gmres_correct(n, k, V, ldv, y.ptr, None, x.ptr, dtype=dtype)
    _bits(x.body("4 GiB apart"), gc.restate_correct(case.V, case.y, None, case.x, dtype), "4 GiB apart: x")
    work.body("4 GiB apart")
    for j in range(k):
        at = guard + j * ldv
        part = big[at - guard:at + n + guard].cpu().numpy()
        assert np.all(np.isnan(part[:guard])) and np.all(np.isnan(part[guard + n:])), "written around vector %d" % j
        _bits(part[guard:guard + n], case.V[j], "vector %d changed" % j)
    del big


# ---- 9: start, column, solve against the restatement ------------------------------------------------------------------------------------------

def _check_column(got, before, k, m, h1, h2, nrm2, what):
    """The state after column k against the restatement from the state BEFORE it, within column_bound."""
    lay = capi.gmres_state_layout(m)
    want = gc.restate_column(before, k, m, h1, h2, nrm2)
    h = [float(h1[j]) + float(h2[j]) for j in range(k + 1)]
    b = gc.column_bound(k, h, math.sqrt(nrm2), before[lay["g"] + k])
    r = lay["r"] + k * (k + 1) // 2
    for name, lo, hi in (("R", r, r + k + 1), ("g", lay["g"] + k, lay["g"] + k + 2), ("state[0]", 0, 1)):
        err = np.max(np.abs(got[lo:hi] - want[lo:hi]))
        assert err <= b, "%s: %s off by %.3e, bound %.3e" % (what, name, err, b)
    c, s = got[lay["c"] + k], got[lay["s"] + k]  # two quotients by one rounded norm: a rotation to a few roundings
    assert abs(c * c + s * s - 1.0) <= 16 * 2.0 ** -53 and s > 0, "%s: c %r, s %r" % (what, c, s)
    _ulp(got[1], 1.0 / math.sqrt(nrm2), what + ": state[1]")
    untouched = np.ones(len(got), dtype=bool)
    for lo, hi in ((0, 2), (lay["g"] + k, lay["g"] + k + 2), (lay["c"] + k, lay["c"] + k + 1), (lay["s"] + k, lay["s"] + k + 1), (r, r + k + 1)):
        untouched[lo:hi] = False
    assert np.array_equal(got[untouched], np.asarray(before)[untouched], equal_nan=True), what + ": written outside column %d" % k


def _check_start(got, want, m, what):
    g = capi.gmres_state_layout(m)["g"]
    _ulp(got[0], want[0], what + ": state[0]")
    _ulp(got[1], want[1], what + ": state[1]")
    assert got[g] == got[0] and np.all(got[g + 1:g + m + 1] == 0.0) and not np.any(np.signbit(got[g + 1:g + m + 1])), what + ": g is not beta e_1"
    assert np.array_equal(got[g + m + 1:], want[g + m + 1:], equal_nan=True), what + ": written behind g"


def _check_solve(state, k, m, y, what):
    resid, bnd = gc.solve_residual_and_bound(state, k, m, y)
    for i, (r, b) in enumerate(zip(resid, bnd)):
        assert r <= b, "%s: row %d, |R y - g| %.3e, bound %.3e" % (what, i, float(r), float(b))


@pytest.mark.parametrize("m", [1, 8, 32])
def test_start_column_and_solve_are_the_restatement_within_the_bounds(m):
    rng = np.random.default_rng(m)
    lay = capi.gmres_state_layout(m)
    count = capi.gmres_state_doubles(m)
    state, nrm2 = Band(np.full(count, np.nan)), Band([7.25])
    capi.gmres_start(m, nrm2.ptr, state.ptr)
    got = state.body("start")
    want = gc.restate_start(m, 7.25)
    _check_start(got, want, m, "start")
    for k in range(m):
        h = rng.standard_normal(k + 2)
        h[k + 1] = abs(h[k + 1]) + 0.25
        h1 = h[:k + 1] * 0.75
        hb1, hb2 = Band(np.concatenate([h1, [np.nan] * ((k + 1) % 2)])), Band(np.concatenate([h[:k + 1] - h1, [np.nan] * ((k + 1) % 2)]))
        nb = Band([h[k + 1] ** 2, np.nan])
        before = state.body("column %d" % k)
        capi.gmres_column(k, m, hb1.ptr, hb2.ptr, nb.ptr, state.ptr)
        _check_column(state.body("column %d" % k), before, k, m, h1, h[:k + 1] - h1, h[k + 1] ** 2, "m %d, column %d" % (m, k))
        for kk in {k + 1, (k + 1) // 2}:
            y = Band(np.full(kk + kk % 2, np.nan))
            snap = state.body("solve")
            capi.gmres_solve(kk, m, state.ptr, y.ptr)
            _check_solve(snap, kk, m, y.body("solve")[:kk], "m %d, solve %d" % (m, kk))
            assert np.all(np.isnan(y.body("solve")[kk:])) and np.array_equal(state.body("solve"), snap, equal_nan=True)
    assert lay["r"] + m * (m + 1) // 2 <= count


# ---- 10 and 11: the chain -------------------------------------------------------------------------------------------------------------------

class Chain:
    """Right-preconditioned GMRES(m) on the upwind operator as the header composes it: one Arnoldi step as seven enqueue-only
    calls, the end of a cycle as five."""

    def __init__(self, dtype, with_minv, m):
        self.dtype, self.with_minv, self.m = np.dtype(dtype), with_minv, m
        self.h = _ChainHost()
        self.kind = "c16_f64" if dtype == np.float64 else "c16_f32xy"
        self.mdev = Dev(self.h, self.kind)
        plan = self.mdev.plan
        self.multiply = plan.spmv_f64_scaled_dots if dtype == np.float64 else plan.spmv_f32xy_scaled_dots
        self.n = n = self.h.rows
        self.es, self.ldv = self.dtype.itemsize, gc.ldv_of(n, dtype)
        self.mh = self.h.minv.astype(dtype) if with_minv else None
        self.bands = {"basis": Band(np.full((m + 1) * self.ldv, np.nan), dtype), "x": Band(np.zeros(n), dtype), "b": Band(self.h.b, dtype)}
        if with_minv:
            self.bands["vhat"] = Band(np.full(n, np.nan), dtype)
        self.minv = Band(self.mh, dtype) if with_minv else None
        for key, count in (("h1", m + 2), ("h2", m + 2), ("dots", 2), ("rr", 2), ("mdots", 2), ("y", m + m % 2), ("state", capi.gmres_state_doubles(m))):
            self.bands[key] = Band(np.full(count, np.nan))
        self.gbytes, self.mbytes = capi.gmres_workspace_bytes(n, m), plan.dots_workspace_bytes()
        self.gwork, self.mwork = Band(np.full(self.gbytes // 8, np.nan)), Band(np.full(self.mbytes // 8, np.nan))

    def ptr(self, key):
        return self.bands[key].ptr

    def vec(self, j):
        return self.ptr("basis") + j * self.ldv * self.es

    def reset(self):
        for key, b in self.bands.items():
            if key != "b":
                b.fill(0.0 if key == "x" else float("nan"))

    def _mult(self, x, alpha, beta, y_in, y_out, dots):
        d = self.mdev
        return lambda s: self.multiply(d.tp.data_ptr(), d.ac, d.av, x, alpha, beta, y_in, y_out, None, dots, self.mwork.ptr, self.mbytes, s)

    def _scale(self, j):
        return lambda s: capi.gmres_scale(self.n, self.ptr("state") + 8, self.vec(j), self.minv.ptr if self.minv else None,
                                          self.ptr("vhat") if self.with_minv else None, s, dtype=self.dtype)

    def restart(self):
        """r = b - A x into V_0 with r' r, the state, V_0 scaled."""
        return [("residual", self._mult(self.ptr("x"), -1.0, 1.0, self.ptr("b"), self.vec(0), self.ptr("rr"))),
                ("start", lambda s: capi.gmres_start(self.m, self.ptr("rr"), self.ptr("state"), s)),
                ("scale 0", self._scale(0))]

    def step(self, k):
        n, dt, V, ldv, w = self.n, self.dtype, self.ptr("basis"), self.ldv, self.vec(k + 1)
        src = self.ptr("vhat") if self.with_minv else self.vec(k)
        gw, gb = self.gwork.ptr, self.gbytes
        return [("multiply %d" % k, self._mult(src, 1.0, 0.0, None, w, self.ptr("mdots"))),
                ("project1 %d" % k, lambda s: capi.gmres_project(n, k + 1, V, ldv, w, self.ptr("h1"), gw, gb, s, dtype=dt)),
                ("update1 %d" % k, lambda s: capi.gmres_update(n, k + 1, V, ldv, self.ptr("h1"), w, self.ptr("dots"), gw, gb, s, dtype=dt)),
                ("project2 %d" % k, lambda s: capi.gmres_project(n, k + 1, V, ldv, w, self.ptr("h2"), gw, gb, s, dtype=dt)),
                ("update2 %d" % k, lambda s: capi.gmres_update(n, k + 1, V, ldv, self.ptr("h2"), w, self.ptr("dots"), gw, gb, s, dtype=dt)),
                ("column %d" % k, lambda s: capi.gmres_column(k, self.m, self.ptr("h1"), self.ptr("h2"), self.ptr("dots"), self.ptr("state"), s)),
                ("scale %d" % (k + 1), self._scale(k + 1))]

    def finish(self):
        m = self.m
        return [("solve", lambda s: capi.gmres_solve(m, m, self.ptr("state"), self.ptr("y"), s)),
                ("correct", lambda s: capi.gmres_correct(self.n, m, self.ptr("basis"), self.ldv, self.ptr("y"), self.minv.ptr if self.minv else None,
                                                         self.ptr("x"), s, dtype=self.dtype))]

    def cycle(self):
        """The calls of one cycle behind a restart, and the restart of the next."""
        return [c for k in range(self.m) for c in self.step(k)] + self.finish() + self.restart()

    def snap(self):
        return {key: b.snap() for key, b in self.bands.items()}

    def bodies(self, snap, what):
        return {key: self.bands[key].body(what, snap[key]) for key in self.bands}

    def close(self):
        self.mdev.close()


def _vectors(st, ch, count):
    b = st["basis"].reshape(ch.m + 1, ch.ldv)
    return [b[j, :ch.n] for j in range(count)]


def _check_multiply(ch, xin, alpha, beta, y_in, got, what):
    h = ch.h
    values = h.values(ch.kind).astype(np.float64)
    prod = values * xin.astype(np.float64)[h.c]
    z, scale = np.add.reduceat(prod, h.p[:-1].astype(np.int64)), np.add.reduceat(np.abs(prod), h.p[:-1].astype(np.int64))
    ref = alpha * z + (beta * y_in.astype(np.float64) if beta else 0.0)
    cast = 0.0 if ch.dtype == np.float64 else 2.0 ** -24 * np.abs(ref) + 2.0 ** -149
    # the row sum in another order, then the scale's product and sum: a rounding of the result each
    assert np.all(np.abs(got.astype(np.float64) - ref) <= 2 * 8 * 2.0 ** -53 * scale * (1 + 2.0 ** -23) + 2.0 ** -52 * np.abs(ref) + cast), what + ": not the product"


@pytest.mark.parametrize("dtype,with_minv", CASES, ids=IDS)
def test_two_cycles_of_gmres_8_enqueued_without_a_host_read_verify_call_by_call(dtype, with_minv):
    import torch
    m = gc.CYCLE
    ch = Chain(dtype, with_minv, m)
    tag = "%s, minv %s" % (np.dtype(dtype).name, with_minv)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        ch.reset()
        s = side.cuda_stream
        snaps = [("reset", ch.snap())]
        for name, call in ch.restart() + ch.cycle() + ch.cycle():
            call(s)
            snaps.append((name, ch.snap()))  # clones on the stream: no host read in between
    side.synchronize()
    states = [(name, ch.bodies(snap, tag + ", " + name)) for name, snap in snaps]
    lay, mh, n = capi.gmres_state_layout(m), ch.mh, ch.n
    rr, estimates = [], []
    for (_, before), (name, after) in zip(states, states[1:]):
        what = tag + ", " + name
        kind = name.split()[0]
        j = int(name.split()[1]) if " " in name else None
        changed = {"residual": {"basis", "rr"}, "start": {"state"}, "scale": {"basis", "vhat"}, "multiply": {"basis", "mdots"},
                   "project1": {"h1"}, "project2": {"h2"}, "update1": {"basis", "dots"}, "update2": {"basis", "dots"}, "column": {"state"},
                   "solve": {"y"}, "correct": {"x"}}[kind]
        for key in before:
            if key not in changed:
                assert np.array_equal(after[key], before[key], equal_nan=True), what + ": %s changed" % key
        Vb, Va = _vectors(before, ch, m + 1), _vectors(after, ch, m + 1)
        only = lambda jj: [np.array_equal(Va[i], Vb[i], equal_nan=True) for i in range(m + 1) if i != jj]
        if kind == "residual":
            _check_multiply(ch, before["x"], -1.0, 1.0, before["b"], Va[0], what)
            r64 = Va[0].astype(np.float64)
            _within(after["rr"][0], r64 * r64, what + ": r' r")
            rr.append(float(after["rr"][0]))
            if len(rr) > 1:
                estimates.append(float(before["state"][0]) ** 2)
        elif kind == "start":
            _check_start(after["state"][:lay["c"]], gc.restate_start(m, before["rr"][0])[:lay["c"]], m, what)
        elif kind == "scale":
            v, vhat = gc.restate_scale(before["state"][1], Vb[j], mh, dtype)
            _bits(Va[j], v, what + ": v")
            assert all(only(j)), what + ": another vector changed"
            if with_minv:
                _bits(after["vhat"], vhat, what + ": vhat")
        elif kind == "multiply":
            _check_multiply(ch, before["vhat"] if with_minv else Vb[j], 1.0, 0.0, None, Va[j + 1], what)
            assert all(only(j + 1)), what + ": another vector changed"
        elif kind in ("project1", "project2"):
            got = after["h1" if kind == "project1" else "h2"]
            for i, t in enumerate(gc.project_products(Vb[:j + 1], Vb[j + 1])):
                _within(got[i], t, "%s: h[%d]" % (what, i))
            was = before["h1" if kind == "project1" else "h2"]  # (the cycle before left its columns there)
            assert np.array_equal(got[j + 2:], was[j + 2:], equal_nan=True), what + ": h written beyond k + 1 doubles"
        elif kind in ("update1", "update2"):
            coef = before["h1" if kind == "update1" else "h2"]
            _bits(Va[j + 1], gc.restate_update(Vb[:j + 1], coef[:j + 1], Vb[j + 1], dtype), what + ": w")
            assert all(only(j + 1)), what + ": another vector changed"
            w64 = Va[j + 1].astype(np.float64)
            _within(after["dots"][0], w64 * w64, what + ": dots[0]")
            assert after["dots"][1] == 0.0
        elif kind == "column":
            assert before["dots"][0] > 0, what + ": a breakdown the operands were chosen to avoid"
            _check_column(after["state"], before["state"], j, m, before["h1"], before["h2"], before["dots"][0], what)
        elif kind == "solve":
            _check_solve(before["state"], m, m, after["y"][:m], what)
        else:
            _bits(after["x"], gc.restate_correct(Vb[:m], before["y"][:m], mh, before["x"], dtype), what + ": x")
    print("%s: r' r of r0 %.6e, after one cycle %.6e, after two %.6e; state[0]^2 %r" % (tag, rr[0], rr[1], rr[2], estimates))
    assert len(rr) == 3 and rr[1] < 0.1 * rr[0] and rr[2] < 0.02 * rr[0]
    for est, true in zip(estimates, rr[1:]):
        assert abs(est - true) <= 1e-6 * true, "%s: state[0]^2 %r, r' r %r" % (tag, est, true)
    ch.gwork.body(tag)
    ch.mwork.body(tag)
    ch.close()


@pytest.mark.parametrize("dtype,with_minv", CASES, ids=IDS)
def test_one_captured_cycle_of_gmres_4_replayed_twice_is_two_direct_cycles(dtype, with_minv):
    """A call that synchronised or allocated would invalidate the capture; the launches of a cycle form a line."""
    import torch
    ch = Chain(dtype, with_minv, 4)
    tag = "%s, minv %s" % (np.dtype(dtype).name, with_minv)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        s = side.cuda_stream
        ch.reset()
        for _, call in ch.restart() + ch.cycle() + ch.cycle():
            call(s)
        side.synchronize()
        direct = ch.bodies(ch.snap(), tag + ", direct")
        assert np.all(np.isfinite(direct["x"])) and np.any(direct["x"] != 0) and direct["rr"][0] > 0
        ch.reset()
        ch.gwork.fill()
        ch.mwork.fill()
        for _, call in ch.restart():
            call(s)
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for _, call in ch.cycle():
                call(s)
        for replay in range(2):
            g.replay()
        side.synchronize()
        got = ch.bodies(ch.snap(), tag + ", replayed")
        for key in direct:
            assert np.array_equal(got[key].view(np.uint8), direct[key].view(np.uint8)), "%s: %s after two replays against two direct cycles" % (tag, key)
        ch.gwork.body(tag)
        ch.mwork.body(tag)
        del g
    ch.close()


# ---- 12: the gate ----------------------------------------------------------------------------------------------------------------------------

def test_gate_project_and_update_are_not_slower_than_gemv_addmv_and_dot():
    """n = 2^22 doubles and k = 16: the basis is 537 MB, beyond the 256 MiB Infinity Cache (asserted).  One project plus one update
    against torch.mv(V, w), w.addmv_(V.T, h, alpha=-1) and torch.dot(w, w) -- no host read in either -- alternating in one process,
    three warm-up rounds, 25 rounds, medians.  By bytes the fused pair moves (2 k + 3) / (2 k + 4) = 0.972 of the composition; the
    bytes are near equal, so the gate is the project's margin for equal-byte comparisons: the pair takes at most 1.06 x the
    composition (as the residual-form gate of test_gpu_scaled.py).
    Measured: the composition 248.1 us, the fused pair 219.8 us, ratio 0.886 (a second run 0.904; tools/gmres_ab.py in
    another process: 255.5 against 224.6 us, 0.879)."""
    import torch
    n, k = 2 ** 22, 16
    assert k * n * 8 > 256 * 2 ** 20 and n * 8 < 2 ** 32
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(12)
    V = torch.randn(k, n, dtype=torch.float64, device="cuda:0", generator=gen) * (1.0 / math.sqrt(n))
    w = torch.randn(n, dtype=torch.float64, device="cuda:0", generator=gen)
    h = torch.zeros(k + 2, dtype=torch.float64, device="cuda:0")
    dots = torch.zeros(2, dtype=torch.float64, device="cuda:0")
    work = torch.zeros(capi.gmres_workspace_bytes(n, k) // 8, dtype=torch.float64, device="cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    got = {}

    def torch_way():
        got["h"] = torch.mv(V, w)
        w.addmv_(V.T, got["h"], alpha=-1.0)
        got["ww"] = torch.dot(w, w)

    def fused():
        capi.gmres_project(n, k, V, n, w, h, work, None, s)
        capi.gmres_update(n, k, V, n, h, w, dots, work, None, s)

    w0 = w.clone()
    torch_way()
    want_w, want_h, want_ww = w.clone(), got["h"].clone(), float(got["ww"])
    w.copy_(w0)
    fused()
    scale = float((V.abs() @ w0.abs()).max())
    assert float((h[:k] - want_h).abs().max()) <= 1e-10 * scale and float((w - want_w).abs().max()) <= 1e-10 * float(w0.abs().max())
    assert abs(float(dots[0]) - want_ww) <= 1e-10 * want_ww
    del w0, want_w
    med = _alternate({"torch": torch_way, "fused": fused})
    print("n %d, k %d: gemv + addmv_ + dot median %.1f us, project + update median %.1f us, ratio %.3f against %.3f by bytes" % (
        n, k, med["torch"], med["fused"], med["fused"] / med["torch"], (2 * k + 3) / (2 * k + 4)))
    assert med["fused"] <= 1.06 * med["torch"], med
