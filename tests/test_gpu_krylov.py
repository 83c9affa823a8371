"""The conjugate-gradient updates (include/spmv_hip_krylov.h) on the MI355X: spmv_hip_cg_step_{f64,f32} and
spmv_hip_cg_direction_{f64,f32}, through capi.cg_step / capi.cg_direction.

The vectors are held bit for bit to the numpy restatement of the header (krylov_cases.restate_step / restate_direction: every
product and sum rounded in fp64, one cast to float last).  The dots are held (a) bit for bit to sums formed in integers on
operands where every order gives the same sum (krylov_cases.IntCase), at every size up to the two around the reduction's second
stage, and (b) on general operands to n 2^-53 sum |t_i| of math.fsum(t), t_i the rounded products formed in numpy from the r the
GPU returned (test_krylov_cases.py shows without a device that a lost element would exceed it tenfold).  Every device array,
the two scalars, the dots and the workspace lie between NaN guard bands that are checked whenever an array is read back, and the
dots and the workspace are NaN when a call starts: a slot read without having been written by that call shows as NaN."""
import functools
import math

import numpy as np
import pytest

import dots_cases as dc
import helpers
import krylov_cases as kc
import poison
import stream_helpers as sh
from spmv_amd import capi
from test_gpu_dots import _class_of_sum, _same_dots
from test_gpu_scaled import Dev, _alternate, _bits

pytestmark = pytest.mark.gpu

GUARD = 8  # elements of NaN in front of and behind every array (64 or 32 bytes: the body stays 16-byte aligned)
CASES = [(np.float64, True), (np.float64, False), (np.float32, True), (np.float32, False)]
IDS = ["f64-minv", "f64", "f32-minv", "f32"]


def _torch_dtype(dtype):
    import torch
    return {np.dtype(np.float64): torch.float64, np.dtype(np.float32): torch.float32}[np.dtype(dtype)]


class Band:
    """An array on the device, 16-byte aligned, between GUARD elements of NaN."""

    def __init__(self, body, dtype=np.float64):
        import torch
        self.torch, self.dtype = torch, np.dtype(dtype)
        body = np.ascontiguousarray(body, dtype=dtype)
        self.n, self.nbytes = len(body), len(body) * self.dtype.itemsize
        self.t = torch.full((self.n + 2 * GUARD,), float("nan"), dtype=_torch_dtype(dtype), device="cuda:0")
        self.ptr = self.t.data_ptr() + GUARD * self.dtype.itemsize
        assert self.ptr % 16 == 0
        self.set(body)

    def set(self, body):
        if self.n:
            self.t[GUARD:GUARD + self.n] = self.torch.from_numpy(np.ascontiguousarray(body, dtype=self.dtype)).to("cuda:0")

    def fill(self, value=float("nan")):
        self.t[GUARD:GUARD + self.n] = value

    def snap(self):
        return self.t.clone()

    def body(self, what="", snap=None):
        h = (self.t if snap is None else snap).cpu().numpy()
        assert np.all(np.isnan(np.concatenate([h[:GUARD], h[GUARD + self.n:]]))), what + ": written outside its elements"
        return h[GUARD:GUARD + self.n].copy()


class Arrays:
    """The device arrays of one step and one direction over host operands (p, q, x, r, minv); num and den are one Band."""

    def __init__(self, host, dtype, with_minv, num=0.0, den=1.0):
        self.dtype, self.host = np.dtype(dtype), host
        self.n = len(host[0])
        self.p, self.q, self.x, self.r = (Band(a, dtype) for a in host[:4])
        self.minv = Band(host[4], dtype) if with_minv else None
        self.mh = host[4] if with_minv else None
        self.nd = Band([num, den])
        self.bytes = capi.krylov_workspace_bytes(self.n)
        assert self.bytes >= 16 and self.bytes % 16 == 0
        self.dots, self.work = Band(np.full(2, np.nan)), Band(np.full(self.bytes // 8, np.nan))

    def scalars(self, num, den):
        self.nd.set([num, den])

    def reset(self):
        for band, a in zip((self.p, self.q, self.x, self.r), self.host):
            band.set(a)

    def step(self, stream=0, x=None, r=None, dots=None, work=None, fill=True):
        dots, work = dots or self.dots, work or self.work
        if fill:
            dots.fill()
            work.fill()
        capi.cg_step(self.n, self.nd.ptr, self.nd.ptr + 8, self.p.ptr, self.q.ptr, (x or self.x).ptr, (r or self.r).ptr,
                     self.minv.ptr if self.minv else None, dots.ptr, work.ptr, self.bytes, stream, dtype=self.dtype)

    def direction(self, stream=0):
        capi.cg_direction(self.n, self.nd.ptr, self.nd.ptr + 8, self.r.ptr, self.minv.ptr if self.minv else None, self.p.ptr, stream,
                          dtype=self.dtype)

    def read_dots(self, what="", dots=None, work=None):
        (work or self.work).body(what + ", the workspace")
        return (dots or self.dots).body(what + ", the dots")

    def inputs_unchanged(self, num, den, what, p=True):
        if p:
            _bits(self.p.body(what), self.host[0], what + ": p changed")
        _bits(self.q.body(what), self.host[1], what + ": q changed")
        if self.minv:
            _bits(self.minv.body(what), self.host[4], what + ": minv changed")
        _same_dots(self.nd.body(what), [num, den], what + ": num or den changed")


def _within_bound(got, r, minv, what):
    """|dots[k] - fsum(t)| <= n 2^-53 sum |t_i| over the products of r as the GPU stored it; +0.0 where minv is None."""
    for k, t in enumerate(kc.step_products(r, minv)):
        want, b = math.fsum(t), dc.bound(t)
        print("%s: dots[%d] %r, fsum %r, off by %.3e, bound %.3e" % (what, k, got[k], want, abs(got[k] - want), b))
        assert abs(got[k] - want) <= b, "%s: dots[%d] = %r, fsum of the products %r, bound %.3e" % (what, k, got[k], want, b)
    if minv is None:
        _same_dots(got[1:], [0.0], what + ": the second dot without minv is +0.0")


# ---- 1 and 3: general operands: the vectors bit for bit, the dots within the bound ----------------------------------------------------

@functools.lru_cache(maxsize=None)
def _general_runs(dtype, with_minv):
    """Every size and quotient once: [(tag, host operands, num, den, x, r, dots, p of the direction)] as the GPU returned them."""
    out = []
    for n in kc.SIZES:
        host = kc.general_case(n).arrays(dtype)
        dev = Arrays(host, dtype, with_minv)
        for num, den in kc.GENERAL_QUOTIENTS:
            tag = "n %d, %s, a = %r / %r, minv %s" % (n, np.dtype(dtype).name, num, den, with_minv)
            dev.reset()
            dev.scalars(num, den)
            dev.step()
            x, r, d = dev.x.body(tag), dev.r.body(tag), dev.read_dots(tag)
            dev.inputs_unchanged(num, den, tag)
            dev.direction()
            out.append((tag, host, num, den, x, r, d, dev.p.body(tag)))
            _bits(dev.r.body(tag), r, tag + ": the direction changed r")
            dev.inputs_unchanged(num, den, tag, p=False)
    return out


@pytest.mark.parametrize("dtype,with_minv", CASES, ids=IDS)
def test_x_r_and_p_are_the_restatement_bit_for_bit(dtype, with_minv):
    for tag, (p, q, x0, r0, minv), num, den, x, r, d, pd in _general_runs(dtype, with_minv):
        assert x.dtype == r.dtype == pd.dtype == dtype
        want_x, want_r = kc.restate_step(num, den, p, q, x0, r0, dtype)
        _bits(x, want_x, tag + ": x against the restatement")
        _bits(r, want_r, tag + ": r against the restatement")
        _bits(pd, kc.restate_direction(num, den, r, minv if with_minv else None, p, dtype), tag + ": p against the restatement")


@pytest.mark.parametrize("dtype,with_minv", CASES, ids=IDS)
def test_the_dots_of_general_operands_are_within_the_bound(dtype, with_minv):
    for tag, (p, q, x0, r0, minv), num, den, x, r, d, pd in _general_runs(dtype, with_minv):
        _within_bound(d, r, minv if with_minv else None, tag)
        if len(r) == 0:
            _same_dots(d, [0.0, 0.0], tag + ": no element")


# ---- 2: integer operands: both dots are the integer sums, at every size --------------------------------------------------------------

@pytest.mark.parametrize("dtype,with_minv", CASES, ids=IDS)
@pytest.mark.parametrize("sizes", [kc.SIZES, kc.BIG_SIZES[:1], kc.BIG_SIZES[1:]], ids=["small", "one_stage", "two_stages"])
def test_dots_of_integer_operands_are_the_integer_sums_bit_for_bit(sizes, dtype, with_minv):
    for n in sizes:
        h = kc.int_case(n)
        dev = Arrays(h.arrays(dtype), dtype, with_minv)
        for num, den in kc.QUOTIENTS:
            tag = "n %d, %s, a = %g / %g, minv %s" % (n, np.dtype(dtype).name, num, den, with_minv)
            x2, r2, d0, d1 = h.step(num, den, with_minv)  # (the CPU preconditions are asserted there)
            dev.reset()
            dev.scalars(num, den)
            dev.step()
            got = dev.read_dots(tag)
            assert np.array_equal(dev.x.body(tag).astype(np.float64) * 2, x2), tag + ": x"
            assert np.array_equal(dev.r.body(tag).astype(np.float64) * 2, r2), tag + ": r"
            _same_dots(got, [float(d0), float(d1)], tag + ": the dots against the integer sums")
            # the direction on the same operands: p <- z + a p is exact as well
            dev.direction()
            p, q, x, r, minv = h.arrays(np.float64)
            rs = r2 / 2.0
            want = (minv * rs if with_minv else rs) + (num / den) * p
            assert np.array_equal(dev.p.body(tag).astype(np.float64), want), tag + ": p"


# ---- 4: identical bits across two calls, a non-blocking stream behind a delay, and two streams at once --------------------------------

@pytest.fixture(scope="module")
def side():
    s = sh.Side()
    yield s
    s.report()


N_STREAMS = 3 * kc.CHUNK + 7  # three whole chunks and a part with a tail


@pytest.mark.parametrize("dtype,with_minv", CASES, ids=IDS)
def test_two_calls_a_delayed_stream_and_two_streams_at_once_give_identical_bits(side, dtype, with_minv):
    import torch
    n = N_STREAMS
    rng = np.random.default_rng(77)
    host = tuple(np.ascontiguousarray(a.astype(dtype)) for a in [rng.uniform(-1.0, 1.0, size=n) for _ in range(4)] + [rng.uniform(0.5, 2.0, size=n)])
    num, den = 0.625, -1.7
    dev = Arrays(host, dtype, with_minv, num, den)
    tag = "%s, minv %s" % (np.dtype(dtype).name, with_minv)
    # three chained steps on the null stream, then a direction: the reference bits
    chain = []
    for k in range(3):
        dev.step()
        chain.append((dev.x.body(tag), dev.r.body(tag), dev.read_dots(tag)))
    dev.direction()
    want_p = dev.p.body(tag)
    _bits(chain[0][0], kc.restate_step(num, den, *host[:4], dtype)[0], tag + ": x of the first call against the restatement")
    # the same three steps again
    dev.reset()
    for k in range(3):
        dev.step()
        _bits(dev.x.body(tag), chain[k][0], tag + ": x of a second run, call %d" % k)
        _bits(dev.r.body(tag), chain[k][1], tag + ": r of a second run, call %d" % k)
        _same_dots(dev.read_dots(tag), chain[k][2], tag + ": two identical calls, call %d" % k)
    # behind the delay on a non-blocking stream: operands that arrive behind the delay, the call returns while it runs
    pa, qa, nda = sh.operand(host[0]), sh.operand(host[1]), sh.operand(np.array([num, den]))
    ma = sh.operand(host[4]) if with_minv else None
    xa, ra = sh.result(host[2]), sh.result(host[3])
    da, wa = sh.result(np.zeros(2)), sh.result(np.zeros(dev.bytes // 8))
    for a in (pa, qa, xa, ra, da, wa) + ((ma,) if ma else ()):
        assert a.ptr % 16 == 0

    def step(stream):
        capi.cg_step(n, nda.ptr, nda.ptr + 8, pa.ptr, qa.ptr, xa.ptr, ra.ptr, ma.ptr if ma else None, da.ptr, wa.ptr, dev.bytes, stream, dtype=dtype)

    operands = [pa, qa, nda, xa, ra, da, wa] + ([ma] if ma else [])
    (bx, br, bd, _), _ = sh.delayed(side, operands, step, [xa, ra, da, wa], "cg_step behind the delay (%s)" % tag)
    _bits(bx, chain[0][0], tag + ": x behind the delay")
    _bits(br, chain[0][1], tag + ": r behind the delay")
    _same_dots(bd, chain[0][2], tag + ": the dots behind the delay")
    # the direction behind the delay: r as the first step left it, p as it was
    ra.set(chain[0][1])
    pr = sh.result(host[0])

    def direction(stream):
        capi.cg_direction(n, nda.ptr, nda.ptr + 8, ra.ptr, ma.ptr if ma else None, pr.ptr, stream, dtype=dtype)

    (bp,), _ = sh.delayed(side, [nda, ra, pr] + ([ma] if ma else []), direction, [pr], "cg_direction behind the delay (%s)" % tag)
    _bits(bp, kc.restate_direction(num, den, chain[0][1], host[4] if with_minv else None, host[0], dtype), tag + ": p behind the delay")
    # two streams at once: x, r, the dots and a workspace each; three chained steps on each
    own = [(Band(host[2], dtype), Band(host[3], dtype), Band(np.full(2, np.nan)), Band(np.full(dev.bytes // 8, np.nan))) for _ in side.streams]
    torch.cuda.synchronize()
    for rnd in range(3):
        for s, (x, r, d, w) in zip(side.streams, own):
            dev.step(stream=s.cuda_stream, x=x, r=r, dots=d, work=w, fill=False)
    for s in side.streams:
        s.synchronize()
    for x, r, d, w in own:
        _bits(x.body(tag), chain[2][0], tag + ": x of two streams at once")
        _bits(r.body(tag), chain[2][1], tag + ": r of two streams at once")
        _same_dots(dev.read_dots(tag + ", two streams", d, w), chain[2][2], tag + ": the dots of two streams at once")
    assert want_p.dtype == dtype


# ---- 5: den == 0 and non-finite elements ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,with_minv", CASES, ids=IDS)
def test_a_zero_denominator_and_nan_or_inf_in_one_element_go_where_numpy_has_them(dtype, with_minv):
    n = 2 * kc.CHUNK + 7
    clean = kc.general_case(n).arrays(dtype)
    spots = [5, kc.CHUNK + 64 + 3, n - 1]  # a whole chunk's first pass, the second chunk, the tail
    runs = [("den == 0, num 1", clean, 1.0, 0.0), ("den == 0, num -2", clean, -2.0, 0.0), ("0 / 0", clean, 0.0, 0.0)]
    for bad in (np.nan, np.inf, -np.inf):
        for which, name in ((0, "p"), (1, "q"), (3, "r")):
            for i in spots:
                host = [np.array(a, copy=True) for a in clean]
                host[which][i] = bad
                runs.append(("%r in %s[%d]" % (bad, name, i), tuple(host), 0.75, -1.5))
    for what, host, num, den in runs:
        tag = "%s, %s, minv %s" % (what, np.dtype(dtype).name, with_minv)
        dev = Arrays(host, dtype, with_minv, num, den)
        dev.step()
        x, r, d = dev.x.body(tag), dev.r.body(tag), dev.read_dots(tag)
        want_x, want_r = kc.restate_step(num, den, *host[:4], dtype)
        poison.assert_classes(x, want_x, tag + ": x")
        poison.assert_classes(r, want_r, tag + ": r")
        fin = np.isfinite(want_x) & np.isfinite(want_r)
        _bits(x[fin], want_x[fin], tag + ": the finite elements of x")
        _bits(r[fin], want_r[fin], tag + ": the finite elements of r")
        t0, t1 = kc.step_products(r, host[4] if with_minv else None)
        if np.all(np.isfinite(r)):  # the value went into x alone: the dots are those of a finite r
            assert " in p[" in what
            _within_bound(d, r, host[4] if with_minv else None, tag)
        else:
            assert poison.classes(d[:1])[0] == _class_of_sum(t0) != poison.FINITE, tag + ": class of r' r"
            if with_minv:
                assert poison.classes(d[1:])[0] == _class_of_sum(t1) != poison.FINITE, tag + ": class of r' M^-1 r"
            else:
                _same_dots(d[1:], [0.0], tag)
        if "den" in what or "0 / 0" in what:
            assert not np.any(np.isfinite(x)) and not np.any(np.isfinite(r)), tag + ": a is not finite: it reaches every element"
        else:
            assert (~np.isfinite(x)).sum() + (~np.isfinite(r)).sum() == 1, tag + ": the non-finite value left its element"
        dev.direction()
        pd = dev.p.body(tag)
        want_p = kc.restate_direction(num, den, r, host[4] if with_minv else None, host[0], dtype)
        poison.assert_classes(pd, want_p, tag + ": p")
        _bits(pd[np.isfinite(want_p)], want_p[np.isfinite(want_p)], tag + ": the finite elements of p")


# ---- 6: refusals on device arrays ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,with_minv", CASES, ids=IDS)
def test_refusals_launch_nothing_and_write_nothing(dtype, with_minv):
    import torch
    n = kc.SPAN + 1
    host = kc.general_case(n).arrays(dtype)
    dev = Arrays(host, dtype, with_minv, 0.5, 2.0)
    es = np.dtype(dtype).itemsize
    dev.dots.fill(3.5)
    dev.work.fill(3.5)
    a = {"n": n, "num": dev.nd.ptr, "den": dev.nd.ptr + 8, "p": dev.p.ptr, "q": dev.q.ptr, "x": dev.x.ptr, "r": dev.r.ptr,
         "minv": dev.minv.ptr if dev.minv else None, "dots": dev.dots.ptr, "work": dev.work.ptr, "work_bytes": dev.bytes}
    inv, ali = capi.ERR_INVALID, capi.ERR_ALIGN
    steps = [("n < 0", dict(n=-1), inv), ("null x", dict(x=None), inv), ("null num", dict(num=None), inv), ("null dots", dict(dots=None), inv),
             ("work_bytes one byte short", dict(work_bytes=dev.bytes - 1), inv), ("x == p", dict(p=a["x"]), inv), ("r == q", dict(q=a["r"]), inv),
             ("x == r", dict(r=a["x"]), inv), ("q begins in the last bytes of r", dict(q=a["r"] + ((n * es - 1) & ~15)), inv),
             ("dots inside x", dict(dots=a["x"] + 64), inv), ("the workspace inside r", dict(work=a["r"] + 64), inv),
             ("dots inside the workspace", dict(dots=a["work"] + 16), inv), ("num inside dots", dict(num=a["dots"] + 8), inv),
             ("den inside the workspace", dict(den=a["work"] + 8), inv), ("den inside r", dict(den=a["r"] + 16), inv),
             ("num == den inside x", dict(num=a["x"], den=a["x"]), inv),
             ("x off 16-byte alignment", dict(x=a["x"] + es), ali), ("p off 16-byte alignment", dict(p=a["p"] + 8), ali),
             ("dots off 16-byte alignment", dict(dots=a["dots"] + 8), ali), ("the workspace off 16-byte alignment", dict(work=a["work"] + 8), ali),
             ("num off 8-byte alignment", dict(num=a["num"] + 4), ali), ("den off 8-byte alignment", dict(den=a["den"] + 4), ali)]
    if with_minv:
        steps += [("minv == r", dict(minv=a["r"]), inv), ("minv off 16-byte alignment", dict(minv=a["minv"] + es), ali)]
    for what, over, code in steps:
        k = dict(a, **over)
        with pytest.raises(capi.SpmvHipError) as e:
            capi.cg_step(k["n"], k["num"], k["den"], k["p"], k["q"], k["x"], k["r"], k["minv"], k["dots"], k["work"], k["work_bytes"], 0, dtype=dtype)
        assert e.value.code == code, "%s: %s" % (what, e.value)
    directions = [("n < 0", dict(n=-1), inv), ("null p", dict(p=None), inv), ("null den", dict(den=None), inv), ("p == r", dict(r=a["p"]), inv),
                  ("num inside p", dict(num=a["p"] + 8), inv), ("r overlapping the end of p", dict(r=a["p"] + ((n * es - 1) & ~15)), inv),
                  ("p off 16-byte alignment", dict(p=a["p"] + es), ali), ("r off 16-byte alignment", dict(r=a["r"] + 8), ali),
                  ("num off 8-byte alignment", dict(num=a["num"] + 4), ali)]
    if with_minv:
        directions += [("minv == p", dict(minv=a["p"]), inv)]
    for what, over, code in directions:
        k = dict(a, **over)
        with pytest.raises(capi.SpmvHipError) as e:
            capi.cg_direction(k["n"], k["num"], k["den"], k["r"], k["minv"], k["p"], 0, dtype=dtype)
        assert e.value.code == code, "%s: %s" % (what, e.value)
    torch.cuda.synchronize()
    what = "refused calls"
    for band, h in zip((dev.p, dev.q, dev.x, dev.r), host):
        _bits(band.body(what), h, "a refused call wrote a vector")
    if with_minv:
        _bits(dev.minv.body(what), host[4], "a refused call wrote minv")
    _same_dots(dev.nd.body(what), [0.5, 2.0], "a refused call wrote num or den")
    assert np.all(dev.dots.body(what) == 3.5), "a refused call wrote the dots"
    assert np.all(dev.work.body(what) == 3.5), "a refused call wrote the workspace"
    # valid: p == q, num == den (a = 1), a workspace larger than needed
    big = Band(np.full(dev.bytes // 8 + 6, np.nan))
    capi.cg_step(n, a["num"], a["num"], a["p"], a["p"], a["x"], a["r"], a["minv"], a["dots"], big.ptr, big.nbytes, 0, dtype=dtype)
    want_x, want_r = kc.restate_step(1.0, 1.0, host[0], host[0], host[2], host[3], dtype)
    _bits(dev.x.body(), want_x, "p == q, num == den: x")
    _bits(dev.r.body(), want_r, "p == q, num == den: r")
    big.body("a larger workspace")
    _within_bound(dev.dots.body(), want_r, host[4] if with_minv else None, "p == q, num == den")


# ---- 7 and 8: the chain on the golden Poisson matrix -----------------------------------------------------------------------------------

class _PoissonHost:
    """What test_gpu_scaled.Dev reads of a host matrix."""

    def __init__(self):
        self.name = "poisson2D.mtx"
        self.rows, self.cols, self.p, self.c, self.v, self.b, self.minv = kc.poisson()
        self.a32 = self.v.astype(np.float32)

    def values(self, kind):
        return self.v if kind == "c16_f64" else self.a32

    def vectors(self, kind):
        dtype = np.float32 if kind == "c16_f32xy" else np.float64
        return np.zeros(self.cols, dtype=dtype), np.zeros(self.rows, dtype=dtype), dtype


class Chain:
    """Preconditioned CG as the header composes it: device state, and one iteration as three enqueue-only calls."""

    def __init__(self, dtype, with_minv):
        import torch
        self.torch, self.dtype, self.with_minv = torch, np.dtype(dtype), with_minv
        self.h = _PoissonHost()
        self.kind = "c16_f64" if dtype == np.float64 else "c16_f32xy"
        self.mdev = Dev(self.h, self.kind)
        plan = self.mdev.plan
        self.multiply = plan.spmv_f64_scaled_dots if dtype == np.float64 else plan.spmv_f32xy_scaled_dots
        self.n = n = self.h.rows
        self.mh = self.h.minv.astype(dtype) if with_minv else None
        self.k = 1 if with_minv else 0  # r' z, or r' r
        self.x, self.r, self.p, self.q = (Band(np.zeros(n), dtype) for _ in range(4))
        self.minv = Band(self.mh, dtype) if with_minv else None
        self.start = Band([0.0, 1.0])
        self.rz = [Band(np.full(2, np.nan)), Band(np.full(2, np.nan))]
        self.pq = Band(np.full(2, np.nan))
        self.kbytes, self.mbytes = capi.krylov_workspace_bytes(n), plan.dots_workspace_bytes()
        self.kwork, self.mwork = Band(np.full(self.kbytes // 8, np.nan)), Band(np.full(self.mbytes // 8, np.nan))
        self.bands = {"x": self.x, "r": self.r, "p": self.p, "q": self.q, "rz0": self.rz[0], "rz1": self.rz[1], "pq": self.pq}

    def reset(self):
        """x0 = 0, r0 = b, p = q = 0 (on the current stream)."""
        self.x.fill(0.0)
        self.p.fill(0.0)
        self.q.fill(0.0)
        self.r.set(self.h.b.astype(self.dtype))
        for b in self.rz + [self.pq]:
            b.fill()

    def _m(self):
        return self.minv.ptr if self.minv else None

    def begin(self, s):
        """{r'r, r'z} of r0 into rz[0] and p = z0: the header's starting idiom."""
        capi.cg_step(self.n, self.start.ptr, self.start.ptr + 8, self.p.ptr, self.q.ptr, self.x.ptr, self.r.ptr, self._m(), self.rz[0].ptr,
                     self.kwork.ptr, self.kbytes, s, dtype=self.dtype)
        capi.cg_direction(self.n, self.start.ptr, self.start.ptr + 8, self.r.ptr, self._m(), self.p.ptr, s, dtype=self.dtype)

    def calls(self, it):
        """The three calls of iteration `it` as (name, function of the stream)."""
        d = self.mdev
        old, new = self.rz[it % 2], self.rz[1 - it % 2]
        k8 = 8 * self.k
        return [("multiply", lambda s: self.multiply(d.tp.data_ptr(), d.ac, d.av, self.p.ptr, 1.0, 0.0, None, self.q.ptr, self.p.ptr, self.pq.ptr,
                                                     self.mwork.ptr, self.mbytes, s)),
                ("step", lambda s: capi.cg_step(self.n, old.ptr + k8, self.pq.ptr + 8, self.p.ptr, self.q.ptr, self.x.ptr, self.r.ptr, self._m(),
                                                new.ptr, self.kwork.ptr, self.kbytes, s, dtype=self.dtype)),
                ("direction", lambda s: capi.cg_direction(self.n, new.ptr + k8, old.ptr + k8, self.r.ptr, self._m(), self.p.ptr, s, dtype=self.dtype))]

    def snap(self):
        return {k: b.snap() for k, b in self.bands.items()}

    def bodies(self, snap, what):
        return {k: self.bands[k].body(what, snap[k]) for k in self.bands}

    def close(self):
        self.mdev.close()


@pytest.mark.parametrize("dtype,with_minv", CASES, ids=IDS)
def test_eight_iterations_enqueued_without_a_host_read_verify_call_by_call(dtype, with_minv):
    import torch
    ch = Chain(dtype, with_minv)
    tag = "%s, minv %s" % (np.dtype(dtype).name, with_minv)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        ch.reset()
        s = side.cuda_stream
        snaps = [("reset", ch.snap())]
        ch.begin(s)
        snaps.append(("begin", ch.snap()))
        for it in range(kc.ITERATIONS):
            for name, call in ch.calls(it):
                call(s)
                snaps.append(("%s of iteration %d" % (name, it), ch.snap()))  # clones on the stream: no host read in between
    side.synchronize()
    states = [(name, ch.bodies(snap, tag + ", " + name)) for name, snap in snaps]
    h, mh, k = ch.h, ch.mh, ch.k
    values = h.values(ch.kind).astype(np.float64)
    # the starting idiom: x and r as they were, the dots of r0, p = z0
    before, after = states[0][1], states[1][1]
    _bits(after["x"], before["x"], tag + ": the starting step changed x")
    _bits(after["r"], before["r"], tag + ": the starting step changed r")
    _within_bound(after["rz0"], after["r"], mh, tag + ": the dots of r0")
    _bits(after["p"], kc.restate_direction(0.0, 1.0, after["r"], mh, before["p"], dtype), tag + ": p = z0")
    first = float(after["rz0"][0])
    for (_, before), (name, after) in zip(states[1:], states[2:]):
        what = tag + ", " + name
        it = int(name.split()[-1])
        old, new = "rz%d" % (it % 2), "rz%d" % (1 - it % 2)
        changed = {"multiply": {"q", "pq"}, "step": {"x", "r", new}, "direction": {"p"}}[name.split()[0]]
        for key in before:
            if key not in changed:
                assert np.array_equal(after[key], before[key], equal_nan=True), what + ": %s changed" % key
        if name.startswith("multiply"):
            ref = np.add.reduceat(values * before["p"].astype(np.float64)[h.c], h.p[:-1].astype(np.int64))
            scale = np.add.reduceat(np.abs(values * before["p"].astype(np.float64)[h.c]), h.p[:-1].astype(np.int64))
            err = np.abs(after["q"].astype(np.float64) - ref)
            cast = 0.0 if dtype == np.float64 else 2.0 ** -24 * np.abs(ref) + 2.0 ** -149
            assert np.all(err <= 2 * 8 * 2.0 ** -53 * scale * (1 + 2.0 ** -23) + cast), what + ": q is not A p"
            for j, t in enumerate(dc.products(after["q"], before["p"])):
                assert abs(after["pq"][j] - math.fsum(t)) <= dc.bound(t), what + ": the multiply's dots[%d]" % j
        elif name.startswith("step"):
            num, den = before[old][k], before["pq"][1]
            want_x, want_r = kc.restate_step(num, den, before["p"], before["q"], before["x"], before["r"], dtype)
            _bits(after["x"], want_x, what + ": x")
            _bits(after["r"], want_r, what + ": r")
            _within_bound(after[new], after["r"], mh, what)
        else:
            num, den = before[new][k], before[old][k]
            _bits(after["p"], kc.restate_direction(num, den, before["r"], mh, before["p"], dtype), what + ": p")
    last = float(states[-1][1]["rz%d" % (kc.ITERATIONS % 2)][0])
    print("%s: r' r of r0 %.6e, after %d iterations %.6e" % (tag, first, kc.ITERATIONS, last))
    assert np.isfinite(last) and last < first
    ch.kwork.body(tag)
    ch.mwork.body(tag)
    ch.close()


@pytest.mark.parametrize("dtype,with_minv", CASES, ids=IDS)
def test_two_captured_iterations_replayed_three_times_are_six_direct_ones(dtype, with_minv):
    """An even and an odd iteration (the two dots buffers change places) captured on one stream -- the multiply, the step, the
    direction and their reductions form a line -- and replayed three times: the bits of six iterations enqueued directly.  A call
    that synchronised or allocated would invalidate the capture."""
    import torch
    ch = Chain(dtype, with_minv)
    tag = "%s, minv %s" % (np.dtype(dtype).name, with_minv)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        s = side.cuda_stream
        ch.reset()
        ch.begin(s)
        for it in range(6):
            for _, call in ch.calls(it):
                call(s)
        side.synchronize()
        direct = ch.bodies(ch.snap(), tag + ", direct")
        assert all(np.all(np.isfinite(direct[k])) for k in direct) and direct["rz0"][0] > 0 and np.any(direct["x"] != 0)
        ch.reset()
        ch.begin(s)
        ch.kwork.fill()
        ch.mwork.fill()
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for it in range(2):
                for _, call in ch.calls(it):
                    call(s)
        for replay in range(3):
            g.replay()
        side.synchronize()
        got = ch.bodies(ch.snap(), tag + ", replayed")
        for key in direct:
            _bits(got[key], direct[key], "%s: %s after three replays against six direct iterations" % (tag, key))
        ch.kwork.body(tag)
        ch.mwork.body(tag)
        del g
    ch.close()


# ---- 9: the gate -----------------------------------------------------------------------------------------------------------------------

def test_gate_fused_step_is_not_slower_than_the_sync_free_torch_way():
    """n = 4096^2 doubles, Level 2, one process, torch events on one stream; three warm-up rounds, 25 rounds alternating the two
    ways, medians.  Asserted: median(spmv_hip_cg_step_f64, minv null) <= 1.00 x median(the torch way), the torch way being a 0-dim
    a = num / den, x.addcmul_(p, a), r.addcmul_(q, a, value=-1), torch.dot(r, r) -- no host read in either.  The fused call moves
    48 bytes per element (p, q, x, r read; x, r written) instead of 56 (r read once more) in no more launches; the four vectors of
    134 MB exceed the 256 MiB Infinity Cache, which is asserted.  A condition, not a measured margin.
    Measured: the torch way 180.2 us, the fused step 147.2 us, ratio 0.817 against 0.857 by bytes (tools/krylov_ab.py in
    another process: 180.5 against 140.0 us, 0.776)."""
    import torch
    n = 4096 * 4096
    assert 4 * n * 8 > 256 * 2 ** 20 and n * 8 < 2 ** 32
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(5)
    p, q, x, r = (torch.rand(n, dtype=torch.float64, device="cuda:0", generator=gen) * 2 - 1 for _ in range(4))
    nd = torch.tensor([1e-3, 1.0], dtype=torch.float64, device="cuda:0")
    num, den = nd[0], nd[1]
    dots = torch.zeros(2, dtype=torch.float64, device="cuda:0")
    work = torch.zeros(capi.krylov_workspace_bytes(n) // 8, dtype=torch.float64, device="cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    got = {}

    def torch_way():
        a = num / den
        x.addcmul_(p, a)
        r.addcmul_(q, a, value=-1.0)
        got["dot"] = torch.dot(r, r)

    def fused():
        capi.cg_step(n, nd.data_ptr(), nd.data_ptr() + 8, p, q, x, r, None, dots, work, None, s)

    x0, r0 = x.clone(), r.clone()
    torch_way()
    want_x, want_r, want_d = x.clone(), r.clone(), float(got["dot"])
    x.copy_(x0)
    r.copy_(r0)
    fused()
    # (torch may contract its update: a rounding apart at the most)
    assert float((x - want_x).abs().max()) <= 2.0 ** -52 and float((r - want_r).abs().max()) <= 2.0 ** -52
    assert abs(float(dots[0]) - want_d) <= 1e-10 * want_d and float(dots[1]) == 0.0
    del x0, r0, want_x, want_r
    med = _alternate({"torch": torch_way, "fused": fused})
    print("n %d: the torch way (div, two addcmul_, dot) median %.1f us, the fused step median %.1f us, ratio %.3f against %.3f by bytes" % (
        n, med["torch"], med["fused"], med["fused"] / med["torch"], 48.0 / 56.0))
    assert med["fused"] <= 1.00 * med["torch"], med
