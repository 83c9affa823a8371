"""The BiCGStab updates (include/spmv_hip_bicgstab.h) on the MI355X: spmv_hip_bicgstab_{s,step,direction}_{f64,f32}, through
capi.bicgstab_s / bicgstab_step / bicgstab_direction.

The vectors are held bit for bit to the numpy restatement of the header (bicgstab_cases.restate_*: every product, quotient and sum
rounded in fp64, one cast to float last, the hatted vectors from the values as stored).  The step's dots are held (a) bit for bit
to sums formed in integers on operands where every order gives the same sum (bicgstab_cases.IntCase), at every size up to the two
around the reduction's second stage, and (b) on general operands to n 2^-53 sum |t_i| of math.fsum(t), t_i the rounded products
formed in numpy from the r the GPU returned (test_bicgstab_cases.py shows without a device that a lost element would exceed it
tenfold).  Every device array, the scalars, the dots and the workspace lie between NaN guard bands that are checked whenever an
array is read back, and the hatted outputs, the dots and the workspace are NaN when a call starts."""
import functools
import math

import numpy as np
import pytest

import bicgstab_cases as bc
import dots_cases as dc
import poison
import stream_helpers as sh
from spmv_amd import capi
from test_gpu_dots import _class_of_sum, _same_dots
from test_gpu_krylov import CASES, IDS, Band
from test_gpu_scaled import Dev, _alternate, _bits

pytestmark = pytest.mark.gpu

WRITTEN = ("r", "x", "p")
Q0 = ((0.0, 1.0), (0.0, 1.0), (0.0, 1.0))


class Arrays:
    """The device arrays of one s, one step and one direction over host operands {v, r, phat, t, rhat, x, p, minv}; the six
    scalars are one Band in the order num_a, den_a, num_w, den_w, num_r, den_r.  With minv: shat (written by s, read by the
    step) and pout (the direction's hatted output)."""

    def __init__(self, host, dtype, with_minv, quotients=Q0):
        self.dtype, self.host, self.with_minv = np.dtype(dtype), host, with_minv
        self.n = n = len(host["v"])
        self.b = {k: Band(host[k], dtype) for k in bc.NAMES if k != "minv" or with_minv}
        if with_minv:
            self.b["shat"], self.b["pout"] = Band(np.full(n, np.nan), dtype), Band(np.full(n, np.nan), dtype)
        self.sc = Band(np.zeros(6))
        self.scalars(quotients)
        self.bytes = capi.krylov_workspace_bytes(n)
        assert self.bytes >= 16 and self.bytes % 16 == 0
        self.dots, self.work = Band(np.full(2, np.nan)), Band(np.full(self.bytes // 8, np.nan))

    def scalars(self, quotients):
        self.q = quotients
        self.sc.set([x for pair in quotients for x in pair])

    def reset(self, host=None):
        self.host = host or self.host
        for k in (bc.NAMES if host else WRITTEN):
            if k in self.b:
                self.b[k].set(self.host[k])
        for k in ("shat", "pout"):
            if k in self.b:
                self.b[k].fill()

    def ptr(self, k):
        return self.b[k].ptr if k in self.b else None

    def s(self, stream=0, **over):
        a = dict(num=self.sc.ptr, den=self.sc.ptr + 8, v=self.ptr("v"), r=self.ptr("r"), minv=self.ptr("minv"), shat=self.ptr("shat"))
        a.update(over)
        capi.bicgstab_s(self.n, a["num"], a["den"], a["v"], a["r"], a["minv"], a["shat"], stream, dtype=self.dtype)

    def step(self, stream=0, fill=True, **over):
        a = dict(num_a=self.sc.ptr, den_a=self.sc.ptr + 8, num_w=self.sc.ptr + 16, den_w=self.sc.ptr + 24, phat=self.ptr("phat"),
                 shat=self.ptr("shat"), t=self.ptr("t"), rhat=self.ptr("rhat"), x=self.ptr("x"), r=self.ptr("r"), dots=self.dots.ptr,
                 work=self.work.ptr, work_bytes=self.bytes)
        a.update(over)
        if fill:
            self.dots.fill()
            self.work.fill()
        capi.bicgstab_step(self.n, a["num_a"], a["den_a"], a["num_w"], a["den_w"], a["phat"], a["shat"], a["t"], a["rhat"], a["x"], a["r"],
                           a["dots"], a["work"], a["work_bytes"], stream, dtype=self.dtype)

    def direction(self, stream=0, **over):
        p = self.sc.ptr
        a = dict(num_r=p + 32, den_r=p + 40, num_a=p, den_a=p + 8, num_w=p + 16, den_w=p + 24, r=self.ptr("r"), v=self.ptr("v"),
                 p=self.ptr("p"), minv=self.ptr("minv"), pout=self.ptr("pout"))
        a.update(over)
        capi.bicgstab_direction(self.n, a["num_r"], a["den_r"], a["num_a"], a["den_a"], a["num_w"], a["den_w"], a["r"], a["v"], a["p"],
                                a["minv"], a["pout"], stream, dtype=self.dtype)

    def get(self, k, what=""):
        return self.b[k].body(what + ", " + k) if k in self.b else None

    def read_dots(self, what=""):
        self.work.body(what + ", the workspace")
        return self.dots.body(what + ", the dots")

    def triple(self, what):
        """s, step, direction on the null stream, every result read back behind its call: {s, shat, x, r, dots, p, pout}."""
        out = {}
        self.s()
        out["s"], out["shat"] = self.get("r", what), self.get("shat", what)
        self.step()
        out["x"], out["r"], out["dots"] = self.get("x", what), self.get("r", what), self.read_dots(what)
        _bits_or_none(self.get("shat", what), out["shat"], what + ": the step changed shat")
        self.direction()
        out["p"], out["pout"] = self.get("p", what), self.get("pout", what)
        _bits(self.get("r", what), out["r"], what + ": the direction changed r")
        _bits(self.get("x", what), out["x"], what + ": the direction changed x")
        _bits_or_none(self.get("shat", what), out["shat"], what + ": the direction changed shat")
        self.inputs_unchanged(what)
        return out

    def inputs_unchanged(self, what):
        for k in ("v", "phat", "t", "rhat", "minv"):
            if k in self.b:
                _bits(self.get(k, what), self.host[k], what + ": %s changed" % k)
        _same_dots(self.sc.body(what), [x for pair in self.q for x in pair], what + ": a scalar changed")


def _bits_or_none(got, want, what):
    assert (got is None) == (want is None), what
    if got is not None:
        _bits(got, want, what)


def _against_restatement(out, host, quotients, with_minv, dtype, what, compare=_bits_or_none):
    """Each call against ITS OWN inputs: the s from the host operands, the step from the s and shat the GPU stored, the direction
    from the r the GPU stored."""
    qa, qw, qr = quotients
    minv = host["minv"] if with_minv else None
    s, shat = bc.restate_s(qa[0], qa[1], host["v"], host["r"], minv, dtype)
    compare(out["s"], s, what + ": s")
    compare(out["shat"], shat, what + ": shat")
    x, r = bc.restate_step(qa, qw, host["phat"], out["shat"], host["t"], host["x"], out["s"], dtype)
    compare(out["x"], x, what + ": x")
    compare(out["r"], r, what + ": r")
    p, phat = bc.restate_direction(qr, qa, qw, out["r"], host["v"], host["p"], minv, dtype)
    compare(out["p"], p, what + ": p")
    compare(out["pout"], phat, what + ": phat")


def _within_bound(got, r, rhat, what):
    """|dots[k] - fsum(t)| <= n 2^-53 sum |t_i| over the products of r as the GPU stored it."""
    for k, t in enumerate(bc.step_products(r, rhat)):
        want, b = math.fsum(t), bc.bound(t)
        print("%s: dots[%d] %r, fsum %r, off by %.3e, bound %.3e" % (what, k, got[k], want, abs(got[k] - want), b))
        assert abs(got[k] - want) <= b, "%s: dots[%d] = %r, fsum of the products %r, bound %.3e" % (what, k, got[k], want, b)


# ---- 1 and 3: general operands: the vectors bit for bit, the dots within the bound ----------------------------------------------------

@functools.lru_cache(maxsize=None)
def _general_runs(dtype, with_minv):
    """Every size and set of quotients once: [(tag, host operands, quotients, what the GPU returned)]."""
    runs = []
    for n in bc.SIZES:
        host = bc.general_case(n).arrays(dtype)
        dev = Arrays(host, dtype, with_minv)
        for quotients in bc.GENERAL_QUOTIENTS:
            tag = "n %d, %s, minv %s, quotients %r" % (n, np.dtype(dtype).name, with_minv, quotients)
            dev.reset()
            dev.scalars(quotients)
            runs.append((tag, host, quotients, dev.triple(tag)))
    return runs


@pytest.mark.parametrize("dtype,with_minv", CASES, ids=IDS)
def test_r_shat_x_p_and_phat_are_the_restatement_bit_for_bit(dtype, with_minv):
    for tag, host, quotients, out in _general_runs(dtype, with_minv):
        assert all(out[k].dtype == dtype for k in ("s", "x", "r", "p")) and (out["shat"] is None) == (out["pout"] is None) == (not with_minv)
        _against_restatement(out, host, quotients, with_minv, dtype, tag)


@pytest.mark.parametrize("dtype,with_minv", CASES, ids=IDS)
def test_the_dots_of_general_operands_are_within_the_bound(dtype, with_minv):
    for tag, host, quotients, out in _general_runs(dtype, with_minv):
        _within_bound(out["dots"], out["r"], host["rhat"], tag)
        if len(out["r"]) == 0:
            _same_dots(out["dots"], [0.0, 0.0], tag + ": no element")


# ---- 2: integer operands: both dots are the integer sums, at every size --------------------------------------------------------------

@pytest.mark.parametrize("dtype,with_minv", CASES, ids=IDS)
@pytest.mark.parametrize("sizes", [bc.SIZES, bc.BIG_SIZES[:1], bc.BIG_SIZES[1:]], ids=["small", "one_stage", "two_stages"])
def test_dots_of_integer_operands_are_the_integer_sums_bit_for_bit(sizes, dtype, with_minv):
    for n in sizes:
        h = bc.int_case(n)
        dev = Arrays(h.arrays(dtype), dtype, with_minv)
        for ia, iw, ir in bc.INT_TRIPLES:
            tag = "n %d, %s, minv %s, a %r, w %r, r %r" % (n, np.dtype(dtype).name, with_minv, bc.QUOTIENTS[ia], bc.QUOTIENTS[iw],
                                                            None if ir is None else bc.QUOTIENTS[ir])
            want, d0, d1 = h.triple(ia, iw, ir, with_minv)  # (the CPU preconditions are asserted there)
            dev.reset()
            dev.scalars((bc.QUOTIENTS[ia], bc.QUOTIENTS[iw], bc.QUOTIENTS[ir if ir is not None else 0]))
            dev.s()
            got = {"s": dev.get("r", tag), "shat": dev.get("shat", tag)}
            dev.step()
            got.update(x=dev.get("x", tag), r=dev.get("r", tag))
            _same_dots(dev.read_dots(tag), [float(d0), float(d1)], tag + ": the dots against the integer sums")
            if ir is not None:
                dev.direction()
                got["p"], got["phat"] = dev.get("p", tag), dev.get("pout", tag)
            for k, (num, den) in want.items():
                if got.get(k) is not None:
                    assert np.array_equal(got[k].astype(np.float64) * den, num), tag + ": " + k


# ---- 4: identical bits across two runs, a non-blocking stream behind a delay, and two streams at once --------------------------------

@pytest.fixture(scope="module")
def side():
    s = sh.Side()
    yield s
    s.report()


N_STREAMS = 3 * bc.CHUNK + 7  # three whole chunks and a part with a tail
CHAIN_QUOTIENTS = ((0.625, -1.7), (0.3, 0.8), (-0.45, 0.9))


def _chained(dev, stream=0, bands=None, fill=True):
    """One s -> step -> direction in which the step reads the hatted direction the call before left (p itself without minv)."""
    b = bands or {}
    own = {k: b[k].ptr for k in ("r", "shat") if k in b}
    dev.s(stream, **own)
    phat = (b.get("pout") or dev.b["pout"]) if dev.with_minv else (b.get("p") or dev.b["p"])
    step = dict(own, phat=phat.ptr, **{k: b[k].ptr for k in ("x", "dots", "work") if k in b})
    dev.step(stream, fill=fill, **step)
    dev.direction(stream, **{k: b[k].ptr for k in ("r", "p", "pout") if k in b})


def _state(dev, tag, bands=None):
    b = dict(dev.b, dots=dev.dots, work=dev.work)
    b.update(bands or {})
    return {k: b[k].body(tag + ", " + k) for k in ("r", "shat", "x", "p", "pout", "dots", "work") if k in b}


def _same_state(got, want, what):
    assert got.keys() == want.keys()
    for k in want:
        if k != "work":
            _bits(got[k], want[k], "%s: %s" % (what, k))


@pytest.mark.parametrize("dtype,with_minv", CASES, ids=IDS)
def test_two_runs_a_delayed_stream_and_two_streams_at_once_give_identical_bits(side, dtype, with_minv):
    import torch
    n = N_STREAMS
    rng = np.random.default_rng(78)
    host = {k: np.ascontiguousarray(rng.uniform(-1.0, 1.0, size=n).astype(dtype)) for k in bc.NAMES[:-1]}
    host["minv"] = np.ascontiguousarray(rng.uniform(0.5, 2.0, size=n).astype(dtype))
    if with_minv:  # the first step reads the hatted direction: it starts as the p it belongs to would leave it
        host["pout"] = (host["minv"].astype(np.float64) * host["p"].astype(np.float64)).astype(dtype)
    dev = Arrays(host, dtype, with_minv, CHAIN_QUOTIENTS)
    tag = "%s, minv %s" % (np.dtype(dtype).name, with_minv)

    def start():
        dev.reset()
        if with_minv:
            dev.b["pout"].set(host["pout"])

    # three chained triples on the null stream: the reference bits
    start()
    chain = []
    for k in range(3):
        _chained(dev)
        chain.append(_state(dev, tag))
    first = dict(host, phat=host["pout"] if with_minv else host["p"])
    out = _first_triple(dev, with_minv, tag, start)
    _against_restatement(out, first, CHAIN_QUOTIENTS, with_minv, dtype, tag + ", the first triple")
    _same_state({k: out[k] for k in chain[0] if k in out}, {k: chain[0][k] for k in chain[0] if k in out},
                tag + ": the first triple read back call by call")
    # the same three again
    start()
    for k in range(3):
        _chained(dev)
        _same_state(_state(dev, tag), chain[k], tag + ": a second run, triple %d" % k)
    # behind the delay on a non-blocking stream: operands that arrive behind the delay, the calls return while it runs
    ro = {k: sh.operand(host[k]) for k in ("v", "t", "rhat") + (("minv",) if with_minv else ())}
    ro["sc"] = sh.operand(np.array([x for pair in CHAIN_QUOTIENTS for x in pair]))
    rw = {k: sh.result(host[k]) for k in WRITTEN + (("pout",) if with_minv else ())}
    if with_minv:
        rw["shat"] = sh.result(np.zeros(n, dtype=dtype))
    rw["dots"], rw["work"] = sh.result(np.zeros(2)), sh.result(np.zeros(dev.bytes // 8))
    for a in list(ro.values()) + list(rw.values()):
        assert a.ptr % 16 == 0
    sc = ro["sc"].ptr

    def triple(stream):
        m, sha, po = (ro["minv"].ptr, rw["shat"].ptr, rw["pout"].ptr) if with_minv else (None, None, None)
        capi.bicgstab_s(n, sc, sc + 8, ro["v"].ptr, rw["r"].ptr, m, sha, stream, dtype=dtype)
        capi.bicgstab_step(n, sc, sc + 8, sc + 16, sc + 24, po if with_minv else rw["p"].ptr, sha, ro["t"].ptr, ro["rhat"].ptr, rw["x"].ptr,
                           rw["r"].ptr, rw["dots"].ptr, rw["work"].ptr, dev.bytes, stream, dtype=dtype)
        capi.bicgstab_direction(n, sc + 32, sc + 40, sc, sc + 8, sc + 16, sc + 24, rw["r"].ptr, ro["v"].ptr, rw["p"].ptr, m, po, stream, dtype=dtype)

    keys = [k for k in ("r", "shat", "x", "p", "pout", "dots", "work") if k in rw]
    bodies, _ = sh.delayed(side, list(ro.values()) + list(rw.values()), triple, [rw[k] for k in keys], "a BiCGStab triple behind the delay (%s)" % tag)
    _same_state(dict(zip(keys, bodies)), chain[0], tag + ": behind the delay")
    # two streams at once: every written array, the dots and a workspace each; three chained triples on each
    own = []
    for _ in side.streams:
        b = {k: Band(host[k], dtype) for k in WRITTEN}
        if with_minv:
            b["shat"], b["pout"] = Band(np.full(n, np.nan), dtype), Band(host["pout"], dtype)
        b["dots"], b["work"] = Band(np.full(2, np.nan)), Band(np.full(dev.bytes // 8, np.nan))
        own.append(b)
    torch.cuda.synchronize()
    for rnd in range(3):
        for s, b in zip(side.streams, own):
            _chained(dev, s.cuda_stream, b, fill=False)
    for s in side.streams:
        s.synchronize()
    for b in own:
        _same_state(_state(dev, tag + ", two streams", b), chain[2], tag + ": two streams at once")


def _first_triple(dev, with_minv, tag, start):
    """The first chained triple once more with every intermediate read back, for the restatement."""
    start()
    out = {}
    dev.s()
    out["s"], out["shat"] = dev.get("r", tag), dev.get("shat", tag)
    dev.step(phat=(dev.b["pout"] if with_minv else dev.b["p"]).ptr)
    out["x"], out["r"] = dev.get("x", tag), dev.get("r", tag)
    dev.direction()
    out["p"], out["pout"] = dev.get("p", tag), dev.get("pout", tag)
    return out


# ---- 5: zero denominators and non-finite elements ----------------------------------------------------------------------------------------

def _classes(got, want, what):
    assert (got is None) == (want is None), what
    if got is None:
        return
    poison.assert_classes(got, want, what)
    fin = np.isfinite(want)
    _bits(got[fin], want[fin], what + ": the finite elements")


@pytest.mark.parametrize("dtype,with_minv", CASES, ids=IDS)
def test_zero_denominators_and_nan_or_inf_in_one_element_go_where_numpy_has_them(dtype, with_minv):
    n = 2 * bc.CHUNK + 7
    clean = bc.general_case(n).arrays(dtype)
    spots = [5, bc.CHUNK + 64 + 3, n - 1]  # a whole chunk's first pass, the second chunk, the tail
    fine = ((0.75, -1.5), (0.4, 0.7), (-0.3, 0.9))
    runs = []  # (what, host operands, quotients, the vectors no element of which stays finite, the one element that may not)
    for place, (name, reached) in enumerate((("a", ("s", "x", "r", "p")), ("w", ("x", "r", "p")), ("r", ("p",)))):
        for num in (1.0, -2.0, 0.0):  # x / 0 and 0 / 0 in each of the three quotients
            q = list(fine)
            q[place] = (num, 0.0)
            runs.append(("den_%s == 0, num %g" % (name, num), clean, tuple(q), reached, None))
    runs.append(("w == 0 in the direction: b = q (a / 0)", clean, (fine[0], (0.0, 1.0), fine[2]), ("p",), None))
    runs.append(("a == 0 and w == 0: 0 / 0 in b", clean, ((0.0, 1.0), (0.0, 1.0), fine[2]), ("p",), None))
    for bad in (np.nan, np.inf, -np.inf):
        for name in bc.NAMES[:-1] + (("minv",) if with_minv else ()):
            for i in spots:
                host = {k: np.array(a, copy=True) for k, a in clean.items()}
                host[name][i] = bad
                runs.append(("%r in %s[%d]" % (bad, name, i), host, fine, (), i))
    dev = Arrays(clean, dtype, with_minv)
    for what, host, quotients, reached, spot in runs:
        tag = "%s, %s, minv %s" % (what, np.dtype(dtype).name, with_minv)
        dev.reset(host)
        dev.scalars(quotients)
        out = dev.triple(tag)
        _against_restatement(out, host, quotients, with_minv, dtype, tag, compare=_classes)
        r, d = out["r"], out["dots"]
        for k, t in enumerate(bc.step_products(r, host["rhat"])):
            if np.all(np.isfinite(t)):
                assert abs(d[k] - math.fsum(t)) <= bc.bound(t), tag + ": dots[%d] of finite products" % k
            else:
                assert poison.classes(d[k:k + 1])[0] == _class_of_sum(t) != poison.FINITE, tag + ": the class of dots[%d]" % k
        for k in reached:
            assert not np.any(np.isfinite(out[k])), "%s: the quotient reaches every element of %s" % (tag, k)
        if spot is not None:
            hit = 0
            for k in ("s", "shat", "x", "r", "p", "pout"):
                if out[k] is not None:
                    off = np.nonzero(~np.isfinite(out[k]))[0]
                    assert set(off.tolist()) <= {spot}, "%s: a non-finite value left its element in %s" % (tag, k)
                    hit += len(off)
            assert hit > 0 or not np.isfinite(d[1]), tag + ": the non-finite value went nowhere"


# ---- 6: refusals on device arrays, and the accepted aliasings ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,with_minv", CASES, ids=IDS)
def test_refusals_write_nothing_and_the_accepted_aliasings_run(dtype, with_minv):
    import torch
    n = 4 * bc.CHUNK + 1
    host = bc.general_case(n).arrays(dtype)
    quotients = ((0.5, 2.0), (-0.3, 0.8), (0.9, 0.7))
    dev = Arrays(host, dtype, with_minv, quotients)
    es = np.dtype(dtype).itemsize
    dev.dots.fill(3.5)
    dev.work.fill(3.5)
    for k in ("shat", "pout"):
        if k in dev.b:
            dev.b[k].fill(3.5)
    P = {k: dev.b[k].ptr for k in dev.b}
    sc, inv, ali = dev.sc.ptr, capi.ERR_INVALID, capi.ERR_ALIGN
    end = lambda k: P[k] + ((n * es - 1) & ~15)
    steps = [("n < 0", dict(n=-1), inv), ("null x", dict(x=None), inv), ("null num_w", dict(num_w=None), inv), ("null dots", dict(dots=None), inv),
             ("null rhat", dict(rhat=None), inv), ("work_bytes one byte short", dict(work_bytes=dev.bytes - 1), inv), ("x == phat", dict(phat=P["x"]), inv),
             ("r == t", dict(t=P["r"]), inv), ("x == r", dict(r=P["x"]), inv), ("rhat begins in the last bytes of r", dict(rhat=end("r")), inv),
             ("dots inside x", dict(dots=P["x"] + 64), inv), ("the workspace inside r", dict(work=P["r"] + 64), inv),
             ("dots inside the workspace", dict(dots=dev.work.ptr + 16), inv), ("num_a inside dots", dict(num_a=dev.dots.ptr + 8), inv),
             ("den_w inside the workspace", dict(den_w=dev.work.ptr + 8), inv), ("den_a inside r", dict(den_a=P["r"] + 16), inv),
             ("num_w == den_w inside x", dict(num_w=P["x"], den_w=P["x"]), inv),
             ("x off 16-byte alignment", dict(x=P["x"] + es), ali), ("phat off 16-byte alignment", dict(phat=P["phat"] + 8), ali),
             ("dots off 16-byte alignment", dict(dots=dev.dots.ptr + 8), ali), ("the workspace off 16-byte alignment", dict(work=dev.work.ptr + 8), ali),
             ("num_a off 8-byte alignment", dict(num_a=sc + 4), ali), ("den_w off 8-byte alignment", dict(den_w=sc + 28), ali)]
    if with_minv:
        steps += [("shat == r", dict(shat=P["r"]), inv), ("shat off 16-byte alignment", dict(shat=P["shat"] + es), ali)]
    ss = [("n < 0", dict(n=-1), inv), ("null r", dict(r=None), inv), ("null den", dict(den=None), inv), ("r == v", dict(v=P["r"]), inv),
          ("num inside r", dict(num=P["r"] + 8), inv), ("v overlapping the end of r", dict(v=end("r")), inv),
          ("r off 16-byte alignment", dict(r=P["r"] + es), ali), ("v off 16-byte alignment", dict(v=P["v"] + 8), ali),
          ("num off 8-byte alignment", dict(num=sc + 4), ali)]
    directions = [("n < 0", dict(n=-1), inv), ("null p", dict(p=None), inv), ("null v", dict(v=None), inv), ("null den_r", dict(den_r=None), inv),
                  ("p == r", dict(r=P["p"]), inv), ("p == v", dict(v=P["p"]), inv), ("num_r inside p", dict(num_r=P["p"] + 8), inv),
                  ("r overlapping the end of p", dict(r=end("p")), inv), ("p off 16-byte alignment", dict(p=P["p"] + es), ali),
                  ("r off 16-byte alignment", dict(r=P["r"] + 8), ali), ("den_w off 8-byte alignment", dict(den_w=sc + 28), ali)]
    if with_minv:
        ss += [("shat == r", dict(shat=P["r"]), inv), ("shat == v", dict(shat=P["v"]), inv), ("minv == r", dict(minv=P["r"]), inv),
               ("minv without shat", dict(shat=None), inv), ("shat without minv", dict(minv=None), inv), ("den inside shat", dict(den=P["shat"] + 8), inv)]
        directions += [("pout == p", dict(pout=P["p"]), inv), ("pout == r", dict(pout=P["r"]), inv), ("minv == p", dict(minv=P["p"]), inv),
                       ("minv without phat", dict(pout=None), inv), ("phat without minv", dict(minv=None), inv)]
    else:
        ss += [("shat without minv", dict(shat=P["t"]), inv)]
        directions += [("phat without minv", dict(pout=P["t"]), inv)]
    for call, cases in ((dev.step, steps), (dev.s, ss), (dev.direction, directions)):
        for what, over, code in cases:
            with pytest.raises(capi.SpmvHipError) as e:
                if "n" in over:
                    dev.n = over.pop("n")
                try:
                    call(**dict(over, fill=False) if call == dev.step else over)
                finally:
                    dev.n = n
            assert e.value.code == code, "%s: %s" % (what, e.value)
    torch.cuda.synchronize()
    what = "refused calls"
    for k in bc.NAMES:
        if k in dev.b:
            _bits(dev.get(k, what), host[k], "a refused call wrote " + k)
    for k in ("shat", "pout"):
        if k in dev.b:
            assert np.all(dev.get(k, what) == 3.5), "a refused call wrote " + k
    _same_dots(dev.sc.body(what), [x for pair in quotients for x in pair], "a refused call wrote a scalar")
    assert np.all(dev.dots.body(what) == 3.5), "a refused call wrote the dots"
    assert np.all(dev.work.body(what) == 3.5), "a refused call wrote the workspace"
    # valid: num == den in s (a = 1); phat == rhat == t and all four scalars one double in the step (a = w = 1), with a workspace
    # larger than needed; v == r and all six scalars one double in the direction (b = 1, w = 1)
    tag = "the accepted aliasings"
    one = ((0.5, 0.5),) * 3
    dev.s(den=sc)
    s = dev.get("r", tag)
    shat = dev.get("shat", tag)
    want_s, want_shat = bc.restate_s(0.5, 0.5, host["v"], host["r"], host["minv"] if with_minv else None, dtype)
    _bits(s, want_s, tag + ": s with num == den")
    _bits_or_none(shat, want_shat, tag + ": shat with num == den")
    big = Band(np.full(dev.bytes // 8 + 6, np.nan))
    dev.step(num_w=sc, den_a=sc, den_w=sc, phat=P["rhat"], t=P["rhat"], work=big.ptr, work_bytes=big.nbytes)
    want_x, want_r = bc.restate_step(one[0], one[1], host["rhat"], shat, host["rhat"], host["x"], s, dtype)
    x, r = dev.get("x", tag), dev.get("r", tag)
    _bits(x, want_x, tag + ": x with phat == rhat == t")
    _bits(r, want_r, tag + ": r with phat == rhat == t")
    big.body("a larger workspace")
    _within_bound(dev.dots.body(tag), r, host["rhat"], tag)
    dev.direction(**{k: sc for k in ("num_r", "den_r", "num_a", "den_a", "num_w", "den_w")}, v=P["r"])
    want_p, want_phat = bc.restate_direction(one[0], one[1], one[2], r, r, host["p"], host["minv"] if with_minv else None, dtype)
    _bits(dev.get("p", tag), want_p, tag + ": p with v == r")
    _bits_or_none(dev.get("pout", tag), want_phat, tag + ": phat with v == r")
    dev.inputs_unchanged(tag)


# ---- 7 and 8: the chain on the upwind operator -------------------------------------------------------------------------------------------

class _ChainHost:
    """What test_gpu_scaled.Dev reads of a host matrix."""

    def __init__(self):
        self.name = "upwind 37 x 37"
        self.rows, self.cols, self.p, self.c, self.v, self.b, self.minv = bc.chain_matrix()
        self.a32 = self.v.astype(np.float32)

    def values(self, kind):
        return self.v if kind == "c16_f64" else self.a32

    def vectors(self, kind):
        dtype = np.float32 if kind == "c16_f32xy" else np.float64
        return np.zeros(self.cols, dtype=dtype), np.zeros(self.rows, dtype=dtype), dtype


class Chain:
    """Right-preconditioned BiCGStab as the header composes it: device state, and one iteration as five enqueue-only calls."""

    def __init__(self, dtype, with_minv):
        self.dtype, self.with_minv = np.dtype(dtype), with_minv
        self.h = _ChainHost()
        self.kind = "c16_f64" if dtype == np.float64 else "c16_f32xy"
        self.mdev = Dev(self.h, self.kind)
        plan = self.mdev.plan
        self.multiply = plan.spmv_f64_scaled_dots if dtype == np.float64 else plan.spmv_f32xy_scaled_dots
        self.n = n = self.h.rows
        self.mh = self.h.minv.astype(dtype) if with_minv else None
        names = ("x", "r", "rhat", "p", "v", "t") + (("phat", "shat") if with_minv else ())
        self.bands = {k: Band(np.zeros(n), dtype) for k in names}
        self.minv = Band(self.mh, dtype) if with_minv else None
        self.start = Band([0.0, 1.0])
        for k in ("rho0", "rho1", "vv", "ts"):
            self.bands[k] = Band(np.full(2, np.nan))
        self.kbytes, self.mbytes = capi.krylov_workspace_bytes(n), plan.dots_workspace_bytes()
        self.kwork, self.mwork = Band(np.full(self.kbytes // 8, np.nan)), Band(np.full(self.mbytes // 8, np.nan))

    def ptr(self, k):
        return self.bands[k].ptr if k in self.bands else None

    def reset(self):
        """x0 = 0, r0 = rhat = b, everything else zero (on the current stream)."""
        for k, b in self.bands.items():
            b.fill(float("nan") if b.n == 2 else 0.0)
        for k in ("r", "rhat"):
            self.bands[k].set(self.h.b.astype(self.dtype))

    def _m(self):
        return self.minv.ptr if self.minv else None

    def begin(self, s):
        """{r'r, rhat'r} of r0 into rho0 and p = r0, phat = M^-1 r0: the header's starting idiom."""
        z, o = self.start.ptr, self.start.ptr + 8
        capi.bicgstab_step(self.n, z, o, z, o, self.ptr("phat") or self.ptr("p"), self.ptr("shat"), self.ptr("t"), self.ptr("rhat"), self.ptr("x"),
                           self.ptr("r"), self.ptr("rho0"), self.kwork.ptr, self.kbytes, s, dtype=self.dtype)
        capi.bicgstab_direction(self.n, z, o, o, o, o, o, self.ptr("r"), self.ptr("v"), self.ptr("p"), self._m(), self.ptr("phat"), s, dtype=self.dtype)

    def calls(self, it):
        """The five calls of iteration `it` as (name, function of the stream)."""
        d, n, dt = self.mdev, self.n, self.dtype
        old, new = self.ptr("rho%d" % (it % 2)), self.ptr("rho%d" % (1 - it % 2))
        vv, ts = self.ptr("vv"), self.ptr("ts")
        ph, sha = self.ptr("phat") or self.ptr("p"), self.ptr("shat") or self.ptr("r")

        def mult(x, y, w, dots):
            return lambda s: self.multiply(d.tp.data_ptr(), d.ac, d.av, x, 1.0, 0.0, None, y, w, dots, self.mwork.ptr, self.mbytes, s)

        return [("multiply_v", mult(ph, self.ptr("v"), self.ptr("rhat"), vv)),
                ("s", lambda s: capi.bicgstab_s(n, old + 8, vv + 8, self.ptr("v"), self.ptr("r"), self._m(), self.ptr("shat"), s, dtype=dt)),
                ("multiply_t", mult(sha, self.ptr("t"), self.ptr("r"), ts)),
                ("step", lambda s: capi.bicgstab_step(n, old + 8, vv + 8, ts + 8, ts, ph, self.ptr("shat"), self.ptr("t"), self.ptr("rhat"),
                                                      self.ptr("x"), self.ptr("r"), new, self.kwork.ptr, self.kbytes, s, dtype=dt)),
                ("direction", lambda s: capi.bicgstab_direction(n, new + 8, old + 8, old + 8, vv + 8, ts + 8, ts, self.ptr("r"), self.ptr("v"),
                                                                self.ptr("p"), self._m(), self.ptr("phat"), s, dtype=dt))]

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
        for it in range(bc.ITERATIONS):
            for name, call in ch.calls(it):
                call(s)
                snaps.append(("%s of iteration %d" % (name, it), ch.snap()))  # clones on the stream: no host read in between
    side.synchronize()
    states = [(name, ch.bodies(snap, tag + ", " + name)) for name, snap in snaps]
    h, mh = ch.h, ch.mh
    values = h.values(ch.kind).astype(np.float64)
    hat = lambda st, k: st[k + "hat"] if with_minv else st["r" if k == "s" else k]  # the hatted vector, or the plain one it is
    # the starting idiom: x and r as they were, the dots of r0, p = r0 and phat = M^-1 r0
    before, after = states[0][1], states[1][1]
    _bits(after["x"], before["x"], tag + ": the starting step changed x")
    _bits(after["r"], before["r"], tag + ": the starting step changed r")
    _within_bound(after["rho0"], after["r"], after["rhat"], tag + ": the dots of r0")
    _bits(after["p"], after["r"], tag + ": p = r0")
    if with_minv:
        _bits(after["phat"], (mh.astype(np.float64) * after["r"].astype(np.float64)).astype(dtype), tag + ": phat = M^-1 r0")
    first = float(after["rho0"][0])
    assert first > 0 and float(after["rho0"][1]) == first  # rhat is r0
    for (_, before), (name, after) in zip(states[1:], states[2:]):
        what = tag + ", " + name
        kind, it = name.split()[0], int(name.split()[-1])
        old, new = "rho%d" % (it % 2), "rho%d" % (1 - it % 2)
        changed = {"multiply_v": {"v", "vv"}, "s": {"r", "shat"}, "multiply_t": {"t", "ts"}, "step": {"x", "r", new}, "direction": {"p", "phat"}}[kind]
        for key in before:
            if key not in changed:
                assert np.array_equal(after[key], before[key], equal_nan=True), what + ": %s changed" % key
        qa, qw = (before[old][1], before["vv"][1]), (before["ts"][1], before["ts"][0])
        if kind.startswith("multiply"):
            xin, out, w, dots = ((hat(before, "p"), "v", "rhat", "vv") if kind == "multiply_v" else (hat(before, "s"), "t", "r", "ts"))
            prod = values * xin.astype(np.float64)[h.c]
            ref, scale = np.add.reduceat(prod, h.p[:-1].astype(np.int64)), np.add.reduceat(np.abs(prod), h.p[:-1].astype(np.int64))
            err = np.abs(after[out].astype(np.float64) - ref)
            cast = 0.0 if dtype == np.float64 else 2.0 ** -24 * np.abs(ref) + 2.0 ** -149
            assert np.all(err <= 2 * 8 * 2.0 ** -53 * scale * (1 + 2.0 ** -23) + cast), what + ": the product is not A times its operand"
            for j, t in enumerate(dc.products(after[out], before[w])):
                assert abs(after[dots][j] - math.fsum(t)) <= dc.bound(t), what + ": the multiply's dots[%d]" % j
        elif kind == "s":
            assert before["vv"][1] != 0, what + ": rhat' v == 0 (a breakdown the operands were chosen to avoid)"
            want_s, want_shat = bc.restate_s(qa[0], qa[1], before["v"], before["r"], mh, dtype)
            _bits(after["r"], want_s, what + ": s")
            if with_minv:
                _bits(after["shat"], want_shat, what + ": shat")
        elif kind == "step":
            assert before["ts"][0] != 0, what + ": t' t == 0"
            want_x, want_r = bc.restate_step(qa, qw, hat(before, "p"), before["shat"] if with_minv else None, before["t"], before["x"],
                                             before["r"], dtype)
            _bits(after["x"], want_x, what + ": x")
            _bits(after["r"], want_r, what + ": r")
            _within_bound(after[new], after["r"], before["rhat"], what)
        else:
            want_p, want_phat = bc.restate_direction((before[new][1], before[old][1]), qa, qw, before["r"], before["v"], before["p"], mh, dtype)
            _bits(after["p"], want_p, what + ": p")
            if with_minv:
                _bits(after["phat"], want_phat, what + ": phat")
    last = float(states[-1][1]["rho%d" % (bc.ITERATIONS % 2)][0])
    print("%s: r' r of r0 %.6e, after %d iterations %.6e" % (tag, first, bc.ITERATIONS, last))
    assert np.isfinite(last) and last < 0.1 * first
    ch.kwork.body(tag)
    ch.mwork.body(tag)
    ch.close()


@pytest.mark.parametrize("dtype,with_minv", CASES, ids=IDS)
def test_two_captured_iterations_replayed_three_times_are_six_direct_ones(dtype, with_minv):
    """An even and an odd iteration (the two dots buffers change places) captured on one stream -- the two multiplies, the three
    updates and their reductions form a line -- and replayed three times: the bits of six iterations enqueued directly.  A call
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
        assert all(np.all(np.isfinite(direct[k])) for k in direct) and direct["rho0"][0] > 0 and np.any(direct["x"] != 0)
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
    """n = 4096^2 doubles, no minv (shat is r), Level 2, one process, torch events on one stream; three warm-up rounds, 25 rounds
    alternating the two ways, medians.  Asserted: median(spmv_hip_bicgstab_step_f64) <= 1.00 x median(the torch way), the torch way
    being two 0-dim quotients a and w, x.addcmul_(phat, a), x.addcmul_(r, w), r.addcmul_(t, w, value=-1), torch.dot(r, r),
    torch.dot(rhat, r) -- no host read in either.  The bound is from the code: the fused call moves 56 bytes per element (phat,
    t, rhat, x, r read; x, r written) against 96 (0.583) in fewer launches.  The six vectors of 134 MB each exceed the 256 MiB
    Infinity Cache, which is asserted.  A condition, not a measured margin.
    Measured: the torch way 284.3 us, the fused step 166.6 us, ratio 0.586 against 0.583 by bytes (a second run 0.603;
    tools/bicgstab_ab.py in another process: 289.4 against 172.6 us, 0.596)."""
    import torch
    n = 4096 * 4096
    assert 6 * n * 8 > 256 * 2 ** 20 and n * 8 < 2 ** 32
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(6)
    phat, t, rhat, x, r = (torch.rand(n, dtype=torch.float64, device="cuda:0", generator=gen) * 2 - 1 for _ in range(5))
    sc = torch.tensor([1e-3, 1.0, -2e-3, 1.0], dtype=torch.float64, device="cuda:0")
    dots = torch.zeros(2, dtype=torch.float64, device="cuda:0")
    work = torch.zeros(capi.krylov_workspace_bytes(n) // 8, dtype=torch.float64, device="cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    got = {}

    def torch_way():
        a = sc[0] / sc[1]
        w = sc[2] / sc[3]
        x.addcmul_(phat, a)
        x.addcmul_(r, w)
        r.addcmul_(t, w, value=-1.0)
        got["rr"] = torch.dot(r, r)
        got["hr"] = torch.dot(rhat, r)

    def fused():
        p = sc.data_ptr()
        capi.bicgstab_step(n, p, p + 8, p + 16, p + 24, phat, None, t, rhat, x, r, dots, work, None, s)

    x0, r0 = x.clone(), r.clone()
    torch_way()
    want_x, want_r, want_rr, want_hr = x.clone(), r.clone(), float(got["rr"]), float(got["hr"])
    x.copy_(x0)
    r.copy_(r0)
    fused()
    # (torch may contract its updates: a rounding apart per sum at the most)
    assert float((x - want_x).abs().max()) <= 2 * 2.0 ** -52 and float((r - want_r).abs().max()) <= 2.0 ** -52
    scale = float(rhat.abs().dot(r.abs()))
    assert abs(float(dots[0]) - want_rr) <= 1e-10 * want_rr and abs(float(dots[1]) - want_hr) <= 1e-10 * scale
    del x0, r0, want_x, want_r
    med = _alternate({"torch": torch_way, "fused": fused})
    print("n %d: the torch way (two div, three addcmul_, two dot) median %.1f us, the fused step median %.1f us, ratio %.3f against %.3f by bytes" % (
        n, med["torch"], med["fused"], med["fused"] / med["torch"], 56.0 / 96.0))
    assert med["fused"] <= 1.00 * med["torch"], med
