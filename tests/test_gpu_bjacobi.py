"""The point-block Jacobi preconditioner (include/spmv_hip_bjacobi.h) on the MI355X: spmv_hip_bjacobi_setup_{f64,f32},
spmv_hip_bjacobi_apply_{f64,f32} and spmv_hip_bjacobi_apply_add_{f64,f32}, through capi.bjacobi_setup / bjacobi_apply /
bjacobi_apply_add.

The inverse, z and x are held bit for bit to the numpy restatement of the header (bjacobi_cases.extract / invert / apply /
apply_add).  The dots are held (a) bit for bit to sums formed in integers on operands where every order gives the same sum, at
every size up to the one that takes the reduction's second stage, (b) on general operands to n 2^-53 sum |t_i| of math.fsum(t),
t_i the rounded products formed in numpy from the z the GPU returned (test_bjacobi_cases.py shows without a device that a lost
element or a block taken from the wrong chunk would exceed it tenfold), and (c) at b = 1 in doubles bit for bit to dots[1] of
spmv_hip_cg_step_f64.  Every device array of floating-point numbers lies between NaN guard bands that are checked whenever it is
read back, and the dots and the workspace are NaN when a call starts."""
import math

import numpy as np
import pytest

import bjacobi_cases as bc
import dots_cases as dc
import krylov_cases as kc
import stream_helpers as sh
from spmv_amd import capi
from test_gpu_dots import _same_dots
from test_gpu_krylov import Band
from test_gpu_scaled import Dev, _alternate, _bits

pytestmark = pytest.mark.gpu

CASES = [(b, dtype) for dtype in bc.DTYPES for b in bc.BLOCKS]
IDS = ["b%d-%s" % (b, np.dtype(dtype).name) for b, dtype in CASES]


class Arrays:
    """The device arrays of one apply and one apply_add over host operands (inv, r, x)."""

    def __init__(self, host, b, dtype, with_dots=True):
        self.host, self.b, self.dtype = host, b, np.dtype(dtype)
        self.n = len(host[1])
        self.inv, self.r, self.x = (Band(a, dtype) for a in host)
        self.z = Band(np.full(self.n, np.nan), dtype)
        self.bytes = capi.krylov_workspace_bytes(self.n)
        self.dots, self.work = Band(np.full(2, np.nan)), Band(np.full(self.bytes // 8, np.nan))
        self.with_dots = with_dots

    def apply(self, stream=0, z=None, dots=None, work=None, fill=True, with_dots=None):
        dots, work = dots or self.dots, work or self.work
        if fill:
            dots.fill()
            work.fill()
        if self.with_dots if with_dots is None else with_dots:
            capi.bjacobi_apply(self.n, self.b, self.inv.ptr, self.r.ptr, (z or self.z).ptr, dots.ptr, work.ptr, self.bytes, stream, dtype=self.dtype)
        else:
            capi.bjacobi_apply(self.n, self.b, self.inv.ptr, self.r.ptr, (z or self.z).ptr, None, None, 0, stream, dtype=self.dtype)

    def apply_add(self, stream=0, x=None):
        capi.bjacobi_apply_add(self.n, self.b, self.inv.ptr, self.r.ptr, (x or self.x).ptr, stream, dtype=self.dtype)

    def read_dots(self, what="", dots=None, work=None):
        (work or self.work).body(what + ", the workspace")
        return (dots or self.dots).body(what + ", the dots")

    def inputs_unchanged(self, what):
        _bits(self.inv.body(what), self.host[0], what + ": the inverse changed")
        _bits(self.r.body(what), self.host[1], what + ": r changed")


def _within_bound(got, z, r, what):
    for k, t in enumerate(bc.apply_products(z, r)):
        want, b = math.fsum(t), dc.bound(t)
        print("%s: dots[%d] %r, fsum %r, off by %.3e, bound %.3e" % (what, k, got[k], want, abs(got[k] - want), b))
        assert abs(got[k] - want) <= b, "%s: dots[%d] = %r, fsum of the products %r, bound %.3e" % (what, k, got[k], want, b)


# ---- 1: the setup, bit for bit the restatement -------------------------------------------------------------------------------------

def _setup(b, dtype, rows, p, c, v):
    import torch
    tp, tc, tv = (torch.from_numpy(a).to("cuda:0") for a in (p, c, v))
    inv = Band(np.full(rows * b, np.nan), dtype)
    status = torch.full((2,), 77, dtype=torch.int32, device="cuda:0")
    capi.bjacobi_setup(rows, b, tp, tc, tv, inv.ptr, status, 0, dtype=dtype)
    got = inv.body("setup, b %d" % b)
    assert np.array_equal(tp.cpu().numpy(), p) and np.array_equal(tc.cpu().numpy(), c)
    assert np.array_equal(tv.cpu().numpy().view(np.uint64), v.view(np.uint64)), "setup changed the values"
    return got.reshape(rows // b, b, b), status.cpu().numpy().tolist()


@pytest.mark.parametrize("b,dtype", CASES, ids=IDS)
def test_setup_is_the_restatement_bit_for_bit_and_counts_the_singular_blocks(b, dtype):
    rows, p, c, v = bc.setup_matrix(b)
    want, count, first = bc.invert(bc.extract(rows, b, p, c, v), dtype)
    assert count >= 2 and first == 3  # (block 3 has a zero column, block 7 no entry)
    got, status = _setup(b, dtype, rows, p, c, v)
    assert got.dtype == dtype
    _bits(got.ravel(), want.ravel(), "b %d, %s: the inverse against the restatement" % (b, np.dtype(dtype).name))
    assert status == [count, first], status
    assert np.array_equal(got[3], np.eye(b)) and np.array_equal(got[7], np.eye(b)), "a singular block stores the identity"
    # a NaN in block 9 and an Inf in block 12: every other block keeps its bits
    bad = v.copy()
    row = np.repeat(np.arange(rows), np.diff(p))
    for k, value in ((9, np.nan), (12, np.inf)):
        at = np.flatnonzero((row // b == k) & (c // b == k))
        assert len(at)
        bad[at[len(at) // 2]] = value
    want_bad, count_bad, first_bad = bc.invert(bc.extract(rows, b, p, c, bad), dtype)
    got_bad, status_bad = _setup(b, dtype, rows, p, c, bad)
    others = np.array([k not in (9, 12) for k in range(rows // b)])
    _bits(got_bad[others].ravel(), got[others].ravel(), "b %d: a non-finite entry left its block" % b)
    assert np.array_equal(np.isnan(got_bad), np.isnan(want_bad)) and np.array_equal(np.isinf(got_bad), np.isinf(want_bad))
    assert not np.all(np.isfinite(got_bad[9])) and status_bad == [count_bad, first_bad]
    fin = np.isfinite(want_bad)
    _bits(got_bad[fin], want_bad[fin], "b %d: the finite entries of the blocks with a non-finite entry" % b)
    # a matrix without a singular block: {0, -1}; and no rows at all
    clean = bc.dominant_blocks(b, 5, 17)
    rows2 = 5 * b
    p2 = (np.arange(rows2 + 1) * b).astype(np.int32)
    c2 = (np.repeat(np.arange(5), b * b) * b + np.tile(np.arange(b), rows2)).astype(np.int32)
    got2, status2 = _setup(b, dtype, rows2, p2, c2, clean.ravel().copy())
    _bits(got2.ravel(), bc.invert(clean, dtype)[0].ravel(), "b %d: dominant blocks" % b)
    assert status2 == [0, -1]
    import torch
    status0 = torch.full((2,), 77, dtype=torch.int32, device="cuda:0")
    tz = torch.zeros(4, dtype=torch.int32, device="cuda:0")
    tv = torch.zeros(4, dtype=torch.float64, device="cuda:0")
    ti = torch.zeros(4, dtype=torch.float64, device="cuda:0")
    capi.bjacobi_setup(0, b, tz, tz, tv, ti.data_ptr(), status0, 0, dtype=dtype)
    assert status0.cpu().numpy().tolist() == [0, -1]


# ---- 2 and 3: the apply and the apply_add bit for bit; the dots ------------------------------------------------------------------------

@pytest.mark.parametrize("b,dtype", CASES, ids=IDS)
def test_z_and_x_are_the_restatement_bit_for_bit_and_the_dots_are_within_the_bound(b, dtype):
    for n in bc.sizes(b):
        general = n <= bc.GENERAL_LIMIT
        host = bc.general_case(n, b).arrays(dtype) if general else bc.int_case(n, b).arrays(dtype)
        tag = "n %d, b %d, %s, %s operands" % (n, b, np.dtype(dtype).name, "general" if general else "integer")
        dev = Arrays(host, b, dtype)
        dev.apply()
        z, d = dev.z.body(tag), dev.read_dots(tag)
        assert z.dtype == dtype
        _bits(z, bc.apply(host[0], host[1], b, dtype), tag + ": z against the restatement")
        if general:
            _within_bound(d, z, host[1], tag)
        dev.z.fill()
        dev.apply(with_dots=False)
        _bits(dev.z.body(tag), z, tag + ": z of the call without dots")
        assert np.all(np.isnan(dev.read_dots(tag))), tag + ": a call without dots wrote the dots or the workspace"
        dev.apply_add()
        _bits(dev.x.body(tag), bc.apply_add(host[0], host[1], host[2], b, dtype), tag + ": x against the restatement")
        dev.inputs_unchanged(tag)
    # no element: +0.0, +0.0 with dots, nothing without
    dev = Arrays(tuple(np.zeros(0, dtype=dtype) for _ in range(3)), b, dtype)
    dev.apply()
    _same_dots(dev.read_dots("n 0"), [0.0, 0.0], "n 0")
    dev.apply(with_dots=False)
    dev.apply_add()


@pytest.mark.parametrize("b,dtype", CASES, ids=IDS)
def test_dots_of_integer_operands_are_the_integer_sums_bit_for_bit(b, dtype):
    for n in bc.sizes(b):
        h = bc.int_case(n, b)
        zi, xi, d0, d1 = h.results()
        tag = "n %d, b %d, %s" % (n, b, np.dtype(dtype).name)
        dev = Arrays(h.arrays(dtype), b, dtype)
        dev.apply()
        got = dev.read_dots(tag)
        assert np.array_equal(dev.z.body(tag).astype(np.float64), zi), tag + ": z"
        _same_dots(got, [float(d0), float(d1)], tag + ": the dots against the integer sums")
        dev.apply_add()
        assert np.array_equal(dev.x.body(tag).astype(np.float64), xi), tag + ": x"


def test_b_1_in_doubles_is_the_second_dot_of_the_cg_step_bit_for_bit():
    for n in kc.SIZES[1:] + [65537]:
        rng = np.random.default_rng(n + 5)
        r, minv = rng.uniform(-1.0, 1.0, size=n), rng.uniform(0.5, 2.0, size=n)
        tag = "n %d" % n
        dev = Arrays((minv, r, np.zeros(n)), 1, np.float64)
        dev.apply()
        got = dev.read_dots(tag)
        zero, x, rr, m = (Band(a) for a in (np.zeros(n), np.zeros(n), r, minv))
        nd = Band([0.0, 1.0])
        dots, work = Band(np.full(2, np.nan)), Band(np.full(dev.bytes // 8, np.nan))
        capi.cg_step(n, nd.ptr, nd.ptr + 8, zero.ptr, zero.ptr, x.ptr, rr.ptr, m.ptr, dots.ptr, work.ptr, dev.bytes, 0, dtype=np.float64)
        _bits(rr.body(tag), r, tag + ": a step with a = 0 changed r")
        _same_dots(got[:1], dots.body(tag)[1:], tag + ": r'z of the apply against r' M^-1 r of the step")


@pytest.mark.parametrize("dtype", bc.DTYPES, ids=["float64", "float32"])
def test_a_diagonal_inverse_gives_the_same_bits_for_every_b(dtype):
    n = 840 * 3  # a multiple of every b, two chunks and a part
    rng = np.random.default_rng(3)
    r, m = rng.uniform(-1.0, 1.0, size=n).astype(dtype), rng.uniform(0.5, 2.0, size=n).astype(dtype)
    seen = []
    for b in bc.BLOCKS:
        inv = np.zeros((n // b, b, b), dtype=dtype)
        d = np.arange(b)
        inv[:, d, d] = m.reshape(n // b, b)
        dev = Arrays((inv.ravel(), r, np.zeros(n, dtype=dtype)), b, dtype)
        dev.apply()
        seen.append((dev.z.body(), dev.read_dots()))
        _bits(seen[-1][0], seen[0][0], "b %d: z of a diagonal inverse" % b)
        _same_dots(seen[-1][1], seen[0][1], "b %d: the dots of a diagonal inverse" % b)


# ---- 4: identical bits across calls, streams and a captured graph ----------------------------------------------------------------------

@pytest.fixture(scope="module")
def side():
    s = sh.Side()
    yield s
    s.report()


@pytest.mark.parametrize("b,dtype", [(3, np.float64), (8, np.float64), (3, np.float32), (7, np.float32)], ids=["b3-f64", "b8-f64", "b3-f32", "b7-f32"])
def test_two_runs_a_delayed_stream_two_streams_and_a_replayed_graph_give_identical_bits(side, b, dtype):
    import torch
    n = bc.nearest(3 * bc.CHUNK + 7, b)
    host = bc.general_case(n, b).arrays(dtype)
    dev = Arrays(host, b, dtype)
    tag = "b %d, %s" % (b, np.dtype(dtype).name)
    dev.apply()
    z, d = dev.z.body(tag), dev.read_dots(tag)
    dev.apply_add()
    x = dev.x.body(tag)
    _bits(z, bc.apply(host[0], host[1], b, dtype), tag + ": z against the restatement")
    dev.z.fill()
    dev.apply()
    _bits(dev.z.body(tag), z, tag + ": z of a second run")
    _same_dots(dev.read_dots(tag), d, tag + ": the dots of a second run")
    # behind the delay on a non-blocking stream
    ia, ra = sh.operand(host[0]), sh.operand(host[1])
    za, xa = sh.result(np.zeros(n, dtype=dtype)), sh.result(host[2])
    da, wa = sh.result(np.zeros(2)), sh.result(np.zeros(dev.bytes // 8))

    def call(stream):
        capi.bjacobi_apply(n, b, ia.ptr, ra.ptr, za.ptr, da.ptr, wa.ptr, dev.bytes, stream, dtype=dtype)
        capi.bjacobi_apply_add(n, b, ia.ptr, ra.ptr, xa.ptr, stream, dtype=dtype)

    (bz, bx, bd, _), _ = sh.delayed(side, [ia, ra, za, xa, da, wa], call, [za, xa, da, wa], "bjacobi_apply behind the delay (%s)" % tag)
    _bits(bz, z, tag + ": z behind the delay")
    _bits(bx, x, tag + ": x behind the delay")
    _same_dots(bd, d, tag + ": the dots behind the delay")
    # two streams at once: z, the dots and a workspace each
    own = [(Band(np.full(n, np.nan), dtype), Band(np.full(2, np.nan)), Band(np.full(dev.bytes // 8, np.nan))) for _ in side.streams]
    torch.cuda.synchronize()
    for rnd in range(3):
        for s, (zz, dd, ww) in zip(side.streams, own):
            dev.apply(stream=s.cuda_stream, z=zz, dots=dd, work=ww, fill=False)
    for s in side.streams:
        s.synchronize()
    for zz, dd, ww in own:
        _bits(zz.body(tag), z, tag + ": z of two streams at once")
        _same_dots(dev.read_dots(tag + ", two streams", dd, ww), d, tag + ": the dots of two streams at once")
    # a captured graph of apply, apply without dots and apply_add, replayed twice: x takes two corrections
    cap = torch.cuda.Stream()
    z2 = Band(np.full(n, np.nan), dtype)
    dev.x.set(host[2])
    dev.z.fill()
    dev.dots.fill()
    dev.work.fill()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cap):
        s = torch.cuda.current_stream().cuda_stream
        dev.apply(stream=s, fill=False)
        dev.apply(stream=s, z=z2, fill=False, with_dots=False)
        dev.apply_add(stream=s)
    for replay in range(2):
        g.replay()
    torch.cuda.synchronize()
    _bits(dev.z.body(tag), z, tag + ": z of the replayed graph")
    _bits(z2.body(tag), z, tag + ": z without dots of the replayed graph")
    _same_dots(dev.read_dots(tag), d, tag + ": the dots of the replayed graph")
    _bits(dev.x.body(tag), bc.apply_add(host[0], host[1], x, b, dtype), tag + ": x after two replays")
    del g
    dev.inputs_unchanged(tag)


# ---- 5: an inverse beyond 4 GiB ----------------------------------------------------------------------------------------------------------

def test_an_inverse_beyond_4_gib_is_addressed_in_64_bits():
    import torch
    b, n = 8, 2 ** 26 + 8
    assert n * b * 8 > 2 ** 32 and n * 8 < 2 ** 32
    tail = 4 * b  # the last four blocks: the last of them lies wholly beyond 4 GiB
    rng = np.random.default_rng(8)
    inv_tail = rng.integers(-2, 3, size=tail * b).astype(np.float64)
    r_tail = rng.integers(1, 9, size=tail).astype(np.float64)
    inv = torch.zeros(n * b, dtype=torch.float64, device="cuda:0")
    r = torch.ones(n, dtype=torch.float64, device="cuda:0")
    z = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda:0")
    inv[(n - tail) * b:] = torch.from_numpy(inv_tail).to("cuda:0")
    r[n - tail:] = torch.from_numpy(r_tail).to("cuda:0")
    dots = torch.full((2,), float("nan"), dtype=torch.float64, device="cuda:0")
    work = torch.full((capi.krylov_workspace_bytes(n) // 8,), float("nan"), dtype=torch.float64, device="cuda:0")
    capi.bjacobi_apply(n, b, inv, r, z, dots, work)
    want = bc.apply(inv_tail, r_tail, b, np.float64)
    assert np.any(want[-b:] != 0)
    _bits(z[n - tail:].cpu().numpy(), want, "the last blocks of z")
    assert int(torch.count_nonzero(z[:n - tail])) == 0, "z in front of the last blocks is +-0.0"
    _same_dots(dots.cpu().numpy(), [float(np.sum(want * r_tail)), float(np.sum(want * want))], "the dots")
    x = torch.ones(n, dtype=torch.float64, device="cuda:0")
    capi.bjacobi_apply_add(n, b, inv, r, x)
    _bits(x[n - tail:].cpu().numpy(), 1.0 + want, "the last blocks of x")
    assert bool(torch.all(x[:n - tail] == 1.0))


# ---- 6: refusals on device arrays ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", bc.DTYPES, ids=["float64", "float32"])
def test_refusals_launch_nothing_and_write_nothing(dtype):
    import torch
    b, n = 3, bc.nearest(4097, 3)
    host = bc.general_case(n, b).arrays(dtype)
    dev = Arrays(host, b, dtype)
    es = np.dtype(dtype).itemsize
    dev.dots.fill(3.5)
    dev.work.fill(3.5)
    dev.z.fill(3.5)
    a = {"n": n, "b": b, "inv": dev.inv.ptr, "r": dev.r.ptr, "z": dev.z.ptr, "dots": dev.dots.ptr, "work": dev.work.ptr, "work_bytes": dev.bytes}
    inv, ali = capi.ERR_INVALID, capi.ERR_ALIGN
    applies = [("n < 0", dict(n=-3), inv), ("b 0", dict(b=0), inv), ("b 9", dict(b=9), inv), ("n % b", dict(b=4), inv),
               ("null inv", dict(inv=None), inv), ("null r", dict(r=None), inv), ("null z", dict(z=None), inv),
               ("dots without work", dict(work=None), inv), ("work without dots", dict(dots=None), inv),
               ("work_bytes one byte short", dict(work_bytes=dev.bytes - 1), inv), ("z == r", dict(z=a["r"]), inv),
               ("z inside the inverse", dict(z=a["inv"] + 16 * b), inv), ("z begins in the last bytes of r", dict(z=a["r"] + ((n * es - 1) & ~15)), inv),
               ("dots inside r", dict(dots=a["r"] + 64), inv), ("the workspace inside the inverse", dict(work=a["inv"] + 64), inv),
               ("dots inside the workspace", dict(dots=a["work"] + 16), inv),
               ("z off 16-byte alignment", dict(z=a["z"] + es), ali), ("r off 16-byte alignment", dict(r=a["r"] + 8), ali),
               ("the inverse off 16-byte alignment", dict(inv=a["inv"] + 8), ali), ("dots off 16-byte alignment", dict(dots=a["dots"] + 8), ali),
               ("the workspace off 16-byte alignment", dict(work=a["work"] + 8), ali)]
    for what, over, code in applies:
        k = dict(a, **over)
        with pytest.raises(capi.SpmvHipError) as e:
            capi.bjacobi_apply(k["n"], k["b"], k["inv"], k["r"], k["z"], k["dots"], k["work"], k["work_bytes"], 0, dtype=dtype)
        assert e.value.code == code, "%s: %s" % (what, e.value)
    adds = [("n < 0", dict(n=-3), inv), ("b 9", dict(b=9), inv), ("n % b", dict(b=5), inv), ("null u", dict(r=None), inv), ("x == u", dict(z=a["r"]), inv),
            ("x inside the inverse", dict(z=a["inv"]), inv), ("x off 16-byte alignment", dict(z=a["z"] + es), ali)]
    for what, over, code in adds:
        k = dict(a, **over)
        with pytest.raises(capi.SpmvHipError) as e:
            capi.bjacobi_apply_add(k["n"], k["b"], k["inv"], k["r"], k["z"], 0, dtype=dtype)
        assert e.value.code == code, "%s: %s" % (what, e.value)
    # the setup: the inverse is what it writes
    rows, p, c, v = bc.setup_matrix(b)
    tp, tc, tv = (torch.from_numpy(x).to("cuda:0") for x in (p, c, v))
    out = Band(np.full(rows * b, 3.5), dtype)
    status = torch.full((4,), 77, dtype=torch.int32, device="cuda:0")
    s = {"rows": rows, "b": b, "p": tp.data_ptr(), "c": tc.data_ptr(), "v": tv.data_ptr(), "inv": out.ptr, "status": status.data_ptr()}
    setups = [("rows < 0", dict(rows=-3), inv), ("b 0", dict(b=0), inv), ("b 9", dict(b=9), inv), ("rows % b", dict(b=2), inv),
              ("null row_ptr", dict(p=None), inv), ("null columns", dict(c=None), inv), ("null values", dict(v=None), inv),
              ("null inverse", dict(inv=None), inv), ("null status", dict(status=None), inv), ("the inverse over row_ptr", dict(inv=s["p"]), inv),
              ("the status inside the inverse", dict(status=s["inv"] + 32), inv), ("the values inside the inverse", dict(v=s["inv"] + 16), inv),
              ("the inverse off 16-byte alignment", dict(inv=s["inv"] + es), ali), ("the status off 4-byte alignment", dict(status=s["status"] + 2), ali),
              ("the values off 8-byte alignment", dict(v=s["v"] + 4), ali)]
    for what, over, code in setups:
        k = dict(s, **over)
        with pytest.raises(capi.SpmvHipError) as e:
            capi.bjacobi_setup(k["rows"], k["b"], k["p"], k["c"], k["v"], k["inv"], k["status"], 0, dtype=dtype)
        assert e.value.code == code, "%s: %s" % (what, e.value)
    torch.cuda.synchronize()
    what = "refused calls"
    dev.inputs_unchanged(what)
    _bits(dev.x.body(what), host[2], "a refused call wrote x")
    for band in (dev.z, dev.dots, dev.work, out):
        assert np.all(band.body(what) == 3.5), "a refused call wrote"
    assert status.cpu().numpy().tolist() == [77] * 4
    # valid: a workspace larger than needed
    big = Band(np.full(dev.bytes // 8 + 6, np.nan))
    capi.bjacobi_apply(n, b, a["inv"], a["r"], a["z"], a["dots"], big.ptr, big.nbytes, 0, dtype=dtype)
    big.body("a larger workspace")
    _bits(dev.z.body(), bc.apply(host[0], host[1], b, dtype), "a larger workspace: z")


# ---- 7: eight PCG iterations on the 432-unknown case ------------------------------------------------------------------------------------

class _SpdHost:
    """What test_gpu_scaled.Dev reads of a host matrix."""

    def __init__(self):
        self.name = "spd_432"
        self.rows, self.p, self.c, self.v, self.b = bc.spd_case()
        self.cols = self.rows
        self.a32 = self.v.astype(np.float32)

    def values(self, kind):
        return self.v if kind == "c16_f64" else self.a32

    def vectors(self, kind):
        dtype = np.float32 if kind == "c16_f32xy" else np.float64
        return np.zeros(self.cols, dtype=dtype), np.zeros(self.rows, dtype=dtype), dtype


@pytest.mark.parametrize("dtype", bc.DTYPES, ids=["float64", "float32"])
def test_eight_pcg_iterations_with_3_by_3_blocks_verify_call_by_call(dtype):
    import torch
    b = 3
    h = _SpdHost()
    kind = "c16_f64" if dtype == np.float64 else "c16_f32xy"
    mdev = Dev(h, kind)
    plan = mdev.plan
    multiply = plan.spmv_f64_scaled_dots if dtype == np.float64 else plan.spmv_f32xy_scaled_dots
    n = h.rows
    tag = np.dtype(dtype).name
    # the inverse by the setup, from the fp64 values
    tp, tc, tv = (torch.from_numpy(a).to("cuda:0") for a in (h.p, h.c, h.v))
    inv = Band(np.full(n * b, np.nan), dtype)
    status = torch.full((2,), 77, dtype=torch.int32, device="cuda:0")
    capi.bjacobi_setup(n, b, tp, tc, tv, inv.ptr, status, 0, dtype=dtype)
    invh = inv.body(tag)
    _bits(invh, bc.spd_inverse(b, dtype), tag + ": the inverse of the setup")
    assert status.cpu().numpy().tolist() == [0, -1]
    x, r, p, q, z = (Band(np.zeros(n), dtype) for _ in range(5))
    r.set(h.b.astype(dtype))
    start = Band([0.0, 1.0])
    rz = [Band(np.full(2, np.nan)), Band(np.full(2, np.nan))]
    rr, pq = Band(np.full(2, np.nan)), Band(np.full(2, np.nan))
    kbytes, mbytes = capi.krylov_workspace_bytes(n), plan.dots_workspace_bytes()
    kwork, mwork = Band(np.full(kbytes // 8, np.nan)), Band(np.full(mbytes // 8, np.nan))
    bands = {"x": x, "r": r, "p": p, "q": q, "z": z, "rz0": rz[0], "rz1": rz[1], "rr": rr, "pq": pq}

    def snap():
        return {k: v.snap() for k, v in bands.items()}

    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        s = side.cuda_stream
        snaps = [("reset", snap())]
        capi.bjacobi_apply(n, b, inv.ptr, r.ptr, z.ptr, rz[0].ptr, kwork.ptr, kbytes, s, dtype=dtype)
        capi.cg_direction(n, start.ptr, start.ptr + 8, z.ptr, None, p.ptr, s, dtype=dtype)
        snaps.append(("begin", snap()))
        for it in range(bc.ITERATIONS):
            old, new = rz[it % 2], rz[1 - it % 2]
            multiply(mdev.tp.data_ptr(), mdev.ac, mdev.av, p.ptr, 1.0, 0.0, None, q.ptr, p.ptr, pq.ptr, mwork.ptr, mbytes, s)
            snaps.append(("multiply %d" % it, snap()))
            capi.cg_step(n, old.ptr, pq.ptr + 8, p.ptr, q.ptr, x.ptr, r.ptr, None, rr.ptr, kwork.ptr, kbytes, s, dtype=dtype)
            snaps.append(("step %d" % it, snap()))
            capi.bjacobi_apply(n, b, inv.ptr, r.ptr, z.ptr, new.ptr, kwork.ptr, kbytes, s, dtype=dtype)
            snaps.append(("apply %d" % it, snap()))
            capi.cg_direction(n, new.ptr, old.ptr, z.ptr, None, p.ptr, s, dtype=dtype)
            snaps.append(("direction %d" % it, snap()))
    side.synchronize()
    states = [(name, {k: bands[k].body(tag + ", " + name, sn[k]) for k in bands}) for name, sn in snaps]
    values = h.values(kind).astype(np.float64)
    before, after = states[0][1], states[1][1]
    _bits(after["z"], bc.apply(invh, before["r"], b, dtype), tag + ": z0")
    _within_bound(after["rz0"], after["z"], after["r"], tag + ": the dots of z0")
    _bits(after["p"], after["z"], tag + ": p = z0")
    first = float(np.sum(after["r"].astype(np.float64) ** 2))
    for (_, before), (name, after) in zip(states[1:], states[2:]):
        what = tag + ", " + name
        it = int(name.split()[-1])
        old, new = "rz%d" % (it % 2), "rz%d" % (1 - it % 2)
        changed = {"multiply": {"q", "pq"}, "step": {"x", "r", "rr"}, "apply": {"z", new}, "direction": {"p"}}[name.split()[0]]
        for key in before:
            if key not in changed:
                assert np.array_equal(after[key], before[key], equal_nan=True), what + ": %s changed" % key
        if name.startswith("multiply"):
            prod = values * before["p"].astype(np.float64)[h.c]
            ref, scale = np.add.reduceat(prod, h.p[:-1].astype(np.int64)), np.add.reduceat(np.abs(prod), h.p[:-1].astype(np.int64))
            err = np.abs(after["q"].astype(np.float64) - ref)
            cast = 0.0 if dtype == np.float64 else 2.0 ** -24 * np.abs(ref) + 2.0 ** -149
            assert np.all(err <= 2 * 16 * 2.0 ** -53 * scale * (1 + 2.0 ** -23) + cast), what + ": q is not A p"  # (rows of up to 15 entries)
            for j, t in enumerate(dc.products(after["q"], before["p"])):
                assert abs(after["pq"][j] - math.fsum(t)) <= dc.bound(t), what + ": the multiply's dots[%d]" % j
        elif name.startswith("step"):
            want_x, want_r = kc.restate_step(before[old][0], before["pq"][1], before["p"], before["q"], before["x"], before["r"], dtype)
            _bits(after["x"], want_x, what + ": x")
            _bits(after["r"], want_r, what + ": r")
        elif name.startswith("apply"):
            _bits(after["z"], bc.apply(invh, before["r"], b, dtype), what + ": z")
            _within_bound(after[new], after["z"], after["r"], what)
        else:
            _bits(after["p"], kc.restate_direction(before[new][0], before[old][0], before["z"], None, before["p"], dtype), what + ": p")
    last = float(states[-1][1]["rr"][0])
    diag = bc.pcg_restated(dtype, 1)[-1]
    print("%s: r'r of r0 %.6e, after %d iterations with 3 x 3 blocks %.6e (the restated diagonal run: %.6e)" % (tag, first, bc.ITERATIONS, last, diag))
    assert np.isfinite(last) and last < diag
    if dtype == np.float64:
        assert last < 1e-5 * first
    kwork.body(tag)
    mwork.body(tag)
    mdev.close()


# ---- 8: the gate ---------------------------------------------------------------------------------------------------------------------------

def test_gate_fused_apply_is_not_slower_than_bmm_and_dot():
    """n = 3 * 2^22 doubles, b = 3, one process, torch events on one stream; three warm-up rounds, 25 rounds alternating the two
    ways, medians.  Asserted: median(spmv_hip_bjacobi_apply_f64 with dots) <= 1.00 x median(the torch way), the torch way being
    torch.bmm of the (n / 3, 3, 3) view with r as (n / 3, 3, 1) into z, then torch.dot(r, z) -- no host read in either.  By bytes
    the fused call moves 40 n (the inverse 24, r 8, z 8 written) against 56 n (r and z read once more).  The inverse, r and z
    are 503 MB: beyond the 256 MiB Infinity Cache, which is asserted.  A condition, not a measured margin.
    Measured: the torch way 6768.4 us, the fused apply 97.4 us, ratio 0.014 against 0.714 by bytes; the apply moves its bytes at
    5.17 TB/s, 0.899 of the same-process triad (tools/bjacobi_ab.py in another process: 6824.8 against 96.2 us, and
    270.3 us for (inv3 * r3).sum(-1) + dot, the composition without the batched-GEMM dispatch)."""
    import torch
    b, n = 3, 3 * 2 ** 22
    assert (b + 2) * n * 8 > 256 * 2 ** 20 and n * 8 < 2 ** 32
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(5)
    inv = torch.rand(n * b, dtype=torch.float64, device="cuda:0", generator=gen) * 2 - 1
    r = torch.rand(n, dtype=torch.float64, device="cuda:0", generator=gen) * 2 - 1
    z, zt = torch.zeros(n, dtype=torch.float64, device="cuda:0"), torch.zeros(n, dtype=torch.float64, device="cuda:0")
    dots = torch.zeros(2, dtype=torch.float64, device="cuda:0")
    work = torch.zeros(capi.krylov_workspace_bytes(n) // 8, dtype=torch.float64, device="cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    inv3, r3, z3 = inv.view(n // b, b, b), r.view(n // b, b, 1), zt.view(n // b, b, 1)
    got = {}

    def torch_way():
        torch.bmm(inv3, r3, out=z3)
        got["dot"] = torch.dot(r, zt)

    def fused():
        capi.bjacobi_apply(n, b, inv, r, z, dots, work, None, s)

    torch_way()
    fused()
    # (torch may contract or reorder its three-term sums: a few roundings apart at the most)
    assert float((z - zt).abs().max()) <= 4 * 3 * 2.0 ** -53
    assert abs(float(dots[0]) - float(got["dot"])) <= 1e-10 * float(dots[1])
    med = _alternate({"torch": torch_way, "fused": fused})
    print("n %d, b %d: the torch way (bmm, dot) median %.1f us, the fused apply median %.1f us, ratio %.3f against %.3f by bytes; "
          "the fused apply moves %.2f TB/s" % (n, b, med["torch"], med["fused"], med["fused"] / med["torch"], 40.0 / 56.0,
                                                40.0 * n / med["fused"] * 1e-6))
    assert med["fused"] <= 1.00 * med["torch"], med
