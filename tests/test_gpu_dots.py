"""The scaled multiplies with dots (include/spmv_hip_dots.h) on the MI355X: spmv_hip_csr_spmv_{f32,c16,c16_f64,c16_f32xy}_scaled_dots,
spmv_hip_run_scaled_dots and spmv_hip_get_dots.

y_out is held bit for bit to the scaled sibling's.  The dots are held (a) bit for bit to integer sums on operands where every
order gives the same sum (dots_cases.IntHost), and (b) on test_gpu_scaled.Host's operands to rows 2^-53 sum |t_i| of
math.fsum(t), t_i the rounded products formed in numpy from the y_out the GPU returned: the a-priori bound of any summation order
over identically rounded products (test_dots_cases.py shows without a device that a lost row would exceed it tenfold).  Level 2
runs in test_gpu_scaled.py's guard scheme, with sentinels around the two dots and around the workspace, and the workspace (and
the dots) filled with NaN before every call: a slot that is read without having been written by that call shows as NaN."""
import json
import math
import subprocess

import numpy as np
import pytest

import dots_cases as dc
import helpers
import poison
import stream_helpers as sh
from spmv_amd import capi
from test_gpu_scaled import BUS, CLI, GUARD, KINDS, MATRICES, PAD, PAIRS, SENTINEL, UPLOADS, Dev, Vec, _alternate, _bits, _gate, host

pytestmark = pytest.mark.gpu

EDGE = 6  # doubles of sentinel in front of and behind the dots and the workspace (48 bytes: the body stays 16-byte aligned)


class Block:
    """n doubles on the device between EDGE sentinels; fill() makes the body NaN."""

    def __init__(self, n):
        import torch
        self.n = n
        self.t = torch.full((n + 2 * EDGE,), SENTINEL, dtype=torch.float64, device="cuda:0")
        self.ptr = self.t.data_ptr() + 8 * EDGE
        assert self.ptr % 16 == 0
        self.fill()

    def fill(self, value=float("nan")):
        self.t[EDGE:EDGE + self.n] = value

    def body(self, what=""):
        h = self.t.cpu().numpy()
        assert np.all(np.concatenate([h[:EDGE], h[EDGE + self.n:]]) == SENTINEL), what + ": written outside its elements"
        return h[EDGE:EDGE + self.n].copy()


class Dots:
    """A Dev (test_gpu_scaled.py) with the dots entry point of its kind, the two dots and a workspace of the plan's size."""

    def __init__(self, dev):
        self.dev, p = dev, dev.plan
        self.bytes = p.dots_workspace_bytes()
        assert self.bytes >= 16 and self.bytes % 16 == 0
        self.fn = {"f32": p.spmv_scaled_dots, "c16": p.spmv_scaled_dots, "c16_f64": getattr(p, "spmv_f64_scaled_dots", None),
                   "c16_f32xy": getattr(p, "spmv_f32xy_scaled_dots", None)}[dev.kind]
        self.dots, self.work = Block(2), Block(self.bytes // 8)

    def call(self, alpha, beta, y_in, y_out, w=None, matrix=True, x=True, stream=None, dots=None, work=None, fill=True):
        """One call; y_in and w a Vec, an address or None.  The dots and the workspace are NaN when it starts (filled on the current
        stream; fill=False: the caller has done that, for a call on another stream)."""
        d = self.dev
        dots, work = dots or self.dots, work or self.work
        if fill:
            dots.fill()
            work.fill()
        yi = y_in.ptr if isinstance(y_in, Vec) else y_in
        wp = w.ptr if isinstance(w, Vec) else w
        m = (d.tp.data_ptr(), d.ac, d.av) if matrix else (0, 0, 0)
        self.fn(m[0], m[1], m[2], d.x.ptr if x else 0, alpha, beta, yi, y_out.ptr, wp, dots.ptr, work.ptr, self.bytes,
                d.stream if stream is None else stream)

    def read(self, what="", dots=None, work=None):
        (work or self.work).body(what + ", the workspace")
        return (dots or self.dots).body(what + ", the dots")


def _same_dots(a, b, what):
    assert np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64)), "%s: %r against %r" % (what, a, b)


def _within_bound(got, v, w, what):
    """|dots[k] - fsum(t)| <= rows 2^-53 sum |t_i| over the products of v (y_out as the GPU stored it); +0.0 where w is None."""
    for k, t in enumerate(dc.products(v, w)):
        want, b = math.fsum(t), dc.bound(t)
        print("%s: dots[%d] %r, fsum %r, off by %.3e, bound %.3e" % (what, k, got[k], want, abs(got[k] - want), b))
        assert abs(got[k] - want) <= b, "%s: dots[%d] = %r, fsum of the products %r, bound %.3e" % (what, k, got[k], want, b)
    if w is None:
        _same_dots(got[1:], [0.0], what + ": the second dot without w is +0.0")


# ---- 1 and 3: y_out is the sibling's, the dots are within the bound, two calls and both placements give the same bits ------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", MATRICES)
def test_y_out_is_the_siblings_and_the_dots_are_within_the_bound(name, kind):
    h = host(name)
    wh = dc.general_w(h, kind)
    for flags in (0, capi.FLAG_EXACT_ORDER):
        dev = Dev(h, kind, flags)
        dd = Dots(dev)
        w_own = dev.vec(wh)
        for alpha, beta in PAIRS:
            tag = "%s, %s, flags %d, alpha %g, beta %g" % (name, kind, flags, alpha, beta)
            # the sibling, out of place
            y_in, ref = dev.vec(dev.y0), dev.out()
            dev.call(alpha, beta, y_in, ref)
            want = ref.body(tag)
            # out of place, w an array of its own
            out = dev.out()
            dd.call(alpha, beta, y_in, out, w_own)
            got = out.body(tag)
            d_out = dd.read(tag)
            _bits(got, want, tag + ": y_out out of place against the scaled sibling")
            _bits(y_in.body(tag), dev.y0, tag + ": y_in changed")
            _within_bound(d_out, got, wh, tag + ", w its own array")
            if alpha == 0.0 and beta == 0.0:
                _same_dots(d_out, [0.0, 0.0], tag + ": y_out is +0.0")
            # again: identical bits
            again = dev.out()
            dd.call(alpha, beta, y_in, again, w_own)
            _bits(again.body(tag), want, tag + ": y_out of a second call")
            _same_dots(dd.read(tag), d_out, tag + ": two identical calls")
            # in place: the same bits of y and of the dots
            y = dev.vec(dev.y0, SENTINEL)
            dd.call(alpha, beta, y, y, w_own)
            _bits(y.body(tag), want, tag + ": y_out in place against the scaled sibling")
            _same_dots(dd.read(tag), d_out, tag + ": in place against out of place")
            # w = x (square matrices: x' A x), else no w
            wx = dev.x if h.rows == h.cols else None
            out = dev.out()
            dd.call(alpha, beta, y_in, out, wx)
            got = out.body(tag)
            _bits(got, want, tag + ": y_out with w = x or null")
            _within_bound(dd.read(tag), got, dev.xh if wx is not None else None, tag + (", w = x" if wx is not None else ", w null"))
        dev.inputs_unchanged()
        _bits(w_own.body(), wh, "w changed")
        dev.close()


# ---- 2: exact dots ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", MATRICES)
def test_dots_of_integer_operands_are_the_integer_sums_bit_for_bit(name, kind):
    h = dc.int_host(name)
    for flags in (0, capi.FLAG_EXACT_ORDER):
        dev = Dev(h, kind, flags)
        dd = Dots(dev)
        for which in ("null", "own") + (("x",) if h.rows == h.cols else ()):
            wh = h.w_for(kind, which)[0]
            w = None if wh is None else (dev.x if which == "x" else dev.vec(wh))
            for alpha, beta in dc.INT_PAIRS:
                tag = "%s, %s, flags %d, alpha %d, beta %d, w %s" % (name, kind, flags, alpha, beta, which)
                steps = h.chain(alpha, beta, which)  # (the CPU precondition is asserted there)
                y = dev.vec(dev.y0, SENTINEL)
                for k, (yk, yy, wy) in enumerate(steps):
                    dd.call(float(alpha), float(beta), y, y, w)
                    got = dd.read(tag)
                    assert np.array_equal(y.body(tag).astype(np.float64), yk.astype(np.float64)), tag + ": y after call %d" % (k + 1)
                    _same_dots(got, [float(yy), float(wy)], tag + ": the dots of call %d against the integer sums" % (k + 1))
        dev.inputs_unchanged()
        dev.close()


# ---- 4: determinism across Level 1, streams and graph replay ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def side():
    s = sh.Side()
    yield s
    s.report()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["queen_40_32_24", "empty_rows", "no_entries"])
def test_run_scaled_dots_is_level_2_bit_for_bit(name, kind):
    h = host(name)
    upload, fmt = UPLOADS[kind]
    f32xy = kind == "c16_f32xy"
    for flags in (0, capi.FLAG_EXACT_ORDER):
        dev = Dev(h, kind, flags)
        dd = Dots(dev)
        with capi.Context(0, flags) as ctx:
            getattr(ctx, upload)(h.rows, h.cols, h.p, h.c, h.v)
            assert ctx.info()["format"] == fmt
            if h.cols:
                (ctx.set_x_f32 if f32xy else ctx.set_x)(dev.xh)
            for alpha, beta in PAIRS:
                tag = "%s, %s, flags %d, alpha %g, beta %g: level 1 against level 2" % (name, kind, flags, alpha, beta)
                (ctx.set_y_f32 if f32xy else ctx.set_y)(dev.y0)
                ctx.run_scaled_dots(alpha, beta, runs=3)
                got_d = ctx.get_dots()
                got = (ctx.get_y_f32 if f32xy else ctx.get_y)()[:h.rows]
                y = dev.vec(dev.y0, SENTINEL)
                for _ in range(3):
                    dd.call(alpha, beta, y, y, dev.x if h.rows == h.cols else None)
                _bits(got, y.body(), tag)
                _same_dots(got_d, dd.read(tag), tag + ", the dots")
                if h.rows and len(h.c):
                    assert ctx.last_run_ns() > 0
        dev.close()


@pytest.mark.parametrize("kind", KINDS)
def test_behind_a_delay_on_a_non_blocking_stream_and_on_two_streams_at_once(side, kind):
    """The call only enqueues: behind stream_helpers' delay on a non-blocking stream it returns while the delay runs, reads
    operands that arrive behind the delay, and gives the bits of a call on the null stream.  Two streams at once, each with its
    own workspace, dots and y_out, give those bits too."""
    import torch
    h = host("mixed_mesh_and_graph")
    dev = Dev(h, kind)
    dd = Dots(dev)
    y_in, ref = dev.vec(dev.y0), dev.out()
    dd.call(-1.0, 1.0, y_in, ref, dev.x if h.rows == h.cols else None)
    want_y, want_d = ref.body(), dd.read("null stream")
    xa, ya = sh.operand(dev.xh), sh.operand(dev.y0)
    ra = sh.result(np.zeros(h.rows, dtype=dev.dtype))
    db, wb = Block(2), Block(dd.bytes // 8)

    def call(stream):
        dd.fn(dev.tp.data_ptr(), dev.ac, dev.av, xa.ptr, -1.0, 1.0, ya.ptr, ra.ptr, xa.ptr if h.rows == h.cols else 0, db.ptr, wb.ptr, dd.bytes, stream)

    (body,), _ = sh.delayed(side, [xa, ya], call, [ra], "spmv_%s_scaled_dots behind the delay" % kind)
    _bits(body, want_y, kind + ": y_out behind the delay")
    wb.body("workspace behind the delay")
    _same_dots(db.body("dots behind the delay"), want_d, kind + ": the dots behind the delay")
    # two streams at once
    outs = [dev.out(), dev.out()]
    blocks = [(Block(2), Block(dd.bytes // 8)) for _ in side.streams]
    torch.cuda.synchronize()
    for rnd in range(3):
        for s, o, (d, w) in zip(side.streams, outs, blocks):
            dd.call(-1.0, 1.0, y_in, o, dev.x if h.rows == h.cols else None, stream=s.cuda_stream, dots=d, work=w, fill=False)
    for s in side.streams:
        s.synchronize()
    for o, (d, w) in zip(outs, blocks):
        _bits(o.body(), want_y, kind + ": y_out of two streams at once")
        _same_dots(dd.read("two streams", d, w), want_d, kind + ": the dots of two streams at once")
    dev.inputs_unchanged()
    dev.close()


@pytest.mark.parametrize("kind", KINDS)
def test_an_overwrite_call_captured_and_replayed_twice(kind):
    """q = 0.375 A x with x' q (beta == 0, y_in null), captured on one stream -- the tile kernel and the reduction behind it form a
    line -- and replayed twice: the bits of eager execution.  A call that synchronised or allocated would invalidate the capture."""
    import torch
    h = host("queen_40_32_24")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        dev = Dev(h, kind)
        dd = Dots(dev)
        q = dev.out()
        dd.call(0.375, 0.0, None, q, dev.x, stream=side.cuda_stream)
        side.synchronize()
        eager_q, eager_d = q.body("eager"), dd.read("eager")
        assert np.all(np.isfinite(eager_q)) and np.any(eager_q != 0) and np.all(np.isfinite(eager_d)) and eager_d[0] > 0
        dd.dots.fill()
        dd.work.fill()
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            dd.fn(dev.tp.data_ptr(), dev.ac, dev.av, dev.x.ptr, 0.375, 0.0, None, q.ptr, dev.x.ptr, dd.dots.ptr, dd.work.ptr, dd.bytes, side.cuda_stream)
        for replay in range(2):
            q.t[GUARD:GUARD + q.n] = float("nan")
            dd.dots.fill()
            dd.work.fill()
            g.replay()
            side.synchronize()
            _bits(q.body("replay"), eager_q, "%s: y_out of replay %d" % (kind, replay))
            _same_dots(dd.read("replay"), eager_d, "%s: the dots of replay %d" % (kind, replay))
        del g
        dev.inputs_unchanged()
        dev.close()


# ---- 5: non-finite data -----------------------------------------------------------------------------------------------------------

def _class_of_sum(t):
    """The class of a sum of products in any order: NaN if any is NaN or infinities of both signs meet, else the infinity's."""
    with np.errstate(invalid="ignore", over="ignore"):
        return poison.classes(np.array([np.sum(t)]))[0]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("where", ["x", "values", "y_in"])
def test_nan_and_inf_in_one_row_reach_the_dots_as_numpy_has_it(where, kind):
    """NaN, then +Inf, in what one row reads: through x (one column that only a few rows hold), through that row's stored values,
    through its y_in.  y_out keeps them in the rows that read them -- its classes are those of the clean result elsewhere, bit for
    bit -- and the classes of both dots are numpy's over the v the GPU stored."""
    h = host("rows_0_to_7_ragged_end")
    clean = Dev(h, kind)
    y_in, ref = clean.vec(clean.y0), clean.out()
    clean.call(1.0, 1.0, y_in, ref)
    clean_y = ref.body()
    wh = dc.general_w(h, kind)
    lens = np.diff(h.p.astype(np.int64))
    cand = np.nonzero(lens >= 2)[0]
    row = int(cand[len(cand) // 3])
    col = int(h.c[h.p[row]])
    for bad in (np.nan, np.inf):
        dev = Dev(h, kind)
        y0 = np.array(dev.y0, copy=True)
        if where == "x":
            xh = np.array(dev.xh, copy=True)
            xh[col] = bad
            dev.x, dev.xh = dev.vec(xh), xh
            hit = np.zeros(h.rows, dtype=bool)
            hit[np.repeat(np.arange(h.rows), lens)[h.c == col]] = True
        elif where == "values":
            vals = np.array(h.values(kind), copy=True)
            vals[h.p[row]] = bad
            import torch
            dev.bv[PAD:PAD + len(vals)] = torch.from_numpy(vals).to("cuda:0")
            hit = np.arange(h.rows) == row
        else:
            y0[row] = bad
            hit = np.arange(h.rows) == row
        assert hit.any() and hit.sum() < h.rows // 10
        dd = Dots(dev)
        tag = "%s, %s in %s" % (kind, bad, where)
        out = dev.out()
        dd.call(1.0, 1.0, dev.vec(y0), out, dev.vec(wh))
        got, d = out.body(tag), dd.read(tag)
        assert np.all(~np.isfinite(got[hit])) and np.all(np.isfinite(got[~hit])), tag + ": the non-finite value left its rows"
        poison.assert_finite_rows_bitwise(got, clean_y, np.where(hit, np.nan, 0.0), tag)
        t0, t1 = dc.products(got, wh)
        assert poison.classes(d[:1])[0] == _class_of_sum(t0) != poison.FINITE, tag + ": class of y' y"
        assert poison.classes(d[1:])[0] == _class_of_sum(t1) != poison.FINITE, tag + ": class of w' y"
        dev.close()
    clean.close()


@pytest.mark.parametrize("kind", KINDS)
def test_beta_0_with_y_in_full_of_nan_gives_finite_dots(kind):
    h = host("queen_40_32_24")
    dev = Dev(h, kind)
    dd = Dots(dev)
    for alpha in (1.0, 0.0):
        out = dev.out()
        dd.call(alpha, 0.0, dev.vec(np.full(h.rows, np.nan)), out, dev.x, matrix=alpha != 0.0, x=alpha != 0.0)
        d = dd.read()
        assert np.all(np.isfinite(out.body())) and np.all(np.isfinite(d)), (kind, alpha, d)
        ref = dev.out()
        dd.call(alpha, 0.0, None, ref, dev.x, matrix=alpha != 0.0, x=alpha != 0.0)
        _same_dots(dd.read(), d, "%s, alpha %g: y_in null against y_in full of NaN" % (kind, alpha))
    dev.close()


# ---- 6: refusals -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_refusals_launch_nothing_and_write_nothing(kind):
    h = host("queen_40_32_24")
    dev = Dev(h, kind)
    dd = Dots(dev)
    es = 4 if kind == "c16_f32xy" else 8
    tp, ac, av, x = dev.tp.data_ptr(), dev.ac, dev.av, dev.x.ptr
    big = dev.vec(np.concatenate([dev.y0, dev.y0]), SENTINEL)
    y_in, w = dev.vec(dev.y0), dev.vec(dc.general_w(h, kind))
    D, W, B, s = dd.dots.ptr, dd.work.ptr, dd.bytes, dev.stream
    dd.dots.fill(3.5)
    dd.work.fill(3.5)
    inv, ali = capi.ERR_INVALID, capi.ERR_ALIGN

    def inside(ptr):  # a 16-byte aligned address some way into the array at ptr
        return (ptr + 64 + 15) & ~15

    cases = [  # the sibling's
        ("y_out == x", (tp, ac, av, x, 1.0, 1.0, y_in.ptr, x, w.ptr, D, W, B), inv),
        ("partial overlap of y_in and y_out", (tp, ac, av, x, 1.0, 1.0, big.ptr, big.ptr + es * (h.rows // 2), w.ptr, D, W, B), inv),
        ("misaligned columns", (tp, ac + 4, av, x, 1.0, 1.0, y_in.ptr, big.ptr, w.ptr, D, W, B), ali),
        ("misaligned values", (tp, ac, av + 8, x, 1.0, 1.0, y_in.ptr, big.ptr, w.ptr, D, W, B), ali),
        ("null y_in with beta != 0", (tp, ac, av, x, 1.0, 0.5, 0, big.ptr, w.ptr, D, W, B), inv),
        ("null y_out", (tp, ac, av, x, 1.0, 0.0, 0, 0, w.ptr, D, W, B), inv),
        ("null values", (tp, ac, 0, x, 1.0, 1.0, y_in.ptr, big.ptr, w.ptr, D, W, B), inv),
        ("null x with alpha != 0", (tp, ac, av, 0, 1.0, 1.0, y_in.ptr, big.ptr, w.ptr, D, W, B), inv),
        # the dots' own
        ("null dots", (tp, ac, av, x, 1.0, 1.0, y_in.ptr, big.ptr, w.ptr, 0, W, B), inv),
        ("null workspace", (tp, ac, av, x, 1.0, 1.0, y_in.ptr, big.ptr, w.ptr, D, 0, B), inv),
        ("work_bytes one byte short", (tp, ac, av, x, 1.0, 1.0, y_in.ptr, big.ptr, w.ptr, D, W, B - 1), inv),
        ("work_bytes 0 with alpha == 0", (0, 0, 0, 0, 0.0, 1.0, y_in.ptr, big.ptr, w.ptr, D, W, 0), inv),
        ("dots off 16-byte alignment", (tp, ac, av, x, 1.0, 1.0, y_in.ptr, big.ptr, w.ptr, D + 8, W, B), ali),
        ("workspace off 16-byte alignment", (tp, ac, av, x, 1.0, 1.0, y_in.ptr, big.ptr, w.ptr, D, W + 8, B), ali),
        ("w == y_out", (tp, ac, av, x, 1.0, 1.0, y_in.ptr, big.ptr, big.ptr, D, W, B), inv),
        ("w overlapping y_out by one element", (tp, ac, av, x, 1.0, 1.0, y_in.ptr, big.ptr, big.ptr + es * (h.rows - 1), D, W, B), inv),
        ("w == y_in == y_out, in place", (tp, ac, av, x, 1.0, 1.0, big.ptr, big.ptr, big.ptr, D, W, B), inv),
        ("dots inside the workspace", (tp, ac, av, x, 1.0, 1.0, y_in.ptr, big.ptr, w.ptr, W + 16, W, B), inv),
        ("dots inside y_out", (tp, ac, av, x, 1.0, 1.0, y_in.ptr, big.ptr, w.ptr, inside(big.ptr), W, B), inv),
        ("dots inside x", (tp, ac, av, x, 1.0, 1.0, y_in.ptr, big.ptr, w.ptr, inside(x), W, B), inv),
        ("dots inside w", (tp, ac, av, x, 1.0, 1.0, y_in.ptr, big.ptr, w.ptr, inside(w.ptr), W, B), inv),
        ("dots inside y_in", (tp, ac, av, x, 1.0, 1.0, y_in.ptr, big.ptr, w.ptr, inside(y_in.ptr), W, B), inv),
        ("dots inside the values", (tp, ac, av, x, 1.0, 1.0, y_in.ptr, big.ptr, w.ptr, inside(av), W, B), inv),
        ("dots inside the columns", (tp, ac, av, x, 1.0, 1.0, y_in.ptr, big.ptr, w.ptr, inside(ac), W, B), inv),
        ("dots inside row_ptr", (tp, ac, av, x, 1.0, 1.0, y_in.ptr, big.ptr, w.ptr, inside(tp), W, B), inv),
        ("workspace inside the values", (tp, ac, av, x, 1.0, 1.0, y_in.ptr, big.ptr, w.ptr, D, inside(av), B), inv),
        ("workspace ending inside the dots", (tp, ac, av, x, 1.0, 1.0, y_in.ptr, big.ptr, w.ptr, D, D - B + 16, B), inv)]
    if kind == "c16_f32xy":
        cases += [("misaligned float w", (tp, ac, av, x, 1.0, 1.0, y_in.ptr, big.ptr, w.ptr + 2, D, W, B), ali),
                  ("misaligned float y_out", (tp, ac, av, x, 1.0, 0.0, 0, big.ptr + 2, w.ptr, D, W, B), ali)]
    for what, args, code in cases:
        with pytest.raises(capi.SpmvHipError) as e:
            dd.fn(*args, s)
        assert e.value.code == code, "%s: %s" % (what, e.value)
    dev.torch.cuda.synchronize()
    _bits(big.body("refused calls"), np.concatenate([dev.y0, dev.y0]), "a refused call wrote y")
    _bits(y_in.body("refused calls"), dev.y0, "a refused call wrote y_in")
    assert np.all(dd.dots.body("refused calls") == 3.5), "a refused call wrote the dots"
    assert np.all(dd.work.body("refused calls") == 3.5), "a refused call wrote the workspace"
    # valid: w == x (x' A x), w == y_in out of place, and a workspace larger than needed
    assert h.rows == h.cols
    out, ref = dev.out(), dev.out()
    dd.call(1.0, 1.0, y_in, out, dev.x)
    d1 = dd.read()
    dd.call(1.0, 1.0, y_in, ref, dev.vec(dev.xh))
    _same_dots(d1, dd.read(), "w == x against w a copy of x")
    dd.call(1.0, 1.0, y_in, out, y_in)
    d2 = dd.read()
    dd.call(1.0, 1.0, y_in, ref, dev.vec(dev.y0))
    _same_dots(d2, dd.read(), "w == y_in against w a copy of y_in")
    dev.inputs_unchanged()
    dev.close()


def test_a_plan_whose_x_spans_4_gib_is_refused():
    """cols * 8 >= 2^32 with one stored entry: the plan is a few bytes, and the call is refused before any array is looked at."""
    import torch
    cols = 2 ** 29
    p = np.array([0, 1], dtype=np.int32)
    c = np.array([0], dtype=np.int32)
    plan = capi.C16Plan(1, cols, p, c, 0, torch.cuda.current_stream().cuda_stream)
    d, w = Block(2), Block(plan.dots_workspace_bytes() // 8)
    d.fill(3.5)
    buf = torch.zeros(8, dtype=torch.float64, device="cuda:0")
    with pytest.raises(capi.SpmvHipError) as e:
        plan.spmv_f64_scaled_dots(buf.data_ptr(), buf.data_ptr() + 16, buf.data_ptr() + 32, buf.data_ptr() + 48, 0.0, 0.0, None,
                                  buf.data_ptr() + 56, None, d.ptr, w.ptr, plan.dots_workspace_bytes(), 0)
    assert e.value.code == capi.ERR_INVALID and "4 GiB" in str(e.value)
    torch.cuda.synchronize()
    assert np.all(d.body() == 3.5) and torch.all(buf == 0)
    plan.close()


def test_run_scaled_dots_and_get_dots_refuse_other_states_and_leave_y_untouched():
    h = host("queen_40_32_24")
    with capi.Context(0) as ctx:
        for fn in (lambda: ctx.run_scaled_dots(1.0, 0.0), ctx.get_dots):
            with pytest.raises(capi.SpmvHipError) as e:
                fn()
            assert e.value.code == capi.ERR_STATE
        with pytest.raises(capi.SpmvHipError) as e:
            ctx.run_scaled_dots(1.0, 0.0)
        assert "format 0" in str(e.value)
        ctx.upload_csr(h.rows, h.cols, h.p, h.c, h.v)
        ctx.set_x(h.x)
        ctx.set_y(h.y0)
        with pytest.raises(capi.SpmvHipError) as e:
            ctx.run_scaled_dots(2.0, 0.0)
        assert e.value.code == capi.ERR_STATE and "format 1" in str(e.value)
        helpers.assert_bitexact(ctx.get_y(), h.y0, "a refused run_scaled_dots changed y")
        ctx.upload_csr_compact_f64(h.rows, h.cols, h.p, h.c, h.v)
        ctx.set_x(h.x)
        ctx.set_y(h.y0)
        with pytest.raises(capi.SpmvHipError) as e:
            ctx.get_dots()  # no run yet
        assert e.value.code == capi.ERR_STATE
        ctx.run_scaled_dots(-1.0, 1.0)
        d = ctx.get_dots()
        assert np.all(np.isfinite(d)) and d[0] > 0
        for other in (ctx.run, lambda: ctx.run_scaled(1.0, 1.0)):
            other()
            with pytest.raises(capi.SpmvHipError) as e:
                ctx.get_dots()  # the last run was a plain one
            assert e.value.code == capi.ERR_STATE
            ctx.run_scaled_dots(0.0, 1.0)
            ctx.get_dots()
        ctx.upload_csr_compact_f64(h.rows, h.cols, h.p, h.c, h.v)
        with pytest.raises(capi.SpmvHipError) as e:
            ctx.get_dots()  # a re-upload: the dots were another matrix's
        assert e.value.code == capi.ERR_STATE
    with capi.Context(num_gpus=1) as m:
        m.upload_csr(h.rows, h.cols, h.p, h.c, h.v)
        m.set_y(h.y0)
        for fn in (lambda: m.run_scaled_dots(1.0, 1.0), m.get_dots):
            with pytest.raises(capi.SpmvHipError) as e:
                fn()
            assert e.value.code == capi.ERR_STATE
        helpers.assert_bitexact(m.get_y(), h.y0, "a refused run_scaled_dots changed y of the multi-device context")


# ---- 7: the host program -------------------------------------------------------------------------------------------------------------

def test_cli_compact_f64_residual_steps_with_dots_check():
    base = [CLI, "--csr", BUS, "--device", "hip", "--compact=f64", "--alpha", "-1", "--beta", "1", "--threads", "1", "--profile", "4", "--check"]
    r = subprocess.run(base + ["--dots"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    doc = json.loads(r.stdout)  # one JSON document
    assert doc
    text = r.stdout
    assert '"hip-csr-spmv-compact-f64"' in text and '"alpha": -1' in text and '"beta": 1' in text
    import re
    m = json.loads("[" + re.search(r'"dots":\s*\[([^\]]*)\]', text).group(1) + "]")
    assert len(m) == 2 and all(isinstance(v, float) or isinstance(v, int) for v in m) and m[0] > 0
    assert '"restated": [' in text and '"bound": [' in text and '"pass": false' not in text and text.count('"pass": true') == 2, text[-1200:]
    plain = subprocess.run(base, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert plain.returncode == 0 and "dots" not in plain.stdout and '"restated": [' not in plain.stdout


# ---- the two gates -----------------------------------------------------------------------------------------------------------------

def _gate_dots():
    import torch
    d = _gate()
    if "dots" not in d:
        d["bytes"] = d["plan"].dots_workspace_bytes()
        d["dots"] = torch.zeros(2, dtype=torch.float64, device="cuda:0")
        d["work"] = torch.zeros(d["bytes"] // 8, dtype=torch.float64, device="cuda:0")
    return d


def test_gate_fused_x_dot_q_is_not_slower_than_the_multiply_and_a_dot():
    """Gate (a): q = A p with p' q on Poisson 4096^2 through a C16Plan, Level 2, one process, torch events on one stream.  Asserted:
    median(spmv_hip_csr_spmv_c16_scaled_dots, alpha 1, beta 0, w = x) <= 1.00 x median(spmv_hip_csr_spmv_c16_scaled + torch.dot(x, y)):
    the fused call reads two vectors less, plus the few MB of slots, in no more launches.  A condition, not a measured margin.
    Printed, not asserted: the ratio the byte counts promise, and fused / the scaled sibling alone (the price of the epilogue and
    the reduction).
    Measured: scaled + torch.dot 240.4 us, fused 212.0 us, ratio 0.882 against 0.881 by bytes; the scaled sibling alone 186.0 us,
    fused / sibling 1.140 (tools/dots_ab.py in another process: 238.0 against 212.1 us, 0.891)."""
    import torch
    d = _gate_dots()
    plan, rows, s = d["plan"], d["rows"], torch.cuda.current_stream().cuda_stream
    streamed = d["info"]["streamed_bytes"] - 8 * rows  # the overwrite form: y is written, not read
    assert streamed > 256 * 2 ** 20
    P, A, X, Y, D, W = (d[k].data_ptr() for k in ("p", "a32", "x", "y", "dots", "work"))
    B = d["bytes"]
    slots = 2 * 16 * d["info"]["tiles"]  # written by the tiles, read by the reduction
    print("streamed bytes: scaled %d + dot %d, fused %d + slots %d: expected ratio %.3f" % (
        streamed, 16 * rows, streamed + 8 * rows, slots, (streamed + 8 * rows + slots) / (streamed + 16 * rows)))
    got = {}

    def two_step():
        plan.spmv_scaled(P, 0, A, X, 1.0, 0.0, None, Y, s)
        got["dot"] = torch.dot(d["x"], d["y"])

    two_step()
    want_y = d["y"].clone()
    d["y"].zero_()
    plan.spmv_scaled_dots(P, 0, A, X, 1.0, 0.0, None, Y, X, D, W, B, s)
    assert torch.equal(d["y"], want_y)
    fused, ref = float(d["dots"][1]), float(got["dot"])
    assert abs(fused - ref) <= 1e-10 * float(torch.dot(d["x"].abs(), d["y"].abs())), (fused, ref)
    med = _alternate({"scaled + torch.dot": two_step,
                      "fused": lambda: plan.spmv_scaled_dots(P, 0, A, X, 1.0, 0.0, None, Y, X, D, W, B, s),
                      "scaled alone": lambda: plan.spmv_scaled(P, 0, A, X, 1.0, 0.0, None, Y, s)})
    print("scaled + torch.dot median %.1f us, fused median %.1f us, ratio %.3f; scaled alone %.1f us, fused / scaled alone %.3f" % (
        med["scaled + torch.dot"], med["fused"], med["fused"] / med["scaled + torch.dot"], med["scaled alone"], med["fused"] / med["scaled alone"]))
    assert med["fused"] <= 1.00 * med["scaled + torch.dot"], med


def test_gate_fused_residual_norm_is_not_slower_than_the_residual_and_a_dot():
    """Gate (b): r = b - A x with r' r through spmv_hip_csr_spmv_c16_f64_scaled_dots (alpha -1, beta 1, y_in = b, w null) against
    spmv_hip_csr_spmv_c16_f64_scaled followed by torch.dot(r, r), on the same matrix.  Asserted: fused <= 1.00 x the two-step way.
    Measured: scaled + torch.dot 285.2 us, fused 251.2 us, ratio 0.881 against 0.909 by bytes; the scaled sibling alone 241.1 us,
    fused / sibling 1.042 (tools/dots_ab.py in another process: 282.8 against 250.7 us, 0.886)."""
    import torch
    d = _gate_dots()
    plan, rows, s = d["plan"], d["rows"], torch.cuda.current_stream().cuda_stream
    streamed = d["info"]["streamed_bytes"] + 4 * d["info"]["stored_entries"]
    assert streamed > 256 * 2 ** 20
    P, A, X, Bv, R, D, W = (d[k].data_ptr() for k in ("p", "a64", "x", "b", "r", "dots", "work"))
    B = d["bytes"]
    slots = 2 * 16 * d["info"]["tiles"]
    print("streamed bytes: scaled %d + dot %d, fused %d + slots %d: expected ratio %.3f" % (
        streamed, 8 * rows, streamed, slots, (streamed + slots) / (streamed + 8 * rows)))
    got = {}

    def two_step():
        plan.spmv_f64_scaled(P, 0, A, X, -1.0, 1.0, Bv, R, s)
        got["dot"] = torch.dot(d["r"], d["r"])

    two_step()
    want_r = d["r"].clone()
    d["r"].zero_()
    plan.spmv_f64_scaled_dots(P, 0, A, X, -1.0, 1.0, Bv, R, None, D, W, B, s)
    assert torch.equal(d["r"], want_r)
    fused, ref = float(d["dots"][0]), float(got["dot"])
    assert abs(fused - ref) <= 1e-10 * ref and float(d["dots"][1]) == 0.0, (fused, ref)
    med = _alternate({"scaled + torch.dot": two_step,
                      "fused": lambda: plan.spmv_f64_scaled_dots(P, 0, A, X, -1.0, 1.0, Bv, R, None, D, W, B, s),
                      "scaled alone": lambda: plan.spmv_f64_scaled(P, 0, A, X, -1.0, 1.0, Bv, R, s)})
    print("scaled + torch.dot median %.1f us, fused median %.1f us, ratio %.3f; scaled alone %.1f us, fused / scaled alone %.3f" % (
        med["scaled + torch.dot"], med["fused"], med["fused"] / med["scaled + torch.dot"], med["scaled alone"], med["fused"] / med["scaled alone"]))
    assert med["fused"] <= 1.00 * med["scaled + torch.dot"], med
