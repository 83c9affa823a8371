"""include/spmv_hip_coarse.h on the MI355X: spmv_hip_coarse_setup_{f64,f32} and spmv_hip_coarse_apply_{f64,f32}, through
capi.coarse_setup and capi.coarse_apply.

The inverse, its padding, the status and every z are held bit for bit to the numpy restatement of the header (coarse_cases;
test_coarse_cases.py holds that restatement to numpy.linalg.inv without a device): NaNs in the same positions, every other value
the same bits.  Every device array lies between guards that are checked whenever it is read back."""
import math

import numpy as np
import pytest

import agg_cases as ac
import agg_mis2_cases as a2
import coarse_cases as cc
import dots_cases as dc
import mcgs_cases as mc
from spmv_amd import capi
from test_coarse_cases import RESIDUAL_RATIO
from test_gpu_agg import _body, _ints, _t
from test_gpu_agg_mis2 import Level2
from test_gpu_krylov import GUARD, Band
from test_gpu_mcgs import _Host, _pcg
from test_gpu_scaled import Dev, _bits

pytestmark = pytest.mark.gpu


def _same(got, want, what):
    assert np.asarray(got).dtype == np.asarray(want).dtype and cc.same(got, want), what + ": not the restatement's bits"


class Coarse:
    """A CSR matrix on the device (or the device arrays of a level) and what spmv_hip_coarse_setup_* makes of it."""

    def __init__(self, n, p, c, v, dtype, device=None):
        import torch
        self.n, self.ld, self.dtype = n, cc.ld_of(n), np.dtype(dtype)
        self.p, self.c, self.v = device or (_t(p, np.int32), _t(np.concatenate([c, [0]]), np.int32), _t(np.concatenate([v, [0.0]]), np.float64))
        self.inv = Band(np.full(n * self.ld, np.nan), dtype)
        self.status = _ints(3)
        self.bytes = capi.coarse_workspace_bytes(n)
        assert self.bytes == cc.workspace_of(n)
        self.work = torch.full((self.bytes // 8 + 2,), float("nan"), dtype=torch.float64, device="cuda:0")

    def setup(self, stream=0):
        capi.coarse_setup(self.n, self.p, self.c, self.v, self.inv.ptr, self.status, self.work, self.bytes, stream, dtype=self.dtype)

    def read(self, what):
        """(inv (n, ld), status) with the guards and the end of the workspace looked at."""
        assert np.all(np.isnan(self.work[self.bytes // 8:].cpu().numpy())), what + ": setup wrote behind its workspace"
        return self.inv.body(what).reshape(self.n, self.ld), _body(self.status, 3, what + ": d_status").tolist()


# ---- 1: the set-up, bit for bit the restatement --------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", cc.CASES)
def test_inverse_padding_and_status_are_the_restatement(name):
    n, p, c, v, status, _ = cc.case(name)
    for dtype in cc.DTYPES:
        tag = "%s, %s" % (name, np.dtype(dtype).name)
        want, want_status = cc.restated(name, dtype)
        m = Coarse(n, p, c, v, dtype)
        m.setup()
        got, got_status = m.read(tag)
        print("%s: %d rows, status %s" % (tag, n, got_status))
        assert got_status == want_status == status, tag
        _same(got, want, tag + ": the inverse")
        assert np.all(got[:, n:] == 0.0) and not np.signbit(got[:, n:]).any(), tag + ": the padding columns are +0.0"
        if name in ("nan", "inf"):
            assert np.array_equal(np.isnan(got), np.isnan(want))
        assert np.array_equal(m.p.cpu().numpy(), p) and np.array_equal(m.c.cpu().numpy()[:-1], c), tag + ": the matrix changed"
        assert np.array_equal(m.v.cpu().numpy()[:-1].view(np.uint64), v.view(np.uint64)), tag + ": the values changed"


# ---- 2: the apply ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", cc.DTYPES, ids=["float64", "float32"])
def test_apply_is_the_restatement_bit_for_bit_at_every_size(dtype):
    for n in cc.SIZES:
        tag = "%d rows, %s" % (n, np.dtype(dtype).name)
        z = Band(np.full(n, np.nan), dtype)
        # integers: every order of every sum is exact
        ih, rh, zh = cc.int_operands(n, dtype)
        inv, r = Band(ih.ravel(), dtype), Band(rh, dtype)
        capi.coarse_apply(n, inv.ptr, r.ptr, z.ptr, dtype=dtype)
        got = z.body(tag)
        assert got.dtype == dtype
        _bits(got, zh, tag + ": z of integer operands")
        # general values, NaN in the padding columns
        gh, rg = cc.general_operands(n, dtype)
        inv.set(gh.ravel())
        r.set(rg)
        z.fill()
        capi.coarse_apply(n, inv.ptr, r.ptr, z.ptr, dtype=dtype)
        want = cc.apply(gh, n, rg, dtype)
        got = z.body(tag)
        assert np.all(np.isfinite(got)), tag + ": a padding column was read into a sum"
        _bits(got, want, tag + ": z of general operands")
        # a NaN and an Inf in one row of the inverse reach that z alone
        for i, j, bad in ((0, n - 1, np.nan), (n // 2, 0, np.inf), (n - 1, n // 2, np.nan)) if n else ():
            hurt = gh.copy()
            hurt[i, j] = bad
            inv.set(hurt.ravel())
            z.fill()
            capi.coarse_apply(n, inv.ptr, r.ptr, z.ptr, dtype=dtype)
            got = z.body(tag)
            assert np.flatnonzero(~np.isfinite(got)).tolist() == [i], (tag, i, j)
            keep = np.arange(n) != i
            _bits(got[keep], want[keep], tag + ": the other rows beside a non-finite inv[%d][%d]" % (i, j))
        _bits(r.body(tag), rg, tag + ": r changed")
        _same(inv.body(tag), (hurt if n else gh).ravel(), tag + ": the inverse changed")


# ---- 3: two calls, a stream, a graph --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", cc.DTYPES, ids=["float64", "float32"])
def test_two_calls_a_side_stream_and_a_replayed_graph_give_identical_bits(dtype):
    import torch
    n, p, c, v, _, _ = cc.case("size_65")
    tag = np.dtype(dtype).name
    want, want_status = cc.restated("size_65", dtype)
    rh = np.random.default_rng(65).uniform(-1.0, 1.0, size=n).astype(dtype)
    want_z = cc.apply(want, n, rh, dtype)
    m = Coarse(n, p, c, v, dtype)
    r, z = Band(rh, dtype), Band(np.full(n, np.nan), dtype)

    def both(stream):
        m.setup(stream)
        capi.coarse_apply(n, m.inv.ptr, r.ptr, z.ptr, stream, dtype=dtype)

    def check(want_inv, want_z, what):
        got, status = m.read(what)
        assert status == want_status
        _same(got, want_inv, what + ": the inverse")
        _bits(z.body(what), want_z, what + ": z")

    for run in range(2):
        m.inv.fill()
        z.fill()
        both(0)
        torch.cuda.synchronize()
        check(want, want_z, "%s, call %d" % (tag, run))
    side = torch.cuda.Stream()
    m.inv.fill()
    z.fill()
    torch.cuda.synchronize()
    both(side.cuda_stream)
    side.synchronize()
    check(want, want_z, tag + ", a side stream")
    # a captured graph of set-up and apply, replayed twice, the second time behind a change of the values
    cap = torch.cuda.Stream()
    m.inv.fill()
    z.fill()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cap):
        both(torch.cuda.current_stream().cuda_stream)
    assert np.all(np.isnan(z.body(tag))) and np.all(np.isnan(m.inv.body(tag))), tag + ": the capture ran the calls"
    g.replay()
    torch.cuda.synchronize()
    check(want, want_z, tag + ", the replayed graph")
    v2 = np.random.default_rng(66).uniform(-1.0, 1.0, size=len(v))
    m.v[:len(v)] = _t(v2, np.float64)
    g.replay()
    torch.cuda.synchronize()
    want2, status2 = cc.setup(n, p, c, v2, dtype)
    assert status2 == want_status and not cc.same(want2, want)
    check(want2, cc.apply(want2, n, rh, dtype), tag + ", the graph replayed behind a change of d_value")
    del g


# ---- 4: the largest matrix ------------------------------------------------------------------------------------------------------------

def test_2048_rows_in_doubles_by_residual_and_2049_refused():
    import torch
    n, p, c, v, A = cc.banded_2048()
    m = Coarse(n, p, c, v, np.float64)
    m.setup()
    got, status = m.read("2048 rows")
    assert status == [0, -1, 0]
    Ad = _t(A, np.float64)
    eye = torch.eye(n, dtype=torch.float64, device="cuda:0")
    mine = float((Ad @ _t(got[:, :n], np.float64) - eye).abs().max())
    torchs = float((Ad @ torch.linalg.inv(Ad) - eye).abs().max())
    print("2048 rows, seven diagonals: max |A X - I| %.3e, torch.linalg.inv's %.3e, ratio %.2f" % (mine, torchs, mine / max(torchs, 2.0 ** -53)))
    assert mine <= RESIDUAL_RATIO * max(torchs, 2.0 ** -53)
    for call in (lambda: capi.coarse_setup(2049, m.p, m.c, m.v, m.inv.ptr, m.status, m.work, 2 ** 40, dtype=np.float64),
                 lambda: capi.coarse_apply(2049, m.inv.ptr, m.inv.ptr, m.inv.ptr, dtype=np.float64),
                 lambda: capi.coarse_workspace_bytes(2049)):
        with pytest.raises(capi.SpmvHipError) as e:
            call()
        assert e.value.code == capi.ERR_INVALID
    _same(m.read("2048 rows behind the refusals")[0], got, "a refused call wrote")


# ---- 5: eight PCG iterations on poisson2D.mtx ---------------------------------------------------------------------------------------------

def test_eight_pcg_iterations_on_poisson2d_with_the_library_solving_the_coarse_level():
    """The two-level cycle of test_gpu_agg_mis2.py with spmv_hip_coarse_setup_f64 and spmv_hip_coarse_apply_f64 for the coarse
    solve.  Every call is held to ITS OWN inputs as the device stored them: the smoothing steps, the restriction, the coarse solve
    (against the restated apply of the restated inverse) and the prolongation bit for bit, the multiplies to two summation orders.
    The final r'r is the recorded one of the cycle with torch.linalg.inv to 1e-6: the two solves differ by rounding only.
    Measured: r'r 6.721731e-03 after eight iterations (relative difference from the recorded value below 1e-7)."""
    import torch
    dtype, omega = np.float64, 1.0
    h = _Host()
    mdev = Dev(h, "c16_f64")
    m = Level2(*ac.matrix("poisson2D"))
    m.aggregate_mis2()
    m.plan_()
    m.symbolic()
    pl, _ = a2.plan("poisson2D")
    co = a2.coarse("poisson2D")
    G = capi.agg_group(m.plan)
    n, na = h.rows, pl.aggregates
    assert na == 38
    cv = m.numeric()
    _bits(cv, co.values(h.v), "the coarse values")
    coarse = Coarse(na, None, None, None, dtype, device=(m.cp, m.cc, m.cv))
    coarse.setup()
    inv_h, status = coarse.read("the coarse level of poisson2D")
    want_inv, want_status = cc.restated("poisson2D_Ac", dtype)
    assert status == want_status == [0, -1, 0]
    _same(inv_h, want_inv, "the inverse of the coarse level")
    assert np.all(_body(m.cp, na + 1, "d_coarse_row_ptr") == co.row_ptr), "the set-up changed the level's arrays"
    smooth_h = ac.smoother_of(n, h.p, h.c, h.v, dtype)
    smooth = Band(smooth_h)
    t, rc, ec = Band(np.full(n, np.nan)), Band(np.full(na, np.nan)), Band(np.full(na, np.nan))
    multiply = mdev.plan.spmv_f64_scaled
    taken = []

    def view(band):
        return band.t[GUARD:GUARD + band.n]

    def cycle(r, z, dots, work, nbytes, s):
        shots = []
        capi.bjacobi_apply(n, 1, smooth.ptr, r.ptr, z.ptr, None, None, 0, s, dtype=dtype)
        shots.append(z.snap())
        multiply(mdev.tp.data_ptr(), mdev.ac, mdev.av, z.ptr, -1.0, 1.0, r.ptr, t.ptr, s)
        shots.append(t.snap())
        capi.agg_restrict_group(m.plan, G, t.ptr, rc.ptr, s, dtype=dtype)
        shots.append(rc.snap())
        capi.coarse_apply(na, coarse.inv.ptr, rc.ptr, ec.ptr, s, dtype=dtype)
        shots.append(ec.snap())
        capi.agg_prolong_add(m.plan, omega, ec.ptr, z.ptr, s, dtype=dtype)
        shots.append(z.snap())
        multiply(mdev.tp.data_ptr(), mdev.ac, mdev.av, z.ptr, -1.0, 1.0, r.ptr, t.ptr, s)
        shots.append(t.snap())
        capi.bjacobi_apply_add(n, 1, smooth.ptr, t.ptr, z.ptr, s, dtype=dtype)
        view(dots)[0] = torch.dot(view(r), view(z))
        view(dots)[1] = 0.0
        taken.append(shots)

    values = h.v.astype(np.float64)
    longest = int(np.diff(h.p).max())
    starts = h.p[:-1].astype(np.int64)

    def residual_ok(got, r, z, what):
        prod = values * z[h.c]
        ref, scale = r - np.add.reduceat(prod, starts), np.abs(r) + np.add.reduceat(np.abs(prod), starts)
        assert np.all(np.abs(got - ref) <= 2 * (longest + 2) * 2.0 ** -53 * scale), what + ": not r - A z"

    def _of(snap, count):
        a = snap.cpu().numpy()
        assert np.all(np.isnan(np.concatenate([a[:GUARD], a[GUARD + count:]])))
        return a[GUARD:GUARD + count].copy()

    def cycle_verify(r, z, dots, what):
        shots = taken.pop(0)
        z1, z2 = _of(shots[0], n), _of(shots[4], n)
        t1, rc1, ec1, t2 = t.body(what, shots[1]), rc.body(what, shots[2]), ec.body(what, shots[3]), t.body(what, shots[5])
        _bits(z1, smooth_h * r, what + ": z = minv r")
        residual_ok(t1, r, z1, what + ", the first residual")
        _bits(rc1, a2.restrict_group(pl, G, t1, dtype), what + ": r_c against the restatement")
        _bits(ec1, cc.apply(want_inv, na, rc1, dtype), what + ": e_c = inv r_c against the restatement")
        _bits(z2, ac.prolong_add(pl, omega, ec1, z1, dtype), what + ": z += omega P e_c against the restatement")
        residual_ok(t2, r, z2, what + ", the second residual")
        _bits(z, z2 + smooth_h * t2, what + ": z += minv t")
        prod = r * z
        assert abs(dots[0] - math.fsum(prod)) <= dc.bound(prod), what + ": r'z"

    first, last = _pcg(h, mdev, dtype, cycle, cycle_verify)
    assert not taken
    print("r'r of r0 %.6e; after %d iterations with the two-level cycle over %d distance-2 aggregates and the library's coarse solve %.9e, "
          "recorded with torch.linalg.inv %.6e: relative difference %.3e" % (first, ac.ITERATIONS, na, last, cc.PCG_RR, abs(last - cc.PCG_RR) / cc.PCG_RR))
    assert first == 367.0
    assert abs(last - cc.PCG_RR) <= 1e-6 * cc.PCG_RR
    _same(coarse.read("behind the iterations")[0], want_inv, "the iterations changed the inverse")
    mdev.close()


# ---- 6: the 512 x 512 grid's third level, coarsened on the device ----------------------------------------------------------------------

def test_the_376_row_level_of_the_512_grid_is_inverted_as_the_restatement_does_and_solves_to_1e_10():
    rows, p, c, v = mc.grid(512, 512)
    for _ in range(3):
        m = Level2(rows, p, c, v)
        m.aggregate_mis2()
        m.plan_()
        nnz_c = m.symbolic()
        v = m.numeric().copy()
        rows, p, c = m.plan.aggregates, _body(m.cp, m.plan.aggregates + 1, "d_coarse_row_ptr").copy(), _body(m.cc, m.nnz, "d_coarse_column_index")[:nnz_c].copy()
    n, hp, hc, hv = cc.grid_512_level_3()
    assert rows == n == 376 and np.array_equal(p, hp) and np.array_equal(c, hc)
    _bits(v, hv, "the values of the third level")
    want, want_status = cc.restated("grid_512_level_3", np.float64)
    coarse = Coarse(n, None, None, None, np.float64, device=(m.cp, m.cc, m.cv))  # the arrays the Galerkin product wrote
    coarse.setup()
    got, status = coarse.read("376 rows")
    assert status == want_status == [0, -1, 0]
    _same(got, want, "the inverse of the 376-row level")
    rh = np.random.default_rng(376).uniform(-1.0, 1.0, size=n)
    r, z = Band(rh), Band(np.full(n, np.nan))
    capi.coarse_apply(n, coarse.inv.ptr, r.ptr, z.ptr, dtype=np.float64)
    zh = z.body("376 rows")
    _bits(zh, cc.apply(want, n, rh, np.float64), "z on the 376-row level")
    A = cc.densify(n, p, c, v)[0]
    res = np.linalg.norm(A @ zh - rh) / np.linalg.norm(rh)
    print("376 rows: |A_c z - r_c| / |r_c| = %.3e" % res)
    assert res <= 1e-10
