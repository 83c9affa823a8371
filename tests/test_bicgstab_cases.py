"""What must hold of the operands of test_gpu_bicgstab.py before a GPU result is looked at (bicgstab_cases.py), without a device: the
integer operands keep every stored value a float and both sums exact in any order, with no r of zero behind a step; on the general
operands a lost or doubled element would show in all but 1 % of the elements; the restatement is the header's arithmetic; the
chain matrix is the upwind operator the module describes; and the numpy restatement of eight iterations on it brings r' r below
a tenth of that of r0 without meeting a breakdown."""
import math
from fractions import Fraction

import numpy as np
import pytest

import bicgstab_cases as bc
from spmv_amd import capi


@pytest.mark.parametrize("n", bc.SIZES + bc.BIG_SIZES)
def test_integer_operands_are_exact_in_any_order(n):
    h = bc.int_case(n)
    for a in (h.v, h.r, h.phat, h.t, h.rhat, h.x, h.p):
        assert np.all((np.abs(a) >= 1) & (np.abs(a) <= 8))
    assert set(np.unique(h.m2).tolist()) <= {1, 2, 4}
    values = {Fraction(int(num)) / Fraction(int(den)) for num, den in bc.QUOTIENTS}
    assert values == {1, -2, Fraction(1, 2), 0}
    for place in range(3):  # every value as a, as w and as the r-quotient; w == 0 only where no b is formed
        seen = {t[place] for t in bc.INT_TRIPLES if t[place] is not None}
        assert seen == {0, 1, 2, 3}, place
    assert all((bc.QUOTIENTS[iw][0] != 0) == (ir is not None) for _, iw, ir in bc.INT_TRIPLES)
    for dtype in bc.DTYPES:
        for k, a in h.arrays(dtype).items():
            i = h.m2 / 2.0 if k == "minv" else getattr(h, k)
            assert a.dtype == dtype and np.all(a.astype(np.float64) == i)
    for ia, iw, ir in bc.INT_TRIPLES:
        for with_minv in (False, True):
            out, d0, d1 = h.triple(ia, iw, ir, with_minv)  # (asserts the preconditions)
            assert float(d0) == d0 and float(d1) == d1     # fp64 holds both sums
            assert (d0 > 0) == (n > 0)
            # ... and they are what the restatement gives, in floats and in doubles
            quotients = (bc.QUOTIENTS[ia], bc.QUOTIENTS[iw], bc.QUOTIENTS[ir if ir is not None else 0])
            for dtype in bc.DTYPES:
                a = h.arrays(dtype)
                got = bc.restate_triple(a, quotients, with_minv, dtype)
                for k, (num, den) in out.items():
                    if got[k] is None or (ir is None and k in ("p", "phat")):
                        continue
                    assert got[k].dtype == dtype and np.array_equal(got[k].astype(np.float64) * den, num), k
                t0, t1 = bc.step_products(got["r"], a["rhat"])
                assert float(np.sum(t0)) == d0 and float(np.sum(t1)) == d1
                assert float(np.sum(t0[::-1])) == d0 and float(np.sum(t1[::-1])) == d1
                if dtype == np.float64 and not with_minv:  # (r and the dots depend on neither: the exact sum once)
                    assert math.fsum(t0) == d0 and math.fsum(t1) == d1


@pytest.mark.parametrize("dtype", bc.DTYPES)
def test_a_lost_element_would_show_on_the_general_operands(dtype):
    for n in bc.SIZES:
        h = bc.general_case(n)
        assert n <= 4097 and all(np.all(np.abs(h.host[k]) < 1) for k in bc.NAMES[:-1])
        assert np.all((h.host["minv"] >= 0.5) & (h.host["minv"] < 2))
        for quotients in bc.GENERAL_QUOTIENTS:
            for with_minv in (False, True):
                shares = bc.visible_share(n, quotients, dtype, with_minv)
                print("n %d, %s, minv %s: share of the elements within 10 x the bound, per dot: %s" % (n, np.dtype(dtype).name, with_minv, shares))
                assert all(s is None or s <= 0.01 for s in shares), (n, shares)


def test_the_restatement_rounds_every_product_quotient_and_sum_and_casts_last():
    f = np.float64
    v, r, m = np.array([0.3]), np.array([0.1]), np.array([0.7])
    a = bc.quotient(1.0, 3.0)
    assert a == f(1.0) / f(3.0) and np.isinf(bc.quotient(1.0, 0.0)) and np.isnan(bc.quotient(0.0, 0.0))
    s, shat = bc.restate_s(1.0, 3.0, v, r, m, np.float64)
    assert s[0] == f(0.1) - a * f(0.3) and shat[0] == f(0.7) * s[0]
    assert bc.restate_s(1.0, 3.0, v, r, None, np.float64)[1] is None
    # float vectors: s is rounded to float once, and shat is formed from the ROUNDED s
    s32, shat32 = bc.restate_s(1.0, 3.0, v.astype(np.float32), r.astype(np.float32), m.astype(np.float32), np.float32)
    wide = f(np.float32(0.1)) - a * f(np.float32(0.3))
    assert s32.dtype == shat32.dtype == np.float32 and s32[0] == np.float32(wide) and f(s32[0]) != wide
    assert shat32[0] == np.float32(f(np.float32(0.7)) * f(s32[0]))
    # the step: x + a phat first, then + w shat, each product rounded on its own
    w = bc.quotient(-0.37, 0.11)
    ph, sh, t, x = np.array([0.9]), np.array([-0.4]), np.array([0.6]), np.array([0.2])
    xs, rs = bc.restate_step((1.0, 3.0), (-0.37, 0.11), ph, sh, t, x, s, np.float64)
    assert xs[0] == (f(0.2) + a * f(0.9)) + w * f(-0.4) and rs[0] == s[0] - w * f(0.6)
    xs2, _ = bc.restate_step((1.0, 3.0), (-0.37, 0.11), ph, None, t, x, s, np.float64)
    assert xs2[0] == (f(0.2) + a * f(0.9)) + w * s[0]  # no shat: the incoming r
    t0, t1 = bc.step_products(rs, np.array([1.9]))
    assert t0[0] == rs[0] * rs[0] and t1[0] == f(1.9) * rs[0] and bc.bound(t0) == 2.0 ** -53 * abs(t0[0])
    # b: three quotients, a fourth, a product -- not (num_r a) / (den_r w)
    qr = (2.5, 1.7)
    b = bc.beta(qr, (1.0, 3.0), (-0.37, 0.11))
    assert b == (f(2.5) / f(1.7)) * (a / w)
    found = False
    for k in range(1, 40):  # operands on which the other association rounds differently exist
        q = (1.0 + k / 7.0, 1.7)
        found |= bc.beta(q, (1.0, 3.0), (-0.37, 0.11)) != (f(q[0]) * a) / (f(q[1]) * w)
    assert found
    for qa, qw, q in bc.GENERAL_QUOTIENTS:  # ... and the general operands' quotients are among them
        assert bc.beta(q, qa, qw) != (f(q[0]) * bc.quotient(*qa)) / (f(q[1]) * bc.quotient(*qw)), (qa, qw, q)
    p = np.array([-0.8])
    pn, phat = bc.restate_direction(qr, (1.0, 3.0), (-0.37, 0.11), rs, v, p, m, np.float64)
    assert pn[0] == rs[0] + b * (f(-0.8) - w * f(0.3)) and phat[0] == f(0.7) * pn[0]
    # w == 0 where b is formed: a / 0 is Inf, and Inf (p - 0 v) reaches every element
    with np.errstate(all="ignore"):
        assert not np.isfinite(bc.restate_direction(qr, (1.0, 3.0), (0.0, 1.0), rs, v, p, None, np.float64)[0][0])
    # the start of the header: a direction over zeroed p and v with 0/1, 1/1, 1/1 stores p = r
    z = np.zeros(1)
    assert bc.restate_direction((0.0, 1.0), (1.0, 1.0), (1.0, 1.0), rs, z, z, None, np.float64)[0][0] == rs[0]


def test_the_chain_matrix_is_the_scaled_upwind_operator():
    rows, cols, p, c, v, b, minv = bc.chain_matrix()
    g = bc.GRID
    assert rows == cols == g * g == 1369 == bc.CHUNK + 345 and rows % 2 == 1 and rows % 4 == 1  # a tail of one element for both types
    assert len(p) == rows + 1 and p[0] == 0 and p[-1] == len(c) == len(v) == 5 * rows - 4 * g
    row = np.repeat(np.arange(rows), np.diff(p))
    assert np.all(np.diff(c)[np.diff(row) == 0] > 0)  # ascending within a row
    scale = 1.0 / (4.0 * minv)
    assert set(np.unique(scale).tolist()) == {1.0, 2.0, 4.0}
    unit = v / scale[row]
    off = c - row
    for d, val in ((0, 4.0), (-1, -1.5), (1, -0.5), (-g, -1.25), (g, -0.75)):
        assert np.all(unit[off == d] == val) and np.any(off == d)
    assert set(np.unique(off).tolist()) == {0, -1, 1, -g, g}
    assert np.all(v.astype(np.float32).astype(np.float64) == v) and np.all(minv.astype(np.float32).astype(np.float64) == minv)
    assert np.any(minv != minv[0])  # the Jacobi preconditioner is not a multiple of the identity
    assert np.all(b == np.round(b)) and np.all(np.abs(b) <= 8) and np.any(b != 0)
    dense = np.zeros((rows, cols))
    dense[row, c] = v
    assert not np.array_equal(dense, dense.T)
    assert capi.krylov_workspace_bytes(rows) == 48


@pytest.mark.parametrize("with_minv", [False, True])
@pytest.mark.parametrize("dtype", bc.DTYPES)
def test_eight_restated_iterations_bring_the_residual_below_a_tenth_without_a_breakdown(dtype, with_minv):
    norms, rv, tt = bc.bicgstab_restated(dtype, with_minv)
    print("%s, minv %s: r' r of r0 and after each iteration: %s" % (np.dtype(dtype).name, with_minv, ["%.3e" % v for v in norms]))
    assert len(norms) == bc.ITERATIONS + 1 and all(np.isfinite(norms)) and norms[0] > 0
    assert norms[-1] < 0.1 * norms[0]  # (not monotone: only the last value is compared)
    assert len(rv) == len(tt) == bc.ITERATIONS and all(x != 0 and np.isfinite(x) for x in rv + tt)
