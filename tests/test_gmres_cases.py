"""What test_gpu_gmres.py assumes of its operands and of the numpy restatement (gmres_cases.py), asserted without a device: the
integer operands make every sum exact, the restated small calls reproduce a QR factorisation, and GMRES(8) on the chain matrix
converges as the GPU test demands -- so that test's conditions are met by the restatement alone."""
import math

import numpy as np
import pytest

import gmres_cases as gc


def test_sizes_and_ks_cover_the_paths():
    assert gc.BLOCK == 8 and gc.KS == [0, 1, 7, 8, 9, 17, 32]
    assert 0 in gc.SIZES and gc.CHUNK in gc.SIZES and any(n % 4 in (1, 2, 3) for n in gc.SIZES)
    assert gc.BIG_SIZES == [2097152, 2097153]  # 2048 slots: one stage; 2049: two
    for dtype in gc.DTYPES:
        for n in gc.SIZES + gc.BIG_SIZES:
            ldv = gc.ldv_of(n, dtype)
            assert ldv >= n + 1 and ldv * np.dtype(dtype).itemsize % 16 == 0


@pytest.mark.parametrize("n,k", [(n, k) for n in (0, 3, 1025, 4097) for k in gc.KS] + [(n, gc.BIG_K) for n in gc.BIG_SIZES])
def test_integer_operands_are_exact_in_any_order_and_floats_hold_them(n, k):
    ops = gc.int_case(n, k)
    h, w4, d0 = ops.sums()
    assert np.all(np.abs(h) < 2 ** 53) and d0 * 16 < 2 ** 53
    for dtype in gc.DTYPES:
        case = ops.case(dtype)
        assert np.all(np.isnan(case.basis.reshape(k + 1, -1)[:, n:]))  # padding between the vectors
        want = gc.restate_update(case.V, case.h, case.w, dtype)
        assert np.array_equal(want.astype(np.float64) * 4, w4)  # a float holds what is stored
        if n:
            assert np.max(np.abs(want)) <= 520
        t = gc.project_products(case.V, case.w)
        assert [float(np.sum(x)) for x in t] == list(h)
        assert float(np.sum(want.astype(np.float64) ** 2)) == d0
        x = gc.restate_correct(case.V, case.y, case.minv, case.x, dtype)
        assert np.array_equal(x.astype(np.float64), x.astype(np.float32).astype(np.float64))


def test_a_lost_element_of_general_operands_exceeds_the_bound():
    case = gc.general_case(4097, 9, np.float64)
    for t in gc.project_products(case.V, case.w):
        assert np.mean(np.abs(t) > 10 * gc.bound(t)) > 0.99


def test_the_restated_small_calls_are_a_qr_factorisation_of_the_hessenberg_matrix():
    m = 8
    rng = np.random.default_rng(5)
    H = np.triu(rng.standard_normal((m + 1, m)), -1)
    H[np.arange(1, m + 1), np.arange(m)] = np.abs(H[np.arange(1, m + 1), np.arange(m)]) + 0.5
    beta2 = 7.25
    state = gc.restate_start(m, beta2)
    assert state[0] == math.sqrt(beta2) and state[1] == 1.0 / math.sqrt(beta2) and len(state) == gc.state_doubles(m) and len(state) % 2 == 0
    for k in range(m):
        h1 = H[:k + 1, k] * 0.75
        state = gc.restate_column(state, k, m, h1, H[:k + 1, k] - h1, H[k + 1, k] ** 2)
        assert state[1] == 1.0 / H[k + 1, k]
        # the least-squares residual of the first k + 1 columns is |g_{k+1}|
        e = np.zeros(k + 2)
        e[0] = math.sqrt(beta2)
        yk, res = np.linalg.lstsq(H[:k + 2, :k + 1], e, rcond=None)[:2]
        assert abs(state[0] - math.sqrt(res[0])) <= 1e-12 * math.sqrt(beta2)
        assert np.allclose(gc.restate_solve(state, k + 1, m), yk, rtol=1e-10, atol=1e-12)
    resid, bnd = gc.solve_residual_and_bound(state, m, m, gc.restate_solve(state, m, m))
    assert all(r <= b for r, b in zip(resid, bnd))


# r' r of r0, after one and two cycles, and the smallest h_{k+1,k}: (without minv, with minv)
FIGURES = {"rr0": (30652.0, 30652.0), "rr1": (869.0, 1412.9), "rr2": (290.4, 496.5), "subdiagonal": (3.6, 0.345)}


@pytest.mark.parametrize("dtype", gc.DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("with_minv", [False, True], ids=["plain", "minv"])
def test_gmres_8_on_the_chain_matrix_meets_the_gpu_tests_conditions(dtype, with_minv):
    out = gc.gmres_restated(dtype, with_minv)
    rr, i = out["rr"], int(with_minv)
    print(np.dtype(dtype).name, with_minv, out)
    assert rr[0] == FIGURES["rr0"][i]
    assert abs(rr[1] - FIGURES["rr1"][i]) <= 0.06 and abs(rr[2] - FIGURES["rr2"][i]) <= 0.06
    assert abs(min(out["subdiagonal"]) - FIGURES["subdiagonal"][i]) <= (0.05 if i == 0 else 0.0005)
    assert rr[1] < 0.1 * rr[0] and rr[2] < 0.02 * rr[0]  # what test_gpu_gmres.py asks of the GPU's chain
    # state[0]^2 against the true r' r: the issue's figures are 1e-9 (doubles; 1.8e-15 here) and 8e-8 (floats), the latter to
    # the one digit it is given with: 7.0e-8 and 8.4e-8 here.  The GPU test allows 1e-6.
    rel = 1e-9 if dtype == np.float64 else 8.5e-8
    for est, true in zip(out["estimate"], rr[1:]):
        assert abs(est - true) <= rel * true
    # max |V' V - I| with exact inner products: 4.4e-16 in doubles (the issue's figure); in floats 1.9e-8 in the first cycle
    # and 1.1e-8 / 1.2e-8 in the second (the issue: 1.0e-8).  Every entry is held to the bound that gmres_cases.orthogonality
    # derives from the roundings of the stored vectors: the largest entry is at 0.80 of it.  Classical Gram-Schmidt applied
    # once would leave the products of fp32's rounding and the basis's condition there.
    assert max(out["orthogonality_over_bound"]) <= 1.0, out
    if dtype == np.float64:
        assert max(out["orthogonality"]) <= 4.5e-16
