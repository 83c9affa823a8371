"""What must hold of the operands of test_gpu_krylov.py before a GPU result is looked at (krylov_cases.py), without a device: the
integer operands keep every stored value a float and both sums exact in any order, with no r - a q of zero; on the general
operands a lost or doubled element would show in all but 1 % of the elements; the restatement is the header's arithmetic; and the
numpy restatement of the eight-iteration loop on the golden Poisson matrix brings r' r below that of r0."""
import math
from fractions import Fraction

import numpy as np
import pytest

import dots_cases as dc
import krylov_cases as kc
from spmv_amd import capi


def test_the_chunk_is_the_headers_and_the_sizes_surround_every_change_of_path():
    import ctypes as C
    import os
    import re
    header = open(os.path.join(os.path.dirname(capi.HEADER_PATH), "spmv_hip_krylov.h")).read()
    assert int(re.search(r"#define SPMV_HIP_KRYLOV_CHUNK (\d+)", header).group(1)) == kc.CHUNK
    csrc = os.path.join(os.path.dirname(capi.LIB_PATH), "csrc")
    assert int(re.search(r"constexpr int kDotsChunk = (\d+);", open(os.path.join(csrc, "csr_dots.hpp")).read()).group(1)) == kc.DOTS_CHUNK
    for n in (0, 1, 2, 3, 5, 63, 64, 65, kc.CHUNK - 1, kc.CHUNK, kc.CHUNK + 1, kc.SPAN - 1, kc.SPAN + 1):
        assert n in kc.SIZES
    # the workspace is one 16-byte slot per chunk and one per workgroup of the first stage: the two large sizes are the last n
    # with one stage and the first with two
    slots = [-(-n // kc.CHUNK) for n in kc.BIG_SIZES]
    assert slots == [kc.DOTS_CHUNK, kc.DOTS_CHUNK + 1]
    assert [capi.krylov_workspace_bytes(n) for n in kc.BIG_SIZES] == [16 * (slots[0] + 1), 16 * (slots[1] + 2)]
    assert max(kc.BIG_SIZES) * 8 < 2 ** 32


@pytest.mark.parametrize("n", kc.SIZES + kc.BIG_SIZES)
def test_integer_operands_are_exact_in_any_order(n):
    h = kc.int_case(n)
    for a in (h.pi, h.qi, h.xi, h.ri):
        assert np.all((np.abs(a) >= 1) & (np.abs(a) <= 8))
    assert set(np.unique(h.m2).tolist()) <= {1, 2, 4}
    for dtype in kc.DTYPES:
        for a, i in zip(h.arrays(dtype), (h.pi, h.qi, h.xi, h.ri, h.m2 / 2.0)):
            assert a.dtype == dtype and np.all(a.astype(np.float64) == i)
    seen = set()
    for num, den in kc.QUOTIENTS:
        seen.add(Fraction(num) / Fraction(den))
        for with_minv in (False, True):
            x2, r2, d0, d1 = h.step(num, den, with_minv)  # (asserts the preconditions)
            assert float(d0) == d0 and float(d1) == d1  # fp64 holds both sums
            assert (d1 == 0) == (not with_minv or n == 0) and (d0 > 0) == (n > 0)
            # ... and they are what the restatement gives, in floats
            for dtype in kc.DTYPES:
                p, q, x, r, minv = h.arrays(dtype)
                xs, rs = kc.restate_step(num, den, p, q, x, r, dtype)
                assert np.array_equal(xs.astype(np.float64) * 2, x2) and np.array_equal(rs.astype(np.float64) * 2, r2)
                t0, t1 = kc.step_products(rs, minv if with_minv else None)
                assert math.fsum(t0) == d0 and math.fsum(t1) == d1 and float(np.sum(t0[::-1])) == d0
    assert seen == {1, -2, Fraction(1, 2), 0}


@pytest.mark.parametrize("dtype", kc.DTYPES)
def test_a_lost_element_would_show_on_the_general_operands(dtype):
    for n in kc.SIZES:
        h = kc.general_case(n)
        assert n <= 4097 and all(np.all(np.abs(a) < 1) for a in (h.p, h.q, h.x, h.r)) and np.all((h.minv >= 0.5) & (h.minv < 2))
        for num, den in kc.GENERAL_QUOTIENTS:
            for with_minv in (False, True):
                shares = kc.visible_share(n, num, den, dtype, with_minv)
                print("n %d, %s, a = %g / %g, minv %s: share of the elements within 10 x the bound, per dot: %s" % (
                    n, np.dtype(dtype).name, num, den, with_minv, shares))
                assert all(s is None or s <= 0.01 for s in shares), (n, shares)


def test_the_restatement_rounds_every_product_and_casts_last():
    # a p is a rounded fp64 product, then one rounded sum
    p = np.array([2.0 ** -53 + 2.0 ** -105])
    x, r = kc.restate_step(3.0, 1.0, p, p, np.array([1.0]), np.array([-1.0]), np.float64)
    ap = np.float64(3.0) * p[0]
    assert x[0] == np.float64(1.0) + ap and r[0] == -x[0]
    # float vectors: the sum is formed in fp64 and rounded to float once
    one = np.array([1.0], dtype=np.float32)
    tiny = np.array([2.0 ** -24 + 2.0 ** -40], dtype=np.float32)
    x32, _ = kc.restate_step(1.0, 1.0, tiny, tiny, one, one, np.float32)
    assert x32.dtype == np.float32 and x32[0] == np.float32(1.0 + 2.0 ** -23)
    # a is one division: 1 / 3, not a reciprocal times the numerator
    assert kc.quotient(1.0, 3.0) == np.float64(1.0) / np.float64(3.0) and np.isinf(kc.quotient(1.0, 0.0)) and np.isnan(kc.quotient(0.0, 0.0))
    # the direction: z = fl(m r) in fp64, or r
    r3, m3, p3 = np.array([0.1]), np.array([0.7]), np.array([0.3])
    assert kc.restate_direction(1.0, 3.0, r3, m3, p3, np.float64)[0] == np.float64(0.7) * np.float64(0.1) + kc.quotient(1.0, 3.0) * np.float64(0.3)
    assert kc.restate_direction(0.0, 1.0, r3, None, p3, np.float64)[0] == 0.1
    t0, t1 = kc.step_products(np.array([0.1, -0.3]), np.array([0.7, 1.9]))
    assert t1[1] == (np.float64(1.9) * np.float64(-0.3)) * np.float64(-0.3) and t0[0] == np.float64(0.1) * np.float64(0.1)
    assert dc.bound(t0) == 2 * 2.0 ** -53 * float(np.sum(np.abs(t0)))


@pytest.mark.parametrize("with_minv", [False, True])
@pytest.mark.parametrize("dtype", kc.DTYPES)
def test_eight_restated_iterations_on_the_golden_poisson_matrix_reduce_the_residual(dtype, with_minv):
    norms = kc.pcg_restated(dtype, with_minv)
    print("%s, minv %s: r' r of r0 and after each iteration: %s" % (np.dtype(dtype).name, with_minv, ["%.3e" % v for v in norms]))
    assert len(norms) == kc.ITERATIONS + 1 and all(np.isfinite(norms)) and norms[0] > 0
    assert norms[-1] < norms[0]
