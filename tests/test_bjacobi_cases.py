"""What must hold of the operands of test_gpu_bjacobi.py before a GPU result is looked at (bjacobi_cases.py), without a device:
the restatement is the header's arithmetic; the integer operands keep every stored value a float and both sums exact in any
order; the restated inverse is as good as numpy.linalg.inv's up to a constant; on the general operands a lost element or a block
taken from the wrong chunk would exceed the dots' bound tenfold; and eight restated PCG iterations on the 432-unknown SPD case
do with 3 x 3 blocks what the issue promises of them."""
import math

import numpy as np
import pytest

import bjacobi_cases as bc
import dots_cases as dc

# The largest ratio, over every block of the three families at b = 1 ... 8, of max |B X - I| of the restated inverse to that of
# numpy.linalg.inv on the same block (an exact numpy residual counted as one rounding, 2^-53) is 100.05 (rotated SPD
# blocks of condition 1e6 at b = 8; 4 at the most on the dominant and the row-swapping blocks).  Gauss-Jordan and LAPACK's LU
# differ, so a constant is expected, a blow-up is not: pinned at twice that, rounded up to a power of two.
RESIDUAL_RATIO = 256.0


def test_the_sizes_are_the_issues_and_surround_every_change_of_path():
    for b in bc.BLOCKS:
        s = bc.sizes(b)
        assert all(n % b == 0 and n >= b for n in s) and s[0] == b and 2 * b in s
        for t in bc.TARGETS[2:]:
            assert bc.nearest(t, b) in s and abs(bc.nearest(t, b) - t) <= b // 2, (b, t)
        assert max(s) > 2048 * bc.CHUNK, "the largest size takes the reduction's second stage"
        assert max(s) * 8 < 2 ** 32
    assert bc.CHUNK == 1024 and [bc.nearest(t, 3) for t in bc.TARGETS] == [3, 6, 1023, 1023, 1026, 2049, 65538, 2097153]


def test_the_restatement_is_the_headers_arithmetic():
    # extraction: stored order, any column order, a position stored twice, one not stored, entries outside the block ignored
    p, c = np.array([0, 4, 6]), np.array([1, 5, 0, 1, 9, 0])
    v = np.array([1e16, 3.0, 2.0, 1.0, 7.0, 4.0])
    blk = bc.extract(2, 2, p, c, v)
    assert blk.shape == (1, 2, 2) and blk[0, 0, 1] == np.float64(1e16) + 1.0 and blk[0, 0, 0] == 2.0 and blk[0, 1, 0] == 4.0 and blk[0, 1, 1] == 0.0
    v2 = np.array([1.0, 3.0, 2.0, 1e16, 7.0, 4.0])  # the same position in the other order: 0 + 1 + 1e16
    assert bc.extract(2, 2, p, c, v2)[0, 0, 1] == 1e16 + 1.0
    # b == 1: fl(1 / a), and 1 where the diagonal is zero or not stored
    inv, count, first = bc.invert(np.array([[[3.0]], [[0.0]], [[-0.0]], [[-7.0]]]), np.float64)
    assert inv.ravel().tolist() == [1.0 / 3.0, 1.0, 1.0, 1.0 / -7.0] and (count, first) == (2, 1)
    # a 2 x 2 block by hand: the pivot of column 0 is row 1 (|-4| > |1|)
    blk = np.array([[[1.0, 2.0], [-4.0, 3.0]]])
    t = 1.0 / -4.0
    r0 = np.array([-4.0, 3.0, 0.0, 1.0]) * t
    r1 = np.array([1.0, 2.0, 1.0, 0.0]) - 1.0 * r0
    t1 = 1.0 / r1[1]
    r1n = r1 * t1
    r0n = r0 - r0[1] * r1n
    inv, count, first = bc.invert(blk, np.float64)
    assert np.array_equal(inv[0], np.array([r0n[2:], r1n[2:]])) and (count, first) == (0, -1)
    # a NaN never wins the pivot search, and the first of two equal magnitudes does
    blk = np.array([[[1.0, 0.0, 0.0], [np.nan, 1.0, 0.0], [-1.0, 0.0, 1.0]]])
    inv, count, first = bc.invert(blk, np.float64)
    assert count == 0 and np.all(np.isnan(inv[0]))  # row 1 is never swapped up: column 0 eliminates with its NaN
    assert bc.invert(np.array([[[np.nan]]]), np.float64)[1] == 0
    # singular at the second column: the identity, counted
    inv, count, first = bc.invert(np.array([[[2.0, 1.0], [0.0, 1.0]], [[1.0, 2.0], [2.0, 4.0]]]), np.float32)
    assert inv.dtype == np.float32 and np.array_equal(inv[1], np.eye(2)) and (count, first) == (1, 1)
    # the apply: every product rounded, the sum from the first product on, one cast last
    a, r = np.array([0.1, 0.7, 0.3, 0.9]), np.array([0.3, -0.6])
    z = bc.apply(a, r, 2, np.float64)
    assert z[0] == np.float64(0.1) * 0.3 + np.float64(0.7) * -0.6 and z[1] == np.float64(0.3) * 0.3 + np.float64(0.9) * -0.6
    assert np.signbit(bc.apply(np.array([1.0]), np.array([-0.0]), 1, np.float64)[0])  # no 0.0 + in front of the first product
    tiny = np.array([2.0 ** -24 + 2.0 ** -40, 1.0], dtype=np.float32)
    assert bc.apply_add(np.array([1.0], dtype=np.float32), tiny[:1], tiny[1:], 1, np.float32)[0] == np.float32(1.0 + 2.0 ** -23)
    t0, t1 = bc.apply_products(np.array([0.1]), np.array([0.7]))
    assert t0[0] == np.float64(0.1) * 0.7 and t1[0] == np.float64(0.1) * 0.1


@pytest.mark.parametrize("b", bc.BLOCKS)
def test_integer_operands_are_exact_in_any_order(b):
    for n in bc.sizes(b)[:-1] + [bc.sizes(b)[-1]]:
        h = bc.int_case(n, b)
        z, x, d0, d1 = h.results()  # (asserts the preconditions)
        assert float(d0) == d0 and float(d1) == d1 and d1 > 0
        if n > bc.GENERAL_LIMIT and b not in (3, 8):
            continue  # the restatement at two million elements: two block sizes are enough
        for dtype in bc.DTYPES:
            inv, r, x0 = h.arrays(dtype)
            assert all(np.array_equal(a.astype(np.int64), i) for a, i in zip((inv, r, x0), (h.invi, h.ri, h.xi)))
            zs = bc.apply(inv, r, b, dtype)
            assert np.array_equal(zs.astype(np.float64), z) and np.array_equal(bc.apply_add(inv, r, x0, b, dtype).astype(np.float64), x)
            t0, t1 = bc.apply_products(zs, r)
            assert math.fsum(t0) == d0 and math.fsum(t1) == d1 and float(np.sum(t0[::-1])) == d0


@pytest.mark.parametrize("b", bc.BLOCKS)
def test_the_restated_inverse_is_as_good_as_numpys_up_to_a_constant(b):
    worst = 0.0
    for name, blocks in (("dominant", bc.dominant_blocks(b, 200, 7 * b + 1)), ("rotated SPD", bc.rotated_spd_blocks(b, 200, 7 * b + 1)),
                         ("a swap at every column", bc.swap_blocks(b, 200, 7 * b + 1))):
        inv, count, first = bc.invert(blocks, np.float64)
        assert (count, first) == (0, -1)
        mine, numpys = bc.residual(blocks, inv), bc.residual(blocks, np.linalg.inv(blocks))
        ratio = float(np.max(mine / np.maximum(numpys, 2.0 ** -53)))
        print("b %d, %s: max |B X - I| %.3e, numpy's %.3e, largest ratio on one block %.2f" % (b, name, mine.max(), numpys.max(), ratio))
        worst = max(worst, ratio)
        if name.startswith("a swap") and b > 1:  # every column of every block does swap
            assert np.all(np.argmax(np.abs(blocks), axis=1) != np.arange(b))
    assert worst <= RESIDUAL_RATIO


@pytest.mark.parametrize("b", bc.BLOCKS)
def test_the_setup_matrix_has_what_the_setup_must_cope_with(b):
    rows, p, c, v = bc.setup_matrix(b)
    row = np.repeat(np.arange(rows), np.diff(p))
    inside = (c // b == row // b)
    keys = row[inside].astype(np.int64) * rows + c[inside]
    assert len(np.unique(keys)) < len(keys), "no position is stored twice"
    assert np.any(np.diff(c[p[0]:p[1]]) < 0) or b == 1, "sorted columns"
    assert np.max(np.diff(p)) > 128, "no row takes several passes of the wave"
    stored = np.zeros((rows // b, b, b), dtype=bool)
    stored[row[inside] // b, row[inside] % b, c[inside] % b] = True
    assert not stored[7].any() and (b == 1 or not stored[1].all()), "positions that are not stored"
    if b > 1:
        assert not stored[4, b - 1].any() and stored[4, 0].any(), "a row with no entry in its block"
    inv, count, first = bc.invert(bc.extract(rows, b, p, c, v), np.float64)
    assert first == 3 and count >= 2 and np.all(np.isfinite(inv))
    assert np.array_equal(inv[3], np.eye(b)) and np.array_equal(inv[7], np.eye(b))
    good = np.ones(rows // b, dtype=bool)
    good[[3, 7] + ([4, 15, 26] if b > 1 else [])] = False
    assert count == int((~good).sum())
    assert np.max(bc.residual(bc.extract(rows, b, p, c, v)[good], inv[good])) < 1e-9


@pytest.mark.parametrize("dtype", bc.DTYPES, ids=["float64", "float32"])
def test_a_lost_element_or_a_block_from_the_wrong_chunk_would_show(dtype):
    for b in bc.BLOCKS:
        for n in [s for s in bc.sizes(b) if s <= bc.GENERAL_LIMIT]:
            inv, r, x = bc.general_case(n, b).arrays(dtype)
            z = bc.apply(inv, r, b, dtype)
            shares = [float(np.mean(np.abs(t) <= 10.0 * dc.bound(t))) for t in bc.apply_products(z, r)]
            assert all(s <= 0.01 for s in shares), (b, n, shares)  # a lost or doubled element shows in all the others
            if bc.CHUNK % b and n > 2 * bc.CHUNK:  # (a whole second chunk: the defect's blocks stay inside the vector)
                bad = bc.chunk_relative_blocks(inv, r, b, dtype)
                assert np.array_equal(bad[:bc.CHUNK // b * b], z[:bc.CHUNK // b * b]) and not np.array_equal(bad, z)
                for t, tb in zip(bc.apply_products(z, r), bc.apply_products(bad, r)):
                    assert abs(math.fsum(tb) - math.fsum(t)) > 10.0 * dc.bound(t), (b, n)


def test_eight_restated_pcg_iterations_with_blocks_beat_the_diagonal():
    rows, p, c, v, rhs = bc.spd_case()
    assert rows == 432 and np.all(np.linalg.eigvalsh(_dense(rows, p, c, v)) > 0)
    for dtype in bc.DTYPES:
        diag, blocks = bc.pcg_restated(dtype, 1), bc.pcg_restated(dtype, 3)
        print("%s: r'r with the diagonal %s" % (np.dtype(dtype).name, ["%.3e" % x for x in diag]))
        print("%s: r'r with 3 x 3 blocks %s" % (np.dtype(dtype).name, ["%.3e" % x for x in blocks]))
        assert len(blocks) == bc.ITERATIONS + 1 and np.all(np.isfinite(blocks)) and diag[0] == blocks[0] > 0
        assert blocks[-1] < diag[-1]
        if dtype == np.float64:
            assert blocks[-1] < 1e-5 * blocks[0]


def _dense(rows, p, c, v):
    a = np.zeros((rows, rows))
    a[np.repeat(np.arange(rows), np.diff(p)), c] = v
    assert np.array_equal(a, a.T)
    return a
