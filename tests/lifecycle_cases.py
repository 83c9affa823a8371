"""What test_gpu_context_lifecycle.py moves a Level-1 context through, kept apart so that its preconditions can be tested
without a device (test_context_lifecycle_cases.py): a pool of small matrices any two of which differ in rows, in cols and in
stored entries, the part of the pool every upload format accepts, the table of ordered format pairs and a seeded walk.

Formats are the context's own numbers (spmv_hip_ctx_info [0]): 1 CSR, 2 COO, 3 ELLPACK, 4 hybrid, 5 the stored triangle of a
symmetric matrix, 6 the transposed multiply, 7 fp32 values, 8 compact, 9 compact over fp64 values, 10 compact over float
vectors."""
import functools
import os
import tempfile

import numpy as np

from spmv_amd import capi, hostapi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUS = os.path.join(ROOT, "tests", "golden", "bus1138_like.mtx")
FORMATS = tuple(range(1, 11))
MULTI_FORMATS = (1, 2, 3, 4)  # what a context of spmv_hip_create_multi accepts
SCATTERED = "scattered"
TINY = "two_rows"  # fewer rows than the parts of a multi-GPU context; not part of the single-device pool
HOLLOW = "hollow"  # few entries under a long x: the vectors are all its device memory; not part of the pool either


def _arrays(rows, cols, p, c, v):
    return (int(rows), int(cols), np.ascontiguousarray(p, dtype=np.int32), np.ascontiguousarray(c, dtype=np.int32),
            np.ascontiguousarray(v, dtype=np.float64))


def _triangle():
    import scipy.sparse as sp
    rows, cols, p, c, v = synth.random_uniform(2500, 2500, 12, seed=7)
    T = sp.tril(sp.csr_matrix((v, c, p), shape=(rows, cols)), format="csr")
    T.sort_indices()
    return rows, cols, T.indptr, T.indices, T.data


def _bus():
    """The golden file as it is stored: the lower triangle of a symmetric matrix, which every general format takes as the
    triangular matrix it is and format 5 as the symmetric one it stands for."""
    A = hostapi.load(BUS, "csr")
    out = (A.rows, A.cols, np.array(A.row_ptr), np.array(A.column_index), np.array(A.value))
    A.close()
    return out


GENERATORS = {
    "wide": lambda: synth.random_uniform(3000, 7001, 9, seed=3),
    "tall": lambda: synth.random_uniform(9001, 1500, 5, seed=4),
    "poisson64": lambda: synth.poisson2d(64),  # constant coefficients: the default plan carries a value dictionary and stencil tiles
    "triangle": _triangle,
    "bus1138_like": _bus,
    "no_entries": lambda: (50, 30, np.zeros(51, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0)),
    # scattered columns, >= 2^20 entries, >= 4 per row and an x beyond 3 MiB: the bounds of the CSR column panels and of the COO panels
    SCATTERED: lambda: synth.random_uniform(60000, 600001, 20, seed=9),
    TINY: lambda: (2, 7, np.array([0, 2, 3]), np.array([1, 5, 6]), np.array([0.5, -1.25, 2.0])),
    HOLLOW: lambda: synth.random_uniform(700, 4000003, 3, seed=11),
}
POOL = tuple(n for n in GENERATORS if n not in (TINY, HOLLOW))
SMALL = tuple(n for n in POOL if n != SCATTERED)

# the part of the pool a format is given: 5 needs a stored triangle, 6 is given rectangles (rows and cols swap in the operator
# that runs), 3 and 4 the matrices small enough to go through the host library's converters as a Matrix Market file
ACCEPTS = {
    1: POOL, 2: POOL, 3: SMALL, 4: SMALL,
    5: ("triangle", "bus1138_like"),
    6: ("wide", "tall", "no_entries", SCATTERED),
    7: POOL, 8: POOL, 9: POOL, 10: POOL,
}

# (format, matrix) whose result does not depend on the run: rows summed by their owners, no atomics anywhere (spmv_hip_plan.h on
# tiles of rows of up to 512 entries -- no pool matrix has a longer row --, spmv_hip_f32values.h, spmv_hip_compact*.h; COO and
# hybrid uploads run as such row-major tiles unless SPMV_HIP_FLAG_COO_KEEP_ORDER is set, ELLPACK rows one or a few lanes of one
# wave).  Formats 5 and 6 add with atomics, and the scattered matrix runs in column panels that cut rows: those may differ from
# run to run and are held to the oracle instead.
REPRODUCIBLE = frozenset((f, m) for f in (1, 2, 3, 4, 7, 8, 9, 10) for m in ACCEPTS[f] if m != SCATTERED)


@functools.lru_cache(maxsize=None)
def matrix(name):
    return _arrays(*GENERATORS[name]())


_TMP = None


def _mtx_path(name):
    """The matrix as a Matrix Market file for the host library's converters (written once per process)."""
    global _TMP
    if name == "bus1138_like":
        return BUS
    if _TMP is None:
        _TMP = tempfile.TemporaryDirectory(prefix="spmv_lifecycle_")
    path = os.path.join(_TMP.name, name + ".mtx")
    if not os.path.exists(path):
        rows, cols, p, c, v = matrix(name)
        i, j, a = synth.csr_to_coordinate(rows, p, c, v)
        synth.write_mtx(path, rows, cols, i, j, a)
    return path


@functools.lru_cache(maxsize=None)
def converted(name, fmt):
    """hostapi's ELLPACK (fmt 3) or hybrid (fmt 4) conversion: a dict of copies of its arrays."""
    A = hostapi.load(_mtx_path(name), {3: "ell", 4: "hybrid"}[fmt])
    out = {"rows": A.rows, "cols": A.cols, "row_length": A.row_length, "col": np.array(A.column_index), "val": np.array(A.value)}
    if fmt == 4:
        out.update(coo_row=np.array(A.coo_row_index), coo_col=np.array(A.coo_column_index), coo_val=np.array(A.coo_value))
    A.close()
    return out


def operator_shape(fmt, name):
    """(rows, cols, stored entries of the source) of the operator that runs: format 6 runs A'."""
    rows, cols, p, _, _ = matrix(name)
    return (cols, rows, int(p[-1])) if fmt == 6 else (rows, cols, int(p[-1]))


def differ(s, t):
    return s[0] != t[0] and s[1] != t[1] and s[2] != t[2]


def pick(fmt, k, avoid=None):
    """The k-th matrix format `fmt` accepts, stepping on where that is the matrix to avoid."""
    names = ACCEPTS[fmt]
    name = names[k % len(names)]
    if name == avoid:
        name = names[(k + 1) % len(names)]
    return name


# every ordered pair of formats, each format to itself included: (a, Ma) first, then (b, Mb) with another matrix.  The index
# walks through what each format accepts so that every pool matrix is met on both sides.
PAIRS = {}
for _a in FORMATS:
    for _b in FORMATS:
        _ma = pick(_a, _a + 2 * _b)
        PAIRS[(_a, _b)] = ((_a, _ma), (_b, pick(_b, 3 * _a + _b, avoid=_ma)))

# an upload without entries after one that ran as a row-major matrix: COO is the one upload that then plans nothing
PAIRS[(2, 2)] = ((2, "wide"), (2, "no_entries"))
PAIRS[(4, 2)] = ((4, "bus1138_like"), (2, "no_entries"))

# the multi-GPU front: CSR, COO, ELLPACK and hybrid among themselves.  (1, 3) goes from more rows than parts to fewer,
# (3, 2) comes back from there.
MULTI_POOL = ("wide", "tall", "poisson64", "bus1138_like", "no_entries")
MULTI_PAIRS = {}
for _a in MULTI_FORMATS:
    for _b in MULTI_FORMATS:
        _ma = MULTI_POOL[(_a + 2 * _b) % len(MULTI_POOL)]
        _mb = MULTI_POOL[(3 * _a + _b) % len(MULTI_POOL)]
        if _mb == _ma:
            _mb = MULTI_POOL[(3 * _a + _b + 1) % len(MULTI_POOL)]
        MULTI_PAIRS[(_a, _b)] = ((_a, _ma), (_b, _mb))
MULTI_PAIRS[(1, 3)] = ((1, "wide"), (3, TINY))
MULTI_PAIRS[(3, 2)] = ((3, TINY), (2, "tall"))
MULTI_PAIRS[(4, 4)] = ((4, "bus1138_like"), (4, TINY))

WALK_STEPS = 60
WALK_SEED = 2024


def walk(steps=WALK_STEPS, seed=WALK_SEED):
    """`steps` (format, matrix) uploads: every format at least four times (six shuffled rounds of the ten formats), a matrix
    drawn from what the format accepts until its shape differs from the step before in rows, cols and entries.  The scattered
    matrix is met, but in the first round only: it is the one upload that takes longer than a few milliseconds."""
    rng = np.random.default_rng(seed)
    out = []
    for rnd in range(-(-steps // len(FORMATS))):
        for fmt in rng.permutation(FORMATS):
            names = [n for n in ACCEPTS[int(fmt)] if rnd == 0 or n != SCATTERED]
            while True:
                name = names[int(rng.integers(len(names)))]
                if not out or differ(operator_shape(*out[-1]), operator_shape(int(fmt), name)):
                    break
            out.append((int(fmt), name))
    return out[:steps]


def host_check(fmt, name):
    """The host-side checks of format `fmt` on the matrix, without a device: raises where the upload would refuse it."""
    rows, cols, p, c, v = matrix(name)
    assert p[0] == 0 and p[-1] == len(c) == len(v) and np.all(np.diff(p) >= 0)
    assert len(c) == 0 or (c.min() >= 0 and c.max() < cols)
    if fmt in (3, 4):
        E = converted(name, fmt)
        assert (E["rows"], E["cols"]) == (rows, cols) and len(E["col"]) == len(E["val"]) == rows * E["row_length"]
        assert len(E["col"]) == 0 or (E["col"].min() >= 0 and E["col"].max() < cols)
        if fmt == 4:
            assert len(E["coo_row"]) == len(E["coo_col"]) == len(E["coo_val"])
            assert len(E["coo_row"]) == 0 or (E["coo_row"].min() >= 0 and E["coo_row"].max() < rows and E["coo_col"].max() < cols)
            assert np.count_nonzero(E["val"]) + np.count_nonzero(E["coo_val"]) == np.count_nonzero(v)
    elif fmt == 5:
        assert rows == cols
        triangle, _ = capi.csr_triangle(rows, p, c)
        assert triangle in (capi.TRIANGLE_LOWER, capi.TRIANGLE_UPPER, capi.TRIANGLE_DIAGONAL)
    elif fmt == 6:
        info, _ = capi.tr_plan_preview(rows, cols, p, c, table=False)
        assert info["rows"] == rows and info["cols"] == cols and info["stored_entries"] == len(c)
    elif fmt == 7:
        info, _ = capi.f32_plan_preview(rows, cols, p, 0, table=False)
        assert info["rows"] == rows
    elif fmt in (8, 9, 10):
        info = capi.c16_plan_preview(rows, cols, p, c, 0, table=False)[0]
        assert info["rows"] == rows and info["stored_entries"] == len(c)
