"""NaN and Inf in x, in the stored values and in y0 stay in their own rows.

Every multiply of the library reads more than a row stores -- the quad in front of a tile, the clamped pair behind the last
column, three doubles per masked block, window slots past the window, row 0 of X for a masked lane -- and promises not to use the
surplus.  With finite operands a surplus product that is used times a zero adds 0.0 and passes.  Here the operands hold NaN and
+Inf (tests/poison.py): the reference forms exactly the stored products, so WHICH rows of y are NaN, +Inf, -Inf or finite is
fixed by the sparsity pattern alone, whatever the order of the sums.  A kernel that multiplies a padding slot, a clamped gather,
a dropped block entry or a neighbour's quad by zero turns a finite row into NaN; one that skips a stored product turns a NaN row
finite.  Classes are compared exactly; finite rows bitwise with the same plan's result on the clean operand wherever no partial
sums meet in atomics (there: helpers.assert_close against the oracle).

The scaled forms y_out <- alpha A x + beta y_in of the float-tile multiplies (include/spmv_hip_scaled.h) are multiplies of the
library too: their epilogue reads y_in through a clamped row, beta == 0 must not load y_in at all and alpha == 0 must not form
0 * Inf.  Their reference is test_gpu_scaled.restate on the oracle's row sums of the poisoned operand.

Three poisons per case: x by the poison rule (each column with probability min(0.25, 0.3 / mean row length), plus columns 0 and
cols - 1), the first and last stored entry of every 37th non-empty row, every 29th row of y0.  Before the GPU is looked at the
oracle's own result must show >= 5 % non-finite rows, >= 50 % finite rows and >= 5 % finite rows beside a non-finite one.

On Level 2 every device array is a view into a larger buffer: 32 bytes of out-of-range columns / NaN values around the matrix
arrays, NaN around x, one fixed bit pattern around y that must come back unchanged after every multiply; x and y once 16-byte
aligned and once 8- but not 16-byte aligned (the float pair: 4 but not 8).  Every case first shows through plan_info that it
reached its tile class."""
import functools

import numpy as np
import pytest

import compact_cases as cc
import helpers
import poison
from spmv_amd import capi, hostapi, synth
from test_gpu_blocktiles import _scatter_nodes, fem3, fem_ragged
from test_gpu_multivec import _mixed_lengths
from test_gpu_plan_handoffs import mesh_case
from test_gpu_scaled import restate
from test_gpu_stencil_chunks import grid as grid_with_holes
from test_gpu_stencil_runs import band, grid2d
from test_gpu_stencil_sweep import pattern_matrix
from test_gpu_stenciltiles import NINE, STAR7, grid_stencil
from test_gpu_transpose import _quad_matrix, _random

pytestmark = pytest.mark.gpu

PAD_BYTES = 32          # around the row_ptr, column and value arrays: the views stay 16-byte aligned
BACK = 6                # elements behind x and y (the guard column cols + 1 of the column array's padding lies inside them)
FRONTS64 = (4, 5)       # doubles in front of x and y: 16-byte aligned, then 8 but not 16
FRONTS32 = (8, 5)       # floats in front of a float x and y: 16-byte aligned, then 4 but not 8
SURE = 512              # rows of up to this many entries are never cut into chunks that meet in atomics
Y_BITS32 = 0xC0E85EED   # -7.26...: the guard pattern around a float y
NOXW_NOVI = capi.FLAG_NO_X_WINDOW | capi.FLAG_NO_VALUE_INDEX


def _torch():
    import torch
    return torch


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _csr(rows, cols, p, c, v):
    return int(rows), int(cols), _i32(p), _i32(c), np.ascontiguousarray(v, dtype=np.float64)


# ---- device arrays as views into larger buffers ------------------------------------------------------------------------------------

class Guarded:
    """A device vector between `front` and BACK guard elements: NaN around an operand, one fixed bit pattern around a result."""

    def __init__(self, a, front, result=False):
        torch = _torch()
        a = np.ascontiguousarray(a)
        assert a.dtype in (np.float64, np.float32)
        self.n, self.front, self.size, self.result = len(a), front, a.dtype.itemsize, result
        utype, itype = (np.uint64, np.int64) if self.size == 8 else (np.uint32, np.int32)
        pattern = np.array(poison.Y_GUARD_BITS if self.size == 8 else Y_BITS32, dtype=utype) if result else np.array(np.nan, dtype=a.dtype)
        self.bits = pattern.view(itype).item()
        self.raw = torch.full((front + self.n + BACK,), self.bits, dtype=torch.int64 if self.size == 8 else torch.int32, device="cuda:0")
        self.whole = self.raw.view(torch.float64 if self.size == 8 else torch.float32)
        self.whole[front:front + self.n] = torch.from_numpy(a).to("cuda:0")
        self.ptr = self.whole.data_ptr() + self.size * front
        assert self.whole.data_ptr() % 256 == 0  # (the alignment of the view is that of its offset)

    def get(self):
        _torch().cuda.synchronize()
        return self.whole[self.front:self.front + self.n].cpu().numpy().copy()

    def assert_guards(self, what):
        """Bitwise: a changed guard of y is an out-of-bounds store."""
        _torch().cuda.synchronize()
        g = np.concatenate([self.raw[:self.front].cpu().numpy(), self.raw[self.front + self.n:].cpu().numpy()])
        assert np.all(g == self.bits), "%s: %s written outside its %d entries" % (what, "y" if self.result else "x", self.n)


def _padded(a, dtype, front_fill, back_fill):
    """(buffer, address of the view): `a` between PAD_BYTES of fill on either side."""
    torch = _torch()
    a = np.ascontiguousarray(a, dtype=dtype)
    pad = PAD_BYTES // a.dtype.itemsize
    buf = torch.full((len(a) + 2 * pad,), back_fill, dtype=torch.from_numpy(a[:0]).dtype, device="cuda:0")
    buf[:pad] = front_fill
    buf[pad:pad + len(a)] = torch.from_numpy(a).to("cuda:0")
    return buf, buf.data_ptr() + PAD_BYTES


class Matrix:
    """The CSR arrays on the device.  Around row_ptr: 0 and nnz; around the columns: cols + 1, out of range but positive (as an
    index into x or y it lies in their guards); around the values: NaN.  `values`: the dtype of the value array."""

    def __init__(self, rows, cols, p, c, v, values=np.float64):
        self.rows, self.cols, self.host = rows, cols, (p, c, v)
        nnz = int(p[rows])
        self.bp, self.p = _padded(p, np.int32, 0, nnz)
        self.bc, self.c = _padded(c, np.int32, cols + 1, cols + 1)
        self.bv, self.v = _padded(v, values, float("nan"), float("nan"))

    def assert_unchanged(self, what):
        pad = PAD_BYTES // 4
        assert np.array_equal(self.bc.cpu().numpy()[pad:-pad], self.host[1]), what + ": the column array changed"


def _stream():
    return _torch().cuda.current_stream().cuda_stream


# ---- the three poisons and the reference's answers -------------------------------------------------------------------------------

class Operands:
    """x, y0 and their poisoned twins for a (rows x cols) operator given as CSR arrays, the values' twin, and the oracle's
    results -- the vacuity conditions are asserted here, from the oracle alone."""

    def __init__(self, oracle, what, rows, cols, p, c, v, x=None, y0=None):
        self.what, self.rows, self.cols, self.p, self.c, self.v = what, rows, cols, p, c, v
        self.lens = np.diff(p.astype(np.int64))
        self.nterms = max(4096, int(self.lens.max()) + 1)
        self.x = synth.x_vector(cols, seed=3) if x is None else x
        self.y0 = np.random.default_rng(7).uniform(-1.0, 1.0, size=rows) if y0 is None else y0
        self.xp = poison.x_vector(self.x, p)
        self.vp, self.value_rows = poison.values(p, v)
        self.y0p = poison.y0_vector(self.y0)
        mul = lambda val, xx, yy, runs=1: oracle.csr_spmv(rows, p, c, val, np.asarray(xx, dtype=np.float64),
                                                          y=np.asarray(yy, dtype=np.float64), num_threads=1, runs=runs)
        self.clean1 = mul(v, self.x, self.y0)
        self.ref_x = mul(v, self.xp, self.y0)
        poison.assert_not_vacuous(self.ref_x, what)
        self.ref_v = mul(self.vp, self.x, self.y0)
        assert np.all(poison.classes(self.ref_v)[self.value_rows] != poison.FINITE)
        self.ref_y1 = mul(v, self.x, self.y0p)
        self.ref_y3 = mul(v, self.x, self.y0p, 3)
        assert np.all(poison.classes(self.ref_y1)[::poison.Y0_ROW_STRIDE] != poison.FINITE)
        with np.errstate(invalid="ignore"):
            self.scale_x = helpers.abs_products(rows, p, c, v, np.abs(self.xp)) + np.abs(self.y0)
            self.scale_v = helpers.abs_products(rows, p, c, np.abs(self.vp), self.x) + np.abs(self.y0)
            self.scale_y = helpers.abs_products(rows, p, c, v, self.x) + np.abs(self.y0p)


def _compare(got, ref, what, clean, sure, scale, nterms, exact_ref=None):
    """Classes exactly; finite rows bitwise against `clean` where `sure`, within the tolerance of the oracle elsewhere; with
    exact_ref (FLAG_EXACT_ORDER) finite rows bitwise against the oracle."""
    poison.assert_classes(got, ref, what)
    if clean is not None and (sure is None or np.any(sure)):
        poison.assert_finite_rows_bitwise(got, clean, ref, what + " (finite rows against the clean run)", only=sure)
    if sure is not None and not np.all(sure):
        poison.assert_finite_rows_close(got, ref, scale, what + " (finite rows against the oracle)", nterms)
    if exact_ref is not None:
        poison.assert_finite_rows_bitwise(got, exact_ref, ref, what + " (exact order: finite rows against the oracle)")


# ---- the default plan, Level 2 ----------------------------------------------------------------------------------------------------

CLASS_KEYS = ("row_blocks", "long_blocks", "narrow_tiles", "uniform_tiles", "shifted_tiles", "xwin_tiles", "blockwin_tiles",
              "panel_tiles", "balanced", "indexed_values", "segwin_tiles", "value_row_tiles", "dictionary_launch_tiles", "block_tiles",
              "multi_window_tiles", "masked_block_tiles", "stencil_mask_tiles", "group_tiles", "run_chunks", "run_masked_chunks",
              "run_rest_tiles", "run_variant")


def _counts(info):
    return {k: info[k] for k in CLASS_KEYS}


class DefaultPlan:
    def __init__(self, A, flags, index_values):
        rows, cols, p, c, v = A
        self.rows = rows
        self.m = Matrix(rows, cols, p, c, v)
        self.plan = capi.CsrPlan(rows, cols, p, capi.CSR_AUTO, 0, flags)
        self.plan.compress(self.m.c, _stream())
        self.plan.repack(self.m.p, self.m.c, self.m.v, _stream())
        if index_values:
            self.plan.index_values(self.m.v, _stream())
        self.info = self.plan.info()

    def spmv(self, x, y, what, runs=1):
        for _ in range(runs):
            self.plan.spmv(self.m.p, self.m.c, self.m.v, x.ptr, y.ptr, _stream())
            y.assert_guards(what)
        return y.get()

    def spmv_out(self, x, y_in, front, what):
        """y_out = y_in + A x into an output filled with NaN; y_in comes back as it was."""
        src = Guarded(y_in, front, result=True)
        out = Guarded(np.full(self.rows, np.nan), front, result=True)
        self.plan.spmv_out(self.m.p, self.m.c, self.m.v, x.ptr, src.ptr, out.ptr, _stream())
        out.assert_guards(what)
        src.assert_guards(what + " (y_in)")
        assert np.array_equal(src.get().view(np.uint64), np.ascontiguousarray(y_in).view(np.uint64)), what + ": y_in changed"
        return out.get()

    def close(self):
        self.m.assert_unchanged("default plan")
        self.plan.close()


def check_default_plan(oracle, what, A, flags=0, index_values=False, reached=None):
    A = _csr(*A)
    rows, cols, p, c, v = A
    ops = Operands(oracle, what, rows, cols, p, c, v)
    exact = bool(flags & capi.FLAG_EXACT_ORDER)
    plan = DefaultPlan(A, flags, index_values)
    info = plan.info
    print("%s: plan_info %s" % (what, {k: n for k, n in _counts(info).items() if n}))
    assert reached(info), (what, _counts(info))
    sure = (ops.lens <= SURE) if info["panel_tiles"] == 0 else np.zeros(rows, dtype=bool)
    for front in FRONTS64:
        tag = "%s, x and y %d bytes into their buffers" % (what, 8 * front)
        X, XP = Guarded(ops.x, front), Guarded(ops.xp, front)
        assert X.ptr % 16 == (0 if front % 2 == 0 else 8)
        clean = plan.spmv(X, Guarded(ops.y0, front, result=True), tag + ", clean")
        if exact:
            helpers.assert_bitexact(clean, ops.clean1, tag + ", clean, exact order")
        # 1. x: two launches, each into its own NaN-filled output (a plan that alternates its sweep: both directions)
        for launch in (1, 2):
            got = plan.spmv_out(XP, ops.y0, front, "%s, poisoned x, launch %d" % (tag, launch))
            _compare(got, ops.ref_x, "%s, poisoned x, launch %d" % (tag, launch), clean, sure, ops.scale_x, ops.nterms,
                     ops.ref_x if exact else None)
        # 3. y0: in place, three accumulating runs, and through spmv_out
        clean3 = plan.spmv(X, Guarded(ops.y0, front, result=True), tag + ", clean, three runs", runs=3)
        got3 = plan.spmv(X, Guarded(ops.y0p, front, result=True), tag + ", poisoned y0, three runs", runs=3)
        _compare(got3, ops.ref_y3, tag + ", poisoned y0, three runs", clean3, sure, 3 * ops.scale_y, 3 * ops.nterms,
                 ops.ref_y3 if exact else None)
        got1 = plan.spmv_out(X, ops.y0p, front, tag + ", poisoned y0, y_out")
        _compare(got1, ops.ref_y1, tag + ", poisoned y0, y_out", clean, sure, ops.scale_y, ops.nterms, ops.ref_y1 if exact else None)
        X.assert_guards(tag)
        XP.assert_guards(tag)
    # 2. values: another matrix, poisoned before planning
    front = FRONTS64[0]
    X = Guarded(ops.x, front)
    clean = plan.spmv(X, Guarded(ops.y0, front, result=True), what + ", clean")
    plan.close()
    plan_v = DefaultPlan((rows, cols, p, c, ops.vp), flags, index_values)
    same_classes = _counts(plan_v.info) == _counts(info)
    print("%s: poisoned values, %s tile-class counts" % (what, "the same" if same_classes else "other"))
    got = plan_v.spmv(X, Guarded(ops.y0, front, result=True), what + ", poisoned values")
    plan_v.close()
    if same_classes:
        _compare(got, ops.ref_v, what + ", poisoned values", clean, sure, ops.scale_v, ops.nterms, ops.ref_v if exact else None)
    else:
        _compare(got, ops.ref_v, what + ", poisoned values", None, np.zeros(rows, dtype=bool), ops.scale_v, ops.nterms,
                 ops.ref_v if exact else None)
    return info


def _pattern(A):
    rows, cols, p, c, v = A
    return rows, cols, p, c, np.ones(len(v))


def _powerlaw():
    return synth.powerlaw(30000, 30000, seed=4, max_len=600)[:5]


DEFAULT_CASES = {
    # name: (builder, flags, index_values, what plan_info must show)
    "plain tiles, ragged ends": (lambda: cc.matrix("rows_0_to_7_ragged_end"), 0, False, lambda i: i["narrow_tiles"] > 0),
    # (a 5-point grid has too few uses per window slot for the x window -- test_gpu_parity.test_x_window_variant_bit_identical pins
    # that -- so grid2d(257) shows the shifted tiles, in row chunks by default, and that test's 15 diagonals of a 3-D stencil show them
    # through the window, which is a handful of merged runs there)
    "shifted tiles, grid2d(257)": (lambda: grid2d(257), 0, False, lambda i: i["shifted_tiles"] > 0),
    "shifted tiles through the x window": (lambda: synth.banded(64000, [-1600, -41, -40, -39, -3, -2, -1, 0, 1, 2, 3, 39, 40, 41, 1600], seed=4),
                                           0, False, lambda i: i["shifted_tiles"] > 0 and i["xwin_tiles"] > 0),
    "stencil run chunks, grid with a hole": (lambda: grid_with_holes(1000, 1000, holes=[(100, 140, 200, 260)]), NOXW_NOVI, False,
                                             lambda i: i["run_chunks"] > 0 and i["run_masked_chunks"] > 0 and i["run_variant"] & 4),
    "stencil run chunks, misaligned triple": (lambda: pattern_matrix(6000, (-9, 2, 3, 4, 20)), NOXW_NOVI, False,
                                              lambda i: i["run_chunks"] > 0 and i["run_masked_chunks"] > 0 and i["run_variant"] & 4),
    "stencil run chunks, band": (lambda: band(4099, 1), NOXW_NOVI, False, lambda i: i["run_chunks"] > 0 and i["run_variant"] & 4),
    "masked stencil tiles, 7-point 60^3 with holes": (lambda: grid_stencil((60, 60, 60), STAR7, seed=5, hole_share=0.05), 0, True,
                                                      lambda i: i["stencil_mask_tiles"] > 0),
    "masked stencil tiles, 9-point 257 x 129": (lambda: grid_stencil((257, 129), NINE, seed=6), 0, True, lambda i: i["stencil_mask_tiles"] > 0),
    "block tiles": (lambda: fem3(20000, 6, 30, seed=7), 0, True, lambda i: i["block_tiles"] > 0),
    "masked block tiles": (lambda: fem_ragged(6000, 20, 34, seed=12, drop=0.1, odd_every=40), 0, True,
                           lambda i: i["block_tiles"] > 0 and i["masked_block_tiles"] > 0),
    "wide block tiles": (lambda: _scatter_nodes(*fem3(6000, 20, 34, seed=9), factor=170, seed=1), capi.FLAG_NO_COLUMN_PANELS, False,
                         lambda i: i["masked_block_tiles"] > 0 and i["panel_tiles"] == 0),
    "group tiles, 2 per node": (lambda: synth.mesh_dofs((30, 24, 20), 2, seed=2), 0, False, lambda i: i["group_tiles"] > 0),
    "group tiles, 4 per node": (lambda: synth.mesh_dofs((24, 20, 16), 4, seed=4), 0, False, lambda i: i["group_tiles"] > 0),
    "wide group tiles": (lambda: synth.delaunay_mesh(40000, 2, seed=8, order="random"), 0, False,
                         lambda i: i["group_tiles"] > 0 and i["narrow_tiles"] < 0.2 * i["row_blocks"]),
    "balanced tiles": (_powerlaw, 0, False, lambda i: i["balanced"] == 1),
    "balanced tiles with a dictionary": (lambda: _pattern(_powerlaw()), 0, True, lambda i: i["balanced"] == 1 and i["indexed_values"] > 0),
    "long rows": (_mixed_lengths, 0, False, lambda i: i["multi_window_tiles"] > 0 or i["long_blocks"] > 0),
    "segment windows": (lambda: mesh_case(2, broken=0.2), 0, False, lambda i: i["segwin_tiles"] > 0),
    "block windows": (lambda: mesh_case(3, far_share=0.15), capi.FLAG_NO_BLOCK_TILES, False, lambda i: i["blockwin_tiles"] > 0),
    "constant-row tiles": (lambda: synth.poisson2d(300), 0, True, lambda i: i["value_row_tiles"] > 0),
    "column panels": (lambda: synth.random_uniform(60000, 500000, 24, seed=31), 0, False, lambda i: i["panel_tiles"] > 0),
    # under FLAG_EXACT_ORDER the finite rows are the oracle's, bit for bit
    "exact order, stencil grid with a hole": (lambda: grid_with_holes(1000, 1000, holes=[(100, 140, 200, 260)]),
                                              NOXW_NOVI | capi.FLAG_EXACT_ORDER, False, lambda i: i["block_tiles"] == 0),
    "exact order, block matrix": (lambda: fem_ragged(6000, 20, 34, seed=12, drop=0.1, odd_every=40), capi.FLAG_EXACT_ORDER, True,
                                  lambda i: i["block_tiles"] == 0 and i["masked_block_tiles"] == 0),
}


@pytest.mark.parametrize("name", list(DEFAULT_CASES))
def test_default_plan(oracle, name):
    make, flags, index_values, reached = DEFAULT_CASES[name]
    check_default_plan(oracle, name, make(), flags, index_values, reached)


# ---- Level 1: the context's uploads ------------------------------------------------------------------------------------------------

LEVEL1_MATRICES = {"power law": _powerlaw, "grid2d(257)": lambda: grid2d(257)}


def _context_runs(ctx, upload, ops_list):
    """upload(ctx) once, then every (x, y0, runs) of ops_list: the results in order."""
    upload(ctx)
    out = []
    for x, y0, runs in ops_list:
        ctx.set_x(x)
        ctx.set_y(y0)
        ctx.run(runs)
        out.append(ctx.get_y())
    return out


@pytest.mark.parametrize("fmt", ["csr", "coo", "coo keep order", "ell", "hybrid"])
@pytest.mark.parametrize("matrix", list(LEVEL1_MATRICES))
def test_level1_uploads(oracle, matrix, fmt):
    """The context's own arrays (no guards to set here): every format against the oracle's multiply of the same format -- for
    ELLPACK and hybrid that includes the padding's 0.0 * Inf = NaN, the reference's behaviour."""
    what = "%s as %s" % (matrix, fmt)
    rows, cols, p, c, v = _csr(*LEVEL1_MATRICES[matrix]())
    ops = Operands(oracle, what, rows, cols, p, c, v)
    flags = capi.FLAG_COO_KEEP_ORDER if fmt == "coo keep order" else 0

    def stored(val):
        """(upload(ctx), multiply(x, y0, runs) by the oracle, longest stored row) of the format for the values `val`."""
        i, j, a = synth.csr_to_coordinate(rows, p, c, val)
        if fmt == "csr":
            return (lambda ctx: ctx.upload_csr(rows, cols, p, c, val),
                    lambda x, y, runs: oracle.csr_spmv(rows, p, c, val, x, y=y, runs=runs), int(ops.lens.max()))
        if fmt.startswith("coo"):
            r0, c0 = (i - 1).astype(np.int32), (j - 1).astype(np.int32)
            return (lambda ctx: ctx.upload_coo(rows, cols, r0, c0, val),
                    lambda x, y, runs: oracle.coo_spmv(rows, r0, c0, val, x, y=y, runs=runs), int(ops.lens.max()))
        if fmt == "ell":
            _, L, ec, ev = oracle.ell_from_coordinate(rows, i, j, a)
            return (lambda ctx: ctx.upload_ell(rows, cols, L, ec, ev),
                    lambda x, y, runs: oracle.ell_spmv(rows, L, ec, ev, x, y=y, runs=runs), int(L))
        H = oracle.hybrid_from_coordinate(rows, i, j, a)
        return (lambda ctx: ctx.upload_hybrid(rows, cols, H["row_length"], H["ell_col"], H["ell_val"], H["coo_row"], H["coo_col"], H["coo_val"]),
                lambda x, y, runs: oracle.hybrid_spmv(rows, H, x, y=y, runs=runs), int(max(H["row_length"], ops.lens.max())))

    upload, ref, longest = stored(v)
    upload_v, ref_v, _ = stored(ops.vp)
    ref_x, ref_y3 = ref(ops.xp, ops.y0, 1), ref(ops.x, ops.y0p, 3)
    poison.assert_not_vacuous(ref_x, what + " (the format's own multiply)")
    with capi.Context(0, flags) as ctx:
        clean, got_x, clean3, got_y3 = _context_runs(ctx, upload, [(ops.x, ops.y0, 1), (ops.xp, ops.y0, 1), (ops.x, ops.y0, 3), (ops.x, ops.y0p, 3)])
        info = ctx.info()
        print("%s: ctx_info %s" % (what, {k: n for k, n in info.items() if n}))
        assert info["format"] == {"csr": 1, "coo": 2, "coo keep order": 2, "ell": 3, "hybrid": 4}[fmt], info
        (got_v,) = _context_runs(ctx, upload_v, [(ops.x, ops.y0, 1)])
        info_v = ctx.info()
    # atomics: the COO kernel that keeps the order, column panels, the chunks of rows longer than 512 stored entries
    if fmt == "coo keep order" or info["panel_tiles"] > 0:
        sure = np.zeros(rows, dtype=bool)
    elif fmt in ("ell", "hybrid"):  # (the padding counts: every row of an ELLPACK matrix is L entries long)
        sure = np.full(rows, longest <= SURE)
    else:
        sure = ops.lens <= SURE
    _compare(got_x, ref_x, what + ", poisoned x", clean, sure, ops.scale_x, ops.nterms)
    _compare(got_y3, ref_y3, what + ", poisoned y0, three runs", clean3, sure, 3 * ops.scale_y, 3 * ops.nterms)
    same = all(info[k] == info_v[k] for k in ("row_blocks", "long_blocks", "narrow_tiles", "shifted_tiles", "xwin_tiles", "blockwin_tiles", "panel_tiles", "ell_path"))
    _compare(got_v, ref_v(ops.x, ops.y0, 1), what + ", poisoned values", clean if same else None,
             sure if same else np.zeros(rows, dtype=bool), ops.scale_v, ops.nterms)


# ---- spmv_hip_csr_symv: the oracle is the expanded operator -------------------------------------------------------------------------

def _expand(rows, cols, p, c, v):
    """T + T' - diag(T) as CSR arrays with ascending columns, no arithmetic on the values."""
    r = np.repeat(np.arange(rows, dtype=np.int64), np.diff(p.astype(np.int64)))
    off = r != c
    rr, ccol, vv = np.concatenate([r, c[off]]), np.concatenate([c.astype(np.int64), r[off]]), np.concatenate([v, v[off]])
    order = np.lexsort((ccol, rr))
    ep = np.zeros(rows + 1, dtype=np.int64)
    np.cumsum(np.bincount(rr, minlength=rows), out=ep[1:])
    return rows, rows, _i32(ep), _i32(ccol[order]), vv[order]


def _transpose(rows, cols, p, c, v):
    r = np.repeat(np.arange(rows, dtype=np.int64), np.diff(p.astype(np.int64)))
    order = np.lexsort((r, c))
    tp = np.zeros(cols + 1, dtype=np.int64)
    np.cumsum(np.bincount(c, minlength=cols), out=tp[1:])
    return cols, rows, _i32(tp), _i32(r[order]), v[order]


def _load(spec):
    A = hostapi.load(spec, "csr")
    out = _csr(A.rows, A.cols, np.array(A.row_ptr), np.array(A.column_index), np.array(A.value))
    A.close()
    return out


def _tril(rows, cols, p, c, v):
    r = np.repeat(np.arange(rows, dtype=np.int64), np.diff(p.astype(np.int64)))
    keep = c <= r
    tp = np.zeros(rows + 1, dtype=np.int64)
    np.cumsum(np.bincount(r[keep], minlength=rows), out=tp[1:])
    return _csr(rows, cols, tp, c[keep], v[keep])


def _stored_and_operator(oracle, what, stored, operator_of):
    """Operands for a multiply whose operator (expanded / transposed) differs from the stored arrays: x and y0 by the operator's
    shape and rows, the values poisoned in the STORED arrays (before planning), the oracle on the operator of each."""
    ops = Operands(oracle, what, *operator_of(*stored))
    ops.stored_v = stored[4]
    ops.stored_vp, _ = poison.values(stored[2], stored[4])
    opv = operator_of(stored[0], stored[1], stored[2], stored[3], ops.stored_vp)
    ops.ref_v = oracle.csr_spmv(opv[0], opv[2], opv[3], opv[4], ops.x, y=ops.y0, num_threads=1)
    assert np.any(poison.classes(ops.ref_v) != poison.FINITE) and np.mean(poison.classes(ops.ref_v) == poison.FINITE) > 0.5
    with np.errstate(invalid="ignore"):
        ops.scale_v = helpers.abs_products(opv[0], opv[2], opv[3], np.abs(opv[4]), ops.x) + np.abs(ops.y0)
    return ops


def _atomic_family(what, ops, make_plan, multiply, info_ok):
    """symv / spmv_t: x, y0 and values poisoned, both alignments, finite rows within the tolerance of the oracle (the products
    meet in atomics).  make_plan(values) -> (plan, Matrix); multiply(plan, matrix, x, y)."""
    none = np.zeros(ops.rows, dtype=bool)
    plan, m = make_plan(ops.stored_v)
    info = plan.info()
    print("%s: plan_info %s" % (what, info))
    assert info_ok(info), (what, info)
    for front in FRONTS64:
        tag = "%s, x and y %d bytes into their buffers" % (what, 8 * front)
        X, XP = Guarded(ops.x, front), Guarded(ops.xp, front)

        def run(x, y0, runs, t):
            Y = Guarded(y0, front, result=True)
            for _ in range(runs):
                multiply(plan, m, x, Y)
                Y.assert_guards(t)
            return Y.get()

        got = run(XP, ops.y0, 1, tag + ", poisoned x")
        _compare(got, ops.ref_x, tag + ", poisoned x", None, none, ops.scale_x, ops.nterms)
        got3 = run(X, ops.y0p, 3, tag + ", poisoned y0, three runs")
        _compare(got3, ops.ref_y3, tag + ", poisoned y0, three runs", None, none, 3 * ops.scale_y, 3 * ops.nterms)
        X.assert_guards(tag)
        XP.assert_guards(tag)
    m.assert_unchanged(what)
    plan.close()
    plan, m = make_plan(ops.stored_vp)
    X, Y = Guarded(ops.x, FRONTS64[0]), Guarded(ops.y0, FRONTS64[0], result=True)
    multiply(plan, m, X, Y)
    Y.assert_guards(what + ", poisoned values")
    _compare(Y.get(), ops.ref_v, what + ", poisoned values", None, none, ops.scale_v, ops.nterms)
    plan.close()


@functools.lru_cache(maxsize=1)
def _queen_tril():
    return _load("synthetic:queen:30,24,20:tril")


SYMV_CASES = {
    "queen 30,24,20, lower triangle": (_queen_tril, 0, 0, lambda i: i["stored_entries"] > 0 and i["windows"] > 0),
    "delaunay 3 dof, lower triangle": (lambda: _tril(*_csr(*synth.delaunay_mesh(20000, 3, seed=4, order="rcm"))), 0, 0,
                                       lambda i: i["stored_entries"] > 0 and i["windows"] > 0),
    "queen 30,24,20, one window of 64 doubles": (_queen_tril, 1, 64, lambda i: i["spilled_entries"] > 0 and i["max_windows"] == 1),
}


@pytest.mark.parametrize("name", list(SYMV_CASES))
def test_symv(oracle, name):
    make, max_windows, window_doubles, info_ok = SYMV_CASES[name]
    T = make()
    rows, _, p, c, v = T
    assert capi.csr_triangle(rows, p, c)[0] == capi.TRIANGLE_LOWER
    ops = _stored_and_operator(oracle, "symv, " + name, T, _expand)

    def make_plan(values):
        m = Matrix(rows, rows, p, c, values)
        return capi.SymPlan(rows, p, m.c, capi.SYMMETRIC, max_windows, window_doubles, _stream()), m

    _atomic_family("symv, " + name, ops, make_plan, lambda plan, m, x, y: plan.symv(m.p, m.c, m.v, x.ptr, y.ptr, _stream()), info_ok)


# ---- spmv_hip_csr_spmv_t: the poison rule on A', x by rows, y by columns ------------------------------------------------------------

SPMV_T_CASES = {
    "random 20011 x 6007": (lambda: _random(20011, 6007, 8, 21), 0, 0, lambda i: i["stored_entries"] > 0),
    "row lengths 0..7": (_quad_matrix, 0, 100, lambda i: i["stored_entries"] % 4 != 0 and i["rows_per_range"] == 100),
    "random 20011 x 6007, one window of 32 doubles": (lambda: _random(20011, 6007, 8, 21), 1, 32, lambda i: i["spilled_entries"] > 0),
}


@pytest.mark.parametrize("name", list(SPMV_T_CASES))
def test_spmv_t(oracle, name):
    make, max_windows, window_doubles, info_ok = SPMV_T_CASES[name]
    A = _csr(*make())
    rows, cols, p, c, v = A
    ops = _stored_and_operator(oracle, "spmv_t, " + name, A, _transpose)

    def make_plan(values):
        m = Matrix(rows, cols, p, c, values)
        return capi.TrPlan(rows, cols, p, m.c, max_windows, window_doubles, _stream()), m

    _atomic_family("spmv_t, " + name, ops, make_plan, lambda plan, m, x, y: plan.spmv_t(m.p, m.c, m.v, x.ptr, y.ptr, _stream()), info_ok)


# ---- spmv_hip_csr_spmm: every column of X with its own poisoned set, one column clean -----------------------------------------------

class Guarded2:
    """(n, k) row-major as a view into a wider and longer buffer: 2 guard rows in front and behind, `off` guard columns in front and
    `pad` behind; NaN around X, the fixed bit pattern around Y."""

    def __init__(self, A, off, pad, result=False):
        torch = _torch()
        self.n, self.k = A.shape
        self.ld, self.off, self.result = off + self.k + pad, off, result
        self.bits = (np.array(poison.Y_GUARD_BITS, dtype=np.uint64) if result else np.array(np.nan).view(np.uint64)).view(np.int64).item()
        self.raw = torch.full((self.n + 4, self.ld), self.bits, dtype=torch.int64, device="cuda:0")
        self.view = self.raw.view(torch.float64)[2:2 + self.n, off:off + self.k]
        self.view.copy_(torch.from_numpy(np.ascontiguousarray(A)))
        self.ptr = self.view.data_ptr()

    def get(self):
        _torch().cuda.synchronize()
        return self.view.cpu().numpy().copy()

    def assert_guards(self, what):
        _torch().cuda.synchronize()
        g = self.raw.cpu().numpy().copy()
        g[2:2 + self.n, self.off:self.off + self.k] = self.bits
        assert np.all(g == self.bits), "%s: %s written outside its columns" % (what, "Y" if self.result else "X")


@pytest.mark.parametrize("k", [3, 8])
def test_spmm(oracle, k):
    what = "spmm k=%d on row lengths 1 ... 9000" % k
    rows, cols, p, c, v = _csr(*_mixed_lengths())
    clean_q = 1
    rng = np.random.default_rng(5)
    X = np.ascontiguousarray(synth.x_vector(cols, seed=3)[:, None] * (np.arange(k)[None, :] + 1.0))
    Y0 = rng.uniform(-1.0, 1.0, size=(rows, k))
    XP = X.copy()
    for q in range(k):
        if q != clean_q:
            XP[:, q] = poison.x_vector(X[:, q], p, seed=100 + q)
    vp, _ = poison.values(p, v)
    Y0P = np.stack([poison.y0_vector(Y0[:, q]) for q in range(k)], axis=1)

    def ref(val, XX, YY, runs=1):
        return np.stack([oracle.csr_spmv(rows, p, c, val, np.ascontiguousarray(XX[:, q]), y=np.ascontiguousarray(YY[:, q]), num_threads=1, runs=runs)
                         for q in range(k)], axis=1)

    ref_x, ref_v, ref_y3 = ref(v, XP, Y0), ref(vp, X, Y0), ref(v, X, Y0P, 3)
    for q in range(k):
        if q != clean_q:
            poison.assert_not_vacuous(ref_x[:, q], "%s, column %d" % (what, q))
    assert np.all(np.isfinite(ref_x[:, clean_q]))
    sets = [tuple(np.nonzero(~np.isfinite(XP[:, q]))[0]) for q in range(k)]
    assert len(set(sets)) == k  # every column its own set
    m = Matrix(rows, cols, p, c, v)
    mv = Matrix(rows, cols, p, c, vp)
    for flags in (0, capi.FLAG_EXACT_ORDER):
        with capi.MvPlan(rows, cols, p, k, flags, _stream()) as plan:
            info = plan.info()
            print("%s, flags %x: plan_info %s" % (what, flags, info))
            assert info["k"] == k and info["long_rows"] == (0 if flags else int((np.diff(p) > 4096).sum()))
            for off, pad in ((0, 1), (1, 2)):  # leading dimensions k + 1 and k + 3; the second view starts 8 bytes into a row
                tag = "%s, flags %x, ld %d offset %d" % (what, flags, off + k + pad, off)

                def run(mat, XX, YY, runs=1):
                    gx, gy = Guarded2(XX, off, pad), Guarded2(YY, off, pad, result=True)
                    for _ in range(runs):
                        plan.spmm(mat.p, mat.c, mat.v, gx.ptr, gy.ptr, ldx=gx.ld, ldy=gy.ld, stream=_stream())
                        gy.assert_guards(tag)
                    gx.assert_guards(tag)
                    return gy.get()

                clean, clean3 = run(m, X, Y0), run(m, X, Y0, 3)
                got = run(m, XP, Y0)
                poison.assert_classes(got, ref_x, tag + ", poisoned X")  # column q's classes follow its own set only
                poison.assert_finite_rows_bitwise(got, clean, ref_x, tag + ", poisoned X")
                helpers.assert_bitexact(got[:, clean_q], clean[:, clean_q], tag + ": the clean column")
                got3 = run(m, X, Y0P, 3)
                poison.assert_classes(got3, ref_y3, tag + ", poisoned Y0, three runs")
                poison.assert_finite_rows_bitwise(got3, clean3, ref_y3, tag + ", poisoned Y0, three runs")
                gotv = run(mv, X, Y0)
                poison.assert_classes(gotv, ref_v, tag + ", poisoned values")
                poison.assert_finite_rows_bitwise(gotv, clean, ref_v, tag + ", poisoned values")
                if flags:
                    poison.assert_finite_rows_bitwise(got, ref_x, ref_x, tag + ", poisoned X against the oracle")
                    poison.assert_finite_rows_bitwise(gotv, ref_v, ref_v, tag + ", poisoned values against the oracle")
    m.assert_unchanged(what)


# ---- the float-value families -----------------------------------------------------------------------------------------------------

F32_MATRICES = ["mixed_mesh_and_graph", "banded_five_windows", "dense_row_9000_compact", "rows_0_to_7_ragged_end"]


def _f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).astype(np.float32))


@pytest.mark.parametrize("name", F32_MATRICES)
def test_float_value_families(oracle, name):
    """spmv_hip_csr_spmv_f32, _c16, _c16_f64 and _c16_f32xy, default and exact order.  The float arrays take float NaN / Inf; the
    references are the oracle on the widened floats (on the fp64 values for _c16_f64).  Finite rows bitwise against the same
    plan's clean run -- for the float pair that is its own clean run -- and, for double y under exact order, against the oracle."""
    rows, cols, p, c, v = cc.matrix(name)
    a32 = _f32(v)
    assert np.all(a32 != 0)
    wide = a32.astype(np.float64)
    x32 = _f32(synth.x_vector(cols, seed=3))
    y32 = _f32(np.random.default_rng(7).uniform(-1.0, 1.0, size=rows))
    # three operand sets: fp64 x and y over the widened floats / over the fp64 values, float x and y over the widened floats
    sets = {"f32values": Operands(oracle, name + " (float values)", rows, cols, p, c, wide),
            "f64values": Operands(oracle, name + " (fp64 values)", rows, cols, p, c, v),
            "f32xy": Operands(oracle, name + " (float values, float x and y)", rows, cols, p, c, wide, x=x32, y0=y32)}
    mats = {}
    for key, ops in sets.items():
        dt = np.float64 if key == "f64values" else np.float32
        mats[key] = (Matrix(rows, cols, p, c, ops.v, values=dt), Matrix(rows, cols, p, c, ops.vp, values=dt))
        if dt == np.float32:
            assert np.array_equal(poison.classes(_f32(ops.vp)), poison.classes(ops.vp))
    for flags in (0, capi.FLAG_EXACT_ORDER):
        with capi.F32Plan(rows, cols, p, flags, _stream()) as fplan, capi.C16Plan(rows, cols, p, c, flags, _stream()) as cplan:
            finfo, cinfo = fplan.info(), cplan.info()
            print("%s, flags %x: f32 plan %s; c16 plan %s" % (name, flags, finfo, cinfo))
            assert finfo["tiles"] > 0 and cinfo["tiles"] > 0
            if name == "mixed_mesh_and_graph":
                assert cinfo["compact_tiles"] > 100 and cinfo["wide_tiles"] > 100
            if name == "banded_five_windows":
                assert cinfo["tiles_with_5_windows"] > 0
            if name == "dense_row_9000_compact":
                assert cinfo["long_row_tiles"] == 1 and cinfo["wide_tiles"] == 0 and finfo["long_row_tiles"] == 1
            if name == "rows_0_to_7_ragged_end":
                assert cinfo["stored_entries"] % 4 != 0
            families = {
                "spmv_f32": ("f32values", lambda m, x, y: fplan.spmv(m.p, m.c, m.v, x.ptr, y.ptr, _stream())),
                "spmv_c16": ("f32values", lambda m, x, y: cplan.spmv(m.p, m.c, m.v, x.ptr, y.ptr, _stream())),
                "spmv_c16_f64": ("f64values", lambda m, x, y: cplan.spmv_f64(m.p, m.c, m.v, x.ptr, y.ptr, _stream())),
                "spmv_c16_f32xy": ("f32xy", lambda m, x, y: cplan.spmv_f32xy(m.p, m.c, m.v, x.ptr, y.ptr, _stream())),
            }
            for fam, (key, multiply) in families.items():
                ops, (m, mv) = sets[key], mats[key]
                floats = key == "f32xy"
                for front in (FRONTS32 if floats else FRONTS64):
                    tag = "%s, %s, flags %x, x and y %d bytes into their buffers" % (name, fam, flags, (4 if floats else 8) * front)
                    X, XP = Guarded(ops.x, front), Guarded(ops.xp, front)
                    if floats:
                        assert X.ptr % 8 == (0 if front % 2 == 0 else 4)

                    def run(mat, x, y0, runs=1):
                        Y = Guarded(y0, front, result=True)
                        for _ in range(runs):
                            multiply(mat, x, Y)
                            Y.assert_guards(tag)
                        return Y.get()

                    clean, clean3 = run(m, X, ops.y0), run(m, X, ops.y0, 3)
                    against = None if floats or not flags else True
                    got = run(m, XP, ops.y0)
                    _compare(got, ops.ref_x, tag + ", poisoned x", clean, None, None, None, ops.ref_x if against else None)
                    got3 = run(m, X, ops.y0p, 3)
                    _compare(got3, ops.ref_y3, tag + ", poisoned y0, three runs", clean3, None, None, None, ops.ref_y3 if against else None)
                    gotv = run(mv, X, ops.y0)
                    _compare(gotv, ops.ref_v, tag + ", poisoned values", clean, None, None, None, ops.ref_v if against else None)
                    X.assert_guards(tag)
                    XP.assert_guards(tag)
    for m, mv in mats.values():
        m.assert_unchanged(name)


# ---- the scaled forms of the float-value families: y_out <- alpha A x + beta y_in ---------------------------------------------------

SCALED_KINDS = {"f32": "f32values", "c16": "f32values", "c16_f64": "f64values", "c16_f32xy": "f32xy"}  # kind: its operand set
# (alpha, beta, in place): the residual form both ways; y_in kept beside a NaN-filled y_out; beta == 0, no load of y_in; alpha == 0,
# no tile and no product with a row sum
SCALED_PAIRS = [(-1.0, 1.0, True), (-1.0, 1.0, False), (0.375, -2.5, False), (1.0, 0.0, False), (0.0, 0.5, False)]
BOTH = "poisoned x, +Inf in y_in where the row sum is +Inf"
SCALED_UPLOADS = {"f32": ("upload_csr_f32values", 7), "c16": ("upload_csr_compact", 8), "c16_f64": ("upload_csr_compact_f64", 9),
                  "c16_f32xy": ("upload_csr_compact_f32xy", 10)}


@functools.lru_cache(maxsize=1)
def _scaled_sets(oracle, name):
    """The three operand sets of test_float_value_families for `name`, each with z -- the oracle's CSR kernel run once from
    y = +0.0 -- on the clean operand, on the poisoned x and on the poisoned values."""
    rows, cols, p, c, v = cc.matrix(name)
    a32 = _f32(v)
    assert np.all(a32 != 0)
    wide = a32.astype(np.float64)
    x32 = _f32(synth.x_vector(cols, seed=3))
    y32 = _f32(np.random.default_rng(7).uniform(-1.0, 1.0, size=rows))
    sets = {"f32values": Operands(oracle, name + " (float values)", rows, cols, p, c, wide),
            "f64values": Operands(oracle, name + " (fp64 values)", rows, cols, p, c, v),
            "f32xy": Operands(oracle, name + " (float values, float x and y)", rows, cols, p, c, wide, x=x32, y0=y32)}
    for ops in sets.values():
        mul = lambda val, xx: oracle.csr_spmv(rows, p, c, val, np.asarray(xx, dtype=np.float64), num_threads=1, runs=1)
        ops.z, ops.z_x, ops.z_v = mul(ops.v, ops.x), mul(ops.v, ops.xp), mul(ops.vp, ops.x)
        assert np.all(np.isfinite(ops.z))
        # for the residual form: +Inf in y_in on every other row whose poisoned-x sum is +Inf, where -Inf + (+Inf) must give NaN
        ops.inf_rows = np.nonzero(np.isposinf(ops.z_x))[0][::2]
        ops.y0_inf = np.array(ops.y0, copy=True)
        ops.y0_inf[ops.inf_rows] = np.inf
    return sets


def _restated(alpha, beta, z, y_in, dtype):
    with np.errstate(invalid="ignore", over="ignore"):
        return restate(alpha, beta, z, y_in, dtype)


def _scaled_references(ops, dtype, what):
    """{(alpha, beta, poison): restate(...) of the oracle's z on that poisoned operand}, and what the references must show before
    the GPU is looked at.  A non-zero alpha keeps a non-finite row sum non-finite, so the shares of the poisoned x are those of
    the multiply without a scale; under alpha == 0 no row sum is used and a poisoned x or matrix must leave every row finite."""
    zs = {"poisoned x": (ops.z_x, ops.y0), "poisoned values": (ops.z_v, ops.y0), "poisoned y_in": (ops.z, ops.y0p)}
    refs = {(-1.0, 1.0, BOTH): _restated(-1.0, 1.0, ops.z_x, ops.y0_inf, dtype)}
    assert len(ops.inf_rows) > 0 and np.all(np.isnan(refs[(-1.0, 1.0, BOTH)][ops.inf_rows])), what
    for alpha, beta, _ in SCALED_PAIRS:
        for pname, (z, y_in) in zs.items():
            ref = refs[(alpha, beta, pname)] = _restated(alpha, beta, z, y_in, dtype)
            tag = "%s, alpha %g, beta %g, %s" % (what, alpha, beta, pname)
            if pname == "poisoned y_in":
                assert np.all((poison.classes(ref)[::poison.Y0_ROW_STRIDE] != poison.FINITE) == (beta != 0.0)), tag
            elif alpha == 0.0:
                assert np.all(np.isfinite(ref)), tag + ": 0 * Inf in the reference"
            elif pname == "poisoned x":
                poison.assert_not_vacuous(ref, tag)
            else:
                assert np.all(poison.classes(ref)[ops.value_rows] != poison.FINITE), tag
    # the residual form turns a +Inf row sum into -Inf, and -Inf + (+Inf) into NaN
    zc, rc = poison.classes(ops.z_x), poison.classes(refs[(-1.0, 1.0, "poisoned x")])
    assert np.any(zc == poison.PINF) and np.all(rc[zc == poison.PINF] == poison.NINF), what
    return refs


def _int_bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _scaled_plan(kind, rows, cols, p, c, flags):
    """(plan, its scaled multiply as call(matrix, x address, alpha, beta, y_in address, y_out address))."""
    plan = capi.F32Plan(rows, cols, p, flags, _stream()) if kind == "f32" else capi.C16Plan(rows, cols, p, c, flags, _stream())
    fn = {"f32": "spmv_scaled", "c16": "spmv_scaled", "c16_f64": "spmv_f64_scaled", "c16_f32xy": "spmv_f32xy_scaled"}[kind]
    return plan, lambda m, x, alpha, beta, y_in, y_out: getattr(plan, fn)(m.p, m.c, m.v, x, alpha, beta, y_in, y_out, _stream())


def _reached(name, kind, info):
    assert info["tiles"] > 0
    if kind == "f32":
        if name == "dense_row_9000_compact":
            assert info["long_row_tiles"] == 1
        return
    if name == "mixed_mesh_and_graph":
        assert info["compact_tiles"] > 100 and info["wide_tiles"] > 100
    if name == "banded_five_windows":
        assert info["tiles_with_5_windows"] > 0
    if name == "dense_row_9000_compact":
        assert info["long_row_tiles"] == 1 and info["wide_tiles"] == 0
    if name == "rows_0_to_7_ragged_end":
        assert info["stored_entries"] % 4 != 0


@pytest.mark.parametrize("kind", list(SCALED_KINDS))
@pytest.mark.parametrize("name", F32_MATRICES)
def test_scaled_float_value_families(oracle, name, kind):
    """spmv_hip_csr_spmv_f32_scaled, _c16_scaled, _c16_f64_scaled and _c16_f32xy_scaled (include/spmv_hip_scaled.h), default and
    exact order, x and y at both alignments, y_out between the guard pattern.  The reference is test_gpu_scaled.restate on the
    oracle's z of the poisoned operand: the classes follow from the pattern and the signs of alpha and beta alone.  Finite rows
    are bitwise those of the same plan's scaled call on the clean operand (no atomics in this family: every row) and, under exact
    order, the restatement's.  The epilogue reads y_in through a clamped row for the lanes beyond a tile's rows: a clamped load
    that is USED turns a finite neighbour non-finite under (-1, 1), and lets a row of y_in through under (1, 0)."""
    rows, cols, p, c, v = cc.matrix(name)
    ops = _scaled_sets(oracle, name)[SCALED_KINDS[kind]]
    floats = kind == "c16_f32xy"
    dtype = np.float32 if floats else np.float64
    refs = _scaled_references(ops, dtype, "%s, %s" % (name, kind))
    vdt = np.float64 if kind == "c16_f64" else np.float32
    m, mv = Matrix(rows, cols, p, c, ops.v, values=vdt), Matrix(rows, cols, p, c, ops.vp, values=vdt)
    for flags in (0, capi.FLAG_EXACT_ORDER):
        plan, scaled = _scaled_plan(kind, rows, cols, p, c, flags)
        _reached(name, kind, plan.info())
        for front in (FRONTS32 if floats else FRONTS64):
            X, XP = Guarded(ops.x, front), Guarded(ops.xp, front)
            assert X.ptr % (8 if floats else 16) == (0 if front % 2 == 0 else (4 if floats else 8))
            poisons = {"poisoned x": (m, XP, ops.y0), "poisoned values": (mv, X, ops.y0), "poisoned y_in": (m, X, ops.y0p),
                       BOTH: (m, XP, ops.y0_inf)}

            def run(mat, x, y_in, alpha, beta, in_place, tag):
                if in_place:
                    Y = Guarded(y_in, front, result=True)
                    scaled(mat, x.ptr, alpha, beta, Y.ptr, Y.ptr)
                    Y.assert_guards(tag)
                    return Y.get()
                src, out = Guarded(y_in, front), Guarded(np.full(rows, np.nan, dtype=dtype), front, result=True)
                scaled(mat, x.ptr, alpha, beta, src.ptr, out.ptr)
                out.assert_guards(tag)
                src.assert_guards(tag + " (y_in)")
                assert np.array_equal(_int_bits(src.get()), _int_bits(y_in)), tag + ": y_in changed"  # NaN rows included
                return out.get()

            for alpha, beta, in_place in SCALED_PAIRS:
                base = "%s, %s, flags %x, x and y %d bytes into their buffers, alpha %g, beta %g, %s" % (
                    name, kind, flags, dtype().itemsize * front, alpha, beta, "in place" if in_place else "out of place")
                clean = run(m, X, ops.y0, alpha, beta, in_place, base + ", clean")
                assert np.all(np.isfinite(clean)), base + ", clean"
                if flags:
                    poison.assert_finite_rows_bitwise(clean, _restated(alpha, beta, ops.z, ops.y0, dtype), clean, base + ", clean, against the restatement")
                for pname, (mat, x, y_in) in poisons.items():
                    if (alpha, beta, pname) not in refs:
                        continue
                    tag = "%s, %s" % (base, pname)
                    ref = refs[(alpha, beta, pname)]
                    got = run(mat, x, y_in, alpha, beta, in_place, tag)
                    _compare(got, ref, tag, clean, None, None, None, ref if flags else None)
                    if (alpha == 0.0 and pname != "poisoned y_in") or (beta == 0.0 and pname == "poisoned y_in"):
                        # 0 * Inf is never formed; no row of y_in reaches y_out, the clamped lanes' included
                        assert np.all(np.isfinite(got)) and np.array_equal(_int_bits(got), _int_bits(clean)), tag + ": not the clean run's bits"
            X.assert_guards(name)
            XP.assert_guards(name)
        plan.close()
    m.assert_unchanged(name)
    mv.assert_unchanged(name)


@pytest.mark.parametrize("kind", list(SCALED_KINDS))
def test_run_scaled_on_a_poisoned_x_is_the_level_2_call(oracle, kind):
    """spmv_hip_run_scaled with (-1, 1) on contexts of formats 7 to 10: the classes and the finite bits of the Level-2 call."""
    name = "rows_0_to_7_ragged_end"
    rows, cols, p, c, v = cc.matrix(name)
    ops = _scaled_sets(oracle, name)[SCALED_KINDS[kind]]
    floats = kind == "c16_f32xy"
    dtype = np.float32 if floats else np.float64
    ref = _restated(-1.0, 1.0, ops.z_x, ops.y0, dtype)
    poison.assert_not_vacuous(ref, "%s, %s, level 1" % (name, kind))
    upload, fmt = SCALED_UPLOADS[kind]
    m = Matrix(rows, cols, p, c, ops.v, values=np.float64 if kind == "c16_f64" else np.float32)
    for flags in (0, capi.FLAG_EXACT_ORDER):
        tag = "%s, %s, flags %x: spmv_hip_run_scaled(-1, 1) on a poisoned x" % (name, kind, flags)
        with capi.Context(0, flags) as ctx:
            getattr(ctx, upload)(rows, cols, p, c, ops.v)
            assert ctx.info()["format"] == fmt
            (ctx.set_x_f32 if floats else ctx.set_x)(ops.xp)
            (ctx.set_y_f32 if floats else ctx.set_y)(ops.y0)
            ctx.run_scaled(-1.0, 1.0)
            got = (ctx.get_y_f32 if floats else ctx.get_y)()[:rows]
        plan, scaled = _scaled_plan(kind, rows, cols, p, c, flags)
        front = (FRONTS32 if floats else FRONTS64)[0]
        XP, Y = Guarded(ops.xp, front), Guarded(ops.y0, front, result=True)
        scaled(m, XP.ptr, -1.0, 1.0, Y.ptr, Y.ptr)
        Y.assert_guards(tag)
        want = Y.get()
        plan.close()
        poison.assert_classes(want, ref, tag + " (level 2 against the restatement)")
        poison.assert_classes(got, want, tag)
        poison.assert_finite_rows_bitwise(got, want, ref, tag + " (finite rows against level 2)")
