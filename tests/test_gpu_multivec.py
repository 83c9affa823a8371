"""Y += A X for k vectors (include/spmv_hip_multivec.h) on the MI355X.  For every matrix and k in 1, 2, 3, 4, 5, 6, 8 and 16 -- and
for every other k up to 16 (7 and 9 ... 15: the splits into three passes, 13 = 8 + 4 + 1 and 15 = 8 + 6 + 1, among them) on
rect_wide and lengths_1_to_9000:

  * every column against the oracle (the CPU CSR loop) over three accumulating runs from a random Y, within the project's
    tolerance -- and bit for bit with SPMV_HIP_FLAG_EXACT_ORDER;
  * batch invariance: the k-wide result equals k one-wide multiplies, bit for bit, and so do strided views (ldx, ldy > k, odd
    ones, column slices of wider tensors);
  * two identical runs give identical bits (no atomics);
  * the Level-1 context path gives the bits of Level 2, and leaves the context's single-vector run untouched."""
import functools
import os

import numpy as np
import pytest

import helpers
from spmv_amd import capi, hostapi, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
RUNS = 3
KS = [1, 2, 3, 4, 5, 6, 8, 16]
KS_MORE = [7, 9, 10, 11, 12, 13, 14, 15]  # the remaining k, on MORE_ON only
MORE_ON = ("rect_wide", "lengths_1_to_9000")
WIDTHS = (8, 6, 4, 3, 2, 1)  # the compiled widths of a pass
THREADS = min(16, os.cpu_count() or 1)


def _load(spec, expand=False):
    A = hostapi.load(spec, "csr", expand_symmetric=expand)
    out = (A.rows, A.cols, np.array(A.row_ptr, dtype=np.int32), np.array(A.column_index, dtype=np.int32), np.array(A.value))
    A.close()
    return out


def _rect_random(rows, cols, per_row, seed):
    r, c, p, j, v = synth.random_uniform(rows, cols, per_row, seed=seed)
    return r, c, np.asarray(p, dtype=np.int32), np.asarray(j, dtype=np.int32), np.asarray(v)


def _from_lengths(lens, cols, seed):
    rng = np.random.default_rng(seed)
    p = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=p[1:])
    c = np.concatenate([np.sort(rng.choice(cols, size=int(n), replace=False)) for n in lens] or [np.zeros(0, dtype=np.int64)])
    return len(lens), cols, p.astype(np.int32), c.astype(np.int32), rng.uniform(-1, 1, size=len(c))


def _empty_rows(seed=8):
    rows, cols, p, c, v = _rect_random(4000, 3000, 12, seed)
    keep = np.random.default_rng(seed).random(rows) < 0.5
    lens = np.where(keep, np.diff(p), 0)
    sel = np.repeat(keep, np.diff(p))
    q = np.zeros(rows + 1, dtype=np.int32)
    np.cumsum(lens, out=q[1:])
    return rows, cols, q, c[sel], v[sel]


def _mixed_lengths():
    """Row lengths of 1 ... 9000: the edges of the lane choices (16, 32, ... 1024 entries), of the wave-per-row rows (1024 / 1025)
    and of the workgroup-per-row ones (4096 / 4097), between runs of short rows."""
    rng = np.random.default_rng(21)
    edges = [1, 2, 15, 16, 17, 31, 32, 33, 64, 65, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2048, 4095, 4096, 4097,
             6000, 8191, 9000]
    lens = []
    for e in edges:
        lens += list(rng.integers(0, 40, size=int(rng.integers(1, 90))))
        lens.append(e)
    lens += [9000, 4097, 1, 0, 4097, 9000]
    return _from_lengths(np.array(lens), 12000, seed=22)


MATRICES = {
    "poisson2D_golden": lambda: _load(os.path.join(GOLDEN, "poisson2D.mtx")),
    "bus1138_like": lambda: _load(os.path.join(GOLDEN, "bus1138_like.mtx"), expand=True),
    "rect_wide": lambda: _rect_random(3000, 7001, 9, seed=3),
    "rect_tall": lambda: _rect_random(9001, 1500, 5, seed=4),
    "no_rows": lambda: (0, 5, np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0)),
    "no_entries": lambda: (50, 30, np.zeros(51, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0)),
    "empty_rows": _empty_rows,
    "lengths_1_to_9000": _mixed_lengths,
    "queen_30_24_20": lambda: _load("synthetic:queen:30,24,20"),
    "delaunay_3dof_rcm": lambda: synth.delaunay_mesh(40000, 3, seed=3, order="rcm"),
}


@functools.lru_cache(maxsize=2)
def _matrix(name):
    rows, cols, p, c, v = MATRICES[name]()
    return rows, cols, np.ascontiguousarray(p, dtype=np.int32), np.ascontiguousarray(c, dtype=np.int32), np.ascontiguousarray(v, dtype=np.float64)


def _passes(k):
    """The greedy split of k over the compiled widths: the widest that still fits, until nothing is left."""
    out = []
    while k > 0:
        w = next(w for w in WIDTHS if w <= k)
        out.append(w)
        k -= w
    return out


def _inputs(rows, cols, k, seed=5):
    """X: column c is synth.x_vector scaled by c + 1 (columns differ); Y0 random."""
    x = synth.x_vector(cols)
    X = np.ascontiguousarray(x[:, None] * (np.arange(k)[None, :] + 1.0))
    Y0 = np.random.default_rng(seed).uniform(-1.0, 1.0, size=(rows, k))
    return X, Y0


class Dev:
    """The matrix on the device (torch), with padding so that an empty array still has an address."""

    def __init__(self, rows, cols, p, c, v):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda:0")
        self.stream = torch.cuda.current_stream().cuda_stream
        n = max(1, len(c))
        self.p = torch.from_numpy(p).to(self.dev)
        self.c = torch.zeros(n, dtype=torch.int32, device=self.dev)
        self.v = torch.zeros(n, dtype=torch.float64, device=self.dev)
        if len(c):
            self.c[:len(c)] = torch.from_numpy(c).to(self.dev)
            self.v[:len(c)] = torch.from_numpy(v).to(self.dev)
        self.rows, self.cols = rows, cols

    def tensor(self, A, ld_pad=0, offset=0):
        """A (n, k) on the device as a view of a wider (n, offset + k + ld_pad) tensor: leading dimension offset + k + ld_pad."""
        n, k = A.shape
        big = self.torch.full((max(1, n), offset + k + ld_pad), float("nan"), dtype=self.torch.float64, device=self.dev)
        view = big[:n, offset:offset + k]
        if n:
            view.copy_(self.torch.from_numpy(A))
        return big, view

    def spmm(self, plan, X, Y0, runs=RUNS, ldx_pad=0, ldy_pad=0, xoff=0, yoff=0):
        bigx, tx = self.tensor(X, ldx_pad, xoff)
        bigy, ty = self.tensor(Y0, ldy_pad, yoff)
        # strided torch views as they are; an empty view has no address of its own: the raw address of its base
        ax = tx if X.shape[0] else bigx.data_ptr() + 8 * xoff
        ay = ty if Y0.shape[0] else bigy.data_ptr() + 8 * yoff
        for _ in range(runs):
            plan.spmm(self.p.data_ptr(), self.c.data_ptr(), self.v.data_ptr(), ax, ay, ldx=bigx.stride(0), ldy=bigy.stride(0),
                      stream=self.stream)
        self.torch.cuda.synchronize()
        out = ty.cpu().numpy().copy()
        if ldy_pad or yoff:  # the padding of Y is never written
            rest = bigy.cpu().numpy()[:Y0.shape[0]]
            assert np.isnan(np.delete(rest, np.s_[yoff:yoff + Y0.shape[1]], axis=1)).all()
        return out


def _oracle_columns(oracle, rows, p, c, v, X, Y0):
    k = X.shape[1]
    out = np.empty((rows, k))
    for q in range(k):
        out[:, q] = oracle.csr_spmv(rows, p, c, v, X[:, q], y=Y0[:, q], num_threads=1, runs=RUNS) if rows else np.zeros(0)
    return out


def _scale(rows, cols, p, c, v, X, Y0):
    import scipy.sparse as sp
    if rows == 0:
        return np.zeros((0, X.shape[1]))
    A = sp.csr_matrix((np.abs(v), c, p), shape=(rows, cols))
    return RUNS * (A @ np.abs(X)) + np.abs(Y0)


def _bits(a, b, what):
    helpers.assert_bitexact(np.ascontiguousarray(a).ravel(), np.ascontiguousarray(b).ravel(), what)


@pytest.mark.parametrize("name,k", [(name, k) for name in MATRICES for k in KS] + [(name, k) for name in MORE_ON for k in KS_MORE])
def test_multivec(oracle, name, k):
    rows, cols, p, c, v = _matrix(name)
    X, Y0 = _inputs(rows, cols, k)
    D = Dev(rows, cols, p, c, v)
    want = _oracle_columns(oracle, rows, p, c, v, X, Y0)
    scale = _scale(rows, cols, p, c, v, X, Y0)
    with capi.MvPlan(rows, cols, p, k, 0, D.stream) as plan, capi.MvPlan(rows, cols, p, 1, 0, D.stream) as one:
        info = plan.info()
        assert info["k"] == k and info["rows"] == rows and info["passes"] == len(_passes(k)) and info["widest_pass"] == _passes(k)[0]
        lens = np.diff(p)
        assert info["long_rows"] == int((lens > 4096).sum())
        Y = D.spmm(plan, X, Y0)
        for q in range(k):
            helpers.assert_close(Y[:, q], want[:, q], scale[:, q], what="%s k=%d column %d" % (name, k, q))
        # two identical calls: the same bits
        _bits(D.spmm(plan, X, Y0), Y, "%s k=%d: second run" % (name, k))
        # batch invariance: k one-wide multiplies of the same tiles
        for q in range(k):
            y1 = D.spmm(one, X[:, q:q + 1].copy(), Y0[:, q:q + 1].copy())
            _bits(y1[:, 0], Y[:, q], "%s k=%d: column %d against a one-wide multiply" % (name, k, q))
        # strided views: odd and even leading dimensions, column slices starting 8 bytes into a row
        for ldx_pad, ldy_pad, xoff, yoff in ((3, 0, 0, 0), (0, 5, 0, 0), (1, 2, 1, 1), (2, 1, 0, 3)):
            _bits(D.spmm(plan, X, Y0, ldx_pad=ldx_pad, ldy_pad=ldy_pad, xoff=xoff, yoff=yoff), Y,
                  "%s k=%d: ldx pad %d ldy pad %d offsets %d %d" % (name, k, ldx_pad, ldy_pad, xoff, yoff))
    # exact order: bit-identical to the oracle, per column
    with capi.MvPlan(rows, cols, p, k, capi.FLAG_EXACT_ORDER, D.stream) as exact:
        assert exact.info()["long_rows"] == 0
        _bits(D.spmm(exact, X, Y0), want, "%s k=%d exact order" % (name, k))
    # Level 1: the bits of Level 2, and the single-vector run of the same context untouched by a block run in between
    if rows == 0:
        return
    x = synth.x_vector(cols, seed=99)
    y0 = np.random.default_rng(6).uniform(-1, 1, size=rows)
    with capi.Context(0) as ctx:
        ctx.upload_csr(rows, cols, p, c, v)
        ctx.set_x(x)
        ctx.set_y(y0)
        ctx.run()
        single = ctx.get_y()
        # (the single-vector plan adds the chunks of rows longer than 512 entries with atomics: where two runs of it differ by
        # themselves, the run after the block run is held to the tolerance instead of the bits)
        ctx.set_y(y0)
        ctx.run()
        reproducible = np.array_equal(ctx.get_y().view(np.uint64), single.view(np.uint64))
        ctx.set_block_x(X)
        ctx.set_block_y(Y0)
        ctx.run_block(RUNS)
        assert ctx.last_run_ns() >= 0
        _bits(ctx.get_block_y(k), Y, "%s k=%d: level 1 against level 2" % (name, k))
        ctx.set_y(y0)
        ctx.run()
        if reproducible:
            _bits(ctx.get_y(), single, "%s k=%d: single-vector run after a block run" % (name, k))
        else:
            assert (np.diff(p) > 512).any()
            sw = oracle.csr_spmv(rows, p, c, v, x, y=y0)
            sscale = _scale(rows, cols, p, c, v, x[:, None], y0[:, None])[:, 0] / RUNS
            helpers.assert_close(ctx.get_y(), sw, sscale, what="%s k=%d: single-vector run after a block run" % (name, k))


def test_level1_state_errors():
    rows, cols, p, c, v = _matrix("rect_wide")
    X, Y0 = _inputs(rows, cols, 4)
    with capi.Context(0) as ctx:
        with pytest.raises(capi.SpmvHipError) as e:
            ctx.set_block_x(np.zeros((0, 4)))  # no matrix yet
        assert e.value.code == capi.ERR_STATE
        ctx.upload_csr(rows, cols, p, c, v)
        with pytest.raises(capi.SpmvHipError) as e:
            ctx.run_block()  # no X yet
        assert e.value.code == capi.ERR_STATE
        ctx.set_block_x(X)
        with pytest.raises(capi.SpmvHipError) as e:
            ctx.get_block_y(3)
        assert e.value.code == capi.ERR_STATE
        # a new k starts a new pair: Y zero, and X must be set again
        ctx.set_block_y(Y0[:, :2].copy())
        assert np.array_equal(ctx.get_block_y(2), Y0[:, :2])
        with pytest.raises(capi.SpmvHipError) as e:
            ctx.run_block()
        assert e.value.code == capi.ERR_STATE
        # other uploads: refused
        i, j, a = synth.csr_to_coordinate(rows, p, c, v)
        ctx.upload_coo(rows, cols, i - 1, j - 1, a)
        with pytest.raises(capi.SpmvHipError) as e:
            ctx.set_block_x(X)
        assert e.value.code == capi.ERR_STATE
    with capi.Context(num_gpus=1) as mctx:
        mctx.upload_csr(rows, cols, p, c, v)
        with pytest.raises(capi.SpmvHipError) as e:
            mctx.set_block_x(X)
        assert e.value.code == capi.ERR_STATE


def test_queen_full_size_k8(oracle):
    """queen-like expanded (4.1 M rows, 330 M entries) at k = 8: every column of the whole Y against the oracle."""
    rows, cols, p, c, v = _load("synthetic:queen")
    k = 8
    X, Y0 = _inputs(rows, cols, k)
    D = Dev(rows, cols, p, c, v)
    with capi.MvPlan(rows, cols, p, k, 0, D.stream) as plan:
        info = plan.info()
        assert info["passes"] == 1 and info["long_rows"] == 0
        Y = D.spmm(plan, X, Y0, runs=1)
    del D
    import scipy.sparse as sp
    A = sp.csr_matrix((np.abs(v), c, p), shape=(rows, cols))
    for q in range(k):
        want = oracle.csr_spmv(rows, p, c, v, X[:, q], y=Y0[:, q], num_threads=THREADS)
        scale = A @ np.abs(X[:, q]) + np.abs(Y0[:, q])
        helpers.assert_close(Y[:, q], want, scale, what="queen full size k=8 column %d" % q)
