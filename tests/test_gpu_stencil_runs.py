"""Stencil row runs (csr_runs.hpp, plan_csr.hip build_stencil_runs): runs of shifted, uniform stencil-row tiles that share a row
length and a pattern record are cut into chunks of up to 128 rows and multiplied by csr_wavetile_kernel_runs; the other tiles take
the default kernel over a list.  Every case first shows through plan_info that runs were built (and that
FLAG_NO_STENCIL_RUNS builds none), then checks that y is bit for bit what the plan without runs computes, and the CPU oracle's
wherever that plan is bit-exact with it -- for grids whose runs start at every entry offset mod 4, runs shorter than one chunk,
partial last chunks, accumulation, y_out != y_in, EXACT_ORDER and a context upload."""
import numpy as np
import pytest

from helpers import assert_close
from spmv_amd import capi, synth

pytestmark = pytest.mark.gpu

BASE = capi.FLAG_NO_VALUE_INDEX  # values read as doubles: what the runs are for
OFF = BASE | capi.FLAG_NO_STENCIL_RUNS


def grid2d(n, seed=1):
    """5-point stencil on an n x n grid with random values (the values stream is what the runs read)."""
    rows, cols, p, c, _ = synth.poisson2d(n)
    v = np.random.default_rng(seed).uniform(-1.0, 1.0, size=len(c))
    return rows, cols, p, c, v


def grid3d(n, seed=2):
    """7-point stencil on an n^3 grid, random values (the boundary rows are masked stencil tiles)."""
    N = n ** 3
    r = np.arange(N, dtype=np.int64)
    i, j, k = r // (n * n), (r // n) % n, r % n
    offs = [(-n * n, i > 0), (-n, j > 0), (-1, k > 0), (0, np.ones(N, bool)), (1, k < n - 1), (n, j < n - 1), (n * n, i < n - 1)]
    cnt = sum(m.astype(np.int64) for _, m in offs)
    p = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(cnt, out=p[1:])
    c = np.empty(int(p[-1]), dtype=np.int32)
    pos = p[:-1].copy()
    for o, m in offs:  # column order within a row: ascending
        c[pos[m]] = (r[m] + o).astype(np.int32)
        pos[m] += 1
    v = np.random.default_rng(seed).uniform(-1.0, 1.0, size=len(c))
    return N, N, p.astype(np.int32), c, v


def band(m, lead, seed=3):
    """Pentadiagonal band of m rows (columns r-2 ... r+2, clipped) behind `lead` rows holding only their diagonal: the interior
    run starts at entry lead + 7, so lead = 0 ... 3 covers every entry offset mod 4."""
    rows = lead + m
    ps, cs = [0], []
    for r in range(rows):
        if r < lead:
            cc = [r]
        else:
            cc = [q for q in range(r - 2, r + 3) if lead <= q < rows]
        cs.extend(cc)
        ps.append(len(cs))
    v = np.random.default_rng(seed + lead).uniform(-1.0, 1.0, size=len(cs))
    return rows, rows, np.array(ps, np.int32), np.array(cs, np.int32), v


def multiply(rows, cols, p, c, v, x, y0, flags, runs=1, out_of_place=False):
    import torch
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    tp, tc, tv, tx = (torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in (p, c, v, x))
    plan = capi.CsrPlan(rows, cols, p, capi.CSR_AUTO, 0, flags)
    plan.compress(tc.data_ptr(), stream)
    plan.repack(tp.data_ptr(), tc.data_ptr(), tv.data_ptr(), stream)
    info = plan.info()
    ty = torch.from_numpy(y0.copy()).to(dev)
    if out_of_place:
        tout = torch.full((rows,), np.nan, dtype=torch.float64, device=dev)
        plan.spmv_out(tp.data_ptr(), tc.data_ptr(), tv.data_ptr(), tx.data_ptr(), ty.data_ptr(), tout.data_ptr(), stream)
        ty = tout
    else:
        for _ in range(runs):
            plan.spmv(tp.data_ptr(), tc.data_ptr(), tv.data_ptr(), tx.data_ptr(), ty.data_ptr(), stream)
    torch.cuda.synchronize()
    got = ty.cpu().numpy()
    plan.close()
    return got, info


def check_case(oracle, A, flags=0, runs=1, out_of_place=False, expect_runs=True, what=""):
    rows, cols, p, c, v = A
    x = synth.x_vector(cols)
    y0 = np.random.default_rng(7).uniform(-1.0, 1.0, size=rows)
    on, info_on = multiply(rows, cols, p, c, v, x, y0, BASE | flags, runs, out_of_place)
    off, info_off = multiply(rows, cols, p, c, v, x, y0, OFF | flags, runs, out_of_place)
    assert info_off["run_chunks"] == 0, what
    if expect_runs:
        assert info_on["run_chunks"] > 0 and 2 * info_on["run_entries"] > info_on["nnz"], (what, info_on)
    # the same bytes move: the plan's accounting does not change
    for key in ("streamed_bytes", "shifted_entries", "uniform_rows"):
        assert info_on[key] == info_off[key], (what, key)
    assert np.array_equal(on.view(np.int64), off.view(np.int64)), "%s: y differs between runs on and off (%d rows)" % (
        what, int(np.sum(on != off)))
    want = oracle.csr_spmv(rows, p, c, v, x, y=y0, runs=runs)
    if np.array_equal(off, want):
        assert np.array_equal(on, want), what
    else:
        assert_close(on, want, what=what)
    return info_on


@pytest.fixture(scope="module")
def oracle():
    import oracle_py
    return oracle_py.Oracle()


# A cache-resident grid or band stages x through LDS by default (the x-window launch, which takes no runs): these cases also
# run without x windows, where the runs are built.
@pytest.mark.parametrize("xwin", [True, False])
@pytest.mark.parametrize("n", [24, 64, 97, 130, 257, 1000])
def test_grid2d_small(oracle, n, xwin):
    check_case(oracle, grid2d(n), flags=0 if xwin else capi.FLAG_NO_X_WINDOW, what="5-point %d^2" % n,
               expect_runs=n >= 1000 and not xwin)  # (smaller grids: whether runs form depends on the tiling)


@pytest.mark.parametrize("lead", [0, 1, 2, 3])
@pytest.mark.parametrize("m", [60, 127, 129, 300, 4099])
def test_band_offsets(oracle, m, lead):
    # at most one run per matrix, with partial last chunks of every size class (runs form where the tiling gives uniform tiles)
    check_case(oracle, band(m, lead), flags=capi.FLAG_NO_X_WINDOW, what="band m=%d lead=%d" % (m, lead), expect_runs=m > 1000)


@pytest.mark.parametrize("mode", ["accumulate", "out_of_place", "exact_order"])
def test_grid2d_modes(oracle, mode):
    A = grid2d(1200)
    if mode == "accumulate":
        check_case(oracle, A, runs=3, what=mode)
    elif mode == "out_of_place":
        check_case(oracle, A, out_of_place=True, what=mode)
    else:
        check_case(oracle, A, flags=capi.FLAG_EXACT_ORDER, what=mode)


def test_grid2d_4096(oracle):
    info = check_case(oracle, grid2d(4096), what="5-point 4096^2")
    assert info["run_entries"] > 0.99 * info["nnz"]


def test_grid3d_256(oracle):
    # 7-point rows take no runs (measured slower): the plan and y are those of the flag-off plan
    info = check_case(oracle, grid3d(256), what="7-point 256^3", expect_runs=False)
    assert info["run_chunks"] == 0 and info["stencil_mask_tiles"] > 0


def test_context_upload(oracle):
    rows, cols, p, c, v = grid2d(700)
    x = synth.x_vector(cols)
    y0 = np.random.default_rng(5).uniform(-1.0, 1.0, size=rows)
    got = {}
    for name, flags in (("on", BASE), ("off", OFF)):
        with capi.Context(0, flags) as ctx:
            ctx.set_csr_algorithm(capi.CSR_AUTO, 0)
            ctx.upload_csr(rows, cols, p, c, v)
            ctx.set_x(x)
            ctx.set_y(y0)
            ctx.run(runs=2)
            got[name] = ctx.get_y()
    assert np.array_equal(got["on"], got["off"])
    want = oracle.csr_spmv(rows, p, c, v, x, y=y0, runs=2)
    if np.array_equal(got["off"], want):
        assert np.array_equal(got["on"], want)
    else:
        assert_close(got["on"], want)
