"""Stencil row runs in aligned chunks (csr_runs.hpp, plan_csr.hip build_stencil_runs): every row whose columns are a subset of one
5-entry pattern -- the interior, the first and last grid lines, the line ends and the corners -- goes to chunks cut at absolute
multiples of 128 rows, with row masks where positions are missing, so that a Poisson grid takes one launch.  Every case checks y
bit for bit against the plan without runs (FLAG_NO_STENCIL_RUNS), and against the CPU oracle wherever that plan matches it
exactly: square grids whose side is no multiple of 128, rectangular grids, grids with holes, matrices of fewer than 128 rows,
accumulation, y_out != y_in and a context upload.  The plan-time off switches of the experiments build run in a child process
(tests/experiments/exp_gpu_run_switches.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from spmv_amd import capi, synth
from test_gpu_stencil_runs import BASE, OFF, check_case, grid2d

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOXW = capi.FLAG_NO_X_WINDOW  # a cache-resident grid takes the x-window launch by default, which has no runs


def grid(nx, ny, holes=(), seed=4):
    """5-point stencil on an nx x ny grid (row r = i * nx + j), random values.  A hole (i0, i1, j0, j1) keeps its cells as rows that
    hold only their diagonal, and their neighbours lose the links into it: rows with missing positions inside the grid."""
    N = nx * ny
    r = np.arange(N, dtype=np.int64)
    i, j = r // nx, r % nx
    alive = np.ones(N, bool)
    for i0, i1, j0, j1 in holes:
        alive &= ~((i >= i0) & (i < i1) & (j >= j0) & (j < j1))
    offs = [(-nx, i > 0), (-1, j > 0), (0, np.ones(N, bool)), (1, j < nx - 1), (nx, i < ny - 1)]
    masks = []
    for o, m in offs:
        m = m.copy()
        if o != 0:
            m &= alive
            m[m] &= alive[r[m] + o]
        masks.append(m)
    cnt = sum(m.astype(np.int64) for m in masks)
    p = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(cnt, out=p[1:])
    c = np.empty(int(p[-1]), dtype=np.int32)
    pos = p[:-1].copy()
    for (o, _), m in zip(offs, masks):  # ascending columns within a row
        c[pos[m]] = (r[m] + o).astype(np.int32)
        pos[m] += 1
    v = np.random.default_rng(seed).uniform(-1.0, 1.0, size=len(c))
    return N, N, p.astype(np.int32), c, v


@pytest.fixture(scope="module")
def oracle():
    import oracle_py
    return oracle_py.Oracle()


@pytest.mark.parametrize("n", [100, 127, 129, 300, 1000, 1500])
def test_square_grids(oracle, n):
    # n^2 rows with n no multiple of 128: line ends fall anywhere inside chunks, and the last chunk is short (127^2 = 126 * 128 + 1)
    info = check_case(oracle, grid2d(n), flags=NOXW, what="5-point %d^2" % n, expect_runs=n >= 1000)
    if info["run_chunks"] > 0:
        assert info["run_masked_chunks"] > 0, info


@pytest.mark.parametrize("nx,ny", [(1024, 700), (333, 3000), (4096, 40), (130, 2000)])
def test_rectangular_grids(oracle, nx, ny):
    check_case(oracle, grid(nx, ny), flags=NOXW, what="5-point %d x %d" % (nx, ny), expect_runs=nx * ny >= 1000000)


@pytest.mark.parametrize("holes", [[(100, 140, 200, 260)], [(5, 6, 0, 1000), (300, 310, 500, 520), (700, 999, 997, 999)]])
def test_grids_with_holes(oracle, holes):
    check_case(oracle, grid(1000, 1000, holes), flags=NOXW, what="holes %s" % (holes,))


@pytest.mark.parametrize("n", [2, 3, 5, 8, 11])
def test_fewer_than_128_rows(oracle, n):
    check_case(oracle, grid2d(n), flags=NOXW, what="5-point %d^2" % n, expect_runs=False)


@pytest.mark.parametrize("mode", ["accumulate", "out_of_place"])
def test_modes(oracle, mode):
    A = grid(1500, 900, [(400, 420, 30, 90)])
    if mode == "accumulate":
        check_case(oracle, A, runs=3, what=mode)
    else:
        check_case(oracle, A, out_of_place=True, what=mode)


def test_context_upload(oracle):
    rows, cols, p, c, v = grid(1100, 1000, [(10, 20, 10, 20)])
    x = synth.x_vector(cols)
    y0 = np.random.default_rng(9).uniform(-1.0, 1.0, size=rows)
    got = {}
    for name, flags in (("on", BASE), ("off", OFF)):
        with capi.Context(0, flags) as ctx:
            ctx.set_csr_algorithm(capi.CSR_AUTO, 0)
            ctx.upload_csr(rows, cols, p, c, v)
            ctx.set_x(x)
            ctx.set_y(y0)
            ctx.run(runs=2)
            got[name] = ctx.get_y()
    assert np.array_equal(got["on"].view(np.int64), got["off"].view(np.int64))
    want = oracle.csr_spmv(rows, p, c, v, x, y=y0, runs=2)
    if np.array_equal(got["off"], want):
        assert np.array_equal(got["on"], want)


def test_poisson_4096_one_launch(oracle):
    # every row of the default workload is in a chunk: 131072 chunks of 128 rows, one masked chunk at each end of every grid line
    # (plus the first and last lines'), and no tile left to a second launch
    info = check_case(oracle, grid2d(4096), what="5-point 4096^2")
    assert info["run_rest_tiles"] == 0, info
    assert info["run_chunks"] == 4096 * 4096 // 128, info
    assert info["run_entries"] == info["nnz"], info
    assert info["run_masked_chunks"] == 2 * 4096 + 2 * 30, info


def test_off_switches_in_the_experiments_library():
    env = dict(os.environ, SPMV_HIP_EXPERIMENTS="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "experiments", "exp_gpu_run_switches.py"), "-x", "-q",
                        "-m", "gpu", "-p", "no:cacheprovider"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=1500)
    assert r.returncode == 0, r.stdout[-4000:]
    assert " passed" in r.stdout and "failed" not in r.stdout
