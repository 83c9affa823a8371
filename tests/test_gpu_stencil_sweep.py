"""Stencil row chunks swept in alternating directions (csr_runs.hpp, launch.hip): a plan's odd launches of the run kernel map
workgroup b to the mirrored workgroup ((G - 1 - (b >> 3)) << 3) | (b & 7) of a grid rounded up to 8 G workgroups, so that a multiply
starts on the rows of x and y the one before touched last.  Both directions give the same y.  The other stencil tests only ever
make a plan's first launch (forward); every case here makes at least two on one plan and checks y bit for bit against the plan
without runs (FLAG_NO_STENCIL_RUNS) and against the CPU oracle where that plan matches it."""
import os
import subprocess
import sys

import numpy as np
import pytest

from spmv_amd import capi, synth
from test_gpu_stencil_chunks import NOXW, grid
from test_gpu_stencil_runs import BASE, OFF, band, check_case, grid2d

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWEEPS = 4  # run_variant: + 4 where odd launches sweep backwards


def pattern_matrix(n, rels, seed=11):
    """n rows with the columns row + rel for rel in `rels` (ascending), clipped to the matrix; random values."""
    r = np.arange(n, dtype=np.int64)
    masks = [(r + o >= 0) & (r + o < n) for o in rels]
    p = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(sum(m.astype(np.int64) for m in masks), out=p[1:])
    c = np.empty(int(p[-1]), dtype=np.int32)
    pos = p[:-1].copy()
    for o, m in zip(rels, masks):
        c[pos[m]] = (r[m] + o).astype(np.int32)
        pos[m] += 1
    v = np.random.default_rng(seed).uniform(-1.0, 1.0, size=len(c))
    return n, n, p.astype(np.int32), c, v


@pytest.fixture(scope="module")
def oracle():
    import oracle_py
    return oracle_py.Oracle()


@pytest.mark.parametrize("runs", [2, 3, 4])
def test_poisson_1024_both_directions(oracle, runs):
    info = check_case(oracle, grid2d(1024), flags=NOXW, runs=runs, what="5-point 1024^2 x%d" % runs)
    assert info["run_variant"] & SWEEPS, info


# the last chunks hold 2, 3, 127, 128 and 127 + 2 rows; 1623 workgroups (no multiple of 8: the mirrored grid has workgroups that
# leave at once), and the backward sweep starts on the partial chunk
@pytest.mark.parametrize("nx,ny", [(901, 922), (901, 999), (901, 947), (900, 928), (901, 973)])
def test_last_chunk_sizes_backwards(oracle, nx, ny):
    info = check_case(oracle, grid(nx, ny), flags=NOXW, runs=2, what="5-point %d x %d x2" % (nx, ny))
    assert info["run_masked_chunks"] > 0, info
    if (nx, ny) == (901, 922) and info["run_rest_tiles"] == 0:
        assert (info["run_chunks"] + 3) // 4 == 1623, info


# rel[0] and rel[4] adjacent to the triple, odd leads; 4099 rows are 33 chunks where every row is in one (9 workgroups: G = 2
# with a group of one workgroup), 32 where the plan leaves the first or last rows to a tile of their own (G = 1)
@pytest.mark.parametrize("lead", [0, 1, 2, 3])
def test_band_backwards(oracle, lead):
    info = check_case(oracle, band(4099, lead), flags=NOXW, runs=2, what="band 4099 lead %d x2" % lead)
    print("band(4099, %d): %d chunks, %d tiles beside them" % (lead, info["run_chunks"], info["run_rest_tiles"]))
    assert info["run_chunks"] in (32, 33), info


def test_band_two_groups_with_a_group_of_one(oracle):
    info = check_case(oracle, band(4227, 0), flags=NOXW, runs=2, what="band 4227 x2")
    print("band(4227, 0): %d chunks" % info["run_chunks"])
    assert (info["run_chunks"] + 3) // 4 == 9, info


@pytest.mark.parametrize("A,what", [(grid(901, 922), "901 x 922"), (band(4099, 1), "band 4099 lead 1")], ids=["grid", "band"])
def test_every_chunk_once_in_either_direction(A, what):
    """spmv_out twice on one plan (forward, then backward) into an output pre-filled with NaN: a chunk the mirrored map skips leaves
    NaN, one it takes twice is still right here but shows as the skipped chunk it displaces; each against the plan without runs."""
    import torch
    rows, cols, p, c, v = A
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    x = synth.x_vector(cols)
    y0 = np.random.default_rng(7).uniform(-1.0, 1.0, size=rows)
    tp, tc, tv, tx, ty = (torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in (p, c, v, x, y0))
    got = {}
    for name, flags in (("on", BASE | NOXW), ("off", OFF | NOXW)):
        plan = capi.CsrPlan(rows, cols, p, capi.CSR_AUTO, 0, flags)
        plan.compress(tc.data_ptr(), stream)
        plan.repack(tp.data_ptr(), tc.data_ptr(), tv.data_ptr(), stream)
        assert (plan.info()["run_chunks"] > 0) == (name == "on"), what
        got[name] = []
        for _ in range(2):
            tout = torch.full((rows,), np.nan, dtype=torch.float64, device=dev)
            plan.spmv_out(tp.data_ptr(), tc.data_ptr(), tv.data_ptr(), tx.data_ptr(), ty.data_ptr(), tout.data_ptr(), stream)
            torch.cuda.synchronize()
            got[name].append(tout.cpu().numpy())
        plan.close()
    for k in range(2):
        assert not np.any(np.isnan(got["on"][k])), "%s, launch %d: %d rows not written" % (what, k, int(np.sum(np.isnan(got["on"][k]))))
        assert np.array_equal(got["on"][k].view(np.int64), got["off"][k].view(np.int64)), "%s, launch %d" % (what, k)


def test_pentadiagonal_without_a_consecutive_triple(oracle):
    info = check_case(oracle, pattern_matrix(4099, (-4, -2, 0, 2, 4)), flags=NOXW, runs=2, what="r-4 r-2 r r+2 r+4")
    assert info["run_variant"] & 3 == 1, info


def test_misaligned_triple_with_missing_ends(oracle):
    # the triple +2, +3, +4 is consecutive, its middle pair starts at an odd column for even rows, and the rows at both ends of the
    # matrix miss positions on either side (check_case asserts that runs were built)
    info = check_case(oracle, pattern_matrix(6000, (-9, 2, 3, 4, 20)), flags=NOXW, runs=2, what="-9 +2 +3 +4 +20")
    assert info["run_masked_chunks"] > 0, info


def test_run_variant_says_what_ships(oracle):
    info = check_case(oracle, grid2d(1000), flags=NOXW, runs=2, what="5-point 1000^2")
    assert info["run_variant"] == 1 + SWEEPS, info
    none = capi.CsrPlan(1000, 1000, np.arange(1001, dtype=np.int32), capi.CSR_AUTO, 0, OFF)
    assert none.info()["run_variant"] == 0
    none.close()


def test_switches_in_the_experiments_library():
    # the settings that do not ship (forward only, the other y_in policy, y stored with the default policy) are kernels of the
    # experiments library only: a process of its own, since a process loads one of the two libraries
    env = dict(os.environ, SPMV_HIP_EXPERIMENTS="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "experiments", "exp_gpu_run_sweep_switches.py"), "-x", "-q",
                        "-m", "gpu", "-p", "no:cacheprovider"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    assert " passed" in r.stdout and "failed" not in r.stdout
