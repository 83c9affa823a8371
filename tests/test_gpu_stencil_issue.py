"""Stencil row chunks with every load of a chunk issued in one round trip (csr_runs.hpp): x read as the pair at clamp(c, 0, cols - 2)
with the missing half taken from the other lane of the pair, the value LDS-DMA in 640-double slots with a full chunk's last entry
loaded into a register, the masked path's LDS reads issued together.  Every case checks y bit for bit against the plan without
runs (FLAG_NO_STENCIL_RUNS), which the earlier run kernel matched bit for bit, and against the CPU oracle where that plan matches it.
"""
import numpy as np
import pytest

from test_gpu_stencil_chunks import NOXW, grid
from test_gpu_stencil_runs import check_case, grid2d

pytestmark = pytest.mark.gpu


def chunk_sizes(rows):
    """The chunk row counts of a grid whose rows all lie in one range from row 0 (build_stencil_runs: cuts at multiples of 128,
    no chunk of one row)."""
    sizes = [128] * (rows // 128)
    tail = rows % 128
    if tail == 1:
        sizes[-1:] = [127, 2]
    elif tail:
        sizes.append(tail)
    return sizes


# rows = nx * ny: the last chunk holds 2, 3, 127 or 128 rows, or 127 + 2 (rows = 1 mod 128); the first grid line reads x at
# column -1 (row 0, left), the last one at column cols - 1 + 1 (the last row, right), and a lane's pair straddles both ends
@pytest.mark.parametrize("nx,ny,last", [(901, 922, [2]), (901, 999, [3]), (901, 947, [127]), (900, 928, [128]), (901, 973, [127, 2])])
def test_last_chunk_sizes(oracle, nx, ny, last):
    assert chunk_sizes(nx * ny)[-len(last):] == last
    info = check_case(oracle, grid(nx, ny), flags=NOXW, what="5-point %d x %d" % (nx, ny))
    assert info["run_masked_chunks"] > 0, info
    if info["run_rest_tiles"] == 0:  # every row in chunks: the cuts above
        assert info["run_chunks"] == len(chunk_sizes(nx * ny)), info


@pytest.mark.parametrize("nx,ny", [(2000, 513), (513, 2000), (131, 8000)])
def test_rectangular_edges(oracle, nx, ny):
    # grid lines of every length against the chunk cuts: line ends (columns c - 1 and c + 1 missing) at every lane position
    check_case(oracle, grid(nx, ny), flags=NOXW, what="5-point %d x %d" % (nx, ny))


def test_odd_first_entries_in_masked_chunks(oracle):
    # the first grid line's rows hold 3 or 4 entries: the chunk at row 128 starts at entry 3 + 127 * 4 = 511 (a lead of 1) and is
    # masked; interior line ends shift the parity of every later chunk that holds one
    nx, ny = 1500, 700
    A = grid(nx, ny, [(300, 330, 101, 170)])
    rows, _, p, _, _ = A
    cnt = np.diff(p.astype(np.int64))
    starts = np.arange(0, rows, 128)
    masked = np.array([np.any(cnt[s:s + 128] < 5) for s in starts])
    odd = (p[starts] & 1) == 1
    assert np.sum(masked & odd) > 10 and np.sum(~masked & odd) > 10
    info = check_case(oracle, A, flags=NOXW, what="odd leads")
    assert info["run_masked_chunks"] > 0, info


@pytest.mark.parametrize("runs", [1, 3])
def test_poisson_1024_accumulate(oracle, runs):
    # y_in is the previous launch's y: the y_in load and the store of one chunk see each other's rows only through the lane pairs
    check_case(oracle, grid2d(1024), flags=NOXW, runs=runs, what="5-point 1024^2 x%d" % runs)
