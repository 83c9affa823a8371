"""The plan-time off switches of the stencil row chunks (plan_csr.hip build_stencil_runs; libspmv_hip_experiments.so reads them, the
product library ignores them): SPMV_HIP_RUNS_ALIGN=0 cuts chunks from each range's first row, SPMV_HIP_RUNS_MASKED=0 leaves rows
with missing positions to the second launch, SPMV_HIP_RUNS_EARLY=1 issues x and y_in before the descriptor returns where the chunk
list is dense (off by default), SPMV_HIP_RUNS_NT=0 drops `nt` from the value loads.  Each one flipped alone, and all at once, gives
y bit for bit as the plan without runs.  Run in a
process of its own with SPMV_HIP_EXPERIMENTS=1 (tests/test_gpu_stencil_chunks.py does that)."""
import os

import pytest

from test_gpu_stencil_chunks import NOXW, grid
from test_gpu_stencil_runs import check_case, grid2d

pytestmark = pytest.mark.gpu

FLIPPED = {"SPMV_HIP_RUNS_ALIGN": "0", "SPMV_HIP_RUNS_MASKED": "0", "SPMV_HIP_RUNS_EARLY": "1", "SPMV_HIP_RUNS_NT": "0"}
SWITCHES = list(FLIPPED)


@pytest.fixture
def switched(request):
    names = request.param
    old = {k: os.environ.get(k) for k in SWITCHES}
    for k in names:
        os.environ[k] = FLIPPED[k]
    yield names
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


@pytest.mark.parametrize("switched", [[k] for k in SWITCHES] + [SWITCHES], indirect=True, ids=lambda s: "+".join(s))
@pytest.mark.parametrize("shape", ["1000x1000", "1500x700 hole", "127^2"])
def test_switch_off(oracle, switched, shape):
    if shape == "1000x1000":
        A, flags = grid2d(1000), 0
    elif shape == "1500x700 hole":
        A, flags = grid(1500, 700, [(200, 230, 40, 90)]), NOXW
    else:
        A, flags = grid2d(127), NOXW
    info = check_case(oracle, A, flags=flags | NOXW, what="%s with %s flipped" % (shape, switched), expect_runs=shape != "127^2")
    if "SPMV_HIP_RUNS_MASKED" in switched:
        assert info["run_masked_chunks"] == 0, info
        if info["run_chunks"] > 0:
            assert info["run_rest_tiles"] > 0, info
