"""Round 10's plan-time switches of the stencil row chunks (plan_csr.hip build_stencil_runs; libspmv_hip_experiments.so reads them,
the product library ignores them): SPMV_HIP_RUNS_SWEEP=0 keeps every launch forward, SPMV_HIP_RUNS_YIN_NT=1 reads y_in with `nt`
where the plan would not, SPMV_HIP_RUNS_YOUT_NT=0 stores y with the default policy.  Each one flipped alone, and all at once, gives
y bit for bit as the plan without runs over two launches of one plan.  Run in a process of its own with SPMV_HIP_EXPERIMENTS=1
(tests/test_gpu_stencil_sweep.py does that)."""
import os

import pytest

from test_gpu_stencil_chunks import NOXW, grid
from test_gpu_stencil_runs import check_case, grid2d

pytestmark = pytest.mark.gpu

FLIPPED = {"SPMV_HIP_RUNS_SWEEP": "0", "SPMV_HIP_RUNS_YIN_NT": "1", "SPMV_HIP_RUNS_YOUT_NT": "0"}
SWITCHES = list(FLIPPED)


@pytest.fixture(scope="module")
def oracle():
    import oracle_py
    return oracle_py.Oracle()


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
@pytest.mark.parametrize("shape", ["1000x1000", "901x922"])
def test_switch_flipped(oracle, switched, shape):
    A = grid2d(1000) if shape == "1000x1000" else grid(901, 922)
    info = check_case(oracle, A, flags=NOXW, runs=2, what="%s with %s flipped" % (shape, switched))
    assert bool(info["run_variant"] & 4) == ("SPMV_HIP_RUNS_SWEEP" not in switched), info
