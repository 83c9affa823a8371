"""The workspace rules of the three setup families -- spmv_hip_agg_workspace, spmv_hip_agg_mis2_workspace and
spmv_hip_mcgs_workspace -- return what they returned before the two aggregations came to share one workspace layout and one body
(DESIGN 3.26): the literals below were recorded from the library of the commit before that one, for rows at the edges of the
16-byte rounding and of int32, and are not computed here.  And the shared body refuses as the two bodies did: a workspace one byte
too small names the rule of the entry point that was called, and a theta outside [0, 1] is refused before the workspace is
looked at.  Made-up addresses, no device (test_agg_capi.py)."""
import pytest

from spmv_amd import capi
from test_agg_capi import A, INV, N

ROWS = (0, 1, 15, 16, 17, 4099, 2 ** 24, 2 ** 31 - 1)
NNZ = (0, 1, 7, 2 ** 31 - 1)
# rows: the bytes at the four nnz
AGG = {0: (80, 144, 256, 42949673056), 1: (112, 176, 288, 42949673088), 15: (416, 480, 592, 42949673392),
       16: (480, 544, 656, 42949673456), 17: (512, 576, 688, 42949673488), 4099: (102528, 102592, 102704, 42949775504),
       16777216: (419430480, 419430544, 419430656, 43369103456), 2147483647: (53687091216, 53687091280, 53687091392, 96636764192)}
MIS2 = {0: 80, 1: 128, 15: 432, 16: 496, 17: 544, 4099: 106640, 16777216: 436207696, 2147483647: 55834574864}
MCGS = {0: 288, 1: 576, 15: 576, 16: 576, 17: 592, 4099: 5712, 16777216: 21037344, 2147483647: 2692743456}


def test_the_three_workspace_rules_return_the_recorded_bytes():
    assert tuple(AGG) == tuple(MIS2) == tuple(MCGS) == ROWS
    for rows in ROWS:
        assert tuple(capi.agg_workspace_bytes(rows, nnz) for nnz in NNZ) == AGG[rows], rows
        assert capi.agg_mis2_workspace_bytes(rows) == MIS2[rows], rows
        assert capi.mcgs_workspace_bytes(rows) == MCGS[rows], rows


def _aggregate(call, **o):
    a = dict(A, n=N, theta=0.25, seed=0)
    a.update(o)
    call(a["n"], a["p"], a["c"], a["v"], a["theta"], a["seed"], a["agg"], a["status"], a["work"], a["work_bytes"])


@pytest.mark.parametrize("call, need, rule", [(capi.agg_aggregate, capi.agg_workspace_bytes, r"spmv_hip_agg_workspace\(rows, 0\)"),
                                              (capi.agg_aggregate_mis2, capi.agg_mis2_workspace_bytes, r"spmv_hip_agg_mis2_workspace\(rows\)")],
                         ids=["distance 1", "distance 2"])
def test_a_refused_aggregate_names_its_own_workspace_rule_and_looks_at_theta_first(call, need, rule):
    with pytest.raises(capi.SpmvHipError, match=rule) as e:
        _aggregate(call, work_bytes=need(N) - 1)
    assert e.value.code == INV and "work_bytes" in str(e.value)
    for theta in (float("nan"), -0.1, 1.1):
        for work_bytes in (need(N), need(N) - 1, 0):
            with pytest.raises(capi.SpmvHipError, match="theta") as e:
                _aggregate(call, theta=theta, work_bytes=work_bytes)
            assert e.value.code == INV and "work_bytes" not in str(e.value)
