"""The window plans of the transposed and the symmetric multiply are the ones the library chose before the two planners became
one (csrc/window_plan.hpp): tests/golden/window_plans.json was written from the commit before that change, by
`python tests/test_window_plan_golden.py OUT.json` with that commit's library, and is never regenerated from the code under test.

Transposed, without a GPU: the 14 numbers of spmv_hip_tr_plan_preview and a SHA-256 of the window table's bytes, for every matrix
and setting of test_transpose_capi.py and for cases that take the greedy cover with a binding budget, one of them (columns that
crowd towards the last of 20008) with a window clipped at the last bucket.  Symmetric, on the GPU (it has no preview): the 16
numbers of spmv_hip_sym_plan_info for lower and upper triangles, a mesh, patterns that spill, rows % 32 != 0 over more than one
range, and a skew-symmetric one."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

from spmv_amd import capi, synth

import test_transpose_capi as trc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "window_plans.json")
SYM_SETTINGS = [(0, 0), (1, 0), (2, 64), (8, 32), (8, 0)]


def _random_rows(rows, cols, per_row, seed, lower=0, crowd=0):
    """per_row random columns in every row (repeats dropped), ascending; lower = 1: columns <= the row, 2: columns < the row;
    crowd > 0: the columns lie in the last `crowd` ones and crowd towards the last (cols - 1 - crowd u^2 for uniform u)."""
    rng = np.random.default_rng(seed)
    hi = np.full(rows, cols) if not lower else np.arange(rows) + (2 - lower)
    u = rng.random((rows, per_row))
    j = np.sort((cols - 1 - (crowd * u * u).astype(np.int64)) if crowd else (u * hi[:, None]).astype(np.int64), axis=1)
    keep = np.ones((rows, per_row), dtype=bool)
    keep[:, 1:] = j[:, 1:] != j[:, :-1]
    keep &= (hi > 0)[:, None]
    p = np.zeros(rows + 1, dtype=np.int32)
    np.cumsum(keep.sum(axis=1), out=p[1:])
    return p, j[keep].astype(np.int32)


def _band(n, lo, hi):
    j = np.arange(n)[:, None] + np.arange(lo, hi + 1)[None, :]
    keep = (j >= 0) & (j < n)
    p = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(keep.sum(axis=1), out=p[1:])
    return p, j[keep].astype(np.int32)


def _tr_cases():
    """name -> (rows, cols, row_ptr, column_index, settings)"""
    out = {name: m + (trc.SETTINGS,) for name, m in trc.MATRICES.items()}
    out["greedy_300x20008"] = (300, 20008) + _random_rows(300, 20008, 12, 31) + ([(0, 0), (8, 0), (2, 50), (3, 40)],)
    out["crowded_300x20008"] = (300, 20008) + _random_rows(300, 20008, 12, 36, crowd=12000) + ([(0, 0), (2, 50), (3, 40)],)
    out["greedy_1000x1000"] = (1000, 1000) + _random_rows(1000, 1000, 12, 32) + ([(1, 32), (8, 32)],)
    return out


def _sym_cases():
    """name -> (rows, row_ptr, column_index, kind)"""
    out = {"band7_lower": (3000,) + _band(3000, -3, 0) + (capi.SYMMETRIC,), "band7_upper": (3000,) + _band(3000, 0, 3) + (capi.SYMMETRIC,)}
    rows, _, p, c, _ = synth.poisson2d(64)
    p, c = np.asarray(p, dtype=np.int64), np.asarray(c, dtype=np.int32)
    low = c <= np.repeat(np.arange(rows), np.diff(p))
    lp = np.zeros(rows + 1, dtype=np.int32)
    np.cumsum(np.add.reduceat(low.astype(np.int64), p[:-1]), out=lp[1:])
    out["poisson64_lower"] = (rows, lp, c[low], capi.SYMMETRIC)
    out["random_1000"] = (1000,) + _random_rows(1000, 1000, 12, 33, lower=1) + (capi.SYMMETRIC,)
    out["random_20008"] = (20008,) + _random_rows(20008, 20008, 12, 34, lower=1) + (capi.SYMMETRIC,)
    out["skew_500"] = (500,) + _random_rows(500, 500, 12, 35, lower=2) + (capi.SKEW_SYMMETRIC,)
    return out


TR_CASES = _tr_cases()
SYM_CASES = _sym_cases()
TR_IDS = [(name, mw, wd) for name in sorted(TR_CASES) for mw, wd in TR_CASES[name][4]]
SYM_IDS = [(name, mw, wd) for name in sorted(SYM_CASES) for mw, wd in SYM_SETTINGS]


def _key(name, mw, wd):
    return "%s|%d,%d" % (name, mw, wd)


def _tr_plan(name, mw, wd):
    rows, cols, p, c, _ = TR_CASES[name]
    info, win = capi.tr_plan_preview(rows, cols, p, c, mw, wd)
    assert win.dtype == np.int32 and win.shape == (info["ranges"], info["max_windows"], 2)
    return {"info": [info[k] for k in capi.TR_INFO_KEYS], "table_sha256": hashlib.sha256(np.ascontiguousarray(win).tobytes()).hexdigest()}


def _sym_plan(name, mw, wd):
    import torch
    rows, p, c, kind = SYM_CASES[name]
    tc = torch.from_numpy(c).to("cuda:0")
    with capi.SymPlan(rows, p, tc.data_ptr(), kind, mw, wd, torch.cuda.current_stream().cuda_stream) as plan:
        info = plan.info()
    return [info[k] for k in capi.SymPlan.INFO_KEYS]


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_golden_file_holds_these_cases_and_no_others(golden):
    assert sorted(golden["transposed"]) == sorted(_key(*i) for i in TR_IDS)
    assert sorted(golden["symmetric"]) == sorted(_key(*i) for i in SYM_IDS)
    assert len(TR_IDS) == 6 * len(trc.MATRICES) + 9 and len(SYM_IDS) == 6 * 5


def test_the_greedy_cases_clip_the_last_bucket_and_meet_the_budget(golden):
    """What the added transposed cases are for, read from the golden numbers: a window that ends at cols = 20008 (not a multiple
    of 32), and entries spilled although windows are left, because the LDS budget or the cap is used up."""
    rows, cols, p, c, settings = TR_CASES["crowded_300x20008"]
    for mw, wd in settings:
        _, win = capi.tr_plan_preview(rows, cols, p, c, mw, wd)
        assert cols % 32 and np.any((win[..., 1] % 32 != 0) & (win[..., 0] + win[..., 1] == cols)), (mw, wd)
    keys = capi.TR_INFO_KEYS
    for name, mw, wd in TR_IDS:
        if name.startswith(("greedy", "crowded")):
            info = dict(zip(keys, golden["transposed"][_key(name, mw, wd)]["info"]))
            assert info["spilled_entries"] > 0, (name, mw, wd)


@pytest.mark.parametrize("name, max_windows, window_doubles", TR_IDS)
def test_transposed_plan_is_the_golden_one(golden, name, max_windows, window_doubles):
    want = golden["transposed"][_key(name, max_windows, window_doubles)]
    got = _tr_plan(name, max_windows, window_doubles)
    assert dict(zip(capi.TR_INFO_KEYS, got["info"])) == dict(zip(capi.TR_INFO_KEYS, want["info"]))
    assert got["table_sha256"] == want["table_sha256"]


@pytest.mark.gpu
@pytest.mark.parametrize("name, max_windows, window_doubles", SYM_IDS)
def test_symmetric_plan_is_the_golden_one(golden, name, max_windows, window_doubles):
    want = golden["symmetric"][_key(name, max_windows, window_doubles)]
    got = _sym_plan(name, max_windows, window_doubles)
    keys = capi.SymPlan.INFO_KEYS
    assert len(got) == len(want) == 16
    assert dict(zip(keys, got)) == dict(zip(keys, want))


if __name__ == "__main__":  # writes the golden file from the library that is loaded (needs a GPU for the symmetric part)
    doc = {"transposed": {_key(*i): _tr_plan(*i) for i in TR_IDS}, "symmetric": {_key(*i): _sym_plan(*i) for i in SYM_IDS}}
    with open(sys.argv[1], "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote %d transposed and %d symmetric cases" % (len(doc["transposed"]), len(doc["symmetric"])))
