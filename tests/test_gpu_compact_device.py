"""The compact plan made on the device from device CSR arrays (include/spmv_hip_compact_device.h), on the MI355X.  The coding rule
is integer arithmetic per tile, so the device planner is held to the host planner BIT FOR BIT: the 20 numbers of plan_info, and
the plan read back by spmv_hip_c16_plan_table -- every descriptor field of the table, every base, every code -- against
spmv_hip_c16_plan_preview's restatement of the same arrays on the host; the read-back itself is pinned by the host-made plan's
table.  The multiplies through a device-made plan give the bits of the host-made plan's."""
import ctypes as C
import functools

import numpy as np
import pytest

import compact_cases as cc
import compact_device_cases as dc
import graph_size_cases as gs
from spmv_amd import capi, synth

pytestmark = pytest.mark.gpu

FLAGS = [0, capi.FLAG_EXACT_ORDER]
SENTINEL = 0x5EED5EED0


def _torch():
    import torch
    return torch


def _up(a):
    torch = _torch()
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _stream():
    return _torch().cuda.current_stream().cuda_stream


def _matrix(name):
    return dc.matrix(name) if name in dc.CASES else cc.matrix(name)


@functools.lru_cache(maxsize=2)
def _preview(name, flags):
    rows, cols, p, c, _ = _matrix(name)
    return capi.c16_plan_preview(rows, cols, p, c, flags, codes=True)


def _same_plan(name, flags):
    """Plan on the device, compare with the preview and the host-made plan; returns nothing: every claim is asserted here."""
    rows, cols, p, c, _ = _matrix(name)
    info, tab, codes = _preview(name, flags)
    tp, tc = _up(p), _up(c)
    s = _stream()
    with capi.C16Plan.from_device(rows, cols, tp, tc, flags, s) as dev, capi.C16Plan(rows, cols, p, c, flags, s) as host:
        assert dev.info() == info, (name, flags, "info against the preview")
        assert dev.info() == host.info(), (name, flags, "info against the host-made plan")
        dtab, dcodes = dev.table(codes=True, stream=s)
        htab, hcodes = host.table(codes=True, stream=s)
        assert htab.shape == tab.shape and np.array_equal(htab, tab), (name, flags, "the read-back of the host-made plan")
        assert np.array_equal(hcodes, codes), (name, flags, "the codes read back from the host-made plan")
        assert dtab.shape == tab.shape and np.array_equal(dtab, tab), (name, flags, np.nonzero(np.any(dtab != tab, axis=1))[0][:5])
        assert dcodes.dtype == np.uint16 and np.array_equal(dcodes, codes), (name, flags, np.nonzero(dcodes != codes)[0][:5])
        assert dev.table()[1] is None and np.array_equal(dev.table()[0], tab)
        assert dev.verify(tc.data_ptr(), s) == 0 and host.verify(tc.data_ptr(), s) == 0


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("name", cc.NAMES)
def test_the_device_plan_is_the_host_plan_bit_for_bit(name, flags):
    _same_plan(name, flags)


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("name", dc.NAMES)
def test_the_small_cases_the_existing_matrices_do_not_reach(name, flags):
    _same_plan(name, flags)


# ---- multiplies ---------------------------------------------------------------------------------------------------------------------

def _bits(t):
    return t.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("name", ["poisson_512", "delaunay_60k_3dof_rcm", "mixed_mesh_and_graph", "dense_row_9000_compact", "unsorted_repeats"])
def test_every_family_gives_the_bits_of_the_host_plan(name):
    torch = _torch()
    rows, cols, p, c, v = _matrix(name)
    rng = np.random.default_rng(61)
    tp, tc, tv = _up(p), _up(c), _up(v)
    tf = _up(v.astype(np.float32))
    tx, ty0, tw = _up(synth.x_vector(cols)), _up(rng.uniform(-1.0, 1.0, size=rows)), _up(rng.uniform(-1.0, 1.0, size=rows))
    s = _stream()
    P, J, V, F, X = tp.data_ptr(), tc.data_ptr(), tv.data_ptr(), tf.data_ptr(), tx.data_ptr()
    for flags in FLAGS:
        with capi.C16Plan.from_device(rows, cols, tp, tc, flags, s) as dev, capi.C16Plan(rows, cols, p, c, flags, s) as host:
            assert dev.dots_workspace_bytes() == host.dots_workspace_bytes()
            work = torch.zeros(dev.dots_workspace_bytes() // 8 + 2, dtype=torch.float64, device="cuda:0")
            got = {}
            for which, plan in (("device", dev), ("host", host)):
                y1, y2 = ty0.clone(), ty0.clone()
                y3, y4 = torch.full_like(ty0, float("nan")), torch.full_like(ty0, float("nan"))
                dots = torch.full((2,), float("nan"), dtype=torch.float64, device="cuda:0")
                plan.spmv(P, J, F, X, y1.data_ptr(), s)
                plan.spmv_f64(P, J, V, X, y2.data_ptr(), s)
                plan.spmv_f64_scaled(P, J, V, X, -1.0, 1.0, ty0.data_ptr(), y3.data_ptr(), s)
                plan.spmv_f64_scaled_dots(P, J, V, X, -1.0, 1.0, ty0.data_ptr(), y4.data_ptr(), tw.data_ptr(), dots.data_ptr(), work.data_ptr(),
                                          dev.dots_workspace_bytes(), s)
                torch.cuda.synchronize()
                got[which] = [_bits(t) for t in (y1, y2, y3, y4, dots)]
            for what, a, b in zip(("spmv", "spmv_f64", "spmv_f64_scaled", "spmv_f64_scaled_dots: y", "spmv_f64_scaled_dots: the dots"),
                                  got["device"], got["host"]):
                assert np.array_equal(a, b), (name, flags, what)
            assert not np.any(np.isnan(got["device"][3].view(np.float64))) and not np.array_equal(got["device"][0], _bits(ty0))


# ---- refusals on the device ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bad", [-1, "cols", -2 ** 31])
def test_a_column_out_of_range_is_counted_and_refused(bad):
    torch = _torch()
    lib = capi.load()
    rows, cols, p, c, _ = dc.three_tiles()
    assert capi.c16_plan_preview(rows, cols, p, c, 0, table=False)[0]["tiles"] == 3
    tp, tc = _up(p), _up(c)
    good = int(c[-1])
    s = _stream()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    tc[-1] = cols if bad == "cols" else bad
    h = C.c_void_p(SENTINEL)
    assert lib.spmv_hip_c16_plan_csr_device(C.byref(h), rows, cols, tp.data_ptr(), tc.data_ptr(), 0, s) == capi.ERR_INVALID
    assert h.value == SENTINEL
    assert b"1 column index(es) out of range" in lib.spmv_hip_last_error(), lib.spmv_hip_last_error()
    tc[:3] = tc[-1]  # ... and four of them are counted as four
    with pytest.raises(capi.SpmvHipError, match=r"4 column index\(es\) out of range") as e:
        capi.C16Plan.from_device(rows, cols, tp, tc, 0, s)
    assert e.value.code == capi.ERR_INVALID
    assert torch.cuda.memory_allocated() == before
    # the next valid call on the same arrays, repaired
    tc[:3] = torch.from_numpy(c[:3]).to("cuda:0")
    tc[-1] = good
    with capi.C16Plan.from_device(rows, cols, tp, tc, 0, s) as plan:
        assert plan.info() == capi.c16_plan_preview(rows, cols, p, c, 0, table=False)[0] and plan.verify(tc.data_ptr(), s) == 0
        assert np.array_equal(plan.table(codes=True)[1], capi.c16_plan_preview(rows, cols, p, c, 0, codes=True)[2])
    assert torch.cuda.memory_allocated() == before


def test_a_bad_row_ptr_and_null_columns_are_refused_after_the_read():
    torch = _torch()
    lib = capi.load()
    rows, cols, p, c, _ = dc.three_tiles()
    tc = _up(c)
    s = _stream()
    for make, text in ((lambda q: q.__setitem__(100, q[99] - 1), "non-decreasing"), (lambda q: q.__setitem__(0, 1), "row_ptr[0]")):
        q = p.copy()
        make(q)
        with pytest.raises(capi.SpmvHipError) as host:
            capi.C16Plan(rows, cols, q, c, 0, s)
        tq = _up(q)
        h = C.c_void_p(SENTINEL)
        assert lib.spmv_hip_c16_plan_csr_device(C.byref(h), rows, cols, tq.data_ptr(), tc.data_ptr(), 0, s) == host.value.code == capi.ERR_INVALID
        assert h.value == SENTINEL and text in lib.spmv_hip_last_error().decode()
        assert lib.spmv_hip_last_error().decode() in str(host.value), "the host planner's refusal, with its text"
    h = C.c_void_p(SENTINEL)
    assert lib.spmv_hip_c16_plan_csr_device(C.byref(h), rows, cols, _up(p).data_ptr(), None, 0, s) == capi.ERR_INVALID
    assert h.value == SENTINEL and b"d_column_index is null" in lib.spmv_hip_last_error()
    # no columns are needed where there are no entries; and no column lies in [0, 0)
    with capi.C16Plan.from_device(5, 7, _up(np.zeros(6, dtype=np.int32)), None, 0, s) as plan:
        assert plan.info()["tiles"] == 0 and plan.table(codes=True)[0].shape == (0, 13)
    with pytest.raises(capi.SpmvHipError, match="576 column index") as e:
        capi.C16Plan.from_device(rows, 0, _up(p), tc, 0, s)
    assert e.value.code == capi.ERR_INVALID
    # the table refuses too little room
    with capi.C16Plan.from_device(rows, cols, _up(p), tc, 0, s) as plan:
        tab, cod = np.zeros(3 * 13, dtype=np.int32), np.zeros(len(c), dtype=np.uint16)
        assert lib.spmv_hip_c16_plan_table(plan.h, tab.ctypes.data, 3 * 13 - 1, None, 0, s) == capi.ERR_INVALID
        assert lib.spmv_hip_c16_plan_table(plan.h, None, 0, cod.ctypes.data, len(c) - 1, s) == capi.ERR_INVALID
        assert lib.spmv_hip_c16_plan_table(plan.h, tab.ctypes.data, -1, None, 0, s) == capi.ERR_INVALID
        assert not tab.any() and not cod.any()
        assert lib.spmv_hip_c16_plan_table(plan.h, tab.ctypes.data, 3 * 13, cod.ctypes.data, len(c), s) == 0
        assert np.array_equal(tab.reshape(3, 13), capi.c16_plan_preview(rows, cols, p, c, 0)[1])
    torch.cuda.synchronize()


# ---- composition --------------------------------------------------------------------------------------------------------------------

def test_behind_the_galerkin_product_on_a_side_stream_without_a_synchronisation():
    """The first distance-2 coarse matrix of the 300 x 300 grid, born on the device on a side stream; C16Plan.from_device on that
    stream right behind the numeric product, no synchronisation by the caller in between, the columns never copied to the host
    before the plan is made.  (The symbolic product synchronises by itself and leaves the entry count on the device: that one
    int is read, as every caller of the numeric product must.)"""
    torch = _torch()
    rows, p, c, v = gs.matrix("grid_300x300")
    nnz = len(c)
    i32, f64 = dict(dtype=torch.int32, device="cuda:0"), dict(dtype=torch.float64, device="cuda:0")
    tp, tc, tv = _up(p.astype(np.int32)), _up(c.astype(np.int32)), _up(np.asarray(v, dtype=np.float64))
    agg, status = torch.zeros(rows, **i32), torch.zeros(4, **i32)
    work2 = torch.zeros(capi.agg_mis2_workspace_bytes(rows) // 8, **f64)
    work = torch.zeros(capi.agg_workspace_bytes(rows, nnz) // 8, **f64)
    cc_, order, eptr, cstat = torch.zeros(nnz, **i32), torch.zeros(nnz, **i32), torch.zeros(nnz + 1, **i32), torch.zeros(1, **i32)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    s = side.cuda_stream
    with torch.cuda.stream(side):
        capi.agg_aggregate_mis2(rows, tp, tc, tv, 0.0, gs.SEED, agg, status, work2, None, s)
        na = int(status.cpu()[0])
        mp, mem, cp = torch.zeros(na + 1, **i32), torch.zeros(rows, **i32), torch.zeros(na + 1, **i32)
        side.synchronize()
        aplan = capi.agg_plan(rows, agg, status, mp, mem, work, None, s)
        capi.agg_galerkin_symbolic(aplan, nnz, tp, tc, cp, cc_, order, eptr, cstat, work, None, s)
        nc = int(cstat.cpu()[0])
        cv = torch.zeros(nc, **f64)
        x, b, r = torch.rand(na, **f64), torch.rand(na, **f64), torch.zeros(na, **f64)
        side.synchronize()
        capi.agg_galerkin_numeric(nnz, nc, order, eptr, tv, cv, s)
        plan = capi.C16Plan.from_device(na, na, cp, cc_, 0, s)  # right behind the product
        plan.spmv_f64_scaled(cp.data_ptr(), cc_.data_ptr(), cv.data_ptr(), x.data_ptr(), -1.0, 1.0, b.data_ptr(), r.data_ptr(), s)
        side.synchronize()
        # only now do the arrays visit the host
        hp, hc = cp.cpu().numpy(), cc_.cpu().numpy()[:nc]
        assert na > 1000 and nc == int(hp[-1]) and plan.info()["stored_entries"] == nc
        info, tab, codes = capi.c16_plan_preview(na, na, hp, hc, 0, codes=True)
        dtab, dcodes = plan.table(codes=True, stream=s)
        assert plan.info() == info and np.array_equal(dtab, tab) and np.array_equal(dcodes, codes)
        with capi.C16Plan(na, na, hp, hc, 0, s) as host:
            rh = torch.zeros(na, **f64)
            host.spmv_f64_scaled(cp.data_ptr(), cc_.data_ptr(), cv.data_ptr(), x.data_ptr(), -1.0, 1.0, b.data_ptr(), rh.data_ptr(), s)
            side.synchronize()
            assert np.array_equal(_bits(r), _bits(rh)) and float(r.abs().max()) > 0.0
        plan.close()
    torch.cuda.synchronize()


# ---- lifecycle ------------------------------------------------------------------------------------------------------------------------

def test_destroying_device_made_plans_returns_the_memory():
    torch = _torch()
    rows, cols, p, c, _ = cc.matrix("poisson_512")
    tp, tc = _up(p), _up(c)
    s = _stream()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    free0 = torch.cuda.mem_get_info()[0]
    plan = capi.C16Plan.from_device(rows, cols, tp, tc, 0, s)
    bytes_ = plan.info()["device_bytes"]
    plan.close()
    assert torch.cuda.memory_allocated() == before
    for _ in range(10):
        plan = capi.C16Plan.from_device(rows, cols, tp, tc, 0, s)
        assert plan.verify(tc.data_ptr(), s) == 0
        plan.close()
        plan.close()  # a second close is nothing
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before
    print("a plan of %d bytes made and destroyed eleven times: free device memory moved by %d bytes" % (bytes_, free0 - torch.cuda.mem_get_info()[0]))
