"""The compact multiply, y += fl32(A) x with 16-bit column codes (include/spmv_hip_compact.h), on the MI355X.  Its tiles, lanes,
products and sums are those of spmv_hip_csr_spmv_f32 and only the source of a column differs, so Level 2's y is compared BIT FOR
BIT with spmv_hip_csr_spmv_f32's for the same flags, in default and in exact order; it is also held to the project's tolerance
against the oracle's CSR kernel on A~ (the values rounded to float), and bit for bit under SPMV_HIP_FLAG_EXACT_ORDER.  Level 2
runs with NaN guard elements around x and y, and with the caller's column and float arrays as views into larger device buffers
whose neighbouring entries hold column 0 and value NaN (the guard scheme of test_gpu_f32values.py)."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import compact_cases as cc
import helpers
import oracle_py
from spmv_amd import capi, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "spmv-cache-trace_amd", "spmv-cache-trace-hip")
BUS = os.path.join(ROOT, "tests", "golden", "bus1138_like.mtx")
POISSON_FILE = os.path.join(ROOT, "tests", "golden", "poisson2D.mtx")
RUNS = 3
GUARD = 5   # doubles in front of and behind x and y on the device
PAD = 8     # entries in front of and behind the column and float arrays (32 bytes: the views stay 16-byte aligned)
SENTINEL = -7.25


def _narrow(v):
    with np.errstate(over="ignore"):
        f = np.asarray(v, dtype=np.float64).astype(np.float32)
    return f.astype(np.float64), f


def _expected(rows, cols, p, c, vt, x, y0):
    if rows == 0 or len(c) == 0:
        return y0.copy(), np.abs(y0), 4096
    want = oracle_py.Oracle().csr_spmv(rows, p, c, vt, x, y=y0, num_threads=4, runs=RUNS)
    scale = RUNS * helpers.abs_products(rows, p, c, vt, x) + np.abs(y0)
    return want, scale, max(4096, int(np.max(np.diff(p))))


def _guarded(a):
    import torch
    whole = torch.full((len(a) + 2 * GUARD,), float("nan"), dtype=torch.float64, device="cuda:0")
    if len(a):
        whole[GUARD:GUARD + len(a)] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:0")
    return whole


def _device_csr(p, c, f):
    """row_ptr, and the columns and floats as VIEWS into larger buffers: the PAD entries in front of and behind them hold
    column 0 and value NaN (they may be multiplied, never summed)."""
    import torch
    dev = torch.device("cuda:0")
    n = len(c)
    tp = torch.from_numpy(np.ascontiguousarray(p, dtype=np.int32)).to(dev)
    bc = torch.zeros(n + 2 * PAD, dtype=torch.int32, device=dev)
    bf = torch.full((n + 2 * PAD,), float("nan"), dtype=torch.float32, device=dev)
    if n:
        bc[PAD:PAD + n] = torch.from_numpy(np.ascontiguousarray(c, dtype=np.int32)).to(dev)
        bf[PAD:PAD + n] = torch.from_numpy(np.ascontiguousarray(f, dtype=np.float32)).to(dev)
    return tp, bc, bf, bc.data_ptr() + 4 * PAD, bf.data_ptr() + 4 * PAD


class Device:
    """The caller's arrays of one matrix on the device, and multiplies through either plan type over them."""

    def __init__(self, rows, cols, p, c, f, x, y0):
        import torch
        self.torch = torch
        self.stream = torch.cuda.current_stream().cuda_stream
        self.rows, self.cols, self.p, self.c, self.x, self.y0 = rows, cols, p, c, x, y0
        self.tp, self.bc, self.bf, self.ac, self.af = _device_csr(p, c, f)
        self.xw = _guarded(x)

    def run(self, plan, runs=RUNS, columns=True):
        """`runs` multiplies from y0 through `plan` (F32Plan or C16Plan); columns=False passes a null column pointer."""
        yw = _guarded(self.y0)
        yw[:GUARD] = SENTINEL
        yw[GUARD + self.rows:] = SENTINEL
        for _ in range(runs):
            plan.spmv(self.tp.data_ptr(), self.ac if columns else 0, self.af, self.xw.data_ptr() + 8 * GUARD, yw.data_ptr() + 8 * GUARD, self.stream)
        self.torch.cuda.synchronize()
        yh, xh = yw.cpu().numpy(), self.xw.cpu().numpy()
        assert np.all(yh[:GUARD] == SENTINEL) and np.all(yh[GUARD + self.rows:] == SENTINEL), "y written outside its rows entries"
        assert np.all(np.isnan(xh[:GUARD])) and np.all(np.isnan(xh[GUARD + self.cols:])) and np.array_equal(xh[GUARD:GUARD + self.cols], self.x), "x changed"
        assert np.array_equal(self.bc.cpu().numpy()[PAD:PAD + len(self.c)], self.c), "columns changed"
        return yh[GUARD:GUARD + self.rows].copy()


def _level1(rows, cols, p, c, v, x, y0, flags=0, allow_rounding=True):
    with capi.Context(0, flags) as ctx:
        ctx.upload_csr_compact(rows, cols, p, c, v, allow_rounding)
        if cols:
            ctx.set_x(x)
        if rows:
            ctx.set_y(y0)
        ctx.run(RUNS)
        return ctx.get_y()[:rows], ctx.info(), ctx.last_run_ns()


def _inputs(rows, cols, seed=5):
    rng = np.random.default_rng(seed)
    return synth.x_vector(cols), rng.uniform(-1.0, 1.0, size=rows)


def _in_compact_tiles(rows, cols, p, c, flags):
    """Per stored entry: whether its tile is compact (from the preview's table)."""
    _, tab, _ = capi.c16_plan_preview(rows, cols, p, c, flags)
    k0 = tab[:, 1].astype(np.int64)
    k1 = np.append(k0[1:], len(c))
    mask = np.zeros(len(c), dtype=bool)
    for w in np.nonzero(tab[:, 4] > 0)[0]:
        mask[k0[w]:k1[w]] = True
    return mask


def _verify_counts_altered_columns(plan, dev, rows, cols, p, c, flags, tag, k=29):
    """A copy of the caller's columns with k entries moved to the next column ON THE DEVICE: verify reports exactly those of
    them that lie in compact tiles (a wide tile's columns are not the plan's)."""
    import torch
    if len(c) == 0 or cols < 2:
        return
    pick = np.sort(np.random.default_rng(17).choice(len(c), size=min(k, len(c)), replace=False))
    want = int(_in_compact_tiles(rows, cols, p, c, flags)[pick].sum())
    altered = dev.bc.clone()
    at = torch.from_numpy(pick + PAD).to(altered.device)
    altered[at] = (altered[at] + 1) % cols
    assert plan.verify(altered.data_ptr() + 4 * PAD, dev.stream) == want, tag + ": verify after %d columns were altered" % len(pick)
    assert plan.verify(dev.ac, dev.stream) == 0


def _check(rows, cols, p, c, v, what, level1=True):
    vt, f = _narrow(v)
    x, y0 = _inputs(rows, cols)
    want, scale, nterms = _expected(rows, cols, p, c, vt, x, y0)
    dev = Device(rows, cols, p, c, f, x, y0)
    info = None
    for flags, order in ((0, "default order"), (capi.FLAG_EXACT_ORDER, "exact order")):
        tag = "%s (%s)" % (what, order)
        with capi.C16Plan(rows, cols, p, c, flags, dev.stream) as plan, capi.F32Plan(rows, cols, p, flags, dev.stream) as f32:
            y = dev.run(plan)
            yf = dev.run(f32)
            assert np.all(np.isfinite(y)), tag + ": a neighbouring NaN was summed"
            helpers.assert_bitexact(y, yf, tag + ": against spmv_hip_csr_spmv_f32")
            if flags:
                helpers.assert_bitexact(y, want, tag + ": against the oracle")
            else:
                helpers.assert_close(y, want, scale, what=tag + " (level 2)", nterms=nterms)
            helpers.assert_bitexact(dev.run(plan), y, tag + ": a second run from the same y0")
            pinfo = plan.info()
            assert pinfo == capi.c16_plan_preview(rows, cols, p, c, flags, table=False)[0]  # the device plan and the host preview agree
            # the content guard: 0 on the right columns, and the exact count after some are altered on the device
            assert plan.verify(dev.ac, dev.stream) == 0
            _verify_counts_altered_columns(plan, dev, rows, cols, p, c, flags, tag)
            # the 32-bit columns are read by wide tiles only
            if pinfo["tiles"] and pinfo["wide_tiles"] == 0:
                helpers.assert_bitexact(dev.run(plan, columns=False), y, tag + ": without the 32-bit columns")
            elif pinfo["tiles"]:
                with pytest.raises(capi.SpmvHipError) as e:
                    dev.run(plan, runs=1, columns=False)
                assert e.value.code == capi.ERR_INVALID and "wide tiles" in str(e.value)
        if level1:
            y1, info1, ns = _level1(rows, cols, p, c, v, x, y0, flags)
            helpers.assert_bitexact(y1, y, tag + ": level 1 against level 2")
            assert info1["format"] == 8 and info1["rows"] == rows and info1["cols"] == cols and info1["stored"] == len(c)
            assert info1["streamed_bytes"] == pinfo["streamed_bytes"] and info1["workgroups"] == pinfo["workgroups"]
            if rows and cols and len(c):
                assert ns > 0
        info = info or pinfo
    return info


@pytest.mark.parametrize("name", cc.NAMES)
def test_against_the_fp32_value_multiply_and_the_oracle(name):
    rows, cols, p, c, v = cc.matrix(name)
    info = _check(rows, cols, p, c, v, name)
    if name == "mixed_mesh_and_graph":
        assert info["compact_tiles"] > 100 and info["wide_tiles"] > 100  # both branches in one launch
    if name == "dense_row_9000_compact":
        assert info["long_row_tiles"] == 1 and info["wide_tiles"] == 0
    if name == "rows_0_to_7_ragged_end":
        assert info["stored_entries"] % 4 != 0


@pytest.mark.parametrize("name", ["poisson_512", "banded_five_windows", "dense_row_9000_compact", "mixed_mesh_and_graph"])
def test_verify_counts_the_columns_that_were_altered(name):
    """One-window tiles, multi-window tiles, a compact long row, and compact beside wide tiles: columns altered on the device,
    a few and many, within a window and across windows; entries of wide tiles are not the plan's and do not count."""
    import torch
    rows, cols, p, c, v = cc.matrix(name)
    in_compact = _in_compact_tiles(rows, cols, p, c, 0)
    rng = np.random.default_rng(18)
    tc = torch.from_numpy(c).to("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    with capi.C16Plan(rows, cols, p, c, 0, stream) as plan:
        assert plan.verify(tc.data_ptr(), stream) == 0
        for k, step in ((1, 8192), (37, 1), (min(5000, len(c)), 3)):
            pick = np.sort(rng.choice(len(c), size=k, replace=False))
            at = torch.from_numpy(pick).to("cuda:0")
            altered = tc.clone()
            altered[at] = (altered[at] + step) % cols
            assert plan.verify(altered.data_ptr(), stream) == int(in_compact[pick].sum()), (name, k, step)
        if name == "mixed_mesh_and_graph":
            assert 0 < int(in_compact.sum()) < len(c)
        with pytest.raises(capi.SpmvHipError) as e:
            plan.verify(0, stream)
        assert e.value.code == capi.ERR_INVALID


def test_level1_keeps_neither_fp64_values_nor_32bit_columns():
    rows, cols, p, c, v = cc._csr(*synth.poisson2d(1024)[:5])
    nnz = len(c)
    assert nnz > 5_000_000
    v = np.random.default_rng(71).uniform(-1.0, 1.0, size=nnz)
    pre = capi.c16_plan_preview(rows, cols, p, c, table=False)[0]
    assert pre["wide_tiles"] == 0
    assert pre["device_bytes"] <= 2 * nnz + 6 * 2 * pre["tiles"] + 48 * pre["tiles"] + 32  # 2 bytes per entry, at most 6 slots of padding and 48 bytes per tile
    # what spmv_hip_ctx_info [9] counts: row_ptr, the floats, the vectors (each padded by 64 bytes) and the plan, which holds
    # the codes -- no 4 nnz of columns, no 8 nnz of fp64 values
    base = (4 * (rows + 1) + 64) + (4 * nnz + 64) + (8 * cols + 64) + (8 * rows + 64) + pre["device_bytes"]
    with capi.Context(0) as ctx:
        ctx.upload_csr_compact(rows, cols, p, c, v)
        got = ctx.info()["device_bytes"]
    print("ctx_info[9] = %d, base = %d (%.3f bytes per stored entry beside row_ptr and the vectors)" % (
        got, base, (got - 4 * (rows + 1) - 8 * cols - 8 * rows) / nnz))
    assert base - 5 * 64 <= got <= base + 5 * 64
    assert got < 6.2 * nnz + 4 * (rows + 1) + 8 * cols + 8 * rows
    # with wide tiles the 32-bit columns stay
    rows, cols, p, c, v = cc.matrix("mixed_mesh_and_graph")
    pre = capi.c16_plan_preview(rows, cols, p, c, table=False)[0]
    with capi.Context(0) as ctx:
        ctx.upload_csr_compact(rows, cols, p, c, v)
        got = ctx.info()["device_bytes"]
    base = (4 * (rows + 1) + 64) + 2 * (4 * len(c) + 64) + (8 * cols + 64) + (8 * rows + 64) + pre["device_bytes"]
    assert base - 5 * 64 <= got <= base + 5 * 64


def test_refusals():
    rows, cols, p, c, v = cc.from_lengths(np.full(400, 5), 900, 31)
    x, y0 = _inputs(rows, cols)
    with capi.Context(num_gpus=1) as m:
        with pytest.raises(capi.SpmvHipError) as e:
            m.upload_csr_compact(rows, cols, p, c, v)
        assert e.value.code == capi.ERR_STATE
    inexact = int(np.sum(_narrow(v)[0] != v))
    assert inexact > 0
    with capi.Context(0) as ctx:
        ctx.upload_csr_compact(rows, cols, p, c, v)
        with pytest.raises(capi.SpmvHipError) as e:
            ctx.upload_csr_compact(rows, cols, p, c, v, allow_rounding=False)
        assert e.value.code == capi.ERR_INVALID and ("%d value" % inexact) in str(e.value)
        assert ("entry %d" % int(np.nonzero(_narrow(v)[0] != v)[0][0])) in str(e.value)
        big = v.copy()
        big[3] = 1e300
        with pytest.raises(capi.SpmvHipError) as e:
            ctx.upload_csr_compact(rows, cols, p, c, big)
        assert e.value.code == capi.ERR_OVERFLOW
        with pytest.raises(capi.SpmvHipError) as e:
            ctx.upload_csr_compact(rows, cols - 500, p, c, v)
        assert e.value.code == capi.ERR_INVALID
        # a refused upload leaves the matrix that was there, and the context is usable
        ctx.set_x(x)
        ctx.set_y(y0)
        ctx.run(RUNS)
        want, scale, nterms = _expected(rows, cols, p, c, _narrow(v)[0], x, y0)
        helpers.assert_close(ctx.get_y(), want, scale, what="after refusals", nterms=nterms)
        assert ctx.last_run_ns() > 0
        ctx.flush_caches()
        # there are no fp64 values for the block runs to read
        with pytest.raises(capi.SpmvHipError) as e:
            ctx.set_block_x(np.ones((cols, 2)))
        assert e.value.code == capi.ERR_STATE
        with pytest.raises(capi.SpmvHipError) as e:
            ctx.run_block()
        assert e.value.code == capi.ERR_STATE
        # values that are floats already pass with allow_rounding = 0, and a general upload afterwards is a general multiply
        ctx.upload_csr_compact(rows, cols, p, c, _narrow(v)[0], allow_rounding=False)
        assert ctx.info()["format"] == 8
        ctx.upload_csr(rows, cols, p, c, v)
        assert ctx.info()["format"] == 1


def test_spmv_c16_refuses_x_equal_y_and_misaligned_arrays():
    import torch
    rows, cols, p, c, v = cc.matrix("queen_40_32_24")
    tp, bc, bf, ac, af = _device_csr(p, c, _narrow(v)[1])
    tx = torch.ones(max(rows, cols), dtype=torch.float64, device="cuda:0")
    ty = torch.zeros(rows, dtype=torch.float64, device="cuda:0")
    with capi.C16Plan(rows, cols, p, c) as plan:
        for args, code in [((tp.data_ptr(), ac, af, tx.data_ptr(), tx.data_ptr()), capi.ERR_INVALID),
                           ((tp.data_ptr(), ac + 4, af, tx.data_ptr(), ty.data_ptr()), capi.ERR_ALIGN),
                           ((tp.data_ptr(), ac, af + 4, tx.data_ptr(), ty.data_ptr()), capi.ERR_ALIGN),
                           ((tp.data_ptr(), ac, 0, tx.data_ptr(), ty.data_ptr()), capi.ERR_INVALID)]:
            with pytest.raises(capi.SpmvHipError) as e:
                plan.spmv(*args)
            assert e.value.code == code
    torch.cuda.synchronize()
    assert float(ty.abs().max()) == 0.0  # nothing was launched


# ---- the host program ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("matrix", [POISSON_FILE, BUS])
def test_cli_compact_check(matrix):
    r = subprocess.run([CLI, "--csr", matrix, "--device", "hip", "--compact", "--threads", "1", "--profile", "4", "--check", "--x", "uniform"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    doc = json.loads(r.stdout)  # one JSON document
    assert doc
    text = r.stdout
    assert '"hip-csr-spmv-compact"' in text and '"value_bytes": 4' in text
    for key in ('"values_inexact"', '"max_value_rounding"', '"compact_tiles"', '"wide_tiles": 0', '"streamed_bytes"'):
        assert key in text, key
    assert '"pass": true' in text, text[-800:]


def test_cli_compact_exact():
    def cli(matrix):
        return subprocess.run([CLI, "--csr", matrix, "--device", "hip", "--compact=exact", "--threads", "1", "--profile", "4", "--check", "--x", "uniform"],
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    r = cli("synthetic:poisson2d:200")
    assert r.returncode == 0, r.stderr
    assert '"values_inexact": 0' in r.stdout and '"pass": true' in r.stdout
    r = cli("synthetic:kkt:30")
    assert r.returncode == 1 and r.stdout.strip() == "", (r.returncode, r.stdout[:200])
    assert "value" in r.stderr and "not floats" in r.stderr


# ---- the gate ----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def _gate_matrix(which):
    if which == "delaunay_2m_1dof_rcm":
        return cc._csr(*synth.delaunay_mesh(2000000, 1, seed=2))
    return cc._csr(*synth.mesh_dofs((128, 128, 128), 1))


@pytest.mark.parametrize("which", ["delaunay_2m_1dof_rcm", "mesh_dofs_128_1"])
def test_not_slower_than_the_fp32_value_multiply(which):
    """delaunay:2000000,1,2,rcm (33 M entries) and mesh_dofs(128^3, 1): compact tiles hold >= 0.95 of the stored entries (asserted
    from the preview; 0.9922 of the Delaunay mesh's 33 007 990 entries, whole matrix), so the compact multiply does the
    gathers, products and sums of spmv_hip_csr_spmv_f32 on about three quarters of its entry bytes and must not be slower:
    median launch time <= 1.10 x the fp32-value plan's, both in one process on the same device arrays, launches interleaved,
    25 each after warm-up.  The result is first checked bit for bit against the fp32-value multiply's and against the oracle
    in exact order (the correctness case of this matrix).  Streamed bytes by the two previews: 258.0 against 321.4 MB (0.80)
    and 376.3 against 477.0 MB (0.79).  Measured: 66.9 against 66.8 us (ratio 1.002) on the
    Delaunay mesh, 103.3 against 104.9 us (0.985) on mesh_dofs."""
    import torch
    rows, cols, p, c, v = _gate_matrix(which)
    pre = capi.c16_plan_preview(rows, cols, p, c, table=False)[0]
    fpre = capi.f32_plan_preview(rows, cols, p, 0, table=False)[0]
    share = pre["compact_entries"] / pre["stored_entries"]
    print("%s: %d entries, compact tiles hold %.4f of them (%d compact, %d wide tiles; windows used 1..8: %r)" % (
        which, len(c), share, pre["compact_tiles"], pre["wide_tiles"], [pre["tiles_with_%d_windows" % w] for w in range(1, 9)]))
    assert share >= 0.95
    _check(rows, cols, p, c, v, which)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    tp, tc = (torch.from_numpy(a).to(dev) for a in (p, c))
    tf = torch.from_numpy(_narrow(v)[1]).to(dev)
    tx = torch.from_numpy(synth.x_vector(cols)).to(dev)
    ty = torch.zeros(rows, dtype=torch.float64, device=dev)
    with capi.C16Plan(rows, cols, p, c, 0, stream) as c16, capi.F32Plan(rows, cols, p, 0, stream) as f32:
        ways = {
            "f32": lambda: f32.spmv(tp.data_ptr(), tc.data_ptr(), tf.data_ptr(), tx.data_ptr(), ty.data_ptr(), stream),
            "c16": lambda: c16.spmv(tp.data_ptr(), tc.data_ptr(), tf.data_ptr(), tx.data_ptr(), ty.data_ptr(), stream),
        }
        times = {k: [] for k in ways}
        for rnd in range(3 + 25):  # three warm-up rounds
            for k, run in ways.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run()
                e1.record()
                torch.cuda.synchronize()
                if rnd >= 3:
                    times[k].append(e0.elapsed_time(e1) * 1e3)
    med = {k: float(np.median(t)) for k, t in times.items()}
    print("%s, %d launches each: fp32-value plan median %.1f us, compact plan median %.1f us, ratio %.3f; streamed bytes %d against %d, ratio %.3f" % (
        which, len(times["c16"]), med["f32"], med["c16"], med["c16"] / med["f32"], pre["streamed_bytes"], fpre["streamed_bytes"],
        pre["streamed_bytes"] / fpre["streamed_bytes"]))
    assert len(times["f32"]) == 25 and len(times["c16"]) == 25
    assert med["c16"] <= 1.10 * med["f32"], med
