"""The C ABI of the multiply over fp32-stored values (include/spmv_hip_f32values.h) without a GPU: the symbols are exported and
bound, the header is plain C99 on its own, the host narrowing is numpy's astype(float32) bit for bit, arguments are validated
before any device is touched, and the plan's host part (spmv_hip_f32_plan_preview) is recounted in numpy from the tile table it
returns."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from spmv_amd import capi, synth

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spmv_hip_f32values.h")
NEW = ["spmv_hip_narrow_values_host", "spmv_hip_f32_plan_preview", "spmv_hip_narrow_values", "spmv_hip_f32_plan_csr",
       "spmv_hip_csr_spmv_f32", "spmv_hip_f32_plan_info", "spmv_hip_f32_plan_destroy", "spmv_hip_upload_csr_f32values"]
TILE, TILE_ROWS = 512, 64
OVERFLOW = 2.0 ** 128 - 2.0 ** 103  # the smallest double whose float is infinite (halfway between FLT_MAX and 2^128: ties to even)


def test_symbols_exported_declared_and_bound():
    lib = C.CDLL(capi.LIB_PATH)
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(spmv_hip_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(NEW)
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in capi.SIGNATURES, s
    assert HEADER in [os.path.abspath(h) for h in capi.HEADER_PATHS]
    assert hasattr(capi.Context, "upload_csr_f32values") and hasattr(capi, "F32Plan") and hasattr(capi, "f32_plan_preview")
    assert hasattr(capi, "narrow_values_host") and hasattr(capi, "narrow_values")


def test_header_is_c99_on_its_own_and_keeps_the_small_one_small():
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.dirname(HEADER), "-fsyntax-only", "-x", "c", "-"],
                       input='#include "spmv_hip_f32values.h"\nint main(void) { return SPMV_HIP_F32_INFO + SPMV_HIP_F32_TILE + SPMV_HIP_F32_TILE_ROWS; }\n',
                       text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout
    defines = dict(re.findall(r"#define (SPMV_HIP_[A-Z0-9_]+) (\d+)", open(HEADER).read()))
    assert int(defines["SPMV_HIP_F32_INFO"]) == len(capi.F32_INFO_KEYS)
    assert int(defines["SPMV_HIP_F32_TILE"]) == TILE == capi.F32_TILE and int(defines["SPMV_HIP_F32_TILE_ROWS"]) == TILE_ROWS == capi.F32_TILE_ROWS
    small = re.sub(r"/\*.*?\*/", "", open(capi.HEADER_PATH).read(), flags=re.S)
    assert "f32" not in small and "narrow" not in small


# ---- the narrowing ----------------------------------------------------------------------------------------------------------------

def _recount(v, f):
    back = f.astype(np.float64)
    changed = (back != v) & ~np.isnan(v)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.abs(back - v) / np.abs(v)
    return int(changed.sum()), float(np.max(rel[changed])) if changed.any() else 0.0


def _same_as_numpy(v):
    v = np.ascontiguousarray(v, dtype=np.float64)
    with np.errstate(over="ignore"):
        want = v.astype(np.float32)
    got, inexact, rel = capi.narrow_values_host(v)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert (inexact, rel) == _recount(v, want)
    return got, inexact, rel


def test_narrowing_is_numpy_astype_bit_for_bit():
    rng = np.random.default_rng(1)
    fmax = float(np.finfo(np.float32).max)
    _, inexact, rel = _same_as_numpy(rng.uniform(-1.0, 1.0, size=1_000_000))
    assert inexact > 999_000 and 2.0 ** -25 < rel <= 2.0 ** -24
    _same_as_numpy(rng.uniform(-fmax, fmax, size=200_000))
    # log-uniform over the whole float range, denormal results included, and below it (results 0)
    mag = np.exp(rng.uniform(np.log(2.0 ** -160), np.log(fmax), size=400_000))
    _, _, rel = _same_as_numpy(mag * rng.choice([-1.0, 1.0], size=mag.size))
    assert rel == 1.0  # a value below half the smallest denormal becomes 0
    # values that are floats already: nothing changes
    f = rng.standard_normal(100_000).astype(np.float32)
    got, inexact, rel = _same_as_numpy(f.astype(np.float64))
    assert inexact == 0 and rel == 0.0 and np.array_equal(got.view(np.uint32), f.view(np.uint32))
    den = (rng.integers(1, 2 ** 23, size=1000).astype(np.float64) * 2.0 ** -149)  # every float denormal is a double
    assert _same_as_numpy(den)[1] == 0


def test_ties_go_to_even_and_denormal_results_are_kept():
    ulp = 2.0 ** -23
    # halfway between two floats, the lower neighbour even (1.0, 3.0: down) and odd (1 + ulp, 3 + 2 ulp ... : up)
    v = np.array([1.0 + ulp / 2, (1.0 + ulp) + ulp / 2, 1.0 + 3 * ulp / 2, 3.0 + ulp, (3.0 + 2 * ulp) + ulp, -(1.0 + ulp / 2), -((1.0 + ulp) + ulp / 2)])
    got, inexact, _ = _same_as_numpy(v)
    assert got.tolist() == [1.0, np.float32(1.0 + 2 * ulp), np.float32(1.0 + 2 * ulp), 3.0, np.float32(3.0 + 4 * ulp), -1.0, -np.float32(1.0 + 2 * ulp)]
    assert inexact == len(v)
    d = 2.0 ** -149  # the smallest float denormal; ties between denormals go to even too
    v = np.array([1.5 * d, 2.5 * d, 0.5 * d, 0.75 * d, 2.0 ** -127 + d / 2, 3 * d, 2.0 ** -126 - d / 4])
    got, _, rel = _same_as_numpy(v)
    assert got.astype(np.float64).tolist() == [2 * d, 2 * d, 0.0, d, 2.0 ** -127, 3 * d, 2.0 ** -126]
    assert rel == 1.0


def test_zeros_infinities_nan_and_the_overflow_threshold():
    v = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, np.nextafter(OVERFLOW, 0.0), -np.nextafter(OVERFLOW, 0.0)])
    got, inexact, _ = capi.narrow_values_host(v)
    fmax = np.finfo(np.float32).max
    assert got[:4].view(np.uint32).tolist() == [0, 0x80000000, 0x7F800000, 0xFF800000]
    assert np.isnan(got[4]) and got[5] == fmax and got[6] == -fmax
    assert inexact == 2  # NaN does not count, the infinities are exact
    for bad in (OVERFLOW, -OVERFLOW, 1e300, np.finfo(np.float64).max):
        with pytest.raises(capi.SpmvHipError) as e:
            capi.narrow_values_host(np.array([1.0, bad, 2.0]))
        assert e.value.code == capi.ERR_OVERFLOW and "entry 1" in str(e.value)


def test_narrowing_nothing_and_null_pointers():
    lib = capi.load()
    got, inexact, rel = capi.narrow_values_host(np.zeros(0))
    assert len(got) == 0 and inexact == 0 and rel == 0.0
    assert lib.spmv_hip_narrow_values_host(0, None, None, None, None) == capi.OK
    v, f = np.ones(3), np.zeros(3, dtype=np.float32)
    assert lib.spmv_hip_narrow_values_host(3, v.ctypes.data, f.ctypes.data, None, None) == capi.OK and f.tolist() == [1.0, 1.0, 1.0]
    assert lib.spmv_hip_narrow_values_host(3, None, f.ctypes.data, None, None) == capi.ERR_INVALID
    assert lib.spmv_hip_narrow_values_host(3, v.ctypes.data, None, None, None) == capi.ERR_INVALID
    assert lib.spmv_hip_narrow_values_host(-1, v.ctypes.data, f.ctypes.data, None, None) == capi.ERR_INVALID
    assert lib.spmv_hip_narrow_values(-1, None, None, None, None, None) == capi.ERR_INVALID
    assert lib.spmv_hip_narrow_values(3, None, None, None, None, None) == capi.ERR_INVALID
    assert lib.spmv_hip_narrow_values(0, None, None, None, None, None) == capi.OK


# ---- argument validation ------------------------------------------------------------------------------------------------------------

def test_argument_validation_needs_no_device():
    lib = capi.load()
    p = np.array([0, 1, 2, 3], dtype=np.int32)
    c = np.array([0, 3, 2], dtype=np.int32)
    v = np.ones(3)
    h = C.c_void_p()
    out = np.zeros(12, dtype=np.int64)
    tab = np.zeros(64, dtype=np.int32)
    P, Cc, V, O, T = p.ctypes.data, c.ctypes.data, v.ctypes.data, out.ctypes.data, tab.ctypes.data
    assert lib.spmv_hip_upload_csr_f32values(None, 3, 4, 3, P, Cc, V, 1) == capi.ERR_INVALID
    assert lib.spmv_hip_f32_plan_csr(None, 3, 4, P, 0, None) == capi.ERR_INVALID
    assert lib.spmv_hip_csr_spmv_f32(None, None, None, None, None, None, None) == capi.ERR_INVALID
    assert lib.spmv_hip_f32_plan_info(None, out, 12) == capi.ERR_INVALID
    lib.spmv_hip_f32_plan_destroy(None)  # a no-op
    assert lib.spmv_hip_f32_plan_preview(3, 4, P, 0, None, 12, None, 0) == capi.ERR_INVALID
    assert lib.spmv_hip_f32_plan_preview(3, 4, None, 0, O, 12, None, 0) == capi.ERR_INVALID
    bad = np.array([0, 2, 1, 3], dtype=np.int32)  # decreasing
    nonzero_start = np.array([1, 1, 2, 3], dtype=np.int32)
    for rows, cols, rp, flags, text in [(-1, 4, P, 0, b"rows < 0"), (3, -1, P, 0, b"cols < 0"), (3, 4, bad.ctypes.data, 0, b"non-decreasing"),
                                        (3, 4, nonzero_start.ctypes.data, 0, b"row_ptr[0]"), (3, 4, P, 0x1, b"flag"),
                                        (3, 4, P, capi.FLAG_EXACT_ORDER | 0x80, b"flag"), (3, 4, P, 0x80000000, b"flag")]:
        assert lib.spmv_hip_f32_plan_preview(rows, cols, rp, flags, O, 12, None, 0) == capi.ERR_INVALID
        assert text in lib.spmv_hip_last_error(), (text, lib.spmv_hip_last_error())
        assert lib.spmv_hip_f32_plan_csr(C.byref(h), rows, cols, rp, flags, None) == capi.ERR_INVALID
        assert text in lib.spmv_hip_last_error(), (text, lib.spmv_hip_last_error())
        assert not h.value
    # a tile table with too little room
    assert lib.spmv_hip_f32_plan_preview(3, 4, P, 0, O, 12, T, 3) == capi.ERR_INVALID
    assert lib.spmv_hip_f32_plan_preview(3, 4, P, 0, O, 12, T, -1) == capi.ERR_INVALID
    assert lib.spmv_hip_f32_plan_preview(3, 4, P, 0, O, -1, None, 0) == capi.ERR_INVALID
    assert lib.spmv_hip_f32_plan_preview(3, 4, P, 0, O, 12, T, 64) == capi.OK
    assert lib.spmv_hip_f32_plan_preview(3, 4, P, capi.FLAG_EXACT_ORDER, O, 12, T, 64) == capi.OK


def test_no_gpu_means_failure_not_fallback():
    if capi.device_count() > 0:
        pytest.skip("a GPU is present; this test covers the no-device behaviour")
    p = np.array([0, 1, 2, 3], dtype=np.int32)
    with pytest.raises(capi.SpmvHipError) as e:
        capi.F32Plan(3, 4, p)
    assert e.value.code == capi.ERR_NO_DEVICE
    with pytest.raises(capi.SpmvHipError) as e:
        capi.narrow_values(3, 0x1000, 0x2000)  # device arrays cannot be read without a device
    assert e.value.code in (capi.ERR_NO_DEVICE, capi.ERR_HIP)
    with pytest.raises(capi.SpmvHipError) as e:
        capi.Context(0)  # Level 1 starts with a context: there is none to upload into
    assert e.value.code == capi.ERR_NO_DEVICE


# ---- the plan's host part against a numpy recount ---------------------------------------------------------------------------------

def _lengths(lens):
    p = np.zeros(len(lens) + 1, dtype=np.int32)
    np.cumsum(lens, out=p[1:])
    return p


def _matrices():
    import scipy.sparse as sp
    rng = np.random.default_rng(5)
    out = {}
    rows, cols, p, _, _ = synth.poisson2d(64)
    out["poisson64"] = (rows, cols, np.asarray(p, dtype=np.int32))
    n = 3000
    out["banded"] = (n, n, _lengths([min(n, i + 4) - max(0, i - 3) for i in range(n)]))
    out["wide_300x1000"] = (300, 1000, sp.random(300, 1000, density=0.012, random_state=1, format="csr").indptr.astype(np.int32))
    out["tall_1000x300"] = (1000, 300, sp.random(1000, 300, density=0.04, random_state=2, format="csr").indptr.astype(np.int32))
    out["lengths_0_to_7"] = (10007, 9001, _lengths(rng.integers(0, 8, size=10007)))
    skew = []
    for e in [1, 2, 15, 16, 17, 31, 32, 33, 64, 65, 128, 129, 255, 256, 257, 505, 508, 509, 510, 511, 512, 513, 514, 515, 516, 1023, 1024, 1025, 4097, 9000]:
        skew += list(rng.integers(0, 40, size=int(rng.integers(1, 90)))) + [e]
    out["skewed_1_to_9000"] = (len(skew), 12000, _lengths(skew))
    one = rng.integers(0, 4, size=3000)
    one[1717] = 20000
    out["one_dense_row"] = (3000, 20000, _lengths(one))
    out["uniform_4"] = (5000, 5000, _lengths(np.full(5000, 4)))
    out["no_entries"] = (40, 50, np.zeros(41, dtype=np.int32))
    out["no_rows"] = (0, 50, np.zeros(1, dtype=np.int32))
    out["no_cols"] = (40, 0, np.zeros(41, dtype=np.int32))
    return out


MATRICES = _matrices()


def _recount_plan(rows, cols, p, flags, info, tab):
    """Every claim of the preview, recounted from row_ptr and the tile table."""
    p = p.astype(np.int64)
    nnz = int(p[rows])
    lens = np.diff(p)
    assert info["rows"] == rows and info["cols"] == cols and info["stored_entries"] == nnz and info["flags"] == flags
    assert info["longest_row"] == (int(lens.max()) if rows else 0)
    if rows == 0 or cols == 0 or nnz == 0:  # the multiply does nothing
        assert tab.shape == (0, 4)
        assert all(info[k] == 0 for k in ("tiles", "long_row_tiles", "device_bytes", "streamed_bytes", "uniform_tiles", "scalar_tiles", "workgroups"))
        return
    assert tab.shape == (info["tiles"], 4) and info["tiles"] > 0
    r0, k0, nr, ll = (tab[:, i].astype(np.int64) for i in range(4))
    # the tiles cover rows 0 ... rows and entries 0 ... nnz exactly once and in order
    assert r0[0] == 0 and np.all(nr >= 1) and np.array_equal(r0[1:], (r0 + nr)[:-1]) and r0[-1] + nr[-1] == rows
    assert np.array_equal(k0, p[r0])
    k1 = p[r0 + nr]
    assert k1[-1] == nnz
    assert np.all((nr << ll) <= 64) and np.all(nr <= TILE_ROWS)
    span = k1 - (k0 & ~3)  # entries counted from the tile's 4-aligned first entry
    assert np.all(span[nr > 1] <= TILE)
    long_tiles = (nr == 1) & (span > TILE)
    assert np.all(span[~long_tiles] <= TILE)
    assert info["long_row_tiles"] == int(long_tiles.sum())
    exact = bool(flags & capi.FLAG_EXACT_ORDER)
    if exact:
        assert np.all(ll == 0)
    else:
        assert np.all(ll[long_tiles] == 6)
    uniform = scalar = row_ptr_bytes = 0
    for w in range(len(r0)):
        if long_tiles[w]:
            continue
        tl = lens[r0[w]:r0[w] + nr[w]]
        longest = int(tl.max())
        if not exact:  # lanes per row: the fewest that leave at most 16 entries per lane
            want = 0
            while want < 6 and (16 << want) < longest:
                want += 1
            assert ll[w] == want, (w, longest, ll[w])
        fast = k1[w] > k0[w] and ((k1[w] - 1) & ~3) + 4 <= nnz  # not empty, its last quad inside the arrays
        if not fast:
            scalar += 1
        if fast and tl.min() == longest:
            uniform += 1
        else:
            row_ptr_bytes += 4 * (int(nr[w]) + 1)
        # greedy: the next row would not have fitted
        nxt = r0[w] + nr[w]
        if nxt < rows and not (nr[w] == TILE_ROWS or p[nxt + 1] - (k0[w] & ~3) > TILE):
            l2 = 0
            while l2 < 6 and (16 << l2) < max(longest, int(lens[nxt])):
                l2 += 1
            assert not exact and l2 > 0 and ((int(nr[w]) + 1) << l2) > 64, (w, "the tile ends early")
    assert info["uniform_tiles"] == uniform and info["scalar_tiles"] == scalar
    assert info["device_bytes"] == 16 * (info["tiles"] + 1)
    assert info["workgroups"] == -(-info["tiles"] // 4)
    assert info["streamed_bytes"] == 8 * nnz + row_ptr_bytes + 16 * rows + 8 * cols + 16 * (info["tiles"] + 1)


@pytest.mark.parametrize("flags", [0, capi.FLAG_EXACT_ORDER])
@pytest.mark.parametrize("name", sorted(MATRICES))
def test_preview_against_a_recount(name, flags):
    rows, cols, p = MATRICES[name]
    info, tab = capi.f32_plan_preview(rows, cols, p, flags)
    _recount_plan(rows, cols, p, flags, info, tab)
    assert capi.f32_plan_preview(rows, cols, p, flags, table=False)[0] == info


def test_what_the_preview_says_about_known_shapes():
    rows, cols, p = MATRICES["uniform_4"]
    info, tab = capi.f32_plan_preview(rows, cols, p)
    assert info["uniform_tiles"] == info["tiles"] and info["scalar_tiles"] == 0 and np.all(tab[:-1, 2] == 64)
    assert info["streamed_bytes"] == 8 * 20000 + 16 * rows + 8 * cols + 16 * (info["tiles"] + 1)  # row_ptr is not read at all
    rows, cols, p = MATRICES["one_dense_row"]
    info, tab = capi.f32_plan_preview(rows, cols, p)
    assert info["long_row_tiles"] == 1 and info["longest_row"] == 20000
    w = int(np.nonzero(tab[:, 0] == 1717)[0][0])
    assert tab[w].tolist() == [1717, int(p[1717]), 1, 6]
    rows, cols, p = MATRICES["lengths_0_to_7"]
    info, tab = capi.f32_plan_preview(rows, cols, p)
    assert np.any(tab[:, 1] % 4 != 0)  # tiles that start inside a quad
