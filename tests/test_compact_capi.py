"""The C ABI of the compact multiply (include/spmv_hip_compact.h) without a GPU: the symbols are exported and bound, the header is
plain C99 on its own, arguments are validated before any device is touched, the tile table is spmv_hip_f32_plan_preview's, and
the encoding -- greedy window bases, the compact / wide decision, the codes, every number of plan_info -- is recounted in numpy
(compact_cases.recount)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import compact_cases as cc
from spmv_amd import capi

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spmv_hip_compact.h")
NEW = ["spmv_hip_c16_plan_preview", "spmv_hip_c16_plan_csr", "spmv_hip_csr_spmv_c16", "spmv_hip_c16_plan_verify", "spmv_hip_c16_plan_info",
       "spmv_hip_c16_plan_destroy", "spmv_hip_upload_csr_compact"]


def test_symbols_exported_declared_and_bound():
    lib = C.CDLL(capi.LIB_PATH)
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(spmv_hip_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(NEW)
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in capi.SIGNATURES, s
    assert HEADER in [os.path.abspath(h) for h in capi.HEADER_PATHS]
    assert hasattr(capi.Context, "upload_csr_compact") and hasattr(capi, "C16Plan") and hasattr(capi, "c16_plan_preview")


def test_header_is_c99_on_its_own_and_keeps_the_small_one_small():
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.dirname(HEADER), "-fsyntax-only", "-x", "c", "-"],
                       input='#include "spmv_hip_compact.h"\nint main(void) { return SPMV_HIP_C16_INFO + SPMV_HIP_C16_WINDOWS + SPMV_HIP_C16_WINDOW_SPAN + SPMV_HIP_C16_TILE_INTS; }\n',
                       text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout
    defines = dict(re.findall(r"#define (SPMV_HIP_[A-Z0-9_]+) (\d+)", open(HEADER).read()))
    assert int(defines["SPMV_HIP_C16_INFO"]) == len(capi.C16_INFO_KEYS) == 20
    assert int(defines["SPMV_HIP_C16_WINDOWS"]) == capi.C16_WINDOWS == cc.WINDOWS == 8
    assert int(defines["SPMV_HIP_C16_WINDOW_SPAN"]) == capi.C16_WINDOW_SPAN == cc.SPAN == 8192
    assert int(defines["SPMV_HIP_C16_TILE_INTS"]) == capi.C16_TILE_INTS == 13
    small = re.sub(r"/\*.*?\*/", "", open(capi.HEADER_PATH).read(), flags=re.S)
    assert "c16" not in small and "compact" not in small


def test_argument_validation_needs_no_device():
    lib = capi.load()
    p = np.array([0, 1, 2, 3], dtype=np.int32)
    c = np.array([0, 3, 2], dtype=np.int32)
    v = np.ones(3)
    h = C.c_void_p()
    n = C.c_int64(-5)
    out = np.zeros(20, dtype=np.int64)
    tab = np.zeros(64, dtype=np.int32)
    P, Cc, V, O, T = p.ctypes.data, c.ctypes.data, v.ctypes.data, out.ctypes.data, tab.ctypes.data
    assert lib.spmv_hip_upload_csr_compact(None, 3, 4, 3, P, Cc, V, 1) == capi.ERR_INVALID
    assert lib.spmv_hip_c16_plan_csr(None, 3, 4, P, Cc, 0, None) == capi.ERR_INVALID
    assert lib.spmv_hip_csr_spmv_c16(None, None, None, None, None, None, None) == capi.ERR_INVALID
    assert lib.spmv_hip_c16_plan_info(None, out, 20) == capi.ERR_INVALID
    assert lib.spmv_hip_c16_plan_verify(None, Cc, C.byref(n), None) == capi.ERR_INVALID
    lib.spmv_hip_c16_plan_destroy(None)  # a no-op
    assert lib.spmv_hip_c16_plan_preview(3, 4, P, Cc, 0, None, 20, None, 0, None) == capi.ERR_INVALID
    assert lib.spmv_hip_c16_plan_preview(3, 4, None, Cc, 0, O, 20, None, 0, None) == capi.ERR_INVALID
    bad = np.array([0, 2, 1, 3], dtype=np.int32)  # decreasing
    nonzero_start = np.array([1, 1, 2, 3], dtype=np.int32)
    high = np.array([0, 4, 2], dtype=np.int32)
    negative = np.array([0, -1, 2], dtype=np.int32)
    for rows, cols, rp, col, flags, text in [(-1, 4, P, Cc, 0, b"rows < 0"), (3, -1, P, Cc, 0, b"cols < 0"), (3, 4, bad.ctypes.data, Cc, 0, b"non-decreasing"),
                                             (3, 4, nonzero_start.ctypes.data, Cc, 0, b"row_ptr[0]"), (3, 4, P, Cc, 0x1, b"flag"),
                                             (3, 4, P, Cc, capi.FLAG_EXACT_ORDER | 0x80, b"flag"), (3, 4, P, Cc, 0x80000000, b"flag"),
                                             (3, 4, P, None, 0, b"host_column_index is null"), (3, 4, P, high.ctypes.data, 0, b"out of range"),
                                             (3, 4, P, negative.ctypes.data, 0, b"out of range"), (3, 3, P, Cc, 0, b"out of range")]:
        assert lib.spmv_hip_c16_plan_preview(rows, cols, rp, col, flags, O, 20, None, 0, None) == capi.ERR_INVALID
        assert text in lib.spmv_hip_last_error(), (text, lib.spmv_hip_last_error())
        assert lib.spmv_hip_c16_plan_csr(C.byref(h), rows, cols, rp, col, flags, None) == capi.ERR_INVALID
        assert text in lib.spmv_hip_last_error(), (text, lib.spmv_hip_last_error())
        assert not h.value
    # a tile table with too little room
    assert lib.spmv_hip_c16_plan_preview(3, 4, P, Cc, 0, O, 20, T, 12, None) == capi.ERR_INVALID
    assert lib.spmv_hip_c16_plan_preview(3, 4, P, Cc, 0, O, 20, T, -1, None) == capi.ERR_INVALID
    assert lib.spmv_hip_c16_plan_preview(3, 4, P, Cc, 0, O, -1, None, 0, None) == capi.ERR_INVALID
    assert lib.spmv_hip_c16_plan_preview(3, 4, P, Cc, 0, O, 20, T, 64, None) == capi.OK
    assert lib.spmv_hip_c16_plan_preview(3, 4, P, Cc, capi.FLAG_EXACT_ORDER, O, 20, T, 64, None) == capi.OK
    # no entries: the columns may be null
    assert lib.spmv_hip_c16_plan_preview(3, 4, np.zeros(4, dtype=np.int32).ctypes.data, None, 0, O, 20, None, 0, None) == capi.OK


def test_no_gpu_means_failure_not_fallback():
    if capi.device_count() > 0:
        pytest.skip("a GPU is present; this test covers the no-device behaviour")
    p = np.array([0, 1, 2, 3], dtype=np.int32)
    with pytest.raises(capi.SpmvHipError) as e:
        capi.C16Plan(3, 4, p, np.array([0, 3, 2], dtype=np.int32))
    assert e.value.code == capi.ERR_NO_DEVICE


@pytest.mark.parametrize("flags", [0, capi.FLAG_EXACT_ORDER])
@pytest.mark.parametrize("name", cc.NAMES)
def test_preview_against_a_recount(name, flags):
    rows, cols, p, c, _ = cc.matrix(name)
    info, tab, codes = capi.c16_plan_preview(rows, cols, p, c, flags, codes=True)
    # tile for tile the table of the fp32-value plan
    finfo, ftab = capi.f32_plan_preview(rows, cols, p, flags)
    assert np.array_equal(tab[:, :4], ftab)
    assert info["tiles"] == finfo["tiles"] and info["long_row_tiles"] == finfo["long_row_tiles"] and info["workgroups"] == finfo["workgroups"]
    cc.recount(rows, cols, p, c, flags, info, tab, codes)
    assert capi.c16_plan_preview(rows, cols, p, c, flags, table=False)[0] == info
    # 6 against 8 bytes per entry, 32 bytes of bases per tile: what the two plans stream differs by exactly that
    if info["tiles"]:
        assert info["streamed_bytes"] == finfo["streamed_bytes"] - 2 * info["compact_entries"] + 32 * info["tiles"]


def test_eight_windows_are_compact_and_nine_are_wide():
    rows, cols, p, c, _ = cc.matrix("eight_windows")
    info, tab, codes = capi.c16_plan_preview(rows, cols, p, c, codes=True)
    assert info["tiles"] == 1 and info["compact_tiles"] == 1 and info["wide_tiles"] == 0 and info["tiles_with_8_windows"] == 1
    assert tab[0, 4] == 8 and tab[0, 5:].tolist() == [w * (cc.SPAN + 5) for w in range(8)]
    assert int(codes.max()) >> 13 == 7
    rows, cols, p, c, _ = cc.matrix("nine_windows")
    info, tab, codes = capi.c16_plan_preview(rows, cols, p, c, codes=True)
    assert info["tiles"] == 1 and info["compact_tiles"] == 0 and info["wide_tiles"] == 1 and info["compact_entries"] == 0
    assert tab[0, 4] == 0 and not np.any(tab[0, 5:]) and not np.any(codes)
    assert info["streamed_bytes"] == capi.f32_plan_preview(rows, cols, p)[0]["streamed_bytes"] + 32


def test_a_window_ends_exactly_8192_columns_after_its_base():
    # columns b and b + 8191 share a window; b + 8192 opens the next one
    for last, want in ((cc.SPAN - 1, 1), (cc.SPAN, 2)):
        rows, cols, p, c, _ = cc.from_rows([[5, 5 + last]], 5 + last + 1)
        info, tab, codes = capi.c16_plan_preview(rows, cols, p, c, codes=True)
        assert tab[0, 4] == want and codes.tolist() == ([0, 8191] if want == 1 else [0, 1 << 13])
        assert tab[0, 5:].tolist() == ([5] * 8 if want == 1 else [5] + [5 + cc.SPAN] * 7)


def test_columns_at_the_last_column_and_at_multiples_of_8192_round_trip():
    rows, cols, p, c, _ = cc.matrix("edge_columns")
    assert cols - 1 in c and all(m in c for m in range(0, cols, cc.SPAN)) and cols % cc.SPAN == 1
    info, tab, codes = capi.c16_plan_preview(rows, cols, p, c, codes=True)
    assert info["wide_tiles"] == 0 and info["compact_entries"] == len(c)
    bases = np.repeat(tab[:, 5:].astype(np.int64), np.diff(np.append(tab[:, 1], len(c))), axis=0)  # the bases of every entry's tile
    col = bases[np.arange(len(c)), codes >> 13] + (codes & 0x1FFF)
    assert np.array_equal(col, c) and col.max() == cols - 1


def test_unsorted_columns_within_a_row_are_coded_by_value():
    rng = np.random.default_rng(3)
    rows_of = [rng.permutation(np.arange(0, 40000, 97))[:30] for _ in range(50)] + [rng.permutation(30000)[:2000]]
    rows, cols, p, c, _ = cc.from_rows(rows_of, 40000)
    assert np.any(np.diff(c[:30]) < 0)
    info, tab, codes = capi.c16_plan_preview(rows, cols, p, c, codes=True)
    assert info["long_row_tiles"] == 1
    cc.recount(rows, cols, p, c, 0, info, tab, codes)


def test_what_the_preview_says_about_known_shapes():
    rows, cols, p, c, _ = cc.matrix("poisson_512")
    info = capi.c16_plan_preview(rows, cols, p, c, table=False)[0]
    assert info["wide_tiles"] == 0 and info["tiles_with_1_windows"] == info["tiles"]  # a 2-D stencil: one window everywhere
    rows, cols, p, c, _ = cc.matrix("powerlaw_graph")
    info = capi.c16_plan_preview(rows, cols, p, c, table=False)[0]
    assert info["wide_tiles"] > 0.9 * info["tiles"]  # a graph stays on 32-bit columns
    rows, cols, p, c, _ = cc.matrix("dense_row_9000_compact")
    info, tab, _ = capi.c16_plan_preview(rows, cols, p, c)
    w = int(np.nonzero(tab[:, 0] == 1717)[0][0])
    assert info["long_row_tiles"] == 1 and tab[w, 2] == 1 and tab[w, 3] == 6 and tab[w, 4] == 3
    rows, cols, p, c, _ = cc.matrix("dense_row_9000_wide")
    info, tab, _ = capi.c16_plan_preview(rows, cols, p, c)
    w = int(np.nonzero(tab[:, 0] == 1717)[0][0])
    assert info["long_row_tiles"] == 1 and tab[w, 4] == 0
    rows, cols, p, c, _ = cc.matrix("mixed_mesh_and_graph")
    info = capi.c16_plan_preview(rows, cols, p, c, table=False)[0]
    assert info["compact_tiles"] > 100 and info["wide_tiles"] > 100
