"""ctypes binding of include/spmv_hip.h, spmv_hip_tuning.h, spmv_hip_plan.h, spmv_hip_symmetric.h, spmv_hip_multivec.h,
spmv_hip_transpose.h, spmv_hip_f32values.h, spmv_hip_compact.h, spmv_hip_compact_f64.h, spmv_hip_compact_f32xy.h,
spmv_hip_scaled.h, spmv_hip_dots.h, spmv_hip_krylov.h, spmv_hip_bicgstab.h, spmv_hip_gmres.h, spmv_hip_bjacobi.h,
spmv_hip_cheby.h, spmv_hip_mcgs.h, spmv_hip_agg.h, spmv_hip_agg_mis2.h, spmv_hip_coarse.h and spmv_hip_compact_device.h (the C ABI
of libspmv_hip.so).

This is plumbing: it loads the in-tree shared library and turns negative return
codes into ``SpmvHipError``.  There is deliberately no fallback of any kind: if
the library is missing or a call fails, an exception is raised.
"""
import ctypes as C
import os

import numpy as np

PKG_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LIB_PATH = os.path.join(PKG_ROOT, "libspmv_hip.so")
# tools/ only: SPMV_HIP_EXPERIMENTS=1 loads the build with the timing experiments compiled in
EXPERIMENTS_LIB_PATH = os.path.join(PKG_ROOT, "libspmv_hip_experiments.so")
if os.environ.get("SPMV_HIP_EXPERIMENTS") == "1":
    LIB_PATH = EXPERIMENTS_LIB_PATH
elif os.environ.get("SPMV_HIP_EXPERIMENTS", "").endswith(".so"):  # an ablation build of tools/ablate.sh
    LIB_PATH = os.path.abspath(os.environ["SPMV_HIP_EXPERIMENTS"])
# the drop-in boundary (what an adapter of the reference binds) and the headers that include it (tuning switches; Level 2;
# the symmetric multiply of a stored triangle; Y += A X for several vectors; y += A' x; values stored as floats; ... with 16-bit column codes)
HEADER_PATH = os.path.join(os.path.dirname(PKG_ROOT), "include", "spmv_hip.h")
HEADER_PATHS = [HEADER_PATH] + [os.path.join(os.path.dirname(PKG_ROOT), "include", n)
                                for n in ("spmv_hip_tuning.h", "spmv_hip_plan.h", "spmv_hip_symmetric.h", "spmv_hip_multivec.h",
                                          "spmv_hip_transpose.h", "spmv_hip_f32values.h", "spmv_hip_compact.h",
                                          "spmv_hip_compact_f64.h", "spmv_hip_compact_f32xy.h", "spmv_hip_scaled.h", "spmv_hip_dots.h",
                                          "spmv_hip_krylov.h", "spmv_hip_bicgstab.h", "spmv_hip_gmres.h", "spmv_hip_bjacobi.h",
                                          "spmv_hip_cheby.h", "spmv_hip_mcgs.h", "spmv_hip_agg.h", "spmv_hip_agg_mis2.h",
                                          "spmv_hip_coarse.h", "spmv_hip_compact_device.h")]

OK = 0
ERR_INVALID, ERR_NO_DEVICE, ERR_HIP, ERR_ALLOC, ERR_STATE, ERR_OVERFLOW, ERR_ALIGN = -1, -2, -3, -4, -5, -6, -7
CSR_AUTO, CSR_SCALAR, CSR_VECTOR, CSR_ADAPTIVE, CSR_WAVETILE = 0, 1, 2, 3, 4
FLAG_XCD_REMAP, FLAG_EXACT_ORDER, FLAG_BIG_TILE, FLAG_NO_INDEX_COMPRESSION, FLAG_COO_KEEP_ORDER, FLAG_READ_ROW_PTR, FLAG_ROWS64, FLAG_ROWS128, FLAG_ELL_COLUMN_MAJOR = 0x1, 0x2, 0x8, 0x10, 0x20, 0x40, 0x80, 0x100, 0x200
FLAG_NO_SHIFTED_TILES = 0x400
FLAG_PIPELINE_GATHER = 0x4  # create_multi: gather k on a second stream beside multiply k + 1 (two alternating copies of y)
FLAG_NO_X_WINDOW = 0x800
FLAG_NO_COLUMN_PANELS = 0x1000
FLAG_VERIFY_PLAN = 0x8000
FLAG_NO_BALANCED_TILES = 0x40000
FLAG_NO_RUN_EVENTS = 0x80000
FLAG_NO_VALUE_INDEX = 0x100000
FLAG_PEER_GATHER = 0x200000
FLAG_BALANCE_ENTRIES = 0x400000
FLAG_NO_SEGMENT_WINDOW = 0x800000
FLAG_FUSED_PEER_STORE = 0x1000000
FLAG_NO_BLOCK_TILES = 0x2000000
FLAG_HUB_COLUMNS = 0x4000000  # libspmv_hip_experiments.so only (retired from the product: csrc/internal.hpp)
FLAG_NO_MULTI_WINDOW = 0x8000000
FLAG_NO_MASKED_BLOCKS = 0x20000000
FLAG_NO_STENCIL_RUNS = 0x80000000  # no stencil row runs (csr_runs.hpp): every tile in the default kernel's launch
FLAG_ROW_GROUPS = 0x10000000  # libspmv_hip_experiments.so only (retired from the product: csrc/internal.hpp)
CSR_ALGORITHM_NAMES = {1: "scalar", 2: "vector", 3: "adaptive", 4: "wavetile"}
# spmv_hip_symmetric.h
SYMMETRIC, SKEW_SYMMETRIC = 1, 2
TRIANGLE_MIXED, TRIANGLE_LOWER, TRIANGLE_UPPER, TRIANGLE_DIAGONAL = 0, 1, 2, 3
TRIANGLE_NAMES = {0: "mixed", 1: "lower", 2: "upper", 3: "diagonal"}
# spmv_hip_multivec.h
MV_MAX_VECTORS = 16
# spmv_hip_transpose.h
TR_MAX_WINDOWS = 8

_i32p = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
_f64p = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
_i64p = np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")
_vp = C.c_void_p

# name -> (restype, argtypes); every symbol include/spmv_hip*.h declare
SIGNATURES = {
    "spmv_hip_version": (C.c_int, []),
    "spmv_hip_strerror": (C.c_char_p, [C.c_int]),
    "spmv_hip_last_error": (C.c_char_p, []),
    "spmv_hip_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "spmv_hip_create": (C.c_int, [C.POINTER(_vp), C.c_int, C.c_uint]),
    "spmv_hip_create_multi": (C.c_int, [C.POINTER(_vp), C.c_int, C.c_uint]),
    "spmv_hip_destroy": (None, [_vp]),
    "spmv_hip_set_stream": (C.c_int, [_vp, _vp, C.c_int]),
    "spmv_hip_set_csr_algorithm": (C.c_int, [_vp, C.c_int, C.c_int]),
    "spmv_hip_upload_csr": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int32, _i32p, _i32p, _f64p]),
    "spmv_hip_upload_coo": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int32, _i32p, _i32p, _f64p]),
    "spmv_hip_upload_ell": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int32, _i32p, _f64p]),
    "spmv_hip_upload_hybrid": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int32, _i32p, _f64p, C.c_int32, _i32p, _i32p, _f64p]),
    "spmv_hip_set_x": (C.c_int, [_vp, _f64p]),
    "spmv_hip_set_y": (C.c_int, [_vp, _f64p]),
    "spmv_hip_get_y": (C.c_int, [_vp, _f64p]),
    "spmv_hip_run": (C.c_int, [_vp]),
    "spmv_hip_sync": (C.c_int, [_vp]),
    "spmv_hip_flush_caches": (C.c_int, [_vp]),
    "spmv_hip_last_run_ns": (C.c_int, [_vp, C.POINTER(C.c_uint64)]),
    "spmv_hip_last_run_times": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "spmv_hip_ctx_info": (C.c_int, [_vp, _i64p, C.c_int]),
    "spmv_hip_plan_csr": (C.c_int, [C.POINTER(_vp), C.c_int32, C.c_int32, _i32p, C.c_int, C.c_int, C.c_uint]),
    "spmv_hip_plan_csr_compress": (C.c_int, [_vp, _vp, _vp]),
    "spmv_hip_plan_verify": (C.c_int, [_vp, _vp, _vp]),
    "spmv_hip_plan_csr_repack": (C.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "spmv_hip_plan_csr_refresh_values": (C.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "spmv_hip_plan_csr_index_values": (C.c_int, [_vp, _vp, _vp]),
    "spmv_hip_plan_destroy": (None, [_vp]),
    "spmv_hip_plan_info": (C.c_int, [_vp, _i64p, C.c_int]),
    "spmv_hip_plan_csr_confirm_blocks": (C.c_int, [_vp, _vp, _vp, C.c_void_p, _vp]),
    "spmv_hip_csr_spmv": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "spmv_hip_csr_spmv_out": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "spmv_hip_csr_spmv_out_peers": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(_vp), C.c_int, C.POINTER(C.c_int), _vp]),
    "spmv_hip_partition_rows": (C.c_int, [C.c_int32, C.c_int, _vp, C.c_int, _vp]),
    "spmv_hip_ipc_alloc": (C.c_int, [C.POINTER(_vp), C.c_size_t, C.c_char_p]),
    "spmv_hip_ipc_open": (C.c_int, [C.c_char_p, C.POINTER(_vp)]),
    "spmv_hip_ipc_close": (C.c_int, [_vp]),
    "spmv_hip_ipc_free": (C.c_int, [_vp]),
    "spmv_hip_peer_push": (C.c_int, [_vp, C.POINTER(_vp), C.c_int, C.c_int64, _vp]),
    "spmv_hip_coo_spmv": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "spmv_hip_coo_sort_by_row": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, _vp]),
    "spmv_hip_ell_to_column_major": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp]),
    "spmv_hip_ell_spmv": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp]),
    "spmv_hip_triad": (C.c_int, [C.c_int64, _vp, _vp, _vp, C.c_double, _vp]),
    "spmv_hip_csr_triangle": (C.c_int, [C.c_int32, _vp, _vp, C.POINTER(C.c_int), C.POINTER(C.c_int64)]),
    "spmv_hip_upload_csr_symmetric": (C.c_int, [_vp, C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_int]),
    "spmv_hip_sym_plan_csr": (C.c_int, [C.POINTER(_vp), C.c_int32, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp]),
    "spmv_hip_csr_symv": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "spmv_hip_sym_plan_info": (C.c_int, [_vp, _i64p, C.c_int]),
    "spmv_hip_sym_plan_destroy": (None, [_vp]),
    "spmv_hip_mv_plan_csr": (C.c_int, [C.POINTER(_vp), C.c_int32, C.c_int32, _vp, C.c_int, C.c_uint, _vp]),
    "spmv_hip_csr_spmm": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int64, _vp, C.c_int64, _vp]),
    "spmv_hip_mv_plan_info": (C.c_int, [_vp, _i64p, C.c_int]),
    "spmv_hip_mv_plan_destroy": (None, [_vp]),
    "spmv_hip_set_block_x": (C.c_int, [_vp, C.c_int, _vp]),
    "spmv_hip_set_block_y": (C.c_int, [_vp, C.c_int, _vp]),
    "spmv_hip_get_block_y": (C.c_int, [_vp, C.c_int, _vp]),
    "spmv_hip_run_block": (C.c_int, [_vp]),
    "spmv_hip_upload_csr_transposed": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp]),
    "spmv_hip_tr_plan_preview": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, C.c_int, C.c_int, _vp, C.c_int, _vp, C.c_int64]),
    "spmv_hip_tr_plan_csr": (C.c_int, [C.POINTER(_vp), C.c_int32, C.c_int32, _vp, _vp, C.c_int, C.c_int, _vp]),
    "spmv_hip_csr_spmv_t": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "spmv_hip_tr_plan_info": (C.c_int, [_vp, _i64p, C.c_int]),
    "spmv_hip_tr_plan_destroy": (None, [_vp]),
    "spmv_hip_narrow_values_host": (C.c_int, [C.c_int64, _vp, _vp, C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    "spmv_hip_f32_plan_preview": (C.c_int, [C.c_int32, C.c_int32, _vp, C.c_uint, _vp, C.c_int, _vp, C.c_int64]),
    "spmv_hip_narrow_values": (C.c_int, [C.c_int64, _vp, _vp, C.POINTER(C.c_int64), C.POINTER(C.c_double), _vp]),
    "spmv_hip_f32_plan_csr": (C.c_int, [C.POINTER(_vp), C.c_int32, C.c_int32, _vp, C.c_uint, _vp]),
    "spmv_hip_csr_spmv_f32": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "spmv_hip_f32_plan_info": (C.c_int, [_vp, _i64p, C.c_int]),
    "spmv_hip_f32_plan_destroy": (None, [_vp]),
    "spmv_hip_upload_csr_f32values": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_int]),
    "spmv_hip_c16_plan_preview": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, C.c_uint, _vp, C.c_int, _vp, C.c_int64, _vp]),
    "spmv_hip_c16_plan_csr": (C.c_int, [C.POINTER(_vp), C.c_int32, C.c_int32, _vp, _vp, C.c_uint, _vp]),
    "spmv_hip_csr_spmv_c16": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "spmv_hip_csr_spmv_c16_f64": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "spmv_hip_c16_plan_verify": (C.c_int, [_vp, _vp, C.POINTER(C.c_int64), _vp]),
    "spmv_hip_c16_plan_info": (C.c_int, [_vp, _i64p, C.c_int]),
    "spmv_hip_c16_plan_destroy": (None, [_vp]),
    "spmv_hip_c16_plan_csr_device": (C.c_int, [C.POINTER(_vp), C.c_int32, C.c_int32, _vp, _vp, C.c_uint, _vp]),
    "spmv_hip_c16_plan_table": (C.c_int, [_vp, _vp, C.c_int64, _vp, C.c_int64, _vp]),
    "spmv_hip_upload_csr_compact": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_int]),
    "spmv_hip_upload_csr_compact_f64": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp]),
    "spmv_hip_csr_spmv_c16_f32xy": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "spmv_hip_upload_csr_compact_f32xy": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_int]),
    "spmv_hip_set_x_f32": (C.c_int, [_vp, _vp]),
    "spmv_hip_set_y_f32": (C.c_int, [_vp, _vp]),
    "spmv_hip_get_y_f32": (C.c_int, [_vp, _vp]),
    "spmv_hip_csr_spmv_f32_scaled": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_double, C.c_double, _vp, _vp, _vp]),
    "spmv_hip_csr_spmv_c16_scaled": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_double, C.c_double, _vp, _vp, _vp]),
    "spmv_hip_csr_spmv_c16_f64_scaled": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_double, C.c_double, _vp, _vp, _vp]),
    "spmv_hip_csr_spmv_c16_f32xy_scaled": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_double, C.c_double, _vp, _vp, _vp]),
    "spmv_hip_run_scaled": (C.c_int, [_vp, C.c_double, C.c_double]),
    "spmv_hip_f32_dots_workspace": (C.c_int, [_vp, C.POINTER(C.c_size_t)]),
    "spmv_hip_c16_dots_workspace": (C.c_int, [_vp, C.POINTER(C.c_size_t)]),
    "spmv_hip_csr_spmv_f32_scaled_dots": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_double, C.c_double, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "spmv_hip_csr_spmv_c16_scaled_dots": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_double, C.c_double, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "spmv_hip_csr_spmv_c16_f64_scaled_dots": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_double, C.c_double, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "spmv_hip_csr_spmv_c16_f32xy_scaled_dots": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_double, C.c_double, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "spmv_hip_run_scaled_dots": (C.c_int, [_vp, C.c_double, C.c_double]),
    "spmv_hip_get_dots": (C.c_int, [_vp, _vp]),
    # spmv_hip_krylov.h
    "spmv_hip_krylov_workspace": (C.c_int, [C.c_int32, C.POINTER(C.c_size_t)]),
    "spmv_hip_cg_step_f64": (C.c_int, [C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "spmv_hip_cg_step_f32": (C.c_int, [C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "spmv_hip_cg_direction_f64": (C.c_int, [C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "spmv_hip_cg_direction_f32": (C.c_int, [C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp]),
    # spmv_hip_bicgstab.h
    "spmv_hip_bicgstab_s_f64": (C.c_int, [C.c_int32] + [_vp] * 7),
    "spmv_hip_bicgstab_s_f32": (C.c_int, [C.c_int32] + [_vp] * 7),
    "spmv_hip_bicgstab_step_f64": (C.c_int, [C.c_int32] + [_vp] * 12 + [C.c_size_t, _vp]),
    "spmv_hip_bicgstab_step_f32": (C.c_int, [C.c_int32] + [_vp] * 12 + [C.c_size_t, _vp]),
    "spmv_hip_bicgstab_direction_f64": (C.c_int, [C.c_int32] + [_vp] * 12),
    "spmv_hip_bicgstab_direction_f32": (C.c_int, [C.c_int32] + [_vp] * 12),
    # spmv_hip_gmres.h
    "spmv_hip_gmres_workspace": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_size_t)]),
    "spmv_hip_gmres_state_doubles": (C.c_int, [C.c_int32]),
    "spmv_hip_gmres_project_f64": (C.c_int, [C.c_int32, C.c_int32, _vp, C.c_int64, _vp, _vp, _vp, C.c_size_t, _vp]),
    "spmv_hip_gmres_project_f32": (C.c_int, [C.c_int32, C.c_int32, _vp, C.c_int64, _vp, _vp, _vp, C.c_size_t, _vp]),
    "spmv_hip_gmres_update_f64": (C.c_int, [C.c_int32, C.c_int32, _vp, C.c_int64, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "spmv_hip_gmres_update_f32": (C.c_int, [C.c_int32, C.c_int32, _vp, C.c_int64, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "spmv_hip_gmres_scale_f64": (C.c_int, [C.c_int32] + [_vp] * 5),
    "spmv_hip_gmres_scale_f32": (C.c_int, [C.c_int32] + [_vp] * 5),
    "spmv_hip_gmres_correct_f64": (C.c_int, [C.c_int32, C.c_int32, _vp, C.c_int64, _vp, _vp, _vp, _vp]),
    "spmv_hip_gmres_correct_f32": (C.c_int, [C.c_int32, C.c_int32, _vp, C.c_int64, _vp, _vp, _vp, _vp]),
    "spmv_hip_gmres_start": (C.c_int, [C.c_int32, _vp, _vp, _vp]),
    "spmv_hip_gmres_column": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp]),
    "spmv_hip_gmres_solve": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp]),
    # spmv_hip_bjacobi.h
    "spmv_hip_bjacobi_setup_f64": (C.c_int, [C.c_int32, C.c_int32] + [_vp] * 6),
    "spmv_hip_bjacobi_setup_f32": (C.c_int, [C.c_int32, C.c_int32] + [_vp] * 6),
    "spmv_hip_bjacobi_apply_f64": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "spmv_hip_bjacobi_apply_f32": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "spmv_hip_bjacobi_apply_add_f64": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, _vp]),
    "spmv_hip_bjacobi_apply_add_f32": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, _vp]),
    # spmv_hip_cheby.h
    "spmv_hip_cheby_bound_f64": (C.c_int, [C.c_int32] + [_vp] * 5),
    "spmv_hip_cheby_bound_f32": (C.c_int, [C.c_int32] + [_vp] * 5),
    "spmv_hip_cheby_coeffs": (C.c_int, [C.c_int32, _vp, C.c_double, C.c_double, _vp, _vp]),
    "spmv_hip_cheby_step_f64": (C.c_int, [C.c_int32, C.c_int32, C.c_int32] + [_vp] * 8 + [C.c_size_t, _vp]),
    "spmv_hip_cheby_step_f32": (C.c_int, [C.c_int32, C.c_int32, C.c_int32] + [_vp] * 8 + [C.c_size_t, _vp]),
    # spmv_hip_mcgs.h
    "spmv_hip_mcgs_workspace": (C.c_int, [C.c_int32, C.POINTER(C.c_size_t)]),
    "spmv_hip_mcgs_colour": (C.c_int, [C.c_int32, _vp, _vp, C.c_uint32, _vp, _vp, _vp, C.c_size_t, _vp]),
    "spmv_hip_mcgs_permute": (C.c_int, [C.c_int32, C.c_int32] + [_vp] * 11 + [C.c_size_t, _vp]),
    "spmv_hip_mcgs_sweep_f64": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_double, _vp, _vp, _vp, _vp]),
    "spmv_hip_mcgs_sweep_f32": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_double, _vp, _vp, _vp, _vp]),
    "spmv_hip_mcgs_apply_f64": (C.c_int, [_vp, C.c_double, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "spmv_hip_mcgs_apply_f32": (C.c_int, [_vp, C.c_double, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    # spmv_hip_agg.h
    "spmv_hip_agg_workspace": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_size_t)]),
    "spmv_hip_agg_aggregate": (C.c_int, [C.c_int32, _vp, _vp, _vp, C.c_double, C.c_uint32, _vp, _vp, _vp, C.c_size_t, _vp]),
    "spmv_hip_agg_plan": (C.c_int, [C.c_int32] + [_vp] * 6 + [C.c_size_t, _vp]),
    "spmv_hip_agg_galerkin_symbolic": (C.c_int, [_vp, C.c_int32] + [_vp] * 8 + [C.c_size_t, _vp]),
    "spmv_hip_agg_galerkin_numeric": (C.c_int, [C.c_int32, C.c_int32] + [_vp] * 5),
    "spmv_hip_agg_restrict_f64": (C.c_int, [_vp] * 4),
    "spmv_hip_agg_restrict_f32": (C.c_int, [_vp] * 4),
    "spmv_hip_agg_prolong_add_f64": (C.c_int, [_vp, C.c_double, _vp, _vp, _vp]),
    "spmv_hip_agg_prolong_add_f32": (C.c_int, [_vp, C.c_double, _vp, _vp, _vp]),
    # spmv_hip_agg_mis2.h
    "spmv_hip_agg_mis2_workspace": (C.c_int, [C.c_int32, C.POINTER(C.c_size_t)]),
    "spmv_hip_agg_aggregate_mis2": (C.c_int, [C.c_int32, _vp, _vp, _vp, C.c_double, C.c_uint32, _vp, _vp, _vp, C.c_size_t, _vp]),
    "spmv_hip_agg_restrict_group_f64": (C.c_int, [_vp, C.c_int32, _vp, _vp, _vp]),
    "spmv_hip_agg_restrict_group_f32": (C.c_int, [_vp, C.c_int32, _vp, _vp, _vp]),
    "spmv_hip_agg_group": (C.c_int32, [_vp]),
    # spmv_hip_coarse.h
    "spmv_hip_coarse_ld": (C.c_int32, [C.c_int32]),
    "spmv_hip_coarse_workspace": (C.c_int, [C.c_int32, C.POINTER(C.c_size_t)]),
    "spmv_hip_coarse_setup_f64": (C.c_int, [C.c_int32] + [_vp] * 6 + [C.c_size_t, _vp]),
    "spmv_hip_coarse_setup_f32": (C.c_int, [C.c_int32] + [_vp] * 6 + [C.c_size_t, _vp]),
    "spmv_hip_coarse_apply_f64": (C.c_int, [C.c_int32] + [_vp] * 4),
    "spmv_hip_coarse_apply_f32": (C.c_int, [C.c_int32] + [_vp] * 4),
}


class SpmvHipError(RuntimeError):
    def __init__(self, code, what, detail):
        super().__init__("%s (%d): %s" % (what, code, detail))
        self.code = code


_lib = None
hip_runtime_path = None  # which libamdhip64 the process ended up with (diagnostic)


def _share_torch_hip_runtime():
    """PyTorch-ROCm wheels bundle their own libamdhip64.so (SONAME libamdhip64.so.7) and
    ask for it by file name, so a process that first loads /opt/rocm's copy through
    libspmv_hip.so and then imports torch ends up with TWO HIP runtimes, and the second
    one sees no GPU.  Loading torch's copy first makes the dynamic loader satisfy our
    DT_NEEDED libamdhip64.so.7 with it (SONAME match), and torch later finds the same
    file already mapped.  Set SPMV_HIP_RUNTIME=system to skip this (no torch in the
    process)."""
    global hip_runtime_path
    if os.environ.get("SPMV_HIP_RUNTIME", "torch") == "system":
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
    except Exception:
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        C.CDLL(cand, mode=C.RTLD_GLOBAL)
        hip_runtime_path = cand


def load():
    """Load libspmv_hip.so (in-tree).  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(
                "%s not found: build it with `make -C %s lib` (there is no CPU fallback)"
                % (LIB_PATH, PKG_ROOT))
        _share_torch_hip_runtime()
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            if not hasattr(lib, name) and os.environ.get("SPMV_HIP_EXPERIMENTS", "").endswith(".so"):
                continue  # an A/B against an OLDER build (tools/ab_two_libs.sh): entry points added since are simply not there
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def check(rc):
    if rc != 0:
        lib = load()
        raise SpmvHipError(rc, lib.spmv_hip_strerror(rc).decode(), lib.spmv_hip_last_error().decode())


def device_count():
    n = C.c_int(0)
    check(load().spmv_hip_device_count(C.byref(n)))
    return n.value


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


_EMPTY_I32 = np.zeros(1, dtype=np.int32)
_EMPTY_F64 = np.zeros(1, dtype=np.float64)
_EMPTY_F32 = np.zeros(1, dtype=np.float32)


class Context:
    """Level-1 API: host arrays in, host arrays out (what the C++ adapters use)."""

    def __init__(self, device=0, flags=0, num_gpus=None):
        """One device (`device`), or, with num_gpus, a multi-GPU context over devices 0..num_gpus-1
        (row blocks + one in-place RCCL all-gather per run; CSR only)."""
        self.lib = load()
        h = _vp()
        if num_gpus is None:
            check(self.lib.spmv_hip_create(C.byref(h), device, flags))
        else:
            check(self.lib.spmv_hip_create_multi(C.byref(h), num_gpus, flags))
        self.h = h
        self.rows = self.cols = 0

    def close(self):
        if self.h:
            self.lib.spmv_hip_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream=None):
        """Launch on the caller's stream (a raw hipStream_t, e.g. torch's cuda_stream); None = the
        context's own stream again."""
        check(self.lib.spmv_hip_set_stream(self.h, stream or 0, 1 if stream is None else 0))

    def set_csr_algorithm(self, algorithm, lanes_per_row=0):
        check(self.lib.spmv_hip_set_csr_algorithm(self.h, algorithm, lanes_per_row))

    def upload_csr(self, rows, cols, row_ptr, col, val):
        row_ptr, col, val = _i32(row_ptr), _i32(col), _f64(val)
        nnz = int(row_ptr[rows]) if len(row_ptr) > rows else -1
        if len(col) == 0:
            col, val = _EMPTY_I32, _EMPTY_F64
        check(self.lib.spmv_hip_upload_csr(self.h, rows, cols, nnz, row_ptr, col, val))
        self.rows, self.cols = rows, cols

    def upload_coo(self, rows, cols, row_idx, col, val):
        row_idx, col, val = _i32(row_idx), _i32(col), _f64(val)
        nnz = len(val)
        if nnz == 0:
            row_idx, col, val = _EMPTY_I32, _EMPTY_I32, _EMPTY_F64
        check(self.lib.spmv_hip_upload_coo(self.h, rows, cols, nnz, row_idx, col, val))
        self.rows, self.cols = rows, cols

    def upload_ell(self, rows, cols, row_length, col, val):
        col, val = _i32(col), _f64(val)
        if len(col) == 0:
            col, val = _EMPTY_I32, _EMPTY_F64
        check(self.lib.spmv_hip_upload_ell(self.h, rows, cols, row_length, col, val))
        self.rows, self.cols = rows, cols

    def upload_hybrid(self, rows, cols, row_length, ell_col, ell_val, coo_row, coo_col, coo_val):
        ell_col, ell_val = _i32(ell_col), _f64(ell_val)
        coo_row, coo_col, coo_val = _i32(coo_row), _i32(coo_col), _f64(coo_val)
        n = len(coo_val)
        if len(ell_col) == 0:
            ell_col, ell_val = _EMPTY_I32, _EMPTY_F64
        if n == 0:
            coo_row, coo_col, coo_val = _EMPTY_I32, _EMPTY_I32, _EMPTY_F64
        check(self.lib.spmv_hip_upload_hybrid(self.h, rows, cols, row_length, ell_col, ell_val, n,
                                              coo_row, coo_col, coo_val))
        self.rows, self.cols = rows, cols

    def upload_csr_symmetric(self, rows, row_ptr, col, val, kind=SYMMETRIC):
        """The stored triangle (lower or upper, diagonal included) of a square (skew-)symmetric matrix: runs then add
        (T + T' - diag(T)) x, or (T - T') x for kind=SKEW_SYMMETRIC, to y (include/spmv_hip_symmetric.h)."""
        row_ptr, col, val = _i32(row_ptr), _i32(col), _f64(val)
        nnz = int(row_ptr[rows]) if len(row_ptr) > rows else -1
        if len(col) == 0:
            col, val = _EMPTY_I32, _EMPTY_F64
        check(self.lib.spmv_hip_upload_csr_symmetric(self.h, rows, nnz, row_ptr.ctypes.data, col.ctypes.data, val.ctypes.data, kind))
        self.rows, self.cols = rows, rows

    def upload_csr_transposed(self, rows, cols, row_ptr, col, val):
        """A (rows x cols) as it is: runs then add A' x to y; set_x takes rows entries, set_y / get_y take cols
        (include/spmv_hip_transpose.h)."""
        row_ptr, col, val = _i32(row_ptr), _i32(col), _f64(val)
        nnz = int(row_ptr[rows]) if len(row_ptr) > rows >= 0 else -1
        if len(col) == 0:
            col, val = _EMPTY_I32, _EMPTY_F64
        check(self.lib.spmv_hip_upload_csr_transposed(self.h, rows, cols, nnz, row_ptr.ctypes.data, col.ctypes.data, val.ctypes.data))
        self.rows, self.cols = cols, rows  # of the operator that runs, A'

    def upload_csr_f32values(self, rows, cols, row_ptr, col, val, allow_rounding=True):
        """A with its fp64 values narrowed to floats on the way to the device (no fp64 copy is kept): runs then add fl32(A) x
        to y, every product and sum in fp64.  allow_rounding=False refuses values that are not floats already
        (include/spmv_hip_f32values.h)."""
        row_ptr, col, val = _i32(row_ptr), _i32(col), _f64(val)
        nnz = int(row_ptr[rows]) if len(row_ptr) > rows >= 0 else -1
        if len(col) == 0:
            col, val = _EMPTY_I32, _EMPTY_F64
        check(self.lib.spmv_hip_upload_csr_f32values(self.h, rows, cols, nnz, row_ptr.ctypes.data, col.ctypes.data, val.ctypes.data,
                                                     1 if allow_rounding else 0))
        self.rows, self.cols = rows, cols

    def upload_csr_compact(self, rows, cols, row_ptr, col, val, allow_rounding=True):
        """upload_csr_f32values with the columns of a tile as 16-bit window codes in the plan (6 bytes per stored entry): no fp64
        values are kept and, where the plan has no wide tile, no 32-bit columns either (include/spmv_hip_compact.h)."""
        row_ptr, col, val = _i32(row_ptr), _i32(col), _f64(val)
        nnz = int(row_ptr[rows]) if len(row_ptr) > rows >= 0 else -1
        if len(col) == 0:
            col, val = _EMPTY_I32, _EMPTY_F64
        check(self.lib.spmv_hip_upload_csr_compact(self.h, rows, cols, nnz, row_ptr.ctypes.data, col.ctypes.data, val.ctypes.data,
                                                   1 if allow_rounding else 0))
        self.rows, self.cols = rows, cols

    def upload_csr_compact_f64(self, rows, cols, row_ptr, col, val):
        """upload_csr with the columns of a tile as 16-bit window codes in the plan and the fp64 values as they are (10 bytes per
        stored entry, nothing rounded): every run adds A x to y; no 32-bit columns are kept where the plan has no wide tile
        (include/spmv_hip_compact_f64.h)."""
        row_ptr, col, val = _i32(row_ptr), _i32(col), _f64(val)
        nnz = int(row_ptr[rows]) if len(row_ptr) > rows >= 0 else -1
        if len(col) == 0:
            col, val = _EMPTY_I32, _EMPTY_F64
        check(self.lib.spmv_hip_upload_csr_compact_f64(self.h, rows, cols, nnz, row_ptr.ctypes.data, col.ctypes.data, val.ctypes.data))
        self.rows, self.cols = rows, cols

    def upload_csr_compact_f32xy(self, rows, cols, row_ptr, col, val, allow_rounding=True):
        """upload_csr_compact with x and y as 4-byte floats on the device as well: every run is y <- fl32(y + fl32(A) x), the
        products and sums in fp64 and one rounding per row; the vectors go through set_x_f32 / set_y_f32 / get_y_f32
        (include/spmv_hip_compact_f32xy.h)."""
        row_ptr, col, val = _i32(row_ptr), _i32(col), _f64(val)
        nnz = int(row_ptr[rows]) if len(row_ptr) > rows >= 0 else -1
        if len(col) == 0:
            col, val = _EMPTY_I32, _EMPTY_F64
        check(self.lib.spmv_hip_upload_csr_compact_f32xy(self.h, rows, cols, nnz, row_ptr.ctypes.data, col.ctypes.data, val.ctypes.data,
                                                         1 if allow_rounding else 0))
        self.rows, self.cols = rows, cols

    def set_x_f32(self, x):
        """The float x of a context of upload_csr_compact_f32xy (numpy float32; any other context: ERR_STATE)."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        assert len(x) == self.cols
        check(self.lib.spmv_hip_set_x_f32(self.h, (x if len(x) else _EMPTY_F32).ctypes.data))

    def set_y_f32(self, y):
        y = np.ascontiguousarray(y, dtype=np.float32)
        assert len(y) == self.rows
        check(self.lib.spmv_hip_set_y_f32(self.h, (y if len(y) else _EMPTY_F32).ctypes.data))

    def get_y_f32(self):
        y = np.zeros(max(1, self.rows), dtype=np.float32)
        check(self.lib.spmv_hip_get_y_f32(self.h, y.ctypes.data))
        return y[:self.rows]

    def set_x(self, x):
        x = _f64(x)
        assert len(x) == self.cols
        check(self.lib.spmv_hip_set_x(self.h, x if len(x) else _EMPTY_F64))

    def set_y(self, y):
        y = _f64(y)
        assert len(y) == self.rows
        check(self.lib.spmv_hip_set_y(self.h, y if len(y) else _EMPTY_F64))

    def get_y(self):
        y = np.zeros(max(1, self.rows))
        check(self.lib.spmv_hip_get_y(self.h, y))
        return y[:self.rows]

    def run(self, runs=1, sync=True):
        for _ in range(runs):
            check(self.lib.spmv_hip_run(self.h))
        if sync:
            check(self.lib.spmv_hip_sync(self.h))

    def run_scaled(self, alpha, beta, runs=1, sync=True):
        """y <- alpha A x + beta y, in place, on a context of formats 7 to 10 (include/spmv_hip_scaled.h)."""
        for _ in range(runs):
            check(self.lib.spmv_hip_run_scaled(self.h, alpha, beta))
        if sync:
            check(self.lib.spmv_hip_sync(self.h))

    def run_scaled_dots(self, alpha, beta, runs=1, sync=True):
        """run_scaled, and the dots {y' y, x' y} of the new y on the device (include/spmv_hip_dots.h): get_dots reads them."""
        for _ in range(runs):
            check(self.lib.spmv_hip_run_scaled_dots(self.h, alpha, beta))
        if sync:
            check(self.lib.spmv_hip_sync(self.h))

    def get_dots(self):
        """The two dots of the last run_scaled_dots (waits for the stream); x' y is +0.0 where rows != cols."""
        d = np.zeros(2)
        check(self.lib.spmv_hip_get_dots(self.h, d.ctypes.data))
        return d

    def set_block_x(self, X):
        """X: (cols, k) host array, 1 <= k <= 16 (include/spmv_hip_multivec.h); a new k starts a new X / Y pair (Y zero)."""
        X = _f64(X)
        assert X.ndim == 2 and X.shape[0] == self.cols
        check(self.lib.spmv_hip_set_block_x(self.h, X.shape[1], X.ctypes.data if X.size else _EMPTY_F64.ctypes.data))

    def set_block_y(self, Y):
        Y = _f64(Y)
        assert Y.ndim == 2 and Y.shape[0] == self.rows
        check(self.lib.spmv_hip_set_block_y(self.h, Y.shape[1], Y.ctypes.data if Y.size else _EMPTY_F64.ctypes.data))

    def get_block_y(self, k):
        Y = np.zeros((max(1, self.rows), k))
        check(self.lib.spmv_hip_get_block_y(self.h, k, Y.ctypes.data))
        return Y[:self.rows]

    def run_block(self, runs=1, sync=True):
        """Y += A X with the block vectors (the matrix of upload_csr)."""
        for _ in range(runs):
            check(self.lib.spmv_hip_run_block(self.h))
        if sync:
            check(self.lib.spmv_hip_sync(self.h))

    def flush_caches(self):
        """Evict the device's L2 and Infinity Cache (the device side of --flush-caches)."""
        check(self.lib.spmv_hip_flush_caches(self.h))

    def last_run_ns(self):
        ns = C.c_uint64(0)
        check(self.lib.spmv_hip_last_run_ns(self.h, C.byref(ns)))
        return ns.value

    def last_run_times(self):
        """(kernel_ns, gather_ns) of the last run."""
        k, g = C.c_uint64(0), C.c_uint64(0)
        check(self.lib.spmv_hip_last_run_times(self.h, C.byref(k), C.byref(g)))
        return k.value, g.value

    def info(self):
        out = np.zeros(20, dtype=np.int64)
        check(self.lib.spmv_hip_ctx_info(self.h, out, 20))
        keys = ["format", "rows", "cols", "stored", "algorithm", "lanes_per_row", "workgroups",
                "row_blocks", "long_blocks", "device_bytes", "narrow_tiles", "shifted_tiles", "xwin_tiles",
                "blockwin_tiles", "panel_tiles", "streamed_bytes", "devices", "ell_path", "rccl_ranks", "pipelined"]
        return dict(zip(keys, out.tolist()))


class CsrPlan:
    """Level-2 launch plan for caller-owned device arrays (torch tensors)."""

    def __init__(self, rows, cols, host_row_ptr, algorithm=CSR_AUTO, lanes_per_row=0, flags=0):
        self.lib = load()
        h = _vp()
        check(self.lib.spmv_hip_plan_csr(C.byref(h), rows, cols, _i32(host_row_ptr), algorithm,
                                         lanes_per_row, flags))
        self.h = h

    def close(self):
        if self.h:
            self.lib.spmv_hip_plan_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        out = np.zeros(44, dtype=np.int64)
        check(self.lib.spmv_hip_plan_info(self.h, out, 44))
        keys = ["algorithm", "lanes_per_row", "workgroups", "row_blocks", "long_blocks", "rows",
                "nnz", "meta_bytes", "narrow_tiles", "uniform_tiles", "shifted_tiles", "xwin_tiles", "blockwin_tiles", "panel_tiles",
                "streamed_bytes", "shifted_entries", "narrow_entries", "uniform_rows", "value_snapshot", "balanced", "indexed_values",
                "segwin_tiles", "segwin_slots", "value_row_tiles", "dictionary_launch_tiles", "block_tiles", "block_entries", "hub_columns", "hub_entries", "multi_window_tiles", "row_group_tiles",
                "masked_block_tiles", "masked_block_entries", "stencil_mask_tiles", "stencil_mask_entries",
                "group_tiles", "group_entries", "group_rows", "run_chunks", "run_tiles", "run_entries",
                "run_masked_chunks", "run_rest_tiles", "run_variant"]
        return dict(zip(keys, out.tolist()))

    def confirm_blocks(self, d_row_ptr, d_col, host_row_ptr=None, stream=0):
        """Before compress: a candidate for (masked) block tiles gets its tiles cut on the row groups found in the columns."""
        hp = None if host_row_ptr is None else np.ascontiguousarray(host_row_ptr, dtype=np.int32)
        check(self.lib.spmv_hip_plan_csr_confirm_blocks(self.h, d_row_ptr, d_col, None if hp is None else hp.ctypes.data, stream))

    def compress(self, d_col, stream=0):
        """16-bit column offsets for the tiles that allow it (wave-tile algorithm only)."""
        check(self.lib.spmv_hip_plan_csr_compress(self.h, d_col, stream))

    def repack(self, d_row_ptr, d_col, d_val, stream=0):
        """Column panels for scattered matrices (after compress; a no-op when the matrix does not
        qualify).  The plan then owns a snapshot of the values."""
        check(self.lib.spmv_hip_plan_csr_repack(self.h, d_row_ptr, d_col, d_val, stream))

    def spmv(self, d_row_ptr, d_col, d_val, d_x, d_y, stream=0):
        """All arguments are raw device addresses (ints), e.g. tensor.data_ptr()."""
        check(self.lib.spmv_hip_csr_spmv(self.h, d_row_ptr, d_col, d_val, d_x, d_y, stream))

    def spmv_out(self, d_row_ptr, d_col, d_val, d_x, d_y_in, d_y_out, stream=0):
        """y_out = y_in + A*x (two different arrays, or the same one)."""
        check(self.lib.spmv_hip_csr_spmv_out(self.h, d_row_ptr, d_col, d_val, d_x, d_y_in, d_y_out, stream))

    def verify(self, d_col, stream=0):
        """Raises SpmvHipError (ERR_STATE) if d_col no longer has the contents the plan was compressed from."""
        check(self.lib.spmv_hip_plan_verify(self.h, d_col, stream))

    def index_values(self, d_val, stream=0):
        """Value dictionary for matrices with at most 128 distinct values (a no-op otherwise).  The caller keeps
        d_val unchanged while the plan lives, or calls refresh_values after changing it."""
        check(self.lib.spmv_hip_plan_csr_index_values(self.h, d_val, stream))

    def refresh_values(self, d_row_ptr, d_col, d_val, stream=0):
        """Re-copy the values into the plan's column-panel copy (no-op without panels)."""
        check(self.lib.spmv_hip_plan_csr_refresh_values(self.h, d_row_ptr, d_col, d_val, stream))


def csr_triangle(rows, row_ptr, col):
    """(triangle, diagonal entries) of a square CSR matrix: TRIANGLE_LOWER / _UPPER / _DIAGONAL (no off-diagonal entry) /
    _MIXED.  Host only."""
    row_ptr, col = _i32(row_ptr), _i32(col)
    if len(row_ptr) < rows + 1:
        raise ValueError("row_ptr needs rows + 1 entries")
    if len(col) == 0:
        col = _EMPTY_I32
    t, d = C.c_int(-1), C.c_int64(-1)
    check(load().spmv_hip_csr_triangle(rows, row_ptr.ctypes.data, col.ctypes.data, C.byref(t), C.byref(d)))
    return t.value, d.value


class SymPlan:
    """Level-2 plan of the symmetric multiply of a stored triangle (spmv_hip_sym_plan_*): host row_ptr, device columns.
    max_windows / window_doubles = 0: automatic (small values force spilled entries)."""

    INFO_KEYS = ["ranges", "rows_per_range", "max_windows", "windows", "lds_bytes", "spilled_entries", "atomic_bytes",
                 "stored_entries", "diagonal_entries", "triangle", "device_bytes", "kind", "rows", "streamed_bytes",
                 "window_slots", "multiplied_entries"]

    def __init__(self, rows, host_row_ptr, d_col, kind=SYMMETRIC, max_windows=0, window_doubles=0, stream=0):
        self.lib = load()
        self.h = None
        rp = _i32(host_row_ptr)
        if len(rp) < rows + 1:
            raise ValueError("host_row_ptr needs rows + 1 entries")
        h = _vp()
        check(self.lib.spmv_hip_sym_plan_csr(C.byref(h), rows, rp.ctypes.data, d_col, kind, max_windows, window_doubles, stream))
        self.h = h
        self.rows = rows

    def close(self):
        if self.h:
            self.lib.spmv_hip_sym_plan_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        out = np.zeros(len(self.INFO_KEYS), dtype=np.int64)
        check(self.lib.spmv_hip_sym_plan_info(self.h, out, len(out)))
        return dict(zip(self.INFO_KEYS, out.tolist()))

    def symv(self, d_row_ptr, d_col, d_val, d_x, d_y, stream=0):
        """y += (T + T' - diag(T)) x (or (T - T') x); raw device addresses, d_x != d_y."""
        check(self.lib.spmv_hip_csr_symv(self.h, d_row_ptr, d_col, d_val, d_x, d_y, stream))


TR_INFO_KEYS = ["ranges", "rows_per_range", "max_windows", "windows", "lds_bytes", "spilled_entries", "atomic_bytes",
                "stored_entries", "rows", "cols", "device_bytes", "streamed_bytes", "window_slots", "most_entries_in_a_range"]


def tr_plan_preview(rows, cols, row_ptr, col, max_windows=0, window_doubles=0, table=True):
    """What TrPlan would choose for these HOST arrays, without a device: (info dict, window table).  The table is an int32
    array [ranges, max_windows, 2] of {first column, length} (length 0: unused), or None with table=False."""
    lib = load()
    row_ptr, col = _i32(row_ptr), _i32(col)
    if len(row_ptr) < rows + 1:
        raise ValueError("row_ptr needs rows + 1 entries")
    if len(col) == 0:
        col = _EMPTY_I32
    out = np.zeros(len(TR_INFO_KEYS), dtype=np.int64)
    check(lib.spmv_hip_tr_plan_preview(rows, cols, row_ptr.ctypes.data, col.ctypes.data, max_windows, window_doubles,
                                       out.ctypes.data, len(out), None, 0))
    info = dict(zip(TR_INFO_KEYS, out.tolist()))
    if not table:
        return info, None
    win = np.zeros((info["ranges"], info["max_windows"], 2), dtype=np.int32)
    check(lib.spmv_hip_tr_plan_preview(rows, cols, row_ptr.ctypes.data, col.ctypes.data, max_windows, window_doubles,
                                       out.ctypes.data, len(out), win.ctypes.data if win.size else None, win.size))
    return info, win


class TrPlan:
    """Level-2 plan of the transposed multiply y += A' x (spmv_hip_tr_plan_*): host row_ptr, device columns.
    max_windows / window_doubles = 0: automatic (small values force spilled entries)."""

    INFO_KEYS = TR_INFO_KEYS

    def __init__(self, rows, cols, host_row_ptr, d_col, max_windows=0, window_doubles=0, stream=0):
        self.lib = load()
        self.h = None
        rp = _i32(host_row_ptr)
        if len(rp) < rows + 1:
            raise ValueError("host_row_ptr needs rows + 1 entries")
        h = _vp()
        check(self.lib.spmv_hip_tr_plan_csr(C.byref(h), rows, cols, rp.ctypes.data, d_col, max_windows, window_doubles, stream))
        self.h = h
        self.rows, self.cols = rows, cols

    def close(self):
        if self.h:
            self.lib.spmv_hip_tr_plan_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        out = np.zeros(len(self.INFO_KEYS), dtype=np.int64)
        check(self.lib.spmv_hip_tr_plan_info(self.h, out, len(out)))
        return dict(zip(self.INFO_KEYS, out.tolist()))

    def spmv_t(self, d_row_ptr, d_col, d_val, d_x, d_y, stream=0):
        """y += A' x; raw device addresses, d_x (rows entries) != d_y (cols entries)."""
        check(self.lib.spmv_hip_csr_spmv_t(self.h, d_row_ptr, d_col, d_val, d_x, d_y, stream))


F32_INFO_KEYS = ["rows", "cols", "stored_entries", "tiles", "long_row_tiles", "longest_row", "flags", "device_bytes",
                 "streamed_bytes", "uniform_tiles", "scalar_tiles", "workgroups"]
F32_TILE, F32_TILE_ROWS = 512, 64


def narrow_values_host(value):
    """(float32 array, inexact count, largest relative change) of spmv_hip_narrow_values_host; ERR_OVERFLOW raises."""
    value = _f64(value)
    out = np.zeros(max(1, len(value)), dtype=np.float32)
    inexact, rel = C.c_int64(-1), C.c_double(-1.0)
    check(load().spmv_hip_narrow_values_host(len(value), value.ctypes.data if len(value) else None, out.ctypes.data,
                                             C.byref(inexact), C.byref(rel)))
    return out[:len(value)], inexact.value, rel.value


def f32_plan_preview(rows, cols, row_ptr, flags=0, table=True):
    """What F32Plan would choose for this HOST row_ptr, without a device: (info dict, tile table).  The table is an int32
    array [tiles, 4] of {first row, first entry, rows, lanes_log2} in launch order, or None with table=False."""
    lib = load()
    row_ptr = _i32(row_ptr)
    if len(row_ptr) < rows + 1:
        raise ValueError("row_ptr needs rows + 1 entries")
    out = np.zeros(len(F32_INFO_KEYS), dtype=np.int64)
    check(lib.spmv_hip_f32_plan_preview(rows, cols, row_ptr.ctypes.data, flags, out.ctypes.data, len(out), None, 0))
    info = dict(zip(F32_INFO_KEYS, out.tolist()))
    if not table:
        return info, None
    tab = np.zeros((info["tiles"], 4), dtype=np.int32)
    check(lib.spmv_hip_f32_plan_preview(rows, cols, row_ptr.ctypes.data, flags, out.ctypes.data, len(out),
                                        tab.ctypes.data if tab.size else None, tab.size))
    return info, tab


class F32Plan:
    """Level-2 plan of y += fl32(A) x over the caller's FLOAT value array (spmv_hip_f32_plan_*): host row_ptr only."""

    INFO_KEYS = F32_INFO_KEYS

    def __init__(self, rows, cols, host_row_ptr, flags=0, stream=0):
        self.lib = load()
        self.h = None
        rp = _i32(host_row_ptr)
        if len(rp) < rows + 1:
            raise ValueError("host_row_ptr needs rows + 1 entries")
        h = _vp()
        check(self.lib.spmv_hip_f32_plan_csr(C.byref(h), rows, cols, rp.ctypes.data, flags, stream))
        self.h = h
        self.rows, self.cols = rows, cols

    def close(self):
        if self.h:
            self.lib.spmv_hip_f32_plan_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        out = np.zeros(len(self.INFO_KEYS), dtype=np.int64)
        check(self.lib.spmv_hip_f32_plan_info(self.h, out, len(out)))
        return dict(zip(self.INFO_KEYS, out.tolist()))

    def spmv(self, d_row_ptr, d_col, d_val32, d_x, d_y, stream=0):
        """y += fl32(A) x; raw device addresses, d_val32 a float array, d_x != d_y."""
        check(self.lib.spmv_hip_csr_spmv_f32(self.h, d_row_ptr, d_col, d_val32, d_x, d_y, stream))

    def spmv_scaled(self, d_row_ptr, d_col, d_val32, d_x, alpha, beta, d_y_in, d_y_out, stream=0):
        """y_out <- alpha fl32(A) x + beta y_in (include/spmv_hip_scaled.h); d_y_in may be 0 / None where beta == 0, the matrix
        arrays and d_x where alpha == 0; d_y_in == d_y_out is in place."""
        check(self.lib.spmv_hip_csr_spmv_f32_scaled(self.h, d_row_ptr or None, d_col or None, d_val32 or None, d_x or None, alpha, beta,
                                                    d_y_in or None, d_y_out or None, stream))

    def dots_workspace_bytes(self):
        """The workspace a spmv_scaled_dots call through this plan needs (include/spmv_hip_dots.h)."""
        n = C.c_size_t(0)
        check(self.lib.spmv_hip_f32_dots_workspace(self.h, C.byref(n)))
        return n.value

    def spmv_scaled_dots(self, d_row_ptr, d_col, d_val32, d_x, alpha, beta, d_y_in, d_y_out, d_w, d_dots, d_work, work_bytes, stream=0):
        """spmv_scaled, and d_dots <- {y_out' y_out, w' y_out} (two doubles on the device; d_w may be 0 / None: +0.0)."""
        check(self.lib.spmv_hip_csr_spmv_f32_scaled_dots(self.h, d_row_ptr or None, d_col or None, d_val32 or None, d_x or None, alpha, beta,
                                                         d_y_in or None, d_y_out or None, d_w or None, d_dots or None, d_work or None,
                                                         work_bytes, stream))


C16_INFO_KEYS = ["rows", "cols", "stored_entries", "flags", "workgroups", "tiles", "compact_tiles", "wide_tiles", "long_row_tiles",
                 "compact_entries"] + ["tiles_with_%d_windows" % w for w in range(1, 9)] + ["device_bytes", "streamed_bytes"]
C16_WINDOWS, C16_WINDOW_SPAN, C16_TILE_INTS = 8, 8192, 13


def c16_plan_preview(rows, cols, row_ptr, col, flags=0, table=True, codes=False):
    """What C16Plan would choose for these HOST arrays, without a device: (info dict, tile table, codes).  The table is an
    int32 array [tiles, 13] of {first row, first entry, rows, lanes_log2, windows (0 = wide), base[8]} in launch order (None
    with table=False); codes the uint16 code of every stored entry by entry index, 0 in wide tiles (None with codes=False)."""
    lib = load()
    row_ptr, col = _i32(row_ptr), _i32(col)
    if len(row_ptr) < rows + 1:
        raise ValueError("row_ptr needs rows + 1 entries")
    if rows >= 0 and len(col) < int(row_ptr[rows]):
        raise ValueError("col needs row_ptr[rows] entries")
    cp = col.ctypes.data if len(col) else None
    out = np.zeros(len(C16_INFO_KEYS), dtype=np.int64)
    check(lib.spmv_hip_c16_plan_preview(rows, cols, row_ptr.ctypes.data, cp, flags, out.ctypes.data, len(out), None, 0, None))
    info = dict(zip(C16_INFO_KEYS, out.tolist()))
    if not table and not codes:
        return info, None, None
    tab = np.zeros((info["tiles"], C16_TILE_INTS), dtype=np.int32)
    cod = np.zeros(info["stored_entries"], dtype=np.uint16)
    check(lib.spmv_hip_c16_plan_preview(rows, cols, row_ptr.ctypes.data, cp, flags, out.ctypes.data, len(out),
                                        tab.ctypes.data if tab.size else None, tab.size,
                                        cod.ctypes.data if codes and cod.size else None))
    return info, (tab if table else None), (cod if codes else None)


class C16Plan:
    """Level-2 plan of y += fl32(A) x with 16-bit column codes (spmv_hip_c16_plan_*): host row_ptr and columns."""

    INFO_KEYS = C16_INFO_KEYS

    def __init__(self, rows, cols, host_row_ptr, host_col, flags=0, stream=0):
        self.lib = load()
        self.h = None
        rp, col = _i32(host_row_ptr), _i32(host_col)
        if len(rp) < rows + 1:
            raise ValueError("host_row_ptr needs rows + 1 entries")
        if rows >= 0 and len(col) < int(rp[rows]):
            raise ValueError("host_col needs row_ptr[rows] entries")
        h = _vp()
        check(self.lib.spmv_hip_c16_plan_csr(C.byref(h), rows, cols, rp.ctypes.data, col.ctypes.data if len(col) else None, flags, stream))
        self.h = h
        self.rows, self.cols = rows, cols

    @classmethod
    def from_device(cls, rows, cols, d_row_ptr, d_col, flags=0, stream=0):
        """The same plan from DEVICE row_ptr and columns (spmv_hip_c16_plan_csr_device; raw addresses or torch tensors), read on
        `stream` behind whatever wrote them: the columns do not visit the host."""
        self = cls.__new__(cls)
        self.lib = load()
        self.h = None
        h = _vp()
        rp, col = ((_dev(a)[0] if a is not None else 0) or None for a in (d_row_ptr, d_col))
        check(self.lib.spmv_hip_c16_plan_csr_device(C.byref(h), rows, cols, rp, col, flags, stream))
        self.h = h
        self.rows, self.cols = rows, cols
        return self

    def table(self, codes=False, stream=0):
        """The plan read back in c16_plan_preview's format (spmv_hip_c16_plan_table): the int32 tile table [tiles, 13] and, with
        codes=True, the uint16 code of every stored entry by entry index (None otherwise)."""
        info = self.info()
        tab = np.zeros((info["tiles"], C16_TILE_INTS), dtype=np.int32)
        cod = np.zeros(info["stored_entries"], dtype=np.uint16) if codes else None
        check(self.lib.spmv_hip_c16_plan_table(self.h, tab.ctypes.data if tab.size else None, tab.size,
                                               cod.ctypes.data if codes and cod.size else None, cod.size if codes else 0, stream))
        return tab, cod

    def close(self):
        if self.h:
            self.lib.spmv_hip_c16_plan_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        out = np.zeros(len(self.INFO_KEYS), dtype=np.int64)
        check(self.lib.spmv_hip_c16_plan_info(self.h, out, len(out)))
        return dict(zip(self.INFO_KEYS, out.tolist()))

    def spmv(self, d_row_ptr, d_col, d_val32, d_x, d_y, stream=0):
        """y += fl32(A) x; raw device addresses, d_val32 a float array, d_x != d_y; d_col may be 0 / None where the plan has no
        wide tile."""
        check(self.lib.spmv_hip_csr_spmv_c16(self.h, d_row_ptr, d_col or None, d_val32, d_x, d_y, stream))

    def spmv_f64(self, d_row_ptr, d_col, d_val, d_x, d_y, stream=0):
        """y += A x through the same plan; d_val an fp64 array (16-byte aligned), otherwise as spmv."""
        check(self.lib.spmv_hip_csr_spmv_c16_f64(self.h, d_row_ptr, d_col or None, d_val, d_x, d_y, stream))

    def spmv_f32xy(self, d_row_ptr, d_col, d_val32, d_x32, d_y32, stream=0):
        """y <- fl32(y + fl32(A) x) through the same plan; d_x32 and d_y32 float arrays (4-byte aligned), otherwise as spmv."""
        check(self.lib.spmv_hip_csr_spmv_c16_f32xy(self.h, d_row_ptr, d_col or None, d_val32, d_x32, d_y32, stream))

    def spmv_scaled(self, d_row_ptr, d_col, d_val32, d_x, alpha, beta, d_y_in, d_y_out, stream=0):
        """y_out <- alpha fl32(A) x + beta y_in (include/spmv_hip_scaled.h); d_y_in may be 0 / None where beta == 0, the matrix
        arrays and d_x where alpha == 0; d_y_in == d_y_out is in place."""
        check(self.lib.spmv_hip_csr_spmv_c16_scaled(self.h, d_row_ptr or None, d_col or None, d_val32 or None, d_x or None, alpha, beta,
                                                    d_y_in or None, d_y_out or None, stream))

    def spmv_f64_scaled(self, d_row_ptr, d_col, d_val, d_x, alpha, beta, d_y_in, d_y_out, stream=0):
        """y_out <- alpha A x + beta y_in on fp64 values through the same plan, otherwise as spmv_scaled."""
        check(self.lib.spmv_hip_csr_spmv_c16_f64_scaled(self.h, d_row_ptr or None, d_col or None, d_val or None, d_x or None, alpha, beta,
                                                        d_y_in or None, d_y_out or None, stream))

    def spmv_f32xy_scaled(self, d_row_ptr, d_col, d_val32, d_x32, alpha, beta, d_y_in32, d_y_out32, stream=0):
        """y_out <- fl32(alpha fl32(A) x + beta y_in) on float vectors through the same plan, otherwise as spmv_scaled."""
        check(self.lib.spmv_hip_csr_spmv_c16_f32xy_scaled(self.h, d_row_ptr or None, d_col or None, d_val32 or None, d_x32 or None, alpha, beta,
                                                          d_y_in32 or None, d_y_out32 or None, stream))

    def dots_workspace_bytes(self):
        """The workspace a *_scaled_dots call through this plan needs (include/spmv_hip_dots.h)."""
        n = C.c_size_t(0)
        check(self.lib.spmv_hip_c16_dots_workspace(self.h, C.byref(n)))
        return n.value

    def _dots(self, fn, d_row_ptr, d_col, d_val, d_x, alpha, beta, d_y_in, d_y_out, d_w, d_dots, d_work, work_bytes, stream):
        check(fn(self.h, d_row_ptr or None, d_col or None, d_val or None, d_x or None, alpha, beta, d_y_in or None, d_y_out or None,
                 d_w or None, d_dots or None, d_work or None, work_bytes, stream))

    def spmv_scaled_dots(self, d_row_ptr, d_col, d_val32, d_x, alpha, beta, d_y_in, d_y_out, d_w, d_dots, d_work, work_bytes, stream=0):
        """spmv_scaled, and d_dots <- {y_out' y_out, w' y_out} (two doubles on the device; d_w may be 0 / None: +0.0)."""
        self._dots(self.lib.spmv_hip_csr_spmv_c16_scaled_dots, d_row_ptr, d_col, d_val32, d_x, alpha, beta, d_y_in, d_y_out, d_w, d_dots,
                   d_work, work_bytes, stream)

    def spmv_f64_scaled_dots(self, d_row_ptr, d_col, d_val, d_x, alpha, beta, d_y_in, d_y_out, d_w, d_dots, d_work, work_bytes, stream=0):
        """spmv_f64_scaled, and the dots."""
        self._dots(self.lib.spmv_hip_csr_spmv_c16_f64_scaled_dots, d_row_ptr, d_col, d_val, d_x, alpha, beta, d_y_in, d_y_out, d_w, d_dots,
                   d_work, work_bytes, stream)

    def spmv_f32xy_scaled_dots(self, d_row_ptr, d_col, d_val32, d_x32, alpha, beta, d_y_in32, d_y_out32, d_w32, d_dots, d_work, work_bytes,
                               stream=0):
        """spmv_f32xy_scaled, and the dots of the floats it stored (d_w32 a float array)."""
        self._dots(self.lib.spmv_hip_csr_spmv_c16_f32xy_scaled_dots, d_row_ptr, d_col, d_val32, d_x32, alpha, beta, d_y_in32, d_y_out32, d_w32,
                   d_dots, d_work, work_bytes, stream)

    def verify(self, d_col, stream=0):
        """How many entries of compact tiles decode to a column other than d_col's (the content guard)."""
        n = C.c_int64(-1)
        check(self.lib.spmv_hip_c16_plan_verify(self.h, d_col or None, C.byref(n), stream))
        return n.value


def c16_plan_device_times():
    """Timing hook of libspmv_hip_experiments.so (SPMV_HIP_EXPERIMENTS=1), not part of the C ABI: seconds of the stages of the
    last C16Plan.from_device -- {row_ptr copy, tile cut, windows kernel, codes kernel, the rest} -- or None in the product
    library, which does not wait between the stages."""
    lib = load()
    if not hasattr(lib, "spmv_hip_c16_plan_device_times"):
        return None
    out = (C.c_double * 5)()
    lib.spmv_hip_c16_plan_device_times.argtypes = [C.POINTER(C.c_double)]
    lib.spmv_hip_c16_plan_device_times.restype = None
    lib.spmv_hip_c16_plan_device_times(out)
    return list(out)


def narrow_values(n, d_value, d_out, stream=0):
    """(inexact count, largest relative change) of spmv_hip_narrow_values on device arrays (raw addresses)."""
    inexact, rel = C.c_int64(-1), C.c_double(-1.0)
    check(load().spmv_hip_narrow_values(n, d_value, d_out, C.byref(inexact), C.byref(rel), stream))
    return inexact.value, rel.value


def _dev(a):
    """(device address, leading dimension or None) of a torch tensor, or a raw address as it is."""
    if hasattr(a, "data_ptr"):
        if a.dim() == 2:
            assert a.stride(1) == 1, "row-major rows needed (stride 1 along the vectors)"
            return a.data_ptr(), a.stride(0)
        return a.data_ptr(), None
    return int(a), None


def krylov_workspace_bytes(n):
    """The workspace a cg_step over n elements needs (include/spmv_hip_krylov.h): a function of n alone, at least 16."""
    b = C.c_size_t(0)
    check(load().spmv_hip_krylov_workspace(n, C.byref(b)))
    return b.value


def _krylov_suffix(vectors, dtype):
    """"f64" or "f32": the dtype of the torch tensors among the vectors (one dtype), or `dtype` where all are raw addresses."""
    found = {str(v.dtype).split(".")[-1] for v in vectors if hasattr(v, "data_ptr")}
    if dtype is not None:
        found.add(np.dtype(dtype).name)
    if len(found) != 1 or not found <= {"float64", "float32"}:
        raise TypeError("the vectors are float64 or float32, all of one type (raw addresses: dtype=); got %s" % sorted(found))
    return "f64" if found == {"float64"} else "f32"


def _addr(a):
    return None if a is None else (_dev(a)[0] or None)


def cg_step(n, d_num, d_den, d_p, d_q, d_x, d_r, d_minv, d_dots, d_work, work_bytes=None, stream=0, dtype=None):
    """x += a p, r -= a q in place with a = d_num[0] / d_den[0] read on the device, and d_dots <- {r' r, r' diag(d_minv) r} of the
    new r (d_minv None: +0.0).  Torch tensors or raw device addresses; float64 or float32 vectors by their dtype (raw addresses:
    dtype=), d_num, d_den and d_dots always doubles.  work_bytes defaults to the size of a tensor d_work.  Only enqueues."""
    fn = getattr(load(), "spmv_hip_cg_step_" + _krylov_suffix((d_p, d_q, d_x, d_r, d_minv), dtype))
    if work_bytes is None:
        work_bytes = d_work.numel() * d_work.element_size()
    check(fn(n, _addr(d_num), _addr(d_den), _addr(d_p), _addr(d_q), _addr(d_x), _addr(d_r), _addr(d_minv), _addr(d_dots), _addr(d_work),
             work_bytes, stream))


def cg_direction(n, d_num, d_den, d_r, d_minv, d_p, stream=0, dtype=None):
    """p <- z + b p in place with b = d_num[0] / d_den[0] read on the device and z = diag(d_minv) r (d_minv None: z = r).
    Arguments as for cg_step.  Only enqueues."""
    fn = getattr(load(), "spmv_hip_cg_direction_" + _krylov_suffix((d_r, d_minv, d_p), dtype))
    check(fn(n, _addr(d_num), _addr(d_den), _addr(d_r), _addr(d_minv), _addr(d_p), stream))


def bicgstab_s(n, d_num, d_den, d_v, d_r, d_minv, d_shat, stream=0, dtype=None):
    """r <- s = r - a v in place with a = d_num[0] / d_den[0] read on the device; with d_minv, d_shat <- diag(d_minv) s (both None
    or both given) (include/spmv_hip_bicgstab.h).  Arguments as for cg_step.  Only enqueues."""
    fn = getattr(load(), "spmv_hip_bicgstab_s_" + _krylov_suffix((d_v, d_r, d_minv, d_shat), dtype))
    check(fn(n, _addr(d_num), _addr(d_den), _addr(d_v), _addr(d_r), _addr(d_minv), _addr(d_shat), stream))


def bicgstab_step(n, d_num_a, d_den_a, d_num_w, d_den_w, d_phat, d_shat, d_t, d_rhat, d_x, d_r, d_dots, d_work, work_bytes=None, stream=0,
                  dtype=None):
    """x += a phat + w shat, r <- r - w t in place (r holds s on entry; d_shat None: shat is that r) with a = d_num_a[0] / d_den_a[0]
    and w = d_num_w[0] / d_den_w[0] read on the device, and d_dots <- {r' r, rhat' r} of the new r.  Arguments as for cg_step, the
    workspace krylov_workspace_bytes(n).  Only enqueues."""
    fn = getattr(load(), "spmv_hip_bicgstab_step_" + _krylov_suffix((d_phat, d_shat, d_t, d_rhat, d_x, d_r), dtype))
    if work_bytes is None:
        work_bytes = d_work.numel() * d_work.element_size()
    check(fn(n, _addr(d_num_a), _addr(d_den_a), _addr(d_num_w), _addr(d_den_w), _addr(d_phat), _addr(d_shat), _addr(d_t), _addr(d_rhat),
             _addr(d_x), _addr(d_r), _addr(d_dots), _addr(d_work), work_bytes, stream))


def bicgstab_direction(n, d_num_r, d_den_r, d_num_a, d_den_a, d_num_w, d_den_w, d_r, d_v, d_p, d_minv, d_phat, stream=0, dtype=None):
    """p <- r + b (p - w v) in place with w = d_num_w[0] / d_den_w[0] and b = (d_num_r[0] / d_den_r[0]) ((d_num_a[0] / d_den_a[0]) / w)
    read on the device; with d_minv, d_phat <- diag(d_minv) p (both None or both given).  Arguments as for cg_step.  Only enqueues."""
    fn = getattr(load(), "spmv_hip_bicgstab_direction_" + _krylov_suffix((d_r, d_v, d_p, d_minv, d_phat), dtype))
    check(fn(n, _addr(d_num_r), _addr(d_den_r), _addr(d_num_a), _addr(d_den_a), _addr(d_num_w), _addr(d_den_w), _addr(d_r), _addr(d_v),
             _addr(d_p), _addr(d_minv), _addr(d_phat), stream))


GMRES_MAX_BASIS = 32


def gmres_workspace_bytes(n, k_max):
    """The workspace gmres_project and gmres_update over n elements and up to k_max vectors need (include/spmv_hip_gmres.h): a
    function of n and k_max alone, at least 16, never decreasing in either."""
    b = C.c_size_t(0)
    check(load().spmv_hip_gmres_workspace(n, k_max, C.byref(b)))
    return b.value


def gmres_state_doubles(m):
    """The doubles of the device state of a cycle of m steps (1 <= m <= GMRES_MAX_BASIS)."""
    rc = load().spmv_hip_gmres_state_doubles(m)
    if rc < 0:
        check(rc)
    return rc


def gmres_state_layout(m):
    """Where the parts of the state lie, as the header documents them: the first index of g (m + 1 doubles), of the cosines, of
    the sines (m each) and of R (column j starts at r + j (j + 1) / 2)."""
    return {"g": 2, "c": 3 + m, "s": 3 + 2 * m, "r": 3 + 3 * m}


def _work_bytes(d_work, work_bytes):
    return d_work.numel() * d_work.element_size() if work_bytes is None else work_bytes


def gmres_project(n, k, d_V, ldv, d_w, d_h, d_work, work_bytes=None, stream=0, dtype=None):
    """d_h[j] <- V_j' w for j < k and d_h[k] <- w' w, V_j at d_V + j ldv elements (d_V None where k == 0).  Torch tensors or raw
    device addresses; float64 or float32 vectors by their dtype (raw addresses: dtype=), d_h always doubles.  work_bytes defaults
    to the size of a tensor d_work (gmres_workspace_bytes).  Only enqueues."""
    fn = getattr(load(), "spmv_hip_gmres_project_" + _krylov_suffix((d_V, d_w), dtype))
    check(fn(n, k, _addr(d_V), ldv, _addr(d_w), _addr(d_h), _addr(d_work), _work_bytes(d_work, work_bytes), stream))


def gmres_update(n, k, d_V, ldv, d_h, d_w, d_dots, d_work, work_bytes=None, stream=0, dtype=None):
    """w <- w - sum_j d_h[j] V_j in place, j ascending, with d_h read on the device, and d_dots <- {w' w of the new w, +0.0}.
    Arguments as for gmres_project.  Only enqueues."""
    fn = getattr(load(), "spmv_hip_gmres_update_" + _krylov_suffix((d_V, d_w), dtype))
    check(fn(n, k, _addr(d_V), ldv, _addr(d_h), _addr(d_w), _addr(d_dots), _addr(d_work), _work_bytes(d_work, work_bytes), stream))


def gmres_scale(n, d_scale, d_v, d_minv, d_vhat, stream=0, dtype=None):
    """v <- v d_scale[0] in place with the scale read on the device; with d_minv, d_vhat <- diag(d_minv) v (both None or both
    given).  Only enqueues."""
    fn = getattr(load(), "spmv_hip_gmres_scale_" + _krylov_suffix((d_v, d_minv, d_vhat), dtype))
    check(fn(n, _addr(d_scale), _addr(d_v), _addr(d_minv), _addr(d_vhat), stream))


def gmres_correct(n, k, d_V, ldv, d_y, d_minv, d_x, stream=0, dtype=None):
    """x <- x + diag(d_minv) sum_j d_y[j] V_j (d_minv None: no diagonal), d_y read on the device.  Only enqueues."""
    fn = getattr(load(), "spmv_hip_gmres_correct_" + _krylov_suffix((d_V, d_minv, d_x), dtype))
    check(fn(n, k, _addr(d_V), ldv, _addr(d_y), _addr(d_minv), _addr(d_x), stream))


def gmres_start(m, d_nrm2, d_state, stream=0):
    """The state of a new cycle of m steps from d_nrm2[0] = r' r: g = beta e_1, state[0] = beta, state[1] = 1 / beta."""
    check(load().spmv_hip_gmres_start(m, _addr(d_nrm2), _addr(d_state), stream))


def gmres_column(k, m, d_h1, d_h2, d_nrm2, d_state, stream=0):
    """Column k of the cycle: h = h1 + h2 and h_{k+1} = sqrt(d_nrm2[0]) through the stored rotations and a new one."""
    check(load().spmv_hip_gmres_column(k, m, _addr(d_h1), _addr(d_h2), _addr(d_nrm2), _addr(d_state), stream))


def gmres_solve(k, m, d_state, d_y, stream=0):
    """d_y[0 ... k - 1] <- R[0:k, 0:k]^-1 g[0:k] of the state."""
    check(load().spmv_hip_gmres_solve(k, m, _addr(d_state), _addr(d_y), stream))


class MvPlan:
    """Level-2 plan of Y += A X for k vectors (spmv_hip_mv_plan_*): host row_ptr; X (cols, k) and Y (rows, k) row-major, as
    torch tensors (column slices of wider ones included) or raw device addresses with explicit ldx / ldy."""

    INFO_KEYS = ["rows", "cols", "k", "passes", "tiles", "long_rows", "streamed_bytes", "device_bytes", "stored_entries", "flags",
                 "widest_pass"]

    def __init__(self, rows, cols, host_row_ptr, k, flags=0, stream=0):
        self.lib = load()
        self.h = None
        rp = _i32(host_row_ptr)
        if len(rp) < rows + 1:
            raise ValueError("host_row_ptr needs rows + 1 entries")
        h = _vp()
        check(self.lib.spmv_hip_mv_plan_csr(C.byref(h), rows, cols, rp.ctypes.data, k, flags, stream))
        self.h = h
        self.rows, self.cols, self.k = rows, cols, k

    def close(self):
        if self.h:
            self.lib.spmv_hip_mv_plan_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        out = np.zeros(len(self.INFO_KEYS), dtype=np.int64)
        check(self.lib.spmv_hip_mv_plan_info(self.h, out, len(out)))
        return dict(zip(self.INFO_KEYS, out.tolist()))

    def spmm(self, d_row_ptr, d_col, d_val, X, Y, ldx=None, ldy=None, stream=0):
        """Y += A X.  Tensors give their own address and leading dimension; raw addresses need ldx / ldy."""
        (px, lx), (py, ly) = _dev(X), _dev(Y)
        ldx = lx if ldx is None else ldx
        ldy = ly if ldy is None else ldy
        if ldx is None or ldy is None:
            raise ValueError("ldx / ldy are needed for raw device addresses")
        check(self.lib.spmv_hip_csr_spmm(self.h, _dev(d_row_ptr)[0], _dev(d_col)[0], _dev(d_val)[0], px, ldx, py, ldy, stream))


def ipc_alloc(nbytes):
    """(device address, 64-byte handle) of zeroed device memory other processes can map (ipc_open)."""
    h = C.create_string_buffer(64)
    p = _vp()
    check(load().spmv_hip_ipc_alloc(C.byref(p), nbytes, h))
    return p.value, h.raw


def ipc_open(handle):
    p = _vp()
    check(load().spmv_hip_ipc_open(handle, C.byref(p)))
    return p.value


def ipc_close(addr):
    check(load().spmv_hip_ipc_close(addr))


def ipc_free(addr):
    check(load().spmv_hip_ipc_free(addr))


def peer_push(d_src, d_dst_list, n, stream=0):
    arr = (_vp * len(d_dst_list))(*d_dst_list)
    check(load().spmv_hip_peer_push(d_src, arr, len(d_dst_list), n, stream))


def coo_spmv(rows, nnz, d_row, d_col, d_val, d_x, d_y, stream=0):
    check(load().spmv_hip_coo_spmv(rows, nnz, d_row, d_col, d_val, d_x, d_y, stream))


def coo_variant(variant):
    """Sweep hook of libspmv_hip_experiments.so (SPMV_HIP_EXPERIMENTS=1), not part of the C ABI:
    1 = always the 64-entries-per-wave COO kernel."""
    lib = load()
    if not hasattr(lib, "spmv_hip_coo_variant"):
        raise RuntimeError("spmv_hip_coo_variant needs the experiments build (SPMV_HIP_EXPERIMENTS=1)")
    lib.spmv_hip_coo_variant.argtypes = [C.c_int]
    lib.spmv_hip_coo_variant.restype = None
    lib.spmv_hip_coo_variant(variant)


def coo_sort_by_row(rows, nnz, d_row, d_col, d_val, stream=0):
    """Stable in-place sort of device COO triplets by row index."""
    check(load().spmv_hip_coo_sort_by_row(rows, nnz, d_row, d_col, d_val, stream))


def ell_to_column_major(rows, row_length, d_col_rm, d_val_rm, d_col_cm, d_val_cm, stream=0):
    check(load().spmv_hip_ell_to_column_major(rows, row_length, d_col_rm, d_val_rm, d_col_cm,
                                              d_val_cm, stream))


def ell_spmv(rows, row_length, d_col_cm, d_val_cm, d_x, d_y, stream=0):
    check(load().spmv_hip_ell_spmv(rows, row_length, d_col_cm, d_val_cm, d_x, d_y, stream))


def triad(n, d_a, d_b, d_c, q=3.1, stream=0):
    """a = b + q*c on device arrays (STREAM triad, the empirical bandwidth roofline)."""
    check(load().spmv_hip_triad(n, d_a, d_b, d_c, q, stream))


BJACOBI_MAX_BLOCK = 8


def bjacobi_setup(rows, b, d_row_ptr, d_column_index, d_value, d_inv, d_status, stream=0, dtype=None):
    """d_inv <- the inverses of the rows / b diagonal blocks of the device CSR arrays (d_value doubles), block k row-major at
    d_inv + k b b, and d_status (two int32) <- {singular blocks, the first of them or -1} (include/spmv_hip_bjacobi.h).  Torch
    tensors or raw device addresses; the inverse is float64 or float32 by the dtype of d_inv (a raw address: dtype=).  Only
    enqueues."""
    fn = getattr(load(), "spmv_hip_bjacobi_setup_" + _krylov_suffix((d_inv,), dtype))
    check(fn(rows, b, _addr(d_row_ptr), _addr(d_column_index), _addr(d_value), _addr(d_inv), _addr(d_status), stream))


def bjacobi_apply(n, b, d_inv, d_r, d_z, d_dots=None, d_work=None, work_bytes=None, stream=0, dtype=None):
    """z <- M^-1 r for the block-diagonal inverse d_inv and, with d_dots and d_work (krylov_workspace_bytes(n)), d_dots <-
    {r' z, z' z} of z as stored.  Arguments as for cg_step; work_bytes defaults to the size of a tensor d_work (0 without one).
    Only enqueues."""
    fn = getattr(load(), "spmv_hip_bjacobi_apply_" + _krylov_suffix((d_inv, d_r, d_z), dtype))
    if work_bytes is None:
        work_bytes = d_work.numel() * d_work.element_size() if d_work is not None else 0
    check(fn(n, b, _addr(d_inv), _addr(d_r), _addr(d_z), _addr(d_dots), _addr(d_work), work_bytes, stream))


def bjacobi_apply_add(n, b, d_inv, d_u, d_x, stream=0, dtype=None):
    """x <- x + M^-1 u in place.  Arguments as for bjacobi_apply.  Only enqueues."""
    fn = getattr(load(), "spmv_hip_bjacobi_apply_add_" + _krylov_suffix((d_inv, d_u, d_x), dtype))
    check(fn(n, b, _addr(d_inv), _addr(d_u), _addr(d_x), stream))


CHEBY_MAX_DEGREE = 16


def cheby_bound(rows, d_row_ptr, d_value, d_minv, d_lambda, stream=0, dtype=None):
    """d_lambda (one double) <- max_i |d_minv[i]| sum_j |a_ij| of the device CSR arrays (d_value doubles; d_minv None: 1): the
    Gershgorin bound on lambda_max(M^-1 A) (include/spmv_hip_cheby.h).  Torch tensors or raw device addresses; d_minv is float64
    or float32 by its dtype (a raw address: dtype=; None without dtype=: float64).  Only enqueues."""
    suffix = "f64" if d_minv is None and dtype is None else _krylov_suffix((d_minv,), dtype)
    fn = getattr(load(), "spmv_hip_cheby_bound_" + suffix)
    check(fn(rows, _addr(d_row_ptr), _addr(d_value), _addr(d_minv), _addr(d_lambda), stream))


def cheby_coeffs(degree, d_lambda, scale, ratio, d_coef, stream=0):
    """d_coef (2 degree doubles) <- the pairs {coef[2j], coef[2j + 1]} of the Chebyshev recurrence over [scale lambda / ratio,
    scale lambda], lambda = d_lambda[0] read on the device; scale and ratio are host doubles.  Only enqueues."""
    check(load().spmv_hip_cheby_coeffs(degree, _addr(d_lambda), scale, ratio, _addr(d_coef), stream))


def cheby_step(n, degree, j, d_coef, d_u, d_minv, d_d, d_z, d_r=None, d_dots=None, d_work=None, work_bytes=None, stream=0, dtype=None):
    """Step j of `degree`: d <- coef[2j] d + coef[2j + 1] diag(d_minv) u (d_minv None: u as it is), z <- z + d (j == 0: d and z are
    not read; j == degree - 1: d is not stored; degree == 1: d_d may be None) with the pair read on the device, and -- the last step
    alone, with d_r, d_dots and d_work (krylov_workspace_bytes(n)) -- d_dots <- {r' z, z' z} of z as stored.  Arguments as for
    cg_step; work_bytes defaults to the size of a tensor d_work (0 without one).  Only enqueues."""
    fn = getattr(load(), "spmv_hip_cheby_step_" + _krylov_suffix((d_u, d_minv, d_d, d_z, d_r), dtype))
    if work_bytes is None:
        work_bytes = d_work.numel() * d_work.element_size() if d_work is not None else 0
    check(fn(n, degree, j, _addr(d_coef), _addr(d_u), _addr(d_minv), _addr(d_d), _addr(d_z), _addr(d_r), _addr(d_dots), _addr(d_work),
             work_bytes, stream))


MCGS_MAX_COLOURS = 64


class McgsPlan(C.Structure):
    """spmv_hip_mcgs_plan (include/spmv_hip_mcgs.h): every field public; the four device arrays are the caller's."""
    _fields_ = [("rows", C.c_int32), ("colours", C.c_int32), ("conflicts", C.c_int32), ("group", C.c_int32),
                ("colour_ptr", C.c_int32 * (MCGS_MAX_COLOURS + 1)), ("d_order", _vp), ("d_row_ptr", _vp), ("d_column_index", _vp),
                ("d_value", _vp)]


def _work_bytes(d_work, work_bytes):
    if work_bytes is None:
        return d_work.numel() * d_work.element_size() if d_work is not None else 0
    return work_bytes


def mcgs_workspace_bytes(rows):
    """The workspace mcgs_colour and mcgs_permute need over `rows` rows: a function of rows alone, at least 16."""
    b = C.c_size_t(0)
    check(load().spmv_hip_mcgs_workspace(rows, C.byref(b)))
    return b.value


def mcgs_colour(rows, d_row_ptr, d_column_index, seed, d_colour, d_status, d_work, work_bytes=None, stream=0):
    """d_colour (rows int32) <- the colours 0 ... 63 of the rows of the device CSR pattern, by Jones-Plassmann with first fit under
    `seed`; d_status (four int32) <- {colours, rounds, conflicts, overflowed rows} (include/spmv_hip_mcgs.h).  Torch tensors or raw
    device addresses; work_bytes defaults to the size of a tensor d_work.  SYNCHRONISES the stream."""
    check(load().spmv_hip_mcgs_colour(rows, _addr(d_row_ptr), _addr(d_column_index), seed, _addr(d_colour), _addr(d_status), _addr(d_work),
                                      _work_bytes(d_work, work_bytes), stream))


def mcgs_permute(rows, nnz, d_row_ptr, d_column_index, d_value, d_colour, d_status, d_order, d_perm_row_ptr, d_perm_column_index, d_perm_value,
                 d_work, work_bytes=None, stream=0):
    """The colour-major plan: d_order (rows int32) <- the rows colour by colour, the three d_perm arrays (rows + 1, nnz, nnz) <- the
    matrix with its rows in that order; returns the McgsPlan that points to them (keep the arrays alive).  Arguments as for
    mcgs_colour.  SYNCHRONISES the stream."""
    plan = McgsPlan()
    check(load().spmv_hip_mcgs_permute(rows, nnz, _addr(d_row_ptr), _addr(d_column_index), _addr(d_value), _addr(d_colour), _addr(d_status),
                                       _addr(d_order), _addr(d_perm_row_ptr), _addr(d_perm_column_index), _addr(d_perm_value), C.byref(plan),
                                       _addr(d_work), _work_bytes(d_work, work_bytes), stream))
    return plan


def _plan_ref(plan):
    return None if plan is None else C.byref(plan)


def mcgs_sweep(plan, first, last, omega, d_b, d_minv, d_x, stream=0, dtype=None):
    """The SOR update x_i <- (1 - omega) x_i + omega minv_i (b_i - sum_{j != i} a_ij x_j) of the colours first ... last of the plan
    (descending where last < first), x in place: one launch per colour.  Arguments as for cg_step.  Only enqueues."""
    fn = getattr(load(), "spmv_hip_mcgs_sweep_" + _krylov_suffix((d_b, d_minv, d_x), dtype))
    check(fn(_plan_ref(plan), first, last, omega, _addr(d_b), _addr(d_minv), _addr(d_x), stream))


def mcgs_apply(plan, omega, d_r, d_minv, d_z, d_dots=None, d_work=None, work_bytes=None, stream=0, dtype=None):
    """z <- the SSOR operator of the plan applied to r (z zeroed, a sweep forwards, a sweep backwards) and, with d_dots and d_work
    (krylov_workspace_bytes(rows)), d_dots <- {r' z, z' z} of z as stored.  Arguments as for bjacobi_apply.  Only enqueues."""
    fn = getattr(load(), "spmv_hip_mcgs_apply_" + _krylov_suffix((d_r, d_minv, d_z), dtype))
    check(fn(_plan_ref(plan), omega, _addr(d_r), _addr(d_minv), _addr(d_z), _addr(d_dots), _addr(d_work), _work_bytes(d_work, work_bytes), stream))


class AggPlan(C.Structure):
    """struct spmv_hip_agg_plan (include/spmv_hip_agg.h): every field public; the three device arrays are the caller's."""
    _fields_ = [("rows", C.c_int32), ("aggregates", C.c_int32), ("largest", C.c_int32), ("d_agg", _vp), ("d_member_ptr", _vp),
                ("d_member", _vp)]


def agg_workspace_bytes(rows, nnz=0):
    """The workspace of agg_aggregate and agg_plan (nnz = 0) and of agg_galerkin_symbolic: a function of (rows, nnz) alone."""
    b = C.c_size_t(0)
    check(load().spmv_hip_agg_workspace(rows, nnz, C.byref(b)))
    return b.value


def agg_aggregate(rows, d_row_ptr, d_column_index, d_value, theta, seed, d_agg, d_status, d_work, work_bytes=None, stream=0):
    """d_agg (rows int32) <- the aggregate of every row of the device CSR matrix under `seed`, a neighbour being a stored
    off-diagonal entry with |a_ij| >= theta max_k |a_ik| (d_value None or theta 0: every one); d_status (four int32) <-
    {aggregates, rounds, largest aggregate, singletons} (include/spmv_hip_agg.h).  Arguments as for mcgs_colour.  SYNCHRONISES."""
    check(load().spmv_hip_agg_aggregate(rows, _addr(d_row_ptr), _addr(d_column_index), _addr(d_value), theta, seed, _addr(d_agg), _addr(d_status),
                                        _addr(d_work), _work_bytes(d_work, work_bytes), stream))


def agg_plan(rows, d_agg, d_status, d_member_ptr, d_member, d_work, work_bytes=None, stream=0):
    """d_member_ptr (aggregates + 1 int32), d_member (rows int32) <- the rows aggregate by aggregate, ascending inside one; returns
    the AggPlan that points to them and to d_agg (keep the arrays alive).  SYNCHRONISES the stream."""
    plan = AggPlan()
    check(load().spmv_hip_agg_plan(rows, _addr(d_agg), _addr(d_status), _addr(d_member_ptr), _addr(d_member), C.byref(plan), _addr(d_work),
                                   _work_bytes(d_work, work_bytes), stream))
    return plan


def agg_galerkin_symbolic(plan, nnz, d_row_ptr, d_column_index, d_coarse_row_ptr, d_coarse_column_index, d_entry_order, d_entry_ptr, d_status,
                          d_work, work_bytes=None, stream=0):
    """The pattern of A_c = P' A P (d_coarse_row_ptr: aggregates + 1, d_coarse_column_index: up to nnz) and every coarse entry's run
    of fine entries (d_entry_order: nnz, d_entry_ptr: up to nnz + 1); d_status[0] <- nnz_c.  SYNCHRONISES the stream."""
    check(load().spmv_hip_agg_galerkin_symbolic(_plan_ref(plan), nnz, _addr(d_row_ptr), _addr(d_column_index), _addr(d_coarse_row_ptr),
                                                _addr(d_coarse_column_index), _addr(d_entry_order), _addr(d_entry_ptr), _addr(d_status),
                                                _addr(d_work), _work_bytes(d_work, work_bytes), stream))


def agg_galerkin_numeric(nnz, nnz_c, d_entry_order, d_entry_ptr, d_value, d_coarse_value, stream=0):
    """d_coarse_value[e] <- the fine values of coarse entry e's run, added left to right from +0.0.  Only enqueues."""
    check(load().spmv_hip_agg_galerkin_numeric(nnz, nnz_c, _addr(d_entry_order), _addr(d_entry_ptr), _addr(d_value), _addr(d_coarse_value), stream))


def agg_restrict(plan, d_r, d_rc, stream=0, dtype=None):
    """r_c[I] <- the sum of r over the members of aggregate I in plan order.  Arguments as for cg_step.  Only enqueues."""
    fn = getattr(load(), "spmv_hip_agg_restrict_" + _krylov_suffix((d_r, d_rc), dtype))
    check(fn(_plan_ref(plan), _addr(d_r), _addr(d_rc), stream))


def agg_prolong_add(plan, omega, d_ec, d_x, stream=0, dtype=None):
    """x_i <- x_i + omega e_c[agg[i]] in place.  Arguments as for cg_step.  Only enqueues."""
    fn = getattr(load(), "spmv_hip_agg_prolong_add_" + _krylov_suffix((d_ec, d_x), dtype))
    check(fn(_plan_ref(plan), omega, _addr(d_ec), _addr(d_x), stream))


def agg_mis2_workspace_bytes(rows):
    """The workspace of agg_aggregate_mis2: a function of rows alone (include/spmv_hip_agg_mis2.h)."""
    b = C.c_size_t(0)
    check(load().spmv_hip_agg_mis2_workspace(rows, C.byref(b)))
    return b.value


def agg_aggregate_mis2(rows, d_row_ptr, d_column_index, d_value, theta, seed, d_agg, d_status, d_work, work_bytes=None, stream=0):
    """d_agg, d_status <- the aggregates of a distance-2 independent set of roots: arguments, neighbours, keys and status as for
    agg_aggregate, the workspace agg_mis2_workspace_bytes(rows) (include/spmv_hip_agg_mis2.h).  SYNCHRONISES."""
    check(load().spmv_hip_agg_aggregate_mis2(rows, _addr(d_row_ptr), _addr(d_column_index), _addr(d_value), theta, seed, _addr(d_agg),
                                             _addr(d_status), _addr(d_work), _work_bytes(d_work, work_bytes), stream))


def agg_restrict_group(plan, group, d_r, d_rc, stream=0, dtype=None):
    """r_c[I] <- the sum of r over the members of aggregate I by `group` lanes (a power of two in 1 ... 64) and their butterfly;
    group 1 is agg_restrict.  Arguments as for cg_step.  Only enqueues."""
    fn = getattr(load(), "spmv_hip_agg_restrict_group_" + _krylov_suffix((d_r, d_rc), dtype))
    check(fn(_plan_ref(plan), group, _addr(d_r), _addr(d_rc), stream))


def agg_group(plan):
    """The recommended group of agg_restrict_group: the smallest power of two >= rows / aggregates inside 1 ... 64; host arithmetic."""
    return int(load().spmv_hip_agg_group(_plan_ref(plan)))


COARSE_MAX_N = 2048


def coarse_ld(n):
    """The elements of one row of the inverse of coarse_setup: n rounded up to a multiple of 4, 0 for n <= 0; host arithmetic."""
    return int(load().spmv_hip_coarse_ld(n))


def coarse_workspace_bytes(n):
    """The workspace of coarse_setup over n rows: a function of n alone, at least 16 (include/spmv_hip_coarse.h)."""
    b = C.c_size_t(0)
    check(load().spmv_hip_coarse_workspace(n, C.byref(b)))
    return b.value


def coarse_setup(n, d_row_ptr, d_column_index, d_value, d_inv, d_status, d_work, work_bytes=None, stream=0, dtype=None):
    """d_inv (n rows of coarse_ld(n) elements, row-major) <- the inverse of the n x n device CSR matrix (d_value doubles) by
    Gauss-Jordan with partial pivoting, the identity where it is singular; d_status (three int32) <- {singular, the first column
    with a zero pivot or -1, entries skipped for their column} (include/spmv_hip_coarse.h).  Torch tensors or raw device addresses;
    the inverse is float64 or float32 by the dtype of d_inv (a raw address: dtype=); work_bytes defaults to the size of a tensor
    d_work.  Only enqueues."""
    fn = getattr(load(), "spmv_hip_coarse_setup_" + _krylov_suffix((d_inv,), dtype))
    check(fn(n, _addr(d_row_ptr), _addr(d_column_index), _addr(d_value), _addr(d_inv), _addr(d_status), _addr(d_work),
             _work_bytes(d_work, work_bytes), stream))


def coarse_apply(n, d_inv, d_r, d_z, stream=0, dtype=None):
    """z <- inv r for the dense inverse of coarse_setup, a wave per row.  Arguments as for cg_step.  Only enqueues."""
    fn = getattr(load(), "spmv_hip_coarse_apply_" + _krylov_suffix((d_inv, d_r, d_z), dtype))
    check(fn(n, _addr(d_inv), _addr(d_r), _addr(d_z), stream))
