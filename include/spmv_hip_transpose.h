/*
 * spmv_hip_transpose.h -- the transposed multiply y += A' x of a CSR matrix A (rows x cols, any shape), from the arrays as
 * the caller holds them: row_ptr, column_index and value are read in place, no transposed copy of the matrix is made on the
 * host or on the device, and the plan holds only a table of windows.  x has `rows` entries, y has `cols`.  Same conventions as
 * spmv_hip.h (return codes, host / device pointers, y += ...).
 *
 * Every product a(i,j) x[i] is ADDED to y[j] with fp64 atomics (LDS windows of y per range of rows, global adds for what no
 * window covers), so y is NOT reproducible bit for bit from run to run -- like the symmetric multiply of
 * spmv_hip_symmetric.h -- and SPMV_HIP_FLAG_EXACT_ORDER cannot be honoured.  One device only.  Callers detect the feature by
 * the presence of the symbols.
 */
#ifndef SPMV_HIP_TRANSPOSE_H
#define SPMV_HIP_TRANSPOSE_H

#include "spmv_hip_plan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPMV_HIP_TR_MAX_WINDOWS 8 /* LDS windows of y per range of rows, at most */
#define SPMV_HIP_TR_INFO 14       /* numbers spmv_hip_tr_plan_info and spmv_hip_tr_plan_preview report */

/* ---- Level 1 ------------------------------------------------------------------------------------------------------------
 * Copy A to the device as it is and plan its transposed multiply.  After it spmv_hip_set_x takes `rows` entries, spmv_hip_set_y
 * and spmv_hip_get_y take `cols`; spmv_hip_run / sync / last_run_ns / flush_caches behave as after any upload, and the
 * context's plan info describes the operator that runs: A', cols x rows.  rows, cols or nnz of zero is a valid matrix whose
 * run does nothing.  Refused:
 *   a null pointer, a negative size, a bad row_ptr, a column outside [0, cols): SPMV_HIP_ERR_INVALID;
 *   a context of spmv_hip_create_multi: SPMV_HIP_ERR_STATE (a row partition would need a reduction of y across devices);
 *   a context created with SPMV_HIP_FLAG_EXACT_ORDER: SPMV_HIP_ERR_INVALID (atomic adds keep no order).
 * Everything is checked on the host before anything is freed: a refused upload leaves the previous matrix usable (spmv_hip.h,
 * "uploads"). */
int spmv_hip_upload_csr_transposed(spmv_hip_ctx *ctx, int32_t rows, int32_t cols, int32_t nnz, const int32_t *row_ptr,
                                   const int32_t *column_index, const double *value);

/* ---- Level 2: caller-owned device arrays ---------------------------------------------------------------------------------
 * A plan of its own type, so that no CSR entry point has to learn to reject it. */
typedef struct spmv_hip_tr_plan spmv_hip_tr_plan;

/* What spmv_hip_tr_plan_csr would choose for these HOST arrays, without a device: out[] as for spmv_hip_tr_plan_info, and --
 * where window_table is not null -- the windows themselves, [ranges][windows per range at most]{first column, length}
 * (length 0: unused), window_table_ints int32 values of room (too little: SPMV_HIP_ERR_INVALID; ask out[0] and out[2] with a
 * null table first).  Every number it shares with the plan of the same arguments is equal. */
int spmv_hip_tr_plan_preview(int32_t rows, int32_t cols, const int32_t *host_row_ptr, const int32_t *host_column_index,
                             int max_windows, int window_doubles, int64_t *out, int n, int32_t *window_table,
                             int64_t window_table_ints);

/* Plan the transposed multiply (host row_ptr, DEVICE column indices: read back once, checked against [0, cols), and looked at
 * range by range to choose the LDS windows of y).  max_windows: windows per range (1 .. 8; 0 = automatic, 4); window_doubles:
 * the longest window, in doubles -- it also caps the rows per range (0 = automatic: 2048 rows per range and ~72 KB of
 * windows).  Small values force spilled entries (tests).  Synchronises `stream`.
 * The multiply's correctness does not depend on the windows: they only decide which adds go through LDS, every column is
 * range-checked by the kernel, and an entry outside every window is added to y directly.  So there is no content guard:
 * changed columns (inside [0, cols)) give the product of the changed matrix, possibly slower, and the plan_info numbers then
 * describe the old one; a column outside [0, cols) is skipped. */
int spmv_hip_tr_plan_csr(spmv_hip_tr_plan **plan, int32_t rows, int32_t cols, const int32_t *host_row_ptr,
                         const int32_t *d_column_index, int max_windows, int window_doubles, void *stream);
/* y += A' x: d_x has rows entries, d_y has cols.  d_x and d_y must be different arrays (d_x == d_y: SPMV_HIP_ERR_INVALID);
 * d_column_index and d_value must be 16-byte aligned (SPMV_HIP_ERR_ALIGN).
 * The multiply only enqueues work on `stream`: it neither synchronises nor allocates, and may be captured into a graph
 * (tests/test_gpu_streams.py). */
int spmv_hip_csr_spmv_t(const spmv_hip_tr_plan *plan, const int32_t *d_row_ptr, const int32_t *d_column_index,
                        const double *d_value, const double *d_x, double *d_y, void *stream);
/* out[]: [0] ranges (workgroups)  [1] rows per range  [2] windows per range at most  [3] windows used, summed over the ranges
 *        [4] LDS bytes per workgroup  [5] spilled entries (global atomics per multiply)  [6] bytes of fp64 atomic adds per
 *        multiply (8 per window slot flushed -- an upper bound: zero slots are skipped -- and 8 per spilled entry)
 *        [7] stored entries  [8] rows  [9] cols  [10] plan device bytes (the window table)
 *        [11] bytes one multiply streams (12 per stored entry, row_ptr, x once)  [12] window slots, summed over the ranges
 *        [13] most entries in one range (ranges hold equally many ROWS) */
int spmv_hip_tr_plan_info(const spmv_hip_tr_plan *plan, int64_t *out, int n);
void spmv_hip_tr_plan_destroy(spmv_hip_tr_plan *plan);

#ifdef __cplusplus
}
#endif

#endif /* SPMV_HIP_TRANSPOSE_H */
