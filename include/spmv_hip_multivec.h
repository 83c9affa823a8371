/*
 * spmv_hip_multivec.h -- Y += A X for up to 16 vectors of one CSR matrix: every stored entry is read once per pass and used
 * for all of them.  Same conventions as spmv_hip.h (return codes, host / device pointers, accumulation into Y).
 *
 * Layout: X (cols x k) and Y (rows x k) are ROW-MAJOR with a leading dimension -- vector c of row i is Y[i * ldy + c], the
 * layout of a contiguous torch tensor of shape (n, k) and of its column slices.  1 <= k <= 16, ldx >= k, ldy >= k; any ld
 * is accepted (odd ones run with 8-byte loads).  The column and value arrays are 16-byte aligned like every device array
 * here; X and Y need only 8 bytes, so that a column slice of a wider tensor can be passed (16-byte loads are used where
 * the rows allow them).  X and Y must not be the same array (SPMV_HIP_ERR_INVALID).
 *
 * Guarantees:
 *   - batch invariance: the bits of column c depend only on A and on column c of X and Y, not on k, ldx, ldy or the other
 *     columns -- a k-wide multiply equals k one-wide multiplies of the same plan, bit for bit;
 *   - no atomics: two identical calls give identical bits;
 *   - SPMV_HIP_FLAG_EXACT_ORDER: every row summed left to right by one lane, bit-identical to the CPU CSR loop per column;
 *     otherwise within the usual 1e-10 of it.
 * k = 1, 2, 3, 4, 6 and 8 run in one pass over the matrix; other k in several passes over column groups (plan_info [3]).
 * One device only.  Callers detect the feature by the presence of the symbols.
 */
#ifndef SPMV_HIP_MULTIVEC_H
#define SPMV_HIP_MULTIVEC_H

#include "spmv_hip_plan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPMV_HIP_MV_MAX_VECTORS 16

/* ---- Level 2: caller-owned device arrays ---------------------------------------------------------------------------------
 * A plan of its own type, so that no single-vector entry point has to learn to reject it. */
typedef struct spmv_hip_mv_plan spmv_hip_mv_plan;

/* Plan Y += A X for k vectors from the host row_ptr (rows + 1 entries, row_ptr[0] = 0, non-decreasing).  flags: 0 or
 * SPMV_HIP_FLAG_EXACT_ORDER; any other bit is SPMV_HIP_ERR_INVALID.  The tiles come from row lengths alone.  Copies the plan
 * to the device on `stream` and synchronises it. */
int spmv_hip_mv_plan_csr(spmv_hip_mv_plan **plan, int32_t rows, int32_t cols, const int32_t *host_row_ptr, int k,
                         unsigned flags, void *stream);
/* Y += A X with the plan's k.  d_row_ptr must hold the row_ptr the plan was made from; every column index must lie in
 * [0, cols) (not checked here: spmv_hip_csr_spmv's rule).  d_X == d_Y: SPMV_HIP_ERR_INVALID.
 * The multiply only enqueues work on `stream`: it neither synchronises nor allocates, and may be captured into a graph
 * (tests/test_gpu_streams.py). */
int spmv_hip_csr_spmm(const spmv_hip_mv_plan *plan, const int32_t *d_row_ptr, const int32_t *d_column_index,
                      const double *d_value, const double *d_X, int64_t ldx, double *d_Y, int64_t ldy, void *stream);
/* out[]: [0] rows  [1] cols  [2] k  [3] passes over the matrix  [4] wave tiles  [5] long rows (a workgroup each)
 *        [6] bytes one multiply streams: passes * (12 nnz + 4 (rows + 1)) + 8 k cols + 16 k rows
 *        [7] plan device bytes  [8] stored entries  [9] flags  [10] widest pass (vectors) */
int spmv_hip_mv_plan_info(const spmv_hip_mv_plan *plan, int64_t *out, int n);
void spmv_hip_mv_plan_destroy(spmv_hip_mv_plan *plan);

/* ---- Level 1: after spmv_hip_upload_csr on a context of spmv_hip_create --------------------------------------------------
 * The context keeps its block X (cols x k) and Y (rows x k) apart from x and y: single-vector runs are not disturbed, and
 * the matrix arrays are read as uploaded.  X and Y are dense row-major host arrays (ld = k).  set_block_x / set_block_y
 * with a k other than the current one start a new pair (Y zero).  spmv_hip_run_block adds A X to Y on the context's stream;
 * spmv_hip_sync and spmv_hip_last_run_ns work after it as after spmv_hip_run.  Other uploads, no upload and contexts of
 * spmv_hip_create_multi: SPMV_HIP_ERR_STATE.  get_block_y with another k, or run_block before set_block_x:
 * SPMV_HIP_ERR_STATE. */
int spmv_hip_set_block_x(spmv_hip_ctx *ctx, int k, const double *X);
int spmv_hip_set_block_y(spmv_hip_ctx *ctx, int k, const double *Y);
int spmv_hip_get_block_y(spmv_hip_ctx *ctx, int k, double *Y);
int spmv_hip_run_block(spmv_hip_ctx *ctx);

#ifdef __cplusplus
}
#endif

#endif /* SPMV_HIP_MULTIVEC_H */
