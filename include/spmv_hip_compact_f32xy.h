/*
 * spmv_hip_compact_f32xy.h -- y <- fl32(y + fl32(A) x) on FLOAT x and y: the compact multiply of spmv_hip_compact.h (float values,
 * 16-bit column codes, 6 bytes per stored entry) with the vectors stored and streamed as 4-byte floats as well.  Same conventions
 * as spmv_hip.h.
 *
 *     y[i] <- fl32( (double) y[i] + sum_k (double) a[k] * (double) x[col[k]] )
 *
 * A float times a float is exact in fp64, so only the additions round, in fp64; the sum of a row is added to the widened y[i]
 * and rounded to float ONCE per row and call (to nearest, ties to even; a sum beyond the float range becomes +-inf as an IEEE
 * conversion does).  Nothing is accumulated in fp32.
 *
 * The plan is spmv_hip_compact.h's spmv_hip_c16_plan: it is made from row_ptr and the columns alone and knows neither the value
 * nor the vector type.  One plan object serves spmv_hip_csr_spmv_c16, spmv_hip_csr_spmv_c16_f64 and spmv_hip_csr_spmv_c16_f32xy
 * in any order.
 *
 * Guarantees: those of spmv_hip_compact.h -- no atomics, two identical calls give identical bits, under
 * SPMV_HIP_FLAG_EXACT_ORDER every row is added left to right from +0.0 by one lane, then added to (double) y[i], then rounded;
 * no address outside x[0, cols).  No load or store of x or y is wider than one element.  One device only.  Callers detect the
 * feature by the presence of the symbols (SPMV_HIP_VERSION and SPMV_HIP_C16_INFO are unchanged).
 */
#ifndef SPMV_HIP_COMPACT_F32XY_H
#define SPMV_HIP_COMPACT_F32XY_H

#include "spmv_hip_compact.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Level 2: caller-owned device arrays ------------------------------------------------------------------------------------ */

/* The tiles, lanes, products (a multiply, then an add: no FMA) and sums of spmv_hip_csr_spmv_c16 in the order the plan fixes.
 * The refusals are those of spmv_hip_csr_spmv_c16, and d_x and d_y need only be 4-byte aligned (SPMV_HIP_ERR_ALIGN otherwise),
 * so a slice of a larger float tensor can be passed.  Bytes one multiply streams: spmv_hip_c16_plan_info [19] - 8 * [0] - 4 * [1]
 * (y 8 instead of 16 per row, x 4 instead of 8 per column) where the multiply does something, else 0.
 * The multiply only enqueues work on `stream`: it neither synchronises nor allocates, and may be captured into a graph
 * (tests/test_gpu_streams.py). */
int spmv_hip_csr_spmv_c16_f32xy(const spmv_hip_c16_plan *plan, const int32_t *d_row_ptr, const int32_t *d_column_index,
                                const float *d_value, const float *d_x, float *d_y, void *stream);

/* ---- Level 1 ------------------------------------------------------------------------------------------------------------- */

/* spmv_hip_upload_csr_compact with float vectors: context format 10, spmv_hip_run is spmv_hip_csr_spmv_c16_f32xy.  The values
 * are narrowed and refused as spmv_hip_upload_csr_compact does (allow_rounding).  The context keeps row_ptr, the float values,
 * the plan, FLOAT x and y (zeroed) and -- only where the plan has wide tiles -- the 32-bit columns; no doubles at all.
 * SPMV_HIP_ERR_INVALID: a bad row_ptr, row_ptr[rows] != nnz, a column outside [0, cols); SPMV_HIP_ERR_STATE: a context of
 * spmv_hip_create_multi, and the block runs on a context that holds this upload.  A refused upload leaves the previous matrix
 * usable.  The context's SPMV_HIP_FLAG_EXACT_ORDER is kept.  spmv_hip_ctx_info [15] is the streamed bytes above, [6] the
 * plan's workgroups, [9] the device bytes.  spmv_hip_run, spmv_hip_sync, spmv_hip_last_run_ns and spmv_hip_flush_caches work
 * as on any one-device context. */
int spmv_hip_upload_csr_compact_f32xy(spmv_hip_ctx *ctx, int32_t rows, int32_t cols, int32_t nnz, const int32_t *row_ptr,
                                      const int32_t *column_index, const double *value, int allow_rounding);

/* The vectors of a format-10 context: cols floats in, rows floats in, rows floats out; they synchronise like spmv_hip_set_x,
 * spmv_hip_set_y and spmv_hip_get_y.  Nothing is rounded silently: these three on a context of any other format, and
 * spmv_hip_set_x, spmv_hip_set_y and spmv_hip_get_y on a format-10 context, are SPMV_HIP_ERR_STATE. */
int spmv_hip_set_x_f32(spmv_hip_ctx *ctx, const float *x);
int spmv_hip_set_y_f32(spmv_hip_ctx *ctx, const float *y);
int spmv_hip_get_y_f32(spmv_hip_ctx *ctx, float *y);

#ifdef __cplusplus
}
#endif

#endif /* SPMV_HIP_COMPACT_F32XY_H */
