/*
 * spmv_hip_scaled.h -- y_out <- alpha A x + beta y_in for the four float-tile multiplies: spmv_hip_csr_spmv_f32
 * (spmv_hip_f32values.h), spmv_hip_csr_spmv_c16 (spmv_hip_compact.h), spmv_hip_csr_spmv_c16_f64 (spmv_hip_compact_f64.h) and
 * spmv_hip_csr_spmv_c16_f32xy (spmv_hip_compact_f32xy.h).  Same conventions as spmv_hip.h; the plans are those multiplies' own.
 *
 * With z_i the sum of row i exactly as the multiply without a scale forms it (the same tiles, lanes, products and order; +0.0 for
 * a row without entries), and T the element type of the vectors (double; float for _c16_f32xy):
 *
 *     y_out[i] <- (T)( fl(alpha * z_i) + fl(beta * (double) y_in[i]) )
 *
 * alpha and beta are doubles for every T.  Two multiplies and one add, each rounded in fp64 (no FMA); for float vectors one
 * rounding to float per row and call, as in the multiply without a scale.
 *
 *   beta == 0    y_in is never read and may be null: y_out[i] <- (T) fl(alpha * z_i).  A NaN or Inf in y_in does not reach y_out
 *                (the kernel has no load of y_in).  This is q = A p without a memset of q.
 *   alpha == 0   no tile is launched and neither the matrix nor x is read; d_row_ptr, d_column_index, d_value and d_x may be
 *                null: y_out[i] <- (T) fl(beta * (double) y_in[i]), and +0.0 where beta == 0 as well.  One small vector kernel.
 *   -0.0         counts as zero for both factors (the comparisons are ==): y_in is not read under beta == -0.0, no tile runs
 *                under alpha == -0.0, and alpha == -0.0 with beta == -0.0 stores +0.0.  Every other factor, NaN and +-Inf
 *                included, goes through the formula: alpha < 0 with beta == 0 gives -0.0 in a row without entries, an infinite
 *                alpha gives NaN there (fl(alpha * +0.0)).
 *   alpha = 1, beta = 1, y_in == y_out   the bits of the multiply without a scale.
 *   alpha = -1, beta = 1, y_in = b       the residual r = b - A x, out of place.
 *
 * A plan whose rows, cols or stored entries are zero still performs the beta part on its rows (every z_i is +0.0).
 *
 * Arrays: y_out == y_in (in place) is valid; y_out[0, rows) overlapping y_in[0, rows) in any other way is SPMV_HIP_ERR_INVALID
 * (checked where beta != 0: otherwise y_in is ignored altogether).  y_out == x is SPMV_HIP_ERR_INVALID; y_in == x is valid, both
 * are only read.  A null y_out, and a null y_in with beta != 0, are SPMV_HIP_ERR_INVALID.  Every other refusal and alignment rule
 * is the sibling multiply's, checked by the same code (column and value arrays 16-byte aligned; float vectors, y_in included,
 * 4-byte aligned), and applies where the matrix is read (alpha != 0).  A refused call launches nothing.
 *
 * Guarantees: those of the family -- no atomics; two identical calls give identical bits; under SPMV_HIP_FLAG_EXACT_ORDER every
 * z_i is added left to right from +0.0 by one lane; nothing outside x[0, cols) or y_in[0, rows) is read and nothing outside
 * y_out[0, rows) is written.  A call only enqueues work on `stream`: it neither synchronises nor allocates, and may be captured
 * into a graph.  One device only.  Vectors of 4 GiB and more (the kernels' X32 = false instantiations) are compiled and their
 * resources checked (tests/test_scaled_isa.py) but have not been run.  Callers detect the feature by the presence of the symbols
 * (SPMV_HIP_VERSION is unchanged).
 */
#ifndef SPMV_HIP_SCALED_H
#define SPMV_HIP_SCALED_H

#include "spmv_hip_f32values.h"
#include "spmv_hip_compact_f32xy.h"
#include "spmv_hip_compact_f64.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Level 2: caller-owned device arrays ------------------------------------------------------------------------------------ */

/* y_out <- alpha fl32(A) x + beta y_in over 32-bit columns and float values (the plan and arrays of spmv_hip_csr_spmv_f32) */
int spmv_hip_csr_spmv_f32_scaled(const spmv_hip_f32_plan *plan, const int32_t *d_row_ptr, const int32_t *d_column_index,
                                 const float *d_value, const double *d_x, double alpha, double beta, const double *d_y_in,
                                 double *d_y_out, void *stream);

/* ... over 16-bit column codes and float values (spmv_hip_csr_spmv_c16; d_column_index may be null where the plan has no wide
 * tile) */
int spmv_hip_csr_spmv_c16_scaled(const spmv_hip_c16_plan *plan, const int32_t *d_row_ptr, const int32_t *d_column_index,
                                 const float *d_value, const double *d_x, double alpha, double beta, const double *d_y_in,
                                 double *d_y_out, void *stream);

/* y_out <- alpha A x + beta y_in on the caller's fp64 values beside the codes (spmv_hip_csr_spmv_c16_f64): the exact operator */
int spmv_hip_csr_spmv_c16_f64_scaled(const spmv_hip_c16_plan *plan, const int32_t *d_row_ptr, const int32_t *d_column_index,
                                     const double *d_value, const double *d_x, double alpha, double beta, const double *d_y_in,
                                     double *d_y_out, void *stream);

/* y_out <- fl32(alpha fl32(A) x + beta y_in) on float x, y_in and y_out (spmv_hip_csr_spmv_c16_f32xy) */
int spmv_hip_csr_spmv_c16_f32xy_scaled(const spmv_hip_c16_plan *plan, const int32_t *d_row_ptr, const int32_t *d_column_index,
                                       const float *d_value, const float *d_x, double alpha, double beta, const float *d_y_in,
                                       float *d_y_out, void *stream);

/* ---- Level 1 ------------------------------------------------------------------------------------------------------------- */

/* The context's y <- alpha A x + beta y, in place, on a context of spmv_hip_upload_csr_f32values (format 7),
 * spmv_hip_upload_csr_compact (8), spmv_hip_upload_csr_compact_f64 (9) or spmv_hip_upload_csr_compact_f32xy (10): the scaled
 * form of the multiply spmv_hip_run launches there.  SPMV_HIP_ERR_STATE, with a message that names the format: any other
 * format, no matrix, or a context of spmv_hip_create_multi; y is then untouched.  spmv_hip_last_run_ns, spmv_hip_sync and
 * spmv_hip_set_stream behave as after spmv_hip_run. */
int spmv_hip_run_scaled(spmv_hip_ctx *ctx, double alpha, double beta);

#ifdef __cplusplus
}
#endif

#endif /* SPMV_HIP_SCALED_H */
