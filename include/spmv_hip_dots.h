/*
 * spmv_hip_dots.h -- the scaled multiplies of spmv_hip_scaled.h with two dot products over the vector they have just written:
 * y_out <- alpha A x + beta y_in, and in the same call
 *
 *     dots[0] = sum_i fl(v_i * v_i)                  ||y_out||^2
 *     dots[1] = sum_i fl((double) w[i] * v_i)        w' y_out       (+0.0 where d_w is null)
 *
 * with v_i = (double) y_out[i] AS STORED (for _c16_f32xy: after the one rounding to float).  What a Krylov method does next with
 * the vector: p'q after q = A p (alpha 1, beta 0, w = x), ||r||^2 after r = b - A x (alpha -1, beta 1, w null), rhat' v after v = A p.
 * Same conventions as spmv_hip.h; plans and arrays are the sibling multiply's.
 *
 * y_out is exactly what the scaled sibling stores, bit for bit: the same tiles, lanes, products and order, the same alpha == 0,
 * beta == 0 and -0.0 rules (spmv_hip_scaled.h).  The products of the dots are rounded in fp64 (no FMA) and added in fp64.  w has
 * `rows` elements of the vectors' type T (double; float for _c16_f32xy).  `dots` is two doubles in DEVICE memory, valid once the
 * work enqueued on `stream` has run: the call neither synchronises nor allocates, and its launches (the tiles, then one or two
 * small reductions on the same stream) may be captured into a graph, where they form a line.
 *
 * Summation order: fixed, a function of the plan alone.  Every row is stored by one lane; that lane adds the row's two products
 * to its own pair of sums, the 64 lanes of a wave are added by one butterfly when the wave's tile is done (lanes that stored no
 * row add +0.0), one lane stores the tile's pair in slot `tile` of the caller's workspace, and the reduction adds the slots in
 * an order that depends on their number only.  No floating-point atomics and no counters: two identical calls give identical
 * bits, in place or out of place, on any stream.  SPMV_HIP_FLAG_EXACT_ORDER changes the row sums z_i as before, not the order of
 * the dots.  Where no tile runs (alpha == 0, or a plan without tiles) the dots are those of what the beta part stores, by the same
 * reduction over one slot per 64 rows; a plan without rows stores +0.0, +0.0.
 *
 * Workspace: spmv_hip_{f32,c16}_dots_workspace(plan, &bytes) is what a call through that plan needs, whatever alpha and beta
 * (at least 16).  A call writes and then reads its first bytes; two calls that may run at once need a workspace each.
 *
 * Refusals (nothing is launched, nothing is written): everything the scaled sibling refuses, by the same code;
 * SPMV_HIP_ERR_INVALID for a null d_dots or d_work, a work_bytes below the plan's, d_w overlapping y_out[0, rows), d_dots or
 * d_work overlapping each other or any array of the call; SPMV_HIP_ERR_ALIGN for d_dots or d_work off 16-byte alignment and a
 * float d_w off 4-byte alignment.  d_w == d_x (rows == cols: x' A x) and d_w == d_y_in are valid: all three are only read.  A
 * null d_w is a kernel without a load of w, as beta == 0 is one without a load of y_in.
 *
 * A plan whose x spans 4 GiB or more (cols * sizeof(T) >= 2^32) is SPMV_HIP_ERR_INVALID: the siblings' kernels for such vectors
 * have never run, and these multiplies have none (it halves their instantiations: 4 kernels x beta == 0 x with / without w).
 * Callers detect the feature by the presence of the symbols (SPMV_HIP_VERSION is unchanged).
 */
#ifndef SPMV_HIP_DOTS_H
#define SPMV_HIP_DOTS_H

#include <stddef.h>

#include "spmv_hip_scaled.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Level 2: caller-owned device arrays ------------------------------------------------------------------------------------ */

/* the bytes of workspace a _scaled_dots call through this plan needs: the tile path and the path without tiles, >= 16 */
int spmv_hip_f32_dots_workspace(const spmv_hip_f32_plan *plan, size_t *bytes);
int spmv_hip_c16_dots_workspace(const spmv_hip_c16_plan *plan, size_t *bytes);

/* spmv_hip_csr_spmv_f32_scaled, and dots <- { y_out' y_out, w' y_out } */
int spmv_hip_csr_spmv_f32_scaled_dots(const spmv_hip_f32_plan *plan, const int32_t *d_row_ptr, const int32_t *d_column_index,
                                      const float *d_value, const double *d_x, double alpha, double beta, const double *d_y_in,
                                      double *d_y_out, const double *d_w, double *d_dots, void *d_work, size_t work_bytes,
                                      void *stream);

/* spmv_hip_csr_spmv_c16_scaled, and the dots */
int spmv_hip_csr_spmv_c16_scaled_dots(const spmv_hip_c16_plan *plan, const int32_t *d_row_ptr, const int32_t *d_column_index,
                                      const float *d_value, const double *d_x, double alpha, double beta, const double *d_y_in,
                                      double *d_y_out, const double *d_w, double *d_dots, void *d_work, size_t work_bytes,
                                      void *stream);

/* spmv_hip_csr_spmv_c16_f64_scaled, and the dots */
int spmv_hip_csr_spmv_c16_f64_scaled_dots(const spmv_hip_c16_plan *plan, const int32_t *d_row_ptr, const int32_t *d_column_index,
                                          const double *d_value, const double *d_x, double alpha, double beta,
                                          const double *d_y_in, double *d_y_out, const double *d_w, double *d_dots, void *d_work,
                                          size_t work_bytes, void *stream);

/* spmv_hip_csr_spmv_c16_f32xy_scaled, and the dots of the floats it stored (fp64 products and sums; w is a float array) */
int spmv_hip_csr_spmv_c16_f32xy_scaled_dots(const spmv_hip_c16_plan *plan, const int32_t *d_row_ptr, const int32_t *d_column_index,
                                            const float *d_value, const float *d_x, double alpha, double beta, const float *d_y_in,
                                            float *d_y_out, const float *d_w, double *d_dots, void *d_work, size_t work_bytes,
                                            void *stream);

/* ---- Level 1 ------------------------------------------------------------------------------------------------------------- */

/* spmv_hip_run_scaled, and the two dots of the context's new y: w is the context's x where rows == cols, and null otherwise
 * (dots[1] is then +0.0).  Formats 7 to 10 on a context of spmv_hip_create; otherwise SPMV_HIP_ERR_STATE with the format named,
 * and y untouched.  The workspace and the dots belong to the context: allocated by the first such call after an upload, freed
 * with the matrix.  spmv_hip_last_run_ns brackets all launches of the call. */
int spmv_hip_run_scaled_dots(spmv_hip_ctx *ctx, double alpha, double beta);

/* Waits for the context's stream and copies the two dots.  SPMV_HIP_ERR_STATE unless the last run on this matrix was
 * spmv_hip_run_scaled_dots. */
int spmv_hip_get_dots(spmv_hip_ctx *ctx, double dots[2]);

#ifdef __cplusplus
}
#endif

#endif /* SPMV_HIP_DOTS_H */
