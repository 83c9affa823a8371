/*
 * spmv_hip_compact_f64.h -- y += A x, the EXACT operator on the caller's fp64 values, with the columns of a tile streamed as the
 * 16-bit codes of spmv_hip_compact.h: 10 bytes per stored entry of a compact tile where the plan of spmv_hip_plan_csr streams
 * 12, with no rounding anywhere.  Same conventions as spmv_hip.h.
 *
 * The plan is spmv_hip_compact.h's spmv_hip_c16_plan: it is made from row_ptr and the columns alone and does not know the value
 * type.  One plan object serves spmv_hip_csr_spmv_c16 (float values) and spmv_hip_csr_spmv_c16_f64 (double values) in any order.
 *
 * Guarantees: those of spmv_hip_compact.h -- no atomics, two identical calls give identical bits, under
 * SPMV_HIP_FLAG_EXACT_ORDER every row is added left to right from +0.0 by one lane (bit for bit the reference's CSR kernel),
 * no address outside x[0, cols).  One device only.  Callers detect the feature by the presence of the symbols
 * (SPMV_HIP_VERSION and SPMV_HIP_C16_INFO are unchanged).
 */
#ifndef SPMV_HIP_COMPACT_F64_H
#define SPMV_HIP_COMPACT_F64_H

#include "spmv_hip_compact.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Level 2: caller-owned device arrays ------------------------------------------------------------------------------------ */

/* y += A x on fp64 values through the same plan: the tiles, lanes, products (a multiply, then an add: no FMA) and sums of
 * spmv_hip_csr_spmv_c16, with nothing narrowed or widened -- on values that are floats it gives that multiply's y bit for bit,
 * and under SPMV_HIP_FLAG_EXACT_ORDER the reference's y on any values.  The refusals are those of spmv_hip_csr_spmv_c16; d_value
 * need only be 16-byte aligned (a quad of four doubles is read as two 16-byte loads).  Nothing is read in front of entry 0 or
 * beyond entry nnz - 1 of d_value.  Bytes one multiply streams: spmv_hip_c16_plan_info [19] + 4 * [2] (10 per stored entry of
 * a compact tile, 12 per stored entry of a wide one) where the multiply does something, else 0.
 * The multiply only enqueues work on `stream`: it neither synchronises nor allocates, and may be captured into a graph
 * (tests/test_gpu_streams.py). */
int spmv_hip_csr_spmv_c16_f64(const spmv_hip_c16_plan *plan, const int32_t *d_row_ptr, const int32_t *d_column_index,
                              const double *d_value, const double *d_x, double *d_y, void *stream);

/* ---- Level 1 ------------------------------------------------------------------------------------------------------------- */

/* spmv_hip_upload_csr with the compact plan and the fp64 values as they are: context format 9, spmv_hip_run is
 * spmv_hip_csr_spmv_c16_f64.  The context keeps row_ptr, the fp64 values, the plan and -- only where the plan has wide tiles
 * -- the 32-bit columns: about 10.2 device bytes per stored entry beside row_ptr and the vectors, against 12.  Nothing is
 * rounded, so there is no allow_rounding and no overflow refusal.  SPMV_HIP_ERR_INVALID: a bad row_ptr, row_ptr[rows] != nnz,
 * a column outside [0, cols); SPMV_HIP_ERR_STATE: a context of spmv_hip_create_multi, and the block runs on a context that
 * holds this upload (the columns may be gone).  A refused upload leaves the previous matrix usable.  The context's
 * SPMV_HIP_FLAG_EXACT_ORDER is kept.  spmv_hip_ctx_info [15] is spmv_hip_c16_plan_info [19] + 4 * [2] (0 where the multiply
 * does nothing), [6] the plan's workgroups, [9] the device bytes. */
int spmv_hip_upload_csr_compact_f64(spmv_hip_ctx *ctx, int32_t rows, int32_t cols, int32_t nnz, const int32_t *row_ptr,
                                    const int32_t *column_index, const double *value);

#ifdef __cplusplus
}
#endif

#endif /* SPMV_HIP_COMPACT_F64_H */
