/*
 * spmv_hip_f32values.h -- y += fl32(A) x for a CSR matrix whose VALUES are stored and streamed as 4-byte floats: every product
 * (double) a32[k] * x[j[k]] and every row sum is fp64 (a multiply, then an add: no FMA), x and y are fp64 as everywhere else.
 * With 32-bit columns a stored entry costs 8 bytes per multiply instead of 12.  Same conventions as spmv_hip.h (return codes,
 * host / device pointers, y += ...).
 *
 * fl32(v) is the C conversion (float) v: round to nearest, ties to even, denormal results kept, -0.0, +-inf and NaN kept.  The
 * result is exactly the fp64 CSR multiply of the matrix whose values are (double)(float) v; where every value is a float
 * already the feature is lossless.  A finite double whose float is infinite is never accepted: SPMV_HIP_ERR_OVERFLOW.
 *
 * Guarantees: no atomics anywhere, so two identical calls give identical bits; under SPMV_HIP_FLAG_EXACT_ORDER every row is
 * added left to right from +0.0 by one lane, bit for bit the CPU loop.  One device only.  Callers detect the feature by the
 * presence of the symbols.
 */
#ifndef SPMV_HIP_F32VALUES_H
#define SPMV_HIP_F32VALUES_H

#include "spmv_hip_plan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPMV_HIP_F32_INFO 12      /* numbers spmv_hip_f32_plan_info and spmv_hip_f32_plan_preview report */
#define SPMV_HIP_F32_TILE 512     /* entries of a tile of several rows, at most, counted from its 4-aligned first entry */
#define SPMV_HIP_F32_TILE_ROWS 64 /* rows of a tile, at most */

/* ---- no device needed ----------------------------------------------------------------------------------------------------- */

/* out[k] = (float) value[k] for k < n.  *inexact: how many values have (double)(float) v != v (NaN does not count);
 * *max_rel_err: the largest |fl32(v) - v| / |v| among them (0 if none) -- at most 2^-24 while the result is a normal float,
 * larger for denormal results.  inexact and max_rel_err may be null.  A finite value whose float is infinite:
 * SPMV_HIP_ERR_OVERFLOW (out[] is written all the same, the counts are not).  n == 0 is valid. */
int spmv_hip_narrow_values_host(int64_t n, const double *value, float *out, int64_t *inexact, double *max_rel_err);

/* What spmv_hip_f32_plan_csr would choose for this HOST row_ptr, without a device: out[] as for spmv_hip_f32_plan_info, and --
 * where tile_table is not null -- one record per tile in launch order, {first row, first entry, rows, lanes_log2},
 * tile_table_ints int32 values of room (too little: SPMV_HIP_ERR_INVALID; ask out[3] with a null table first).  Every number
 * it shares with the plan of the same arguments is equal. */
int spmv_hip_f32_plan_preview(int32_t rows, int32_t cols, const int32_t *host_row_ptr, unsigned flags, int64_t *out, int n,
                              int32_t *tile_table, int64_t tile_table_ints);

/* ---- Level 2: caller-owned device arrays -- the value array is the CALLER'S float array ------------------------------------
 * A plan of its own type, so that no CSR entry point has to learn to reject it. */
typedef struct spmv_hip_f32_plan spmv_hip_f32_plan;

/* spmv_hip_narrow_values_host on DEVICE arrays (d_value: n doubles, d_out: n floats; they may not overlap), the same bits and
 * the same counts.  Synchronises `stream`. */
int spmv_hip_narrow_values(int64_t n, const double *d_value, float *d_out, int64_t *inexact, double *max_rel_err, void *stream);

/* Plan the multiply from the HOST row_ptr alone: no column is read, so there is no content guard.  flags: 0 or
 * SPMV_HIP_FLAG_EXACT_ORDER; any other bit is SPMV_HIP_ERR_INVALID.  Copies the tile descriptors to the current device and
 * synchronises `stream`. */
int spmv_hip_f32_plan_csr(spmv_hip_f32_plan **plan, int32_t rows, int32_t cols, const int32_t *host_row_ptr, unsigned flags,
                          void *stream);
/* y += fl32(A) x.  Columns must lie in [0, cols) (not checked here: spmv_hip_csr_spmv's rule).  d_column_index and d_value
 * must be 16-byte aligned (SPMV_HIP_ERR_ALIGN); d_x == d_y is SPMV_HIP_ERR_INVALID; rows, cols or nnz of zero is a valid
 * matrix whose multiply does nothing.  Nothing is read beyond the 16 bytes that hold entry nnz - 1 of either array.
 * The multiply only enqueues work on `stream`: it neither synchronises nor allocates, and may be captured into a graph
 * (tests/test_gpu_streams.py). */
int spmv_hip_csr_spmv_f32(const spmv_hip_f32_plan *plan, const int32_t *d_row_ptr, const int32_t *d_column_index,
                          const float *d_value, const double *d_x, double *d_y, void *stream);
/* out[]: [0] rows  [1] cols  [2] stored entries  [3] tiles (one wave each)  [4] long-row tiles (one row of more entries than a
 *        tile holds, the whole wave in registers)  [5] longest row  [6] flags  [7] plan device bytes (the tile descriptors)
 *        [8] bytes one multiply streams AS THE KERNEL READS THEM: 8 per stored entry, row_ptr 4 * (rows + 1) of every tile
 *        that reads it, y 16 per row, x once (8 * cols), 16 per tile descriptor (tiles + 1 of them); 0 where the multiply
 *        does nothing  [9] tiles whose rows are equally long (row_ptr is not read for them, nor for long-row tiles)
 *        [10] tiles read entry by entry (empty rows only, or the last 16 bytes of the arrays are not whole)
 *        [11] workgroups of a multiply */
int spmv_hip_f32_plan_info(const spmv_hip_f32_plan *plan, int64_t *out, int n);
void spmv_hip_f32_plan_destroy(spmv_hip_f32_plan *plan);

/* ---- Level 1 ------------------------------------------------------------------------------------------------------------
 * Narrow the fp64 values on the host, copy A to the device with 4-byte values and plan its multiply: the context keeps NO fp64
 * copy of the values (8 device bytes per stored entry instead of 12, spmv_hip_ctx_info [9]).  Context format 7.  spmv_hip_set_x
 * / set_y / get_y / run / sync / last_run_ns / flush_caches / set_stream behave as after any upload; spmv_hip_ctx_info [15]
 * reports the streamed bytes of spmv_hip_f32_plan_info [8], [6] its workgroups.  The context's SPMV_HIP_FLAG_EXACT_ORDER is
 * kept; its other flags do not apply.  Refused:
 *   a null pointer, a negative size, a bad row_ptr, a column outside [0, cols): SPMV_HIP_ERR_INVALID;
 *   values that (float) changes while allow_rounding == 0: SPMV_HIP_ERR_INVALID, and spmv_hip_last_error names their count and
 *   the first offending entry;  a finite value whose float is infinite: SPMV_HIP_ERR_OVERFLOW;
 *   a context of spmv_hip_create_multi: SPMV_HIP_ERR_STATE.
 * Everything is checked on the host before anything is freed: a refused upload leaves the previous matrix usable (spmv_hip.h,
 * "uploads").
 * spmv_hip_set_block_x / spmv_hip_run_block ... on a context that holds this upload: SPMV_HIP_ERR_STATE (there are no fp64
 * values for them to read). */
int spmv_hip_upload_csr_f32values(spmv_hip_ctx *ctx, int32_t rows, int32_t cols, int32_t nnz, const int32_t *row_ptr,
                                  const int32_t *column_index, const double *value, int allow_rounding);

#ifdef __cplusplus
}
#endif

#endif /* SPMV_HIP_F32VALUES_H */
