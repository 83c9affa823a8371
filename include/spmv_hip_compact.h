/*
 * spmv_hip_compact.h -- y += fl32(A) x (the operator of spmv_hip_f32values.h: float values, every product and sum in fp64) with
 * the COLUMNS of a tile streamed as 16-bit codes: 6 bytes per stored entry instead of 8.  Same conventions as spmv_hip.h.
 *
 * Tiles are those of spmv_hip_f32_plan_csr (cut from row_ptr alone; spmv_hip_f32_plan_preview returns the same table).  Per
 * tile up to SPMV_HIP_C16_WINDOWS window bases are chosen from its distinct columns in ascending order: base[0] is the
 * smallest column, base[w + 1] the smallest column >= base[w] + SPMV_HIP_C16_WINDOW_SPAN; unused bases repeat the last one.
 * A tile that needs at most 8 windows is COMPACT: entry k is the uint16 code (w << 13) | (column - base[w]), and
 * column = base[code >> 13] + (code & 0x1FFF).  A tile that needs more is WIDE and multiplies from the caller's 32-bit
 * columns exactly as spmv_hip_csr_spmv_f32 does.  A tile without entries counts as compact with one window (bases 0).
 * The codes belong to the plan.  Tiles, lanes, products and sums are those of spmv_hip_csr_spmv_f32: y is bit for bit its y.
 *
 * Guarantees: no atomics in the multiply, so two identical calls give identical bits; under SPMV_HIP_FLAG_EXACT_ORDER every
 * row is added left to right from +0.0 by one lane.  No load forms an address outside x[0, cols): the codes are the plan's
 * own.  One device only.  Callers detect the feature by the presence of the symbols.
 *
 * The plan is made from row_ptr and the columns alone, so it does not depend on the value type: spmv_hip_compact_f64.h
 * multiplies the caller's fp64 values, unrounded, through the same plan object.
 */
#ifndef SPMV_HIP_COMPACT_H
#define SPMV_HIP_COMPACT_H

#include "spmv_hip_f32values.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPMV_HIP_C16_INFO 20          /* numbers spmv_hip_c16_plan_info and spmv_hip_c16_plan_preview report */
#define SPMV_HIP_C16_WINDOWS 8        /* windows of a compact tile, at most */
#define SPMV_HIP_C16_WINDOW_SPAN 8192 /* columns a window covers from its base */
#define SPMV_HIP_C16_TILE_INTS 13     /* int32 values of a tile record of the preview */

/* ---- no device needed ----------------------------------------------------------------------------------------------------- */

/* What spmv_hip_c16_plan_csr would choose for these HOST arrays, without a device: out[] as for spmv_hip_c16_plan_info and --
 * where tile_table is not null -- one record of 13 int32 per tile in launch order, {first row, first entry, rows, lanes_log2,
 * windows (0 = wide), base[8]} (a wide tile's bases are 0), tile_table_ints int32 values of room (too little:
 * SPMV_HIP_ERR_INVALID; ask out[5] with a null table first).  Where codes is not null it receives the stored-entries codes by
 * entry index; entries of wide tiles are 0.  host_column_index may be null only where there are no stored entries; a column
 * outside [0, cols) is SPMV_HIP_ERR_INVALID. */
int spmv_hip_c16_plan_preview(int32_t rows, int32_t cols, const int32_t *host_row_ptr, const int32_t *host_column_index,
                              unsigned flags, int64_t *out, int n, int32_t *tile_table, int64_t tile_table_ints,
                              uint16_t *codes);

/* ---- Level 2: caller-owned device arrays ------------------------------------------------------------------------------------ */
typedef struct spmv_hip_c16_plan spmv_hip_c16_plan;

/* Plan the multiply on the host from the HOST row_ptr and columns (host threads, at most 8), copy the tile descriptors, the
 * window bases and the codes to the current device and synchronise `stream`.  flags: 0 or SPMV_HIP_FLAG_EXACT_ORDER; any
 * other bit is SPMV_HIP_ERR_INVALID. */
int spmv_hip_c16_plan_csr(spmv_hip_c16_plan **plan, int32_t rows, int32_t cols, const int32_t *host_row_ptr,
                          const int32_t *host_column_index, unsigned flags, void *stream);
/* y += fl32(A) x.  d_column_index is read by wide tiles only: it may be null where the plan has none (out[7] == 0), a null
 * pointer with wide tiles present is SPMV_HIP_ERR_INVALID.  Where given it must hold the columns the plan was made from
 * (spmv_hip_c16_plan_verify checks that).  d_column_index (where given) and d_value must be 16-byte aligned
 * (SPMV_HIP_ERR_ALIGN); d_x == d_y is SPMV_HIP_ERR_INVALID; rows, cols or nnz of zero is a valid matrix whose multiply does
 * nothing.  Nothing is read beyond the 16 bytes that hold entry nnz - 1 of either caller array.
 * The multiply only enqueues work on `stream`: it neither synchronises nor allocates, and may be captured into a graph
 * (tests/test_gpu_streams.py). */
int spmv_hip_csr_spmv_c16(const spmv_hip_c16_plan *plan, const int32_t *d_row_ptr, const int32_t *d_column_index,
                          const float *d_value, const double *d_x, double *d_y, void *stream);
/* The content guard: decodes every entry of every compact tile on the device and counts those whose column differs from
 * d_column_index (nnz columns).  Synchronises `stream`. */
int spmv_hip_c16_plan_verify(const spmv_hip_c16_plan *plan, const int32_t *d_column_index, int64_t *mismatches, void *stream);
/* out[]: [0] rows  [1] cols  [2] stored entries  [3] flags  [4] workgroups of a multiply  [5] tiles (one wave each)
 *        [6] compact tiles  [7] wide tiles  [8] long-row tiles (one row of more entries than a tile holds; compact or wide)
 *        [9] stored entries in compact tiles  [10] ... [17] compact tiles that use 1 ... 8 windows
 *        [18] plan device bytes: 16 per descriptor (tiles + 1), 32 of bases per tile, 2 per code slot -- a compact tile's
 *        codes start on a quad of their own: ((last entry - first entry rounded down to 4) / 4 + 1) * 4 slots -- the whole
 *        rounded up to 16
 *        [19] bytes one multiply streams AS THE KERNEL READS THEM: 6 per stored entry of a compact tile, 8 per stored entry of
 *        a wide one, row_ptr 4 * (rows + 1) of every tile that reads it, y 16 per row, x once (8 * cols), 16 per descriptor
 *        (tiles + 1) and 32 of bases per tile; 0 where the multiply does nothing. */
int spmv_hip_c16_plan_info(const spmv_hip_c16_plan *plan, int64_t *out, int n);
void spmv_hip_c16_plan_destroy(spmv_hip_c16_plan *plan);

/* ---- Level 1 ------------------------------------------------------------------------------------------------------------
 * spmv_hip_upload_csr_f32values with the compact plan: context format 8.  The context keeps no fp64 values and, where the
 * plan has no wide tile, NO 32-bit columns either: spmv_hip_ctx_info [9] then shows 6 bytes per stored entry plus row_ptr,
 * the vectors and the plan.  spmv_hip_ctx_info [15] reports spmv_hip_c16_plan_info [19], [6] its workgroups.  Refusals and
 * the SPMV_HIP_FLAG_EXACT_ORDER handling are those of spmv_hip_upload_csr_f32values; a context of spmv_hip_create_multi and
 * the block runs on a context that holds this upload are SPMV_HIP_ERR_STATE.  A refused upload leaves the previous matrix
 * usable. */
int spmv_hip_upload_csr_compact(spmv_hip_ctx *ctx, int32_t rows, int32_t cols, int32_t nnz, const int32_t *row_ptr,
                                const int32_t *column_index, const double *value, int allow_rounding);

#ifdef __cplusplus
}
#endif

#endif /* SPMV_HIP_COMPACT_H */
