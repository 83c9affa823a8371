/*
 * spmv_hip_symmetric.h -- symmetric and skew-symmetric SpMV from the STORED TRIANGLE of a matrix (what a Matrix Market file
 * with a `symmetric` or `skew-symmetric` header holds), without mirroring it: every stored value is read once and used for
 * its row and for its transposed position.  Same conventions as spmv_hip.h (return codes, host / device pointers, y += ...).
 *
 * Input: a square CSR matrix T whose entries all lie in ONE triangle, diagonal included -- lower (j <= i in every row, what
 * Matrix Market files store) or upper (j >= i).  Operation:
 *   SPMV_HIP_SYMMETRIC       y += (T + T' - diag(T)) x
 *   SPMV_HIP_SKEW_SYMMETRIC  y += (T - T') x          (a stored diagonal entry is refused: SPMV_HIP_ERR_INVALID)
 * which is what the general kernels compute on the matrix matrix_market::expand_symmetry builds from the same file, within the
 * usual 1e-10.  The partial sums of a row meet in fp64 atomics (LDS windows of y per range of rows, global adds for the rest),
 * so y is NOT reproducible bit for bit from run to run -- like the column panels of spmv_hip_plan_csr_repack -- and
 * SPMV_HIP_FLAG_EXACT_ORDER cannot be honoured.  One device only.  Callers detect the feature by the presence of the symbols.
 */
#ifndef SPMV_HIP_SYMMETRIC_H
#define SPMV_HIP_SYMMETRIC_H

#include "spmv_hip_plan.h"

#ifdef __cplusplus
extern "C" {
#endif

/* kind */
#define SPMV_HIP_SYMMETRIC 1
#define SPMV_HIP_SKEW_SYMMETRIC 2

/* what spmv_hip_csr_triangle reports */
#define SPMV_HIP_TRIANGLE_MIXED 0    /* entries on both sides of the diagonal: not a stored triangle */
#define SPMV_HIP_TRIANGLE_LOWER 1    /* j <= i everywhere, at least one j < i */
#define SPMV_HIP_TRIANGLE_UPPER 2    /* j >= i everywhere, at least one j > i */
#define SPMV_HIP_TRIANGLE_DIAGONAL 3 /* no entry off the diagonal (an empty matrix included): either triangle */

/* Which triangle the square CSR matrix (rows x rows; row_ptr[0] = 0, non-decreasing; columns in [0, rows)) lies in, and how many
 * of its entries sit on the diagonal.  Host only: needs no device.  SPMV_HIP_ERR_INVALID for a null pointer, a negative size, a
 * bad row_ptr or a column outside [0, rows). */
int spmv_hip_csr_triangle(int32_t rows, const int32_t *host_row_ptr, const int32_t *host_column_index, int *triangle,
                          int64_t *diagonal_entries);

/* ---- Level 1 ------------------------------------------------------------------------------------------------------------
 * Copy the stored triangle to the device and plan its symmetric multiply.  After it spmv_hip_run / sync / get_y / set_x /
 * set_y / last_run_ns / flush_caches behave as for any upload (x and y both have `rows` entries).  Refused:
 *   a matrix that spans both triangles, an unknown kind, a skew-symmetric one with a diagonal entry: SPMV_HIP_ERR_INVALID;
 *   a context of spmv_hip_create_multi: SPMV_HIP_ERR_STATE (a row partition would send transposed products across devices);
 *   a context created with SPMV_HIP_FLAG_EXACT_ORDER: SPMV_HIP_ERR_INVALID (that order cannot be kept).
 * A bad row_ptr, row_ptr[rows] != nnz and a column outside [0, rows) are SPMV_HIP_ERR_INVALID as well.  Everything is checked
 * on the host before anything is freed: a refused upload leaves the previous matrix usable (spmv_hip.h, "uploads"). */
int spmv_hip_upload_csr_symmetric(spmv_hip_ctx *ctx, int32_t rows, int32_t nnz, const int32_t *row_ptr,
                                  const int32_t *column_index, const double *value, int kind);

/* ---- Level 2: caller-owned device arrays ---------------------------------------------------------------------------------
 * A plan of its own type, so that no CSR entry point has to learn to reject it. */
typedef struct spmv_hip_sym_plan spmv_hip_sym_plan;

/* Plan the multiply of the stored triangle (host row_ptr, DEVICE column indices: read back once, checked, and looked at range by
 * range to choose the LDS windows).  max_windows: windows per range, the own rows' included (1 .. 8; 0 = automatic, 4);
 * window_doubles: the longest window, in doubles -- it also caps the rows per range (0 = automatic: 2048 rows per range and
 * up to ~56 KB of windows beside them).  Small values force spilled entries (tests).  Synchronises `stream`.
 * The plan keeps nothing derived from the columns that the multiply's correctness depends on: the windows only decide which
 * adds go through LDS, every column is range-checked by the kernel, and an entry outside every window is added to y directly.
 * So there is no content guard like spmv_hip_plan_verify: changed columns give the y of the changed matrix, only slower (the
 * plan_info numbers then describe the old one).  The triangle and kind are checked here; keep the matrix a triangle. */
int spmv_hip_sym_plan_csr(spmv_hip_sym_plan **plan, int32_t rows, const int32_t *host_row_ptr, const int32_t *d_column_index,
                          int kind, int max_windows, int window_doubles, void *stream);
/* y += (T +- T' [- diag]) x.  d_x and d_y must be different arrays (d_x == d_y: SPMV_HIP_ERR_INVALID).
 * The multiply only enqueues work on `stream`: it neither synchronises nor allocates, and may be captured into a graph
 * (tests/test_gpu_streams.py). */
int spmv_hip_csr_symv(const spmv_hip_sym_plan *plan, const int32_t *d_row_ptr, const int32_t *d_column_index,
                      const double *d_value, const double *d_x, double *d_y, void *stream);
/* out[]: [0] ranges (workgroups)  [1] rows per range  [2] windows per range at most (own rows' included)
 *        [3] windows used, summed over the ranges  [4] LDS bytes per workgroup  [5] spilled entries (global atomics per multiply)
 *        [6] bytes of fp64 atomic adds per multiply (8 per window slot flushed -- an upper bound: zero slots are skipped --
 *            and 8 per spilled entry)  [7] stored entries  [8] diagonal entries  [9] triangle (SPMV_HIP_TRIANGLE_*)
 *        [10] plan device bytes  [11] kind  [12] rows  [13] bytes one multiply streams (12 per stored entry, row_ptr, x once)
 *        [14] window slots, summed over the ranges  [15] entries multiplied, 2 stored - diagonal */
int spmv_hip_sym_plan_info(const spmv_hip_sym_plan *plan, int64_t *out, int n);
void spmv_hip_sym_plan_destroy(spmv_hip_sym_plan *plan);

#ifdef __cplusplus
}
#endif

#endif /* SPMV_HIP_SYMMETRIC_H */
