/*
 * spmv_hip_coarse.h -- the dense solve of a multigrid's coarsest level: the inverse of a small matrix (at most
 * SPMV_HIP_COARSE_MAX_N rows), formed on the device from the CSR arrays the Galerkin product wrote, and its application to a
 * vector.
 *
 *     setup:      inv <- A^-1, from device CSR arrays with fp64 values; d_status <- what it met on the way
 *     apply:      z_i <- fl_T(sum_j inv[i][j] r_j)
 *
 * Same conventions as spmv_hip.h and spmv_hip_bjacobi.h.  T is double (_f64) or float (_f32); 0 <= n <= SPMV_HIP_COARSE_MAX_N.
 * All arithmetic is fp64; every product, quotient, sum and difference is rounded on its own (no FMA); a float gets ONE rounding
 * to float, at its store.  Both calls only enqueue on `stream`: they neither synchronise nor allocate, use no floating-point
 * atomics, and may be captured into a graph (the graph is one chain of nodes).  Behind spmv_hip_agg_galerkin_numeric
 * (spmv_hip_agg.h) on the same stream, setup re-forms the inverse of changed matrix values without a host read.
 *
 * The inverse: ONE caller-owned array, row-major, n rows of ld = spmv_hip_coarse_ld(n) elements of T (n rounded up to a multiple
 * of 4), 16-byte aligned: every row starts 16-byte aligned.  Setup writes the padding columns n ... ld - 1 as +0.0; apply never
 * reads them into a sum.  The layout is public: a caller may fill the array themselves.
 *
 * SETUP.  B (n x n, fp64) starts as +0.0; every stored entry of row i whose column lies in 0 ... n - 1 is added to B[i][column]
 * in stored order (columns may be in any order; a position stored twice is the sum in stored order; a position not stored is 0).
 * An entry whose column lies outside 0 ... n - 1 is skipped and counted; it is never dereferenced.  The inverse is Gauss-Jordan
 * with partial pivoting on [B | I] in fp64, the per-column rule of spmv_hip_bjacobi.h; for column c = 0 ... n - 1:
 *     the pivot row p is the first row >= c with the largest |B[.][c]|: p = c, and a later row i replaces it only where
 *         |B[i][c]| > |B[p][c]| (a NaN never wins);
 *     rows c and p are swapped;
 *     B[c][c] == +-0.0: the matrix is SINGULAR (below);
 *     t = fl(1 / B[c][c]);
 *     the pivot row becomes fl(e t), element by element over all 2 n columns;
 *     every other row i becomes fl(e_i - fl(f e_c)) with f = B[i][c] from before the update and e_c the NEW pivot row.
 * The right half is then stored, rounded once to T.  A singular matrix stores the identity instead: the first column c with a
 * zero pivot is recorded and the columns behind it do nothing.  Non-finite entries are not special-cased.
 *     d_status[0] = 1 where the matrix is singular, else 0
 *     d_status[1] = that column, or -1
 *     d_status[2] = the entries skipped for their column
 * (setup sets the three on the stream before it counts).  The workspace is spmv_hip_coarse_workspace(n) bytes, a function of n
 * alone: [B | I] and one column.  n == 0: the status alone is written.
 *
 * APPLY.  One wave of 64 lanes per row i.  Lane l adds p_j = fl(inv[i][j] r_j) for j = l, l + 64, l + 128, ... < n, ascending,
 * to +0.0: fl(...fl(fl(0 + p_l) + p_{l + 64})...); a lane without an element holds +0.0.  Then the 64 sums are added by the
 * butterfly s_l <- fl(s_l + s_{l ^ step}) for step = 1, 2, 4, 8, 16, 32, and z_i = fl_T(s_0).  A NaN or an Inf in row i of the
 * inverse reaches z_i alone.  n == 0: nothing is launched.
 *
 * Composition (no existing call changes), the coarsest level of the V-cycle of spmv_hip_agg.h, the level above it being L:
 *     r_c = P' t                    spmv_hip_agg_restrict_*(L's plan) or spmv_hip_agg_restrict_group_*
 *     e_c = A_c^-1 r_c              spmv_hip_coarse_apply_*(d_r = r_c, d_z = e_c)
 *     z += w P e_c                  spmv_hip_agg_prolong_add_*(L's plan)
 * and once per change of the matrix values, behind spmv_hip_agg_galerkin_numeric of every level:
 *     inv = A_c^-1                  spmv_hip_coarse_setup_*(the coarsest level's CSR arrays)
 *
 * Refusals (checked before the first HIP call: nothing is launched, nothing is written): SPMV_HIP_ERR_INVALID for n < 0 or
 * n > SPMV_HIP_COARSE_MAX_N, a null required pointer (every one but stream; also where n == 0), work_bytes below
 * spmv_hip_coarse_workspace(n), and a written array (the inverse, the status and the workspace of setup; z) overlapping any other
 * array of the call (of setup's column and value arrays, whose length the host does not know, the first element);
 * SPMV_HIP_ERR_ALIGN for the inverse, a vector or the workspace off 16-byte alignment, d_value off 8-byte and d_row_ptr,
 * d_column_index or d_status off 4-byte alignment.
 *
 * Callers detect the feature by the presence of the symbols (SPMV_HIP_VERSION is unchanged).
 */
#ifndef SPMV_HIP_COARSE_H
#define SPMV_HIP_COARSE_H

#include <stddef.h>

#include "spmv_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the largest matrix */
#define SPMV_HIP_COARSE_MAX_N 2048

/* the elements of one row of the inverse: n rounded up to a multiple of 4; 0 for n <= 0 */
int32_t spmv_hip_coarse_ld(int32_t n);

/* *bytes <- the workspace of spmv_hip_coarse_setup_* over n rows: a function of n alone, at least 16 */
int spmv_hip_coarse_workspace(int32_t n, size_t *bytes);

/* d_inv <- the inverse of the n x n matrix; d_status <- { singular, the first column with a zero pivot or -1, entries skipped } */
int spmv_hip_coarse_setup_f64(int32_t n, const int32_t *d_row_ptr, const int32_t *d_column_index, const double *d_value, double *d_inv,
                              int32_t *d_status, void *d_work, size_t work_bytes, void *stream);
int spmv_hip_coarse_setup_f32(int32_t n, const int32_t *d_row_ptr, const int32_t *d_column_index, const double *d_value, float *d_inv,
                              int32_t *d_status, void *d_work, size_t work_bytes, void *stream);

/* z <- inv r */
int spmv_hip_coarse_apply_f64(int32_t n, const double *d_inv, const double *d_r, double *d_z, void *stream);
int spmv_hip_coarse_apply_f32(int32_t n, const float *d_inv, const float *d_r, float *d_z, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* SPMV_HIP_COARSE_H */
