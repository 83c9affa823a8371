/*
 * spmv_hip_bjacobi.h -- a point-block Jacobi preconditioner for matrices with b unknowns per node, numbered node by node: the
 * inverses of the b x b diagonal blocks, formed on the device from the CSR arrays the multiplies read, and their application
 * fused with the two dots a preconditioned Krylov iteration needs next.
 *
 *     setup:      inv_k <- (A[kb:(k+1)b, kb:(k+1)b])^-1 for every block k, from device CSR arrays with fp64 values
 *     apply:      z_i <- fl_T(sum_j inv[i][j] r[kb + j]), k = i / b, and with z_i AS STORED:
 *                 dots[0] = sum_i fl(z_i r_i)          r' z
 *                 dots[1] = sum_i fl(z_i z_i)          z' z
 *     apply_add:  x_i <- fl_T(x_i + sum_j inv[i][j] u[kb + j])          x += M^-1 u, one rounding at the store
 *
 * Same conventions as spmv_hip.h and spmv_hip_krylov.h.  T is double (_f64) or float (_f32); 1 <= b <= 8 and n % b == 0.  All
 * arithmetic is fp64; every product, quotient, sum and difference is rounded on its own (no FMA); a float gets ONE rounding to
 * float, at its store.  All three calls only enqueue on `stream`: they neither synchronise nor allocate, use no floating-point
 * atomics, and may be captured into a graph.
 *
 * The inverse: ONE caller-owned array of n b elements of T, 16-byte aligned; block k is row-major at d_inv + k b b, so row i of
 * the block-diagonal inverse is the b elements at d_inv + i b.  The layout is public: a caller may fill the array themselves
 * (b == 1: it is the d_minv of the sibling headers).  n b sizeof(T) may exceed 4 GiB; every offset into it is 64-bit.
 *
 * SETUP.  Block k is rows and columns [k b, (k + 1) b).  B starts as +0.0; every stored entry of a row of the block whose column
 * lies in the block is added to its position in stored order (columns may be in any order; a position stored twice is the sum in
 * stored order; a position not stored is 0).  The inverse is Gauss-Jordan with partial pivoting on [B | I] in fp64; for column
 * c = 0 ... b - 1:
 *     the pivot row p is the first row >= c with the largest |B[.][c]|: p = c, and a later row i replaces it only where
 *         |B[i][c]| > |B[p][c]| (a NaN never wins);
 *     rows c and p are swapped;
 *     B[c][c] == +-0.0: the block is SINGULAR (below);
 *     t = fl(1 / B[c][c]);
 *     the pivot row becomes fl(e t), element by element over all 2 b columns;
 *     every other row i becomes fl(e_i - fl(f e_c)) with f = B[i][c] from before the update and e_c the NEW pivot row.
 * The right half is then stored, rounded once to T.  A singular block stores the identity instead and is counted:
 * d_status[0] = the number of such blocks, d_status[1] = the smallest such block index, or -1 where there is none (setup zeroes
 * the two on the stream before it counts).  Non-finite entries are not special-cased: they stay inside their own block.  With
 * b == 1 the result is fl(1 / a_ii), and 1 where row i stores no diagonal entry or a zero one.
 *
 * APPLY.  The sum runs over j ascending, starting from the first product: fl(...fl(fl(p_0 + p_1) + p_2)...), p_j =
 * fl(inv[i][j] r[kb + j]).  The dots are formed from z as stored (a float z: after its rounding).  Summation order, workspace
 * and reduction are those of spmv_hip_cg_step_* (spmv_hip_krylov.h): chunks of SPMV_HIP_KRYLOV_CHUNK elements per wave, lane l
 * takes the 16-byte groups l, l + 64, ... of the chunk in index order, the up to 3 elements behind the last whole group are added
 * last by lanes 0, 1, 2, one butterfly, one slot per chunk, then the reduction of spmv_hip_dots.h.  The workspace is
 * spmv_hip_krylov_workspace(n).  d_dots and d_work may both be null: no sums are formed and no reduction is launched.
 * Two consequences: in doubles with b == 1, dots[0] is bit for bit dots[1] of spmv_hip_cg_step_f64 over the same r and minv; and
 * for an inverse whose blocks happen to be diagonal, z and the dots are the same bits for every b (finite, non-zero operands).
 * n == 0: with dots, +0.0, +0.0 are stored (one reduction over no slots); otherwise nothing is launched.
 *
 * Composition (no existing call changes):
 *
 *   PCG, rz_old / rz_new alternating as in spmv_hip_krylov.h, element [0] of each now r'z:
 *     q = A p, pq = {q'q, p'q}      spmv_hip_csr_spmv_*_scaled_dots(alpha 1, beta 0, w = p, dots = pq)
 *     x += a p, r -= a q            spmv_hip_cg_step_*(d_minv null, num = &rz_old[0], den = &pq[1], dots = its own pair {r'r, 0})
 *     z = M^-1 r, {r'z, z'z}        spmv_hip_bjacobi_apply_*(dots = rz_new)
 *     p = z + b p                   spmv_hip_cg_direction_*(d_r = z, d_minv null, num = &rz_new[0], den = &rz_old[0])
 *
 *   BiCGStab: spmv_hip_bicgstab_s_* and spmv_hip_bicgstab_direction_* with d_minv null, each followed by an apply without dots:
 *     shat = M^-1 s                 spmv_hip_bjacobi_apply_*(d_r = s, d_z = shat, d_dots null, d_work null)
 *     phat = M^-1 p                 spmv_hip_bjacobi_apply_*(d_r = p, d_z = phat, d_dots null, d_work null)
 *
 *   Right-preconditioned GMRES: spmv_hip_gmres_scale_* with d_minv null, then
 *     vhat = M^-1 v                 spmv_hip_bjacobi_apply_*(d_r = v, d_z = vhat, d_dots null, d_work null)
 *   and at the end of a cycle, with a temporary u that starts as zeros,
 *     u = V y                       spmv_hip_gmres_correct_*(d_minv null, d_x = u)
 *     x += M^-1 u                   spmv_hip_bjacobi_apply_add_*(d_u = u)
 *
 * Refusals (checked before the first HIP call: nothing is launched, nothing is written): SPMV_HIP_ERR_INVALID for n (rows) < 0,
 * b outside 1 ... 8, n % b != 0, a null required pointer (every one but stream, and the pair d_dots, d_work; also where n == 0),
 * exactly one of d_dots and d_work null, work_bytes below spmv_hip_krylov_workspace(n), n sizeof(T) >= 2^32, and a written array
 * (the inverse and the status of setup; z, x, dots and the workspace) overlapping any other array of the call (of setup's column
 * and value arrays, whose length the host does not know, the first element); SPMV_HIP_ERR_ALIGN for the inverse, a vector, dots
 * or the workspace off 16-byte alignment, d_value off 8-byte and d_row_ptr, d_column_index or d_status off 4-byte alignment.
 *
 * Callers detect the feature by the presence of the symbols (SPMV_HIP_VERSION is unchanged).
 */
#ifndef SPMV_HIP_BJACOBI_H
#define SPMV_HIP_BJACOBI_H

#include <stddef.h>

#include "spmv_hip_krylov.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the largest block */
#define SPMV_HIP_BJACOBI_MAX_BLOCK 8

/* d_inv <- the inverses of the rows / b diagonal blocks; d_status <- { singular blocks, the first of them or -1 } */
int spmv_hip_bjacobi_setup_f64(int32_t rows, int32_t b, const int32_t *d_row_ptr, const int32_t *d_column_index, const double *d_value,
                               double *d_inv, int32_t *d_status, void *stream);
int spmv_hip_bjacobi_setup_f32(int32_t rows, int32_t b, const int32_t *d_row_ptr, const int32_t *d_column_index, const double *d_value,
                               float *d_inv, int32_t *d_status, void *stream);

/* z <- M^-1 r, and (d_dots, d_work not null) d_dots <- { r'z, z'z } of z as stored */
int spmv_hip_bjacobi_apply_f64(int32_t n, int32_t b, const double *d_inv, const double *d_r, double *d_z, double *d_dots, void *d_work,
                               size_t work_bytes, void *stream);
int spmv_hip_bjacobi_apply_f32(int32_t n, int32_t b, const float *d_inv, const float *d_r, float *d_z, double *d_dots, void *d_work,
                               size_t work_bytes, void *stream);

/* x <- x + M^-1 u */
int spmv_hip_bjacobi_apply_add_f64(int32_t n, int32_t b, const double *d_inv, const double *d_u, double *d_x, void *stream);
int spmv_hip_bjacobi_apply_add_f32(int32_t n, int32_t b, const float *d_inv, const float *d_u, float *d_x, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* SPMV_HIP_BJACOBI_H */
