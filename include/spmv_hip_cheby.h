/*
 * spmv_hip_cheby.h -- a Chebyshev polynomial preconditioner z = p(M^-1 A) M^-1 r whose coefficients never leave the device: a
 * Gershgorin bound on lambda_max(M^-1 A) from the CSR arrays the multiplies read, the recurrence's coefficients from that bound,
 * and the one fused vector update that stands between the polynomial's multiplies.
 *
 *     bound:   lambda[0] <- max_i fl(|m_i| s_i), s_i = sum_j |a_ij| over row i        (>= lambda_max(M^-1 A), M^-1 = diag(m))
 *     coeffs:  coef[0 ... 2 degree - 1] from lambda[0], a scale and the interval's ratio (the table below)
 *     step j:  d <- coef[2j] d + coef[2j + 1] M^-1 u,  z <- z + d,  and behind the last step {r'z, z'z}
 *
 * Same conventions as spmv_hip.h and spmv_hip_krylov.h.  T is double (_f64) or float (_f32).  All arithmetic is fp64; every
 * product, quotient, sum and difference is rounded on its own (no FMA); a float gets ONE rounding to float, at its store.  Every
 * call only enqueues on `stream`: it neither synchronises nor allocates, uses no floating-point atomics, and may be captured into
 * a graph, in which the launches of one call and of consecutive calls form a line.
 *
 * The polynomial is the Chebyshev iteration for M^-1 A z = M^-1 r from z = 0 over the interval [lmin, lmax]: `degree` steps, and
 * between two steps one multiply u = r - A z.  It is a fixed polynomial in M^-1 A applied to M^-1 r -- no dot product, no host
 * read -- so for a symmetric positive definite A and a positive diagonal M it is a fixed symmetric positive definite operator
 * and conjugate gradients stay valid; eigenvalues of M^-1 A below lmin are damped less, not amplified.
 *
 * BOUND.  (rows, d_row_ptr, d_value) are the device CSR arrays with fp64 values; no column index is read.  s_i starts as +0.0 and
 * takes |a_ij| of row i in stored order, one rounding per add; m_i is d_minv[i] (of T), or 1 where d_minv is null.  d_lambda[0],
 * ONE double, receives the largest fl(|m_i| s_i): an integer maximum over the bit patterns of these non-negative doubles, behind
 * a zeroing on the stream, so the result is the same bits on every call and stream.  A row whose product is NaN makes the result
 * NaN (the quiet NaN 0x7ff8000000000000); rows == 0 stores +0.0.
 *
 * COEFFS.  One lane reads d_lambda[0] on the device and writes 2 degree doubles, 1 <= degree <= SPMV_HIP_CHEBY_MAX_DEGREE, with
 * exactly these roundings:
 *     lmax = fl(scale lambda[0]);  lmin = fl(lmax / ratio)
 *     theta = fl(fl(lmax + lmin) 0.5);  delta = fl(fl(lmax - lmin) 0.5);  sigma = fl(theta / delta)
 *     rho_0 = fl(1 / sigma);  coef[0] = +0.0;  coef[1] = fl(1 / theta)
 *     j >= 1:  rho_j = fl(1 / fl(fl(2 sigma) - rho_{j-1}));  coef[2j] = fl(rho_j rho_{j-1});  coef[2j + 1] = fl(fl(2 rho_j) / delta)
 * scale and ratio are host doubles: finite, scale > 0 (1 for a true bound such as the Gershgorin one; 1.05 ... 1.1 for an
 * estimate from below), ratio > 1 (lmax / lmin: 10 ... 30 is usual; the polynomial need not reach the smallest eigenvalue).  A
 * lambda[0] of 0 or NaN gives what IEEE gives; it is not special-cased.
 * The table layout is public: entry j is the pair {coef[2j], coef[2j + 1]} that step j reads, and the first 2 k doubles of the
 * table of a degree are the table of degree k.  A caller may fill the table themselves, or d_lambda from an estimate of their
 * own.  A power iteration on A M^-1, which has the eigenvalues of M^-1 A, composes from existing calls: q = A vhat with
 * dots = {q'q, v'q} by spmv_hip_csr_spmv_*_scaled_dots (alpha 1, beta 0, w = v); 1 / ||q|| by spmv_hip_gmres_start (state[1]);
 * q <- q / ||q|| and vhat <- M^-1 q by spmv_hip_gmres_scale_*, q and v changing places.  For the unit vector v, dots[1] is the
 * Rayleigh quotient, an estimate from below: spmv_hip_cheby_coeffs takes d_lambda = &dots[1] with a scale of 1.1 or so.
 *
 * STEP j of `degree`, c = coef[2j] and e = coef[2j + 1] read by the kernel, s_i = fl(m_i u_i), or u_i where d_minv is null (u is
 * preconditioned already):
 *     j == 0:           d_i = fl(e s_i), z_i = d_i; neither d nor z is read.  The caller passes u = r.
 *     j > 0:            d_i = fl(fl(c d_i) + fl(e s_i)), z_i <- fl_T(z_i + d_i) with the fp64 d_i, before its own rounding to T.
 *                       The caller passes u = r - A z: spmv_hip_csr_spmv_*_scaled(alpha -1, beta 1, y_in = r, y_out = u).
 *     j == degree - 1:  d is not stored.  At degree == 1 d_d is not looked at and may be null.
 * The dots, only at j == degree - 1 and from z AS STORED (a float z: after its rounding): dots[0] = sum_i fl(z_i r_i), dots[1] =
 * sum_i fl(z_i z_i).  Summation order, workspace (spmv_hip_krylov_workspace(n)) and reduction are those of spmv_hip_cg_step_*
 * (spmv_hip_krylov.h).  d_r, d_dots and d_work are all null (no sums are formed, no reduction is launched) or all given; d_u ==
 * d_r is valid, both are only read.  Consequence: with the table {0, 1} at degree 1 in doubles, dots[0] is bit for bit dots[1] of
 * spmv_hip_cg_step_f64 over the same r and minv.  n == 0: with dots, +0.0, +0.0 are stored (one reduction over no slots);
 * otherwise nothing is launched.  A null array has no load and no store.
 * One application costs degree - 1 multiplies and degree updates of 2 ... 6 vector passes each.
 *
 * Composition (no existing call changes):
 *
 *   PCG is the composition of spmv_hip_bjacobi.h with its apply replaced by the polynomial; element [0] of rz_old / rz_new is r'z:
 *     q = A p, pq = {q'q, p'q}      spmv_hip_csr_spmv_*_scaled_dots(alpha 1, beta 0, w = p, dots = pq)
 *     x += a p, r -= a q            spmv_hip_cg_step_*(d_minv null, num = &rz_old[0], den = &pq[1], dots = its own pair {r'r, 0})
 *     z = p(M^-1 A) M^-1 r          spmv_hip_cheby_step_*(j = 0, d_u = r), then for j = 1 ... degree - 1:
 *                                       u = r - A z      spmv_hip_csr_spmv_*_scaled(alpha -1, beta 1, x = z, y_in = r, y_out = u)
 *                                       spmv_hip_cheby_step_*(j, d_u = u)
 *                                   the last of them with d_r = r, d_dots = rz_new and the workspace
 *     p = z + b p                   spmv_hip_cg_direction_*(d_r = z, d_minv null, num = &rz_new[0], den = &rz_old[0])
 *
 *   Point-block Jacobi inside (spmv_hip_bjacobi.h): s = M^-1 u comes from spmv_hip_bjacobi_apply_*(d_r = u, d_z = s, d_dots null,
 *   d_work null) in front of every step, the step gets d_u = s and d_minv null, and lambda is a bound or an estimate of
 *   lambda_max(M^-1 A) of the caller's (the row sums of this header's bound do not see the blocks).
 *
 *   Right-preconditioned BiCGStab and GMRES: the hatted vector (shat, phat, vhat) is the polynomial's z, the steps run without
 *   dots, and spmv_hip_bicgstab_s_*, spmv_hip_bicgstab_direction_*, spmv_hip_gmres_scale_* and spmv_hip_gmres_correct_* get
 *   d_minv null.  The correction at the end of a GMRES cycle: u = V y by spmv_hip_gmres_correct_* into a zeroed u, z the polynomial
 *   of u, then x += z by spmv_hip_bjacobi_apply_add_*(b = 1, d_inv an array of ones, d_u = z).
 *
 * Refusals (checked before the first HIP call: nothing is launched, nothing is written): SPMV_HIP_ERR_INVALID for n (rows) < 0,
 * degree outside 1 ... SPMV_HIP_CHEBY_MAX_DEGREE, j outside 0 ... degree - 1, a scale or ratio that is not finite, scale <= 0,
 * ratio <= 1, a null required pointer (every one but stream, d_minv, the three d_r, d_dots, d_work, and d_d at degree == 1; also
 * where n == 0), one or two of d_r, d_dots, d_work null, dots asked for where j != degree - 1, work_bytes below
 * spmv_hip_krylov_workspace(n), n sizeof(T) >= 2^32, and a written array (d where j < degree - 1, z, dots, the workspace; the
 * table of coeffs; d_lambda of the bound) overlapping any other array of the call, the table of 2 degree doubles among them (of
 * the bound's value array, whose length the host does not know, the first element); SPMV_HIP_ERR_ALIGN for a vector, dots or the
 * workspace off 16-byte alignment, the table, d_lambda or d_value off 8-byte and d_row_ptr off 4-byte alignment.
 *
 * Callers detect the feature by the presence of the symbols (SPMV_HIP_VERSION is unchanged).
 */
#ifndef SPMV_HIP_CHEBY_H
#define SPMV_HIP_CHEBY_H

#include <stddef.h>

#include "spmv_hip_krylov.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the largest degree: a table is at most 32 doubles */
#define SPMV_HIP_CHEBY_MAX_DEGREE 16

/* d_lambda[0] <- max_i |d_minv[i]| sum_j |a_ij|  (d_minv null: 1) */
int spmv_hip_cheby_bound_f64(int32_t rows, const int32_t *d_row_ptr, const double *d_value, const double *d_minv, double *d_lambda,
                             void *stream);
int spmv_hip_cheby_bound_f32(int32_t rows, const int32_t *d_row_ptr, const double *d_value, const float *d_minv, double *d_lambda,
                             void *stream);

/* d_coef[0 ... 2 degree - 1] <- the recurrence's pairs for [scale lambda[0] / ratio, scale lambda[0]] */
int spmv_hip_cheby_coeffs(int32_t degree, const double *d_lambda, double scale, double ratio, double *d_coef, void *stream);

/* d <- coef[2j] d + coef[2j + 1] M^-1 u, z <- z + d, and (j == degree - 1; d_r, d_dots, d_work not null) d_dots <- { r'z, z'z } */
int spmv_hip_cheby_step_f64(int32_t n, int32_t degree, int32_t j, const double *d_coef, const double *d_u, const double *d_minv, double *d_d,
                            double *d_z, const double *d_r, double *d_dots, void *d_work, size_t work_bytes, void *stream);
int spmv_hip_cheby_step_f32(int32_t n, int32_t degree, int32_t j, const double *d_coef, const float *d_u, const float *d_minv, float *d_d,
                            float *d_z, const float *d_r, double *d_dots, void *d_work, size_t work_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* SPMV_HIP_CHEBY_H */
