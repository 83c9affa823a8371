/*
 * spmv_hip_bicgstab.h -- the three vector updates of a BiCGStab iteration (van der Vorst), right-preconditioned by a diagonal
 * M^-1 = d_minv, with their scalars read from DEVICE memory: what spmv_hip_krylov.h is to a symmetric positive definite system,
 * for a nonsymmetric or indefinite one.  Hatted vectors are M^-1 times the plain ones; without a preconditioner (d_minv null) they
 * ARE the plain ones and nothing extra is stored.
 *
 *     s:          a = num[0] / den[0];   r_i <- s_i = fl(r_i - fl(a v_i)) in place;   with d_minv: shat_i = fl(m_i s_i), s_i AS STORED
 *     step:       a = num_a[0] / den_a[0], w = num_w[0] / den_w[0];   r holds s on entry
 *                 x_i <- fl(fl(x_i + fl(a phat_i)) + fl(w shat_i));   r_i <- fl(s_i - fl(w t_i));   in place, and with rho_i the
 *                 r_i AS STORED:   dots[0] = sum_i fl(rho_i rho_i)             r' r
 *                                  dots[1] = sum_i fl(rhat_i rho_i)            rhat' r
 *                 d_shat null: shat is r as it comes in (the s of the call before), read once
 *     direction:  w = num_w[0] / den_w[0];   b = fl(fl(num_r[0] / den_r[0]) fl(fl(num_a[0] / den_a[0]) / w))
 *                 p_i <- fl(r_i + fl(b fl(p_i - fl(w v_i)))) in place;   with d_minv: phat_i = fl(m_i p_i), p_i AS STORED
 *
 * Same conventions as spmv_hip_krylov.h.  T is double (_f64) or float (_f32: the vectors of the c16_f32xy family).  All arithmetic
 * is fp64; every product, quotient and sum is rounded on its own (no FMA); a float vector gets ONE rounding to float, at its store,
 * and the hatted outputs and the dots are formed from the values as stored.  No quotient is special-cased: a zero denominator
 * gives what IEEE gives (Inf or NaN), and that propagates into the vectors and the dots -- this is how a breakdown of the
 * iteration (rhat' v == 0, t' t == 0, rhat' r == 0) shows itself to the caller.  Every scalar is one double, read by the kernel
 * when it runs.
 *
 * The calls only enqueue on `stream`: they neither synchronise nor allocate, and may be captured into a graph, where their
 * launches (s and the direction: one; the step: the update, then one or two small reductions) form a line.  n == 0: s and the
 * direction launch nothing, the step stores +0.0, +0.0 in dots (one reduction over no slots).
 *
 * Summation order of the step's dots: that of spmv_hip_cg_step_*, a function of n alone.  The elements are cut into chunks of
 * SPMV_HIP_KRYLOV_CHUNK (1024) consecutive elements; chunk c belongs to one wave, wherever that wave runs.  Lane l of the wave
 * takes the 16-byte groups (2 doubles, 4 floats) l, l + 64, l + 128, ... of the chunk and adds its products in index order to its
 * own pair of sums; the up to 3 elements behind the last whole group of the vector are added last by lanes 0, 1, 2 of the last
 * chunk's wave.  The 64 pairs are added by one butterfly, stored in slot c of the workspace, and the reduction of spmv_hip_dots.h
 * adds the ceil(n / 1024) slots in an order that depends on their number only.  No floating-point atomics and no counters: two
 * identical calls give identical bits, on any stream.
 *
 * Workspace of the step: spmv_hip_krylov_workspace(n, &bytes) -- the same rule, the same slots.  A step writes and then reads its
 * first bytes; two steps that may run at once need a workspace each.
 *
 * A BiCGStab iteration in five enqueue-only calls, with nothing read by the host:
 *
 *     v = A phat, vv = {v'v, rhat'v}        spmv_hip_csr_spmv_*_scaled_dots(alpha 1, beta 0, x = phat, w = rhat, dots = vv)
 *     r <- s = r - a v, shat = M^-1 s       spmv_hip_bicgstab_s_*(num = &rho_old[1], den = &vv[1])                 a = rhat'r / rhat'v
 *     t = A shat, ts = {t't, s't}           spmv_hip_csr_spmv_*_scaled_dots(alpha 1, beta 0, x = shat, w = r, dots = ts)
 *     x += a phat + w shat, r <- s - w t    spmv_hip_bicgstab_step_*(num_a = &rho_old[1], den_a = &vv[1], num_w = &ts[1],
 *                                               den_w = &ts[0], dots = rho_new)                                    w = s't / t't
 *     p <- r + b (p - w v), phat = M^-1 p   spmv_hip_bicgstab_direction_*(num_r = &rho_new[1], den_r = &rho_old[1], the step's
 *                                               four scalars)                           b = (rhat'r new / old) (a / w)
 *
 * (without a preconditioner phat is p and shat is r: the multiplies read p and r, the step gets d_phat = p and d_shat = null.)
 * rho_old and rho_new are two step-dots buffers that the caller alternates from one iteration to the next.  Given r = b - A x0 and
 * rhat a copy of it, they start with a step over zeroed phat and t with both quotients 0.0 / 1.0, which leaves x and r as they
 * are and yields {r'r, rhat'r} of r0; a direction over zeroed p and v with the quotients 0.0 / 1.0 (r), 1.0 / 1.0 (a) and
 * 1.0 / 1.0 (w) then stores p = r0 (and phat = M^-1 r0).
 *
 * Refusals (checked before the first HIP call: nothing is launched, nothing is written): SPMV_HIP_ERR_INVALID for n < 0, a null
 * required pointer (every one but d_minv, d_shat, d_phat and stream, also where n == 0), d_minv and the hatted output of s or of
 * the direction not both null or both non-null, work_bytes below spmv_hip_krylov_workspace, n * sizeof(T) >= 2^32 (kernels for
 * such vectors have never run), a written array (r and shat of s; x, r, dots and the workspace of the step; p and phat of the
 * direction) overlapping any other array of the call, and a scalar lying inside dots, the workspace or a written vector;
 * SPMV_HIP_ERR_ALIGN for a vector, dots or the workspace off 16-byte alignment and a scalar off 8-byte alignment.  Scalars that
 * are the same double, and vectors that are only read and are the same array (d_phat == d_rhat in the step, d_v == d_r in the
 * direction), are valid.
 *
 * Callers detect the feature by the presence of the symbols (SPMV_HIP_VERSION is unchanged).
 */
#ifndef SPMV_HIP_BICGSTAB_H
#define SPMV_HIP_BICGSTAB_H

#include <stddef.h>

#include "spmv_hip_krylov.h"

#ifdef __cplusplus
extern "C" {
#endif

/* r <- s = r - a v in place, a = d_num[0] / d_den[0]; with d_minv: d_shat <- diag(d_minv) s (d_shat null iff d_minv null) */
int spmv_hip_bicgstab_s_f64(int32_t n, const double *d_num, const double *d_den, const double *d_v, double *d_r,
                            const double *d_minv, double *d_shat, void *stream);
int spmv_hip_bicgstab_s_f32(int32_t n, const double *d_num, const double *d_den, const float *d_v, float *d_r,
                            const float *d_minv, float *d_shat, void *stream);

/* x += a phat + w shat, r <- r - w t (r holds s on entry), d_dots <- { r'r, rhat'r } of the new r.
 * a = d_num_a[0] / d_den_a[0], w = d_num_w[0] / d_den_w[0].  d_shat null: shat is r as it comes in. */
int spmv_hip_bicgstab_step_f64(int32_t n, const double *d_num_a, const double *d_den_a, const double *d_num_w,
                               const double *d_den_w, const double *d_phat, const double *d_shat, const double *d_t, const double *d_rhat,
                               double *d_x, double *d_r, double *d_dots, void *d_work, size_t work_bytes, void *stream);
int spmv_hip_bicgstab_step_f32(int32_t n, const double *d_num_a, const double *d_den_a, const double *d_num_w,
                               const double *d_den_w, const float *d_phat, const float *d_shat, const float *d_t, const float *d_rhat,
                               float *d_x, float *d_r, double *d_dots, void *d_work, size_t work_bytes, void *stream);

/* p <- r + b (p - w v) in place; with d_minv: d_phat <- diag(d_minv) p (d_phat null iff d_minv null).
 * b = (d_num_r[0] / d_den_r[0]) * ((d_num_a[0] / d_den_a[0]) / (d_num_w[0] / d_den_w[0])), w = d_num_w[0] / d_den_w[0] */
int spmv_hip_bicgstab_direction_f64(int32_t n, const double *d_num_r, const double *d_den_r, const double *d_num_a,
                                    const double *d_den_a, const double *d_num_w, const double *d_den_w, const double *d_r,
                                    const double *d_v, double *d_p, const double *d_minv, double *d_phat, void *stream);
int spmv_hip_bicgstab_direction_f32(int32_t n, const double *d_num_r, const double *d_den_r, const double *d_num_a,
                                    const double *d_den_a, const double *d_num_w, const double *d_den_w, const float *d_r,
                                    const float *d_v, float *d_p, const float *d_minv, float *d_phat, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* SPMV_HIP_BICGSTAB_H */
