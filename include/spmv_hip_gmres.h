/*
 * spmv_hip_gmres.h -- the updates of restarted GMRES(m), m <= SPMV_HIP_GMRES_MAX_BASIS, right-preconditioned by a diagonal
 * M^-1 = d_minv, with every scalar read from and written to DEVICE memory: what spmv_hip_bicgstab.h is to a caller whose BiCGStab
 * breaks down or stagnates.  The new vector is orthogonalised against the basis by classical Gram-Schmidt applied twice (CGS2):
 * each pass reads the basis once, whatever k is.
 *
 * The basis is ONE allocation: vector j starts at d_V + j ldv elements, ldv >= n and ldv sizeof(T) a multiple of 16.  The whole
 * basis may exceed 4 GiB (j ldv is 64-bit arithmetic); one vector may not (n sizeof(T) < 2^32, as in the siblings).
 *
 *     project:   h[j] = sum_i fl(V_j[i] w_i) for j < k;   h[k] = sum_i fl(w_i w_i).   0 <= k <= 32, d_h holds k + 1 doubles;
 *                nothing but d_h and the workspace is written.  k == 0 is the plain w' w: a caller starts a cycle with it.
 *     update:    w_i <- fl(...fl(fl(w_i - fl(h_0 V_0[i])) - fl(h_1 V_1[i])) ... - fl(h_{k-1} V_{k-1}[i])) in place, j ascending;
 *                with omega the w AS STORED:   dots[0] = sum_i fl(omega_i omega_i),   dots[1] = +0.0.   d_h holds k doubles.
 *     scale:     v_i <- fl(v_i scale[0]) in place;   with d_minv: vhat_i = fl(m_i v_i), v_i AS STORED
 *     correct:   u_i = fl(...fl(fl(y_0 V_0[i]) + fl(y_1 V_1[i])) ... + fl(y_{k-1} V_{k-1}[i]));
 *                x_i <- fl(x_i + u_i), or with d_minv x_i <- fl(x_i + fl(m_i u_i)).   k == 0 leaves x as it is.
 *
 * Same conventions as spmv_hip_bicgstab.h.  T is double (_f64) or float (_f32).  All arithmetic is fp64; every product, quotient
 * and sum is rounded on its own (no FMA); a float vector gets ONE rounding to float, at its store, and the dots and vhat are formed
 * from the values as stored.  No scalar is special-cased: a zero norm gives what IEEE gives (Inf or NaN) -- this is how a "happy
 * breakdown" (h_{k+1,k} == 0: the solution lies in the space built so far) shows itself to the caller.  d_h, d_y and every scalar
 * are read by the kernels when they run.
 *
 * Every call only enqueues on `stream`: it neither synchronises nor allocates, and may be captured into a graph, where its launches
 * (project and update: the kernel, then one or two small reductions; the others: one) form a line.  n == 0: project stores k + 1
 * times +0.0, update +0.0, +0.0 (one reduction over no slots), scale and correct launch nothing.
 *
 * Summation order of h and of dots[0]: fixed, a function of n alone.  It does not depend on k, on a vector's position j in the
 * basis, or on how the kernel blocks the basis in registers.  The cut is that of spmv_hip_cg_step_*: the elements are cut into
 * chunks of SPMV_HIP_KRYLOV_CHUNK (1024) consecutive elements; chunk c belongs to one wave.  Lane l of the wave takes the 16-byte
 * groups (2 doubles, 4 floats) l, l + 64, l + 128, ... of the chunk and adds its products in index order to ONE sum per basis
 * vector; the up to 3 elements behind the last whole group of the vector are added last by lanes 0, 1, 2 of the last chunk's wave.
 * The 64 sums of a vector are added by one butterfly and stored in the slot of (vector, chunk), and the ceil(n / 1024) slots of
 * each vector are added exactly as the reduction of spmv_hip_dots.h adds that many slots: one stage up to 2048 slots, two beyond.
 * So h[j] of a call over k vectors is bit for bit the h[0] of a call over V_j alone, and h[k] of a project and dots[0] of an
 * update are bit for bit the dots[0] that spmv_hip_cg_step_* returns with the same vector as r (num -> 0.0, den -> 1.0, zeroed
 * p and q).  No floating-point atomics and no counters: two identical calls give identical bits, on any stream.
 *
 * Workspace of project and update: spmv_hip_gmres_workspace(n, k_max, &bytes), a function of n and k_max alone (at least 16,
 * never decreasing in either); a call with k <= k_max needs no more.  A call writes and then reads it; two calls that may run at
 * once need a workspace each.
 *
 * The small calls (one workgroup each, doubles only) keep the Hessenberg bookkeeping of one cycle on the device.  Its state is
 * spmv_hip_gmres_state_doubles(m) doubles, 16-byte aligned:
 *
 *     state[0]                      the current estimate of the residual norm, |g_{k+1}|
 *     state[1]                      the scale for the next spmv_hip_gmres_scale_*: 1 / beta after start, 1 / h_{k+1,k} after column
 *     state[2 ... 2 + m]            g, m + 1 doubles: the right-hand side beta e_1 under the rotations so far
 *     state[3 + m ... 2 + 2m]       the cosines c_0 ... c_{m-1}
 *     state[3 + 2m ... 2 + 3m]      the sines s_0 ... s_{m-1}
 *     state[3 + 3m ...]             R, the triangle column by column: R[i, j], i <= j, is entry j (j + 1) / 2 + i
 *
 *     start:     beta = sqrt(nrm2[0]);   g = beta e_1;   state[0] = beta;   state[1] = 1 / beta
 *     column:    h_j = fl(h1[j] + h2[j]) for j <= k;   h_{k+1} = sqrt(nrm2[0]);   the k stored rotations in order,
 *                (h_i, h_{i+1}) <- (fl(fl(c_i h_i) + fl(s_i h_{i+1})), fl(fl(c_i h_{i+1}) - fl(s_i h_i)));   the new one,
 *                d = sqrt(fl(fl(h_k h_k) + fl(h_{k+1} h_{k+1}))), c_k = h_k / d, s_k = h_{k+1} / d;
 *                R[0 ... k - 1, k] = h,   R[k, k] = fl(fl(c_k h_k) + fl(s_k h_{k+1}));   g_{k+1} = -fl(s_k g_k), g_k <- fl(c_k g_k);
 *                state[0] = |g_{k+1}|;   state[1] = 1 / h_{k+1}.   Only +, -, x, / and sqrt, each rounded.   0 <= k < m.
 *     solve:     y = R[0:k, 0:k]^-1 g[0:k] by back substitution: one thread, rows from k - 1 down, columns ascending,
 *                y_i = fl(fl(...fl(g_i - fl(R[i, i+1] y_{i+1})) ... - fl(R[i, k-1] y_{k-1})) / R[i, i]).   0 <= k <= m.
 *
 * One Arnoldi step, with V_0 ... V_k and vhat = M^-1 V_k ready (without a preconditioner vhat is V_k), in seven enqueue-only
 * calls with nothing read by the host:
 *
 *     V_{k+1} = A vhat                        spmv_hip_csr_spmv_*_scaled(alpha 1, beta 0, y_out = d_V + (k + 1) ldv)
 *     h1 = {V_j' w (j <= k), w' w}            spmv_hip_gmres_project_*(k + 1, w = V_{k+1}, d_h = h1)
 *     w -= V h1                               spmv_hip_gmres_update_*(k + 1, d_h = h1)
 *     h2                                      spmv_hip_gmres_project_*(k + 1, d_h = h2)
 *     w -= V h2, dots = {w' w, 0}             spmv_hip_gmres_update_*(k + 1, d_h = h2, d_dots = dots)
 *     column k, 1 / h_{k+1,k}                 spmv_hip_gmres_column(k, m, h1, h2, d_nrm2 = &dots[0], state)
 *     V_{k+1} *= 1 / h_{k+1,k}, vhat          spmv_hip_gmres_scale_*(d_scale = &state[1], d_v = V_{k+1}, d_minv, d_vhat)
 *
 * and after m steps:
 *
 *     y = R^-1 g                              spmv_hip_gmres_solve(m, m, state, y)
 *     x += M^-1 V y                           spmv_hip_gmres_correct_*(m, d_y = y)
 *     r = b - A x, rr = {r'r, .}              spmv_hip_csr_spmv_*_scaled_dots(alpha -1, beta 1, y_in = b, y_out = V_0, dots = rr)
 *     beta = sqrt(r'r), g = beta e_1          spmv_hip_gmres_start(m, d_nrm2 = &rr[0], state)
 *     V_0 = r / beta, vhat                    spmv_hip_gmres_scale_*(d_scale = &state[1], d_v = V_0, d_minv, d_vhat)
 *
 * Refusals (checked before the first HIP call: nothing is launched, nothing is written): SPMV_HIP_ERR_INVALID for n < 0; k or m
 * outside its range (0 <= k <= 32, 1 <= m <= 32; column: k >= m; solve: k > m); a null required pointer (every one but d_minv,
 * d_vhat, stream, and d_V where k == 0; also where n == 0); ldv < n; ldv sizeof(T) no multiple of 16; d_minv and d_vhat not both
 * null or both non-null; work_bytes below what the call needs; n sizeof(T) >= 2^32; a written array (d_h of project, the
 * workspace; w and dots of update; v and vhat; x; the state of start and column; y of solve) overlapping any other array of the
 * call -- w of an update may not overlap the k vectors that are read, though it may be the vector right behind them -- and a
 * scalar, d_h or d_y lying inside a written array.  SPMV_HIP_ERR_ALIGN for a vector, d_h, d_h1, d_h2, d_y, dots, the state or
 * the workspace off 16-byte alignment and a scalar (d_scale, d_nrm2) off 8-byte alignment.  d_nrm2 == &dots[0] of the update
 * before, and d_scale == &state[1], are the intended uses.
 *
 * Callers detect the feature by the presence of the symbols (SPMV_HIP_VERSION is unchanged).
 */
#ifndef SPMV_HIP_GMRES_H
#define SPMV_HIP_GMRES_H

#include <stddef.h>

#include "spmv_hip_krylov.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the most vectors a call orthogonalises against, and the longest cycle */
#define SPMV_HIP_GMRES_MAX_BASIS 32

/* the bytes of workspace that project and update over n elements and up to k_max vectors need */
int spmv_hip_gmres_workspace(int32_t n, int32_t k_max, size_t *bytes);

/* the doubles of the state of a cycle of m steps (an even number), or SPMV_HIP_ERR_INVALID for m outside 1 ... 32 */
int spmv_hip_gmres_state_doubles(int32_t m);

/* d_h[j] <- V_j' w for j < k, d_h[k] <- w' w */
int spmv_hip_gmres_project_f64(int32_t n, int32_t k, const double *d_V, int64_t ldv, const double *d_w, double *d_h, void *d_work,
                               size_t work_bytes, void *stream);
int spmv_hip_gmres_project_f32(int32_t n, int32_t k, const float *d_V, int64_t ldv, const float *d_w, double *d_h, void *d_work,
                               size_t work_bytes, void *stream);

/* w <- w - sum_j d_h[j] V_j in place, d_dots <- { w'w of the new w, +0.0 } */
int spmv_hip_gmres_update_f64(int32_t n, int32_t k, const double *d_V, int64_t ldv, const double *d_h, double *d_w, double *d_dots,
                              void *d_work, size_t work_bytes, void *stream);
int spmv_hip_gmres_update_f32(int32_t n, int32_t k, const float *d_V, int64_t ldv, const double *d_h, float *d_w, double *d_dots,
                              void *d_work, size_t work_bytes, void *stream);

/* v <- v d_scale[0] in place; with d_minv: d_vhat <- diag(d_minv) v (d_vhat null iff d_minv null) */
int spmv_hip_gmres_scale_f64(int32_t n, const double *d_scale, double *d_v, const double *d_minv, double *d_vhat, void *stream);
int spmv_hip_gmres_scale_f32(int32_t n, const double *d_scale, float *d_v, const float *d_minv, float *d_vhat, void *stream);

/* x <- x + diag(d_minv) sum_j d_y[j] V_j (d_minv null: no diagonal) */
int spmv_hip_gmres_correct_f64(int32_t n, int32_t k, const double *d_V, int64_t ldv, const double *d_y, const double *d_minv,
                               double *d_x, void *stream);
int spmv_hip_gmres_correct_f32(int32_t n, int32_t k, const float *d_V, int64_t ldv, const double *d_y, const float *d_minv,
                               float *d_x, void *stream);

/* the state of a new cycle from d_nrm2[0] = r'r */
int spmv_hip_gmres_start(int32_t m, const double *d_nrm2, double *d_state, void *stream);

/* column k of the cycle from the two projections' h and d_nrm2[0] = w'w of the second update */
int spmv_hip_gmres_column(int32_t k, int32_t m, const double *d_h1, const double *d_h2, const double *d_nrm2, double *d_state,
                          void *stream);

/* d_y[0 ... k - 1] <- the coefficients of the correction after k steps */
int spmv_hip_gmres_solve(int32_t k, int32_t m, const double *d_state, double *d_y, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* SPMV_HIP_GMRES_H */
