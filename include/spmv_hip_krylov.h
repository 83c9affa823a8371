/*
 * spmv_hip_krylov.h -- the two vector updates of a (preconditioned) conjugate-gradient iteration, with their scalars read from
 * DEVICE memory: what a caller of spmv_hip_dots.h does next with the two doubles that header leaves on the device.
 *
 *     step:       a = num[0] / den[0];   x_i <- fl(x_i + fl(a p_i));   r_i <- fl(r_i - fl(a q_i));   in place, and with v_i the
 *                 r_i AS STORED:   dots[0] = sum_i fl(v_i v_i)                 r' r
 *                                  dots[1] = sum_i fl(fl(m_i v_i) v_i)         r' M^-1 r for the diagonal M^-1 = d_minv
 *                                                                              (+0.0 where d_minv is null)
 *     direction:  b = num[0] / den[0];   p_i <- fl(z_i + fl(b p_i)),   z_i = fl(m_i r_i), or r_i where d_minv is null
 *
 * Same conventions as spmv_hip.h and spmv_hip_dots.h.  T is double (_f64) or float (_f32: the vectors of the c16_f32xy family).
 * All arithmetic is fp64; every product is rounded before it is added (no FMA); a float vector gets ONE rounding to float, at its
 * store.  num / den is one IEEE fp64 division on the device and is not special-cased: den[0] == 0 gives what IEEE gives (Inf or
 * NaN), and that propagates into the vectors and the dots.  num and den are one double each, read by the kernel when it runs.
 *
 * Both calls only enqueue on `stream`: they neither synchronise nor allocate, and may be captured into a graph, where their
 * launches (the step: the update, then one or two small reductions; the direction: one) form a line.  n == 0: the step stores
 * +0.0, +0.0 in dots (one reduction over no slots), the direction launches nothing.
 *
 * Summation order of the dots: fixed, a function of n alone.  The elements are cut into chunks of SPMV_HIP_KRYLOV_CHUNK (1024)
 * consecutive elements; chunk c belongs to one wave, wherever that wave runs.  Lane l of the wave takes the 16-byte groups
 * (2 doubles, 4 floats) l, l + 64, l + 128, ... of the chunk and adds its products in index order to its own pair of sums; the
 * up to 3 elements behind the last whole group of the vector (n not a multiple of 2 or 4) are added last by lanes 0, 1, 2 of the
 * last chunk's wave.  The 64 pairs are added by one butterfly, stored in slot c of the workspace, and the reduction of
 * spmv_hip_dots.h adds the ceil(n / 1024) slots in an order that depends on their number only.  No floating-point atomics and no
 * counters: two identical calls give identical bits, on any stream.
 *
 * Workspace: spmv_hip_krylov_workspace(n, &bytes), a function of n alone (at least 16).  A step writes and then reads its first
 * bytes; two steps that may run at once need a workspace each.
 *
 * A CG iteration in three enqueue-only calls, with nothing read by the host (z = M^-1 r is never stored):
 *
 *     q = A p, pq = {q'q, p'q}      spmv_hip_csr_spmv_*_scaled_dots(alpha 1, beta 0, w = p, dots = pq)
 *     x += a p, r -= a q            spmv_hip_cg_step_*(num = &rz_old[1], den = &pq[1], dots = rz_new)       a = r'z / p'q
 *     p = z + b p                   spmv_hip_cg_direction_*(num = &rz_new[1], den = &rz_old[1])             b = r'z new / old
 *
 * rz_old and rz_new are two step-dots buffers that the caller alternates from one iteration to the next (without a
 * preconditioner, element [0] of each: r'r).  They start with a step over zeroed p and q with num -> 0.0 and den -> 1.0, which
 * leaves x and r as they are and yields {r'r, r'z} of r0; a direction with num -> 0.0, den -> 1.0 over a zeroed p then stores
 * p = z0.
 *
 * Refusals (checked before the first HIP call: nothing is launched, nothing is written): SPMV_HIP_ERR_INVALID for n < 0, a null
 * required pointer (every one but d_minv and stream, also where n == 0), work_bytes below spmv_hip_krylov_workspace,
 * n * sizeof(T) >= 2^32 (kernels for such vectors have never run), a written array (x, r, the direction's p, dots, the workspace)
 * overlapping any other array of the call, and num or den lying inside dots, the workspace or a written vector;
 * SPMV_HIP_ERR_ALIGN for a vector, dots or the workspace off 16-byte alignment and num or den off 8-byte alignment.  p == q and
 * num == den are valid: they are only read.
 *
 * Callers detect the feature by the presence of the symbols (SPMV_HIP_VERSION is unchanged).
 */
#ifndef SPMV_HIP_KRYLOV_H
#define SPMV_HIP_KRYLOV_H

#include <stddef.h>

#include "spmv_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* consecutive elements of one wave, and of one slot of the workspace (doubles and floats alike) */
#define SPMV_HIP_KRYLOV_CHUNK 1024

/* the bytes of workspace a step over n elements needs: a function of n alone, >= 16, never decreasing in n */
int spmv_hip_krylov_workspace(int32_t n, size_t *bytes);

/* x += a p, r -= a q with a = d_num[0] / d_den[0], and d_dots <- { r'r, r' diag(d_minv) r } of the new r */
int spmv_hip_cg_step_f64(int32_t n, const double *d_num, const double *d_den, const double *d_p, const double *d_q, double *d_x,
                         double *d_r, const double *d_minv, double *d_dots, void *d_work, size_t work_bytes, void *stream);
int spmv_hip_cg_step_f32(int32_t n, const double *d_num, const double *d_den, const float *d_p, const float *d_q, float *d_x,
                         float *d_r, const float *d_minv, double *d_dots, void *d_work, size_t work_bytes, void *stream);

/* p <- z + b p with b = d_num[0] / d_den[0] and z = diag(d_minv) r (d_minv null: z = r) */
int spmv_hip_cg_direction_f64(int32_t n, const double *d_num, const double *d_den, const double *d_r, const double *d_minv,
                              double *d_p, void *stream);
int spmv_hip_cg_direction_f32(int32_t n, const double *d_num, const double *d_den, const float *d_r, const float *d_minv,
                              float *d_p, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* SPMV_HIP_KRYLOV_H */
