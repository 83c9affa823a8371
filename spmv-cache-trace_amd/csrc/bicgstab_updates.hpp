// bicgstab_updates.hpp -- the three vector updates of a BiCGStab iteration, right-preconditioned by a diagonal, with their scalars
// read from device memory (include/spmv_hip_bicgstab.h): element-wise kernels over the cut of krylov_stream.hpp.  The step keeps
// its two sums in registers and stores them in the slot of its chunk.  An absent array (minv and its hatted output; the step's
// shat) is a template boolean: its variant has no load and no store of it.  bicgstab_direction_kernel keeps its own three paths:
// on krylov_stream its float instantiation with minv needs 64 VGPRs and 20 bytes of scratch.
#pragma once

#include "cg_updates.hpp"

namespace spmv {

// s = r - a v as stored, and what is stored beside it: diag(m) s of the STORED s
template <class T, bool HASM>
__device__ __forceinline__ void bicgstab_s_element(double a, T vv, T mv, T & rv, T & hv)
{
    rv = (T) ((double) rv - a * (double) vv);
    if (HASM)
        hv = (T) ((double) mv * (double) rv);
}

// one element of the step: x and r as stored (r holds s on entry; sv is shat, the incoming r where there is none), and the
// stored r's products onto the lane's sums
template <class T>
__device__ __forceinline__ void bicgstab_step_element(double a, double w, T pv, T sv, T tv, T hv, T & xv, T & rv, double * sums)
{
    xv = (T) (((double) xv + a * (double) pv) + w * (double) sv);
    rv = (T) ((double) rv - w * (double) tv);
    const double rho = (double) rv;
    sums[0] += rho * rho;
    sums[1] += (double) hv * rho;
}

// p = r + b (p - w v) as stored, and diag(m) p of the STORED p beside it
template <class T, bool HASM>
__device__ __forceinline__ void bicgstab_direction_element(double b, double w, T rv, T vv, T mv, T & pv, T & hv)
{
    pv = (T) ((double) rv + b * ((double) pv - w * (double) vv));
    if (HASM)
        hv = (T) ((double) mv * (double) pv);
}

// r <- s = r - a v, shat <- m s
template <class T, bool HASM>
__global__ __launch_bounds__(256, 8) void bicgstab_s_kernel(long long n, const double * __restrict__ num, const double * __restrict__ den, const T * v,
                                                            T * __restrict__ r, const T * minv, T * __restrict__ shat)
{
    const KrylovWave at = krylov_wave(n);
    if (!at.any)
        return;
    const double a = num[0] / den[0];
    const T * const arrays[] = {v, r, minv, shat};
    // six or eight loads in flight per lane
    krylov_stream<T, HASM ? 2 : 4, false, kKrylovRead, kKrylovUpdate, HASM ? kKrylovRead : kKrylovAbsent, HASM ? kKrylovWrite : kKrylovAbsent>(
        n, at, arrays, [&](T * e) { bicgstab_s_element<T, HASM>(a, e[0], e[2], e[1], e[3]); });
}

// x += a phat + w shat, r <- r - w t, slots[chunk] = {sum rho rho, sum rhat rho} over the chunk's r as stored.  HASS false: shat
// is r as it comes in, loaded once for both of its uses.
template <class T, bool HASS>
__global__ __launch_bounds__(256, 8) void bicgstab_step_kernel(long long n, const double * __restrict__ num_a, const double * __restrict__ den_a,
                                                               const double * __restrict__ num_w, const double * __restrict__ den_w, const T * phat,
                                                               const T * shat, const T * t, const T * rhat, T * __restrict__ x, T * __restrict__ r,
                                                               v2d * __restrict__ slots)
{
    // U groups of each of the five or six arrays in flight per lane: two where that fits 64 VGPRs without scratch, which six
    // arrays do not, nor five of floats (four elements of a group widen to eight registers of doubles)
    constexpr int U = HASS || sizeof(T) == 4 ? 1 : 2;
    const KrylovWave at = krylov_wave(n);
    if (!at.any)
        return;
    const double a = num_a[0] / den_a[0];
    const double w = num_w[0] / den_w[0];
    double sums[2] = {0.0, 0.0};
    const T * const arrays[] = {phat, t, rhat, x, r, shat};
    krylov_stream<T, U, true, kKrylovRead, kKrylovRead, kKrylovRead, kKrylovUpdate, kKrylovUpdate, HASS ? kKrylovRead : kKrylovAbsent>(
        n, at, arrays, [&](T * e) { bicgstab_step_element<T>(a, w, e[0], HASS ? e[5] : e[4], e[1], e[2], e[3], e[4], sums); });
    store_wave_dots(slots, (int) at.chunk, sums); // every lane of the wave is active again
}

// p <- r + b (p - w v), phat <- m p
template <class T, bool HASM>
__global__ __launch_bounds__(256, 8) void bicgstab_direction_kernel(long long n, const double * __restrict__ num_r, const double * __restrict__ den_r,
                                                                    const double * __restrict__ num_a, const double * __restrict__ den_a,
                                                                    const double * __restrict__ num_w, const double * __restrict__ den_w, const T * r,
                                                                    const T * v, T * __restrict__ p, const T * minv, T * __restrict__ phat)
{
    typedef typename KrylovGroup<T>::type G;
    constexpr int W = 16 / (int) sizeof(T);
    constexpr int GROUPS = kKrylovChunk / W;
    constexpr int PER_LANE = GROUPS / kWave, U = 2; // six or eight loads in flight per lane
    static_assert(PER_LANE % U == 0, "whole passes");
    const KrylovWave at = krylov_wave(n);
    if (!at.any)
        return;
    const long long chunk = at.chunk;
    const int lane = at.lane();
    const double w = num_w[0] / den_w[0];
    const double b = (num_r[0] / den_r[0]) * ((num_a[0] / den_a[0]) / w);
    const G * rg = reinterpret_cast<const G *>(r);
    const G * vg = reinterpret_cast<const G *>(v);
    const G * mg = reinterpret_cast<const G *>(minv);
    G * pg = reinterpret_cast<G *>(p);
    G * hg = reinterpret_cast<G *>(phat);
    const long long g0 = chunk * GROUPS + lane;
    if ((chunk + 1) * kKrylovChunk <= n) {
#pragma unroll 1
        for (int j = 0; j < PER_LANE; j += U) {
            G vr[U], vv[U], vp[U], vm[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long long g = g0 + (long long) (j + u) * kWave;
                vr[u] = rg[g];
                vv[u] = vg[g];
                vp[u] = pg[g];
                if (HASM)
                    vm[u] = mg[g];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long long g = g0 + (long long) (j + u) * kWave;
                G vh = vp[u];
#pragma unroll
                for (int c = 0; c < W; ++c) {
                    T pv = vp[u][c], hv = (T) 0;
                    bicgstab_direction_element<T, HASM>(b, w, vr[u][c], vv[u][c], HASM ? vm[u][c] : (T) 0, pv, hv);
                    vp[u][c] = pv;
                    vh[c] = hv;
                }
                pg[g] = vp[u];
                if (HASM)
                    hg[g] = vh;
            }
        }
    } else {
        const long long ngroups = n / W;
        for (int j = 0; j < PER_LANE; ++j) {
            const long long g = g0 + (long long) j * kWave;
            if (g < ngroups) {
                const G vr = rg[g], vv = vg[g];
                G vp = pg[g], vm = vp, vh = vp;
                if (HASM)
                    vm = mg[g];
#pragma unroll
                for (int c = 0; c < W; ++c) {
                    T pv = vp[c], hv = (T) 0;
                    bicgstab_direction_element<T, HASM>(b, w, vr[c], vv[c], vm[c], pv, hv);
                    vp[c] = pv;
                    vh[c] = hv;
                }
                pg[g] = vp;
                if (HASM)
                    hg[g] = vh;
            }
        }
        const long long e = ngroups * W + lane;
        if (e < n) {
            T pv = p[e], hv = (T) 0;
            bicgstab_direction_element<T, HASM>(b, w, r[e], v[e], HASM ? minv[e] : (T) 0, pv, hv);
            p[e] = pv;
            if (HASM)
                phat[e] = hv;
        }
    }
}

} // namespace spmv
