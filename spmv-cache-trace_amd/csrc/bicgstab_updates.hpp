// bicgstab_updates.hpp -- the three vector updates of a BiCGStab iteration, right-preconditioned by a diagonal, with their scalars
// read from device memory (include/spmv_hip_bicgstab.h).  The kernels are cut as those of cg_updates.hpp are: chunk c = elements
// [c kKrylovChunk, (c + 1) kKrylovChunk) belongs to wave c of the grid (four to a workgroup), lane l of that wave takes the 16-byte
// groups l, l + 64, ... of the chunk in that order; whole chunks run in unrolled passes of U groups per array without a bounds
// test, the last partial chunk in a tested loop with the up to 3 elements behind the last whole group on lanes 0 ... 2.  The step
// keeps its two sums in registers, adds the 64 pairs by one butterfly and stores them in slot c (store_wave_dots, csr_dots.hpp);
// dots_reduce_kernel adds the slots behind it.  No LDS, no barrier, no atomics; every offset is 64-bit.  An absent array (minv
// and its hatted output; the step's shat) is a template boolean: its variant has no load and no store of it.
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
    typedef typename KrylovGroup<T>::type G;
    constexpr int W = 16 / (int) sizeof(T);
    constexpr int GROUPS = kKrylovChunk / W;
    constexpr int PER_LANE = GROUPS / kWave, U = HASM ? 2 : 4; // six or eight loads in flight per lane
    static_assert(PER_LANE % U == 0, "whole passes");
    const int wave = __builtin_amdgcn_readfirstlane((int) threadIdx.x >> 6);
    const long long chunk = (long long) blockIdx.x * 4 + wave;
    if (chunk * kKrylovChunk >= n)
        return;
    const int lane = (int) threadIdx.x & (kWave - 1);
    const double a = num[0] / den[0];
    const G * vg = reinterpret_cast<const G *>(v);
    const G * mg = reinterpret_cast<const G *>(minv);
    G * rg = reinterpret_cast<G *>(r);
    G * hg = reinterpret_cast<G *>(shat);
    const long long g0 = chunk * GROUPS + lane;
    if ((chunk + 1) * kKrylovChunk <= n) {
#pragma unroll 1
        for (int j = 0; j < PER_LANE; j += U) {
            G vv[U], vr[U], vm[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long long g = g0 + (long long) (j + u) * kWave;
                vv[u] = vg[g];
                vr[u] = rg[g];
                if (HASM)
                    vm[u] = mg[g];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long long g = g0 + (long long) (j + u) * kWave;
                G vh = vr[u];
#pragma unroll
                for (int c = 0; c < W; ++c) {
                    T rv = vr[u][c], hv = (T) 0;
                    bicgstab_s_element<T, HASM>(a, vv[u][c], HASM ? vm[u][c] : (T) 0, rv, hv);
                    vr[u][c] = rv;
                    vh[c] = hv;
                }
                rg[g] = vr[u];
                if (HASM)
                    hg[g] = vh;
            }
        }
    } else { // the last chunk of a vector that does not fill it: whole groups below n, then the elements behind them
        const long long ngroups = n / W;
        for (int j = 0; j < PER_LANE; ++j) {
            const long long g = g0 + (long long) j * kWave;
            if (g < ngroups) {
                const G vv = vg[g];
                G vr = rg[g], vm = vr, vh = vr;
                if (HASM)
                    vm = mg[g];
#pragma unroll
                for (int c = 0; c < W; ++c) {
                    T rv = vr[c], hv = (T) 0;
                    bicgstab_s_element<T, HASM>(a, vv[c], vm[c], rv, hv);
                    vr[c] = rv;
                    vh[c] = hv;
                }
                rg[g] = vr;
                if (HASM)
                    hg[g] = vh;
            }
        }
        const long long t = ngroups * W + lane; // fewer than W elements: lanes 0 ... W - 2 at the most
        if (t < n) {
            T rv = r[t], hv = (T) 0;
            bicgstab_s_element<T, HASM>(a, v[t], HASM ? minv[t] : (T) 0, rv, hv);
            r[t] = rv;
            if (HASM)
                shat[t] = hv;
        }
    }
}

// x += a phat + w shat, r <- r - w t, slots[chunk] = {sum rho rho, sum rhat rho} over the chunk's r as stored.  HASS false: shat
// is r as it comes in, loaded once for both of its uses.
template <class T, bool HASS>
__global__ __launch_bounds__(256, 8) void bicgstab_step_kernel(long long n, const double * __restrict__ num_a, const double * __restrict__ den_a,
                                                               const double * __restrict__ num_w, const double * __restrict__ den_w, const T * phat,
                                                               const T * shat, const T * t, const T * rhat, T * __restrict__ x, T * __restrict__ r,
                                                               v2d * __restrict__ slots)
{
    typedef typename KrylovGroup<T>::type G;
    constexpr int W = 16 / (int) sizeof(T);
    constexpr int GROUPS = kKrylovChunk / W;
    // U groups of each of the five or six arrays in flight per lane: two where that fits 64 VGPRs without scratch, which six
    // arrays do not, nor five of floats (four elements of a group widen to eight registers of doubles)
    constexpr int PER_LANE = GROUPS / kWave, U = HASS || sizeof(T) == 4 ? 1 : 2;
    static_assert(PER_LANE % U == 0, "whole passes");
    const int wave = __builtin_amdgcn_readfirstlane((int) threadIdx.x >> 6);
    const long long chunk = (long long) blockIdx.x * 4 + wave;
    if (chunk * kKrylovChunk >= n)
        return; // the whole wave: no slot behind the last element
    const int lane = (int) threadIdx.x & (kWave - 1);
    const double a = num_a[0] / den_a[0];
    const double w = num_w[0] / den_w[0];
    const G * pg = reinterpret_cast<const G *>(phat);
    const G * sg = reinterpret_cast<const G *>(shat);
    const G * tg = reinterpret_cast<const G *>(t);
    const G * hg = reinterpret_cast<const G *>(rhat);
    G * xg = reinterpret_cast<G *>(x);
    G * rg = reinterpret_cast<G *>(r);
    const long long g0 = chunk * GROUPS + lane;
    double sums[2] = {0.0, 0.0};
    if ((chunk + 1) * kKrylovChunk <= n) {
#pragma unroll 1
        for (int j = 0; j < PER_LANE; j += U) {
            G vp[U], vs[U], vt[U], vh[U], vx[U], vr[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long long g = g0 + (long long) (j + u) * kWave;
                vp[u] = pg[g];
                vt[u] = tg[g];
                vh[u] = hg[g];
                vx[u] = xg[g];
                vr[u] = rg[g];
                if (HASS)
                    vs[u] = sg[g];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long long g = g0 + (long long) (j + u) * kWave;
#pragma unroll
                for (int c = 0; c < W; ++c) {
                    T xv = vx[u][c], rv = vr[u][c];
                    bicgstab_step_element<T>(a, w, vp[u][c], HASS ? vs[u][c] : rv, vt[u][c], vh[u][c], xv, rv, sums);
                    vx[u][c] = xv;
                    vr[u][c] = rv;
                }
                xg[g] = vx[u];
                rg[g] = vr[u];
            }
        }
    } else { // the last chunk of a vector that does not fill it: whole groups below n, then the elements behind them
        const long long ngroups = n / W;
#pragma unroll 1
        for (int j = 0; j < PER_LANE; ++j) {
            const long long g = g0 + (long long) j * kWave;
            if (g < ngroups) {
                const G vp = pg[g], vt = tg[g], vh = hg[g];
                G vx = xg[g], vr = rg[g], vs = vr;
                if (HASS)
                    vs = sg[g];
#pragma unroll
                for (int c = 0; c < W; ++c) {
                    T xv = vx[c], rv = vr[c];
                    bicgstab_step_element<T>(a, w, vp[c], vs[c], vt[c], vh[c], xv, rv, sums);
                    vx[c] = xv;
                    vr[c] = rv;
                }
                xg[g] = vx;
                rg[g] = vr;
            }
        }
        const long long e = ngroups * W + lane; // fewer than W elements: lanes 0 ... W - 2 at the most
        if (e < n) {
            T xv = x[e], rv = r[e];
            bicgstab_step_element<T>(a, w, phat[e], HASS ? shat[e] : rv, t[e], rhat[e], xv, rv, sums);
            x[e] = xv;
            r[e] = rv;
        }
    }
    store_wave_dots(slots, (int) chunk, sums); // every lane of the wave is active again
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
    const int wave = __builtin_amdgcn_readfirstlane((int) threadIdx.x >> 6);
    const long long chunk = (long long) blockIdx.x * 4 + wave;
    if (chunk * kKrylovChunk >= n)
        return;
    const int lane = (int) threadIdx.x & (kWave - 1);
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
