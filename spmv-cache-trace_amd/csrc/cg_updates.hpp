// cg_updates.hpp -- the vector updates of a conjugate-gradient iteration with their scalar read from device memory
// (include/spmv_hip_krylov.h): streaming kernels shaped as triad_kernel is -- 16-byte loads and stores, several independent loads
// per lane in flight -- over a FIXED cut of the vector: chunk c = elements [c kKrylovChunk, (c + 1) kKrylovChunk) belongs to wave
// c of the grid (four to a workgroup), and lane l of that wave takes the 16-byte groups l, l + 64, ... of the chunk in that order.
// The step keeps its two sums in registers, adds the 64 pairs by one butterfly and stores them in slot c (store_wave_dots,
// csr_dots.hpp); dots_reduce_kernel adds the slots behind it.  No LDS, no barrier, no atomics; every offset is 64-bit.
#pragma once

#include "csr_dots.hpp"

namespace spmv {

constexpr int kKrylovChunk = 1024; // SPMV_HIP_KRYLOV_CHUNK: elements per wave and per slot

template <class T>
struct KrylovGroup;
template <>
struct KrylovGroup<double> {
    typedef v2d type;
};
template <>
struct KrylovGroup<float> {
    typedef v4f type;
};

// one element of the step: what is stored in x and r, and r's products onto the lane's sums
template <class T, bool HASM>
__device__ __forceinline__ void cg_step_element(double a, T pv, T qv, T mv, T & xv, T & rv, double * sums)
{
    xv = (T) ((double) xv + a * (double) pv);
    rv = (T) ((double) rv - a * (double) qv);
    const double v = (double) rv;
    sums[0] += v * v;
    if (HASM)
        sums[1] += ((double) mv * v) * v;
}

template <class T, bool HASM>
__device__ __forceinline__ T cg_direction_element(double b, T rv, T mv, T pv)
{
    const double z = HASM ? (double) mv * (double) rv : (double) rv;
    return (T) (z + b * (double) pv);
}

// x += a p, r -= a q, slots[chunk] = {sum v v, sum (m v) v} over the chunk's r as stored
template <class T, bool HASM>
__global__ __launch_bounds__(256, 8) void cg_step_kernel(long long n, const double * __restrict__ num, const double * __restrict__ den, const T * p,
                                                         const T * q, T * __restrict__ x, T * __restrict__ r, const T * __restrict__ minv,
                                                         v2d * __restrict__ slots)
{
    typedef typename KrylovGroup<T>::type G;
    constexpr int W = 16 / (int) sizeof(T);           // elements of a group
    constexpr int GROUPS = kKrylovChunk / W;          // groups of a chunk
    constexpr int PER_LANE = GROUPS / kWave, U = 2;   // U groups of each of the four or five arrays in flight per lane
    static_assert(PER_LANE % U == 0, "whole passes");
    const int wave = __builtin_amdgcn_readfirstlane((int) threadIdx.x >> 6);
    const long long chunk = (long long) blockIdx.x * 4 + wave;
    if (chunk * kKrylovChunk >= n)
        return; // the whole wave: no slot behind the last element
    const int lane = (int) threadIdx.x & (kWave - 1);
    const double a = num[0] / den[0];
    const G * pg = reinterpret_cast<const G *>(p);
    const G * qg = reinterpret_cast<const G *>(q);
    const G * mg = reinterpret_cast<const G *>(minv);
    G * xg = reinterpret_cast<G *>(x);
    G * rg = reinterpret_cast<G *>(r);
    const long long g0 = chunk * GROUPS + lane;
    double sums[2] = {0.0, 0.0};
    if ((chunk + 1) * kKrylovChunk <= n) {
#pragma unroll 1
        for (int j = 0; j < PER_LANE; j += U) {
            G vp[U], vq[U], vx[U], vr[U], vm[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long long g = g0 + (long long) (j + u) * kWave;
                vp[u] = pg[g];
                vq[u] = qg[g];
                vx[u] = xg[g];
                vr[u] = rg[g];
                if (HASM)
                    vm[u] = mg[g];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long long g = g0 + (long long) (j + u) * kWave;
#pragma unroll
                for (int c = 0; c < W; ++c) {
                    T xv = vx[u][c], rv = vr[u][c];
                    cg_step_element<T, HASM>(a, vp[u][c], vq[u][c], HASM ? vm[u][c] : (T) 0, xv, rv, sums);
                    vx[u][c] = xv;
                    vr[u][c] = rv;
                }
                xg[g] = vx[u];
                rg[g] = vr[u];
            }
        }
    } else { // the last chunk of a vector that does not fill it: whole groups below n, then the elements behind them
        const long long ngroups = n / W;
        for (int j = 0; j < PER_LANE; ++j) {
            const long long g = g0 + (long long) j * kWave;
            if (g < ngroups) {
                const G vp = pg[g], vq = qg[g];
                G vx = xg[g], vr = rg[g], vm = vr;
                if (HASM)
                    vm = mg[g];
#pragma unroll
                for (int c = 0; c < W; ++c) {
                    T xv = vx[c], rv = vr[c];
                    cg_step_element<T, HASM>(a, vp[c], vq[c], vm[c], xv, rv, sums);
                    vx[c] = xv;
                    vr[c] = rv;
                }
                xg[g] = vx;
                rg[g] = vr;
            }
        }
        const long long t = ngroups * W + lane; // fewer than W elements: lanes 0 ... W - 2 at the most
        if (t < n) {
            T xv = x[t], rv = r[t];
            cg_step_element<T, HASM>(a, p[t], q[t], HASM ? minv[t] : (T) 0, xv, rv, sums);
            x[t] = xv;
            r[t] = rv;
        }
    }
    store_wave_dots(slots, (int) chunk, sums); // every lane of the wave is active again
}

// p <- z + b p, z = m r or r: the same cut, no sums
template <class T, bool HASM>
__global__ __launch_bounds__(256, 8) void cg_direction_kernel(long long n, const double * __restrict__ num, const double * __restrict__ den,
                                                              const T * __restrict__ r, const T * __restrict__ minv, T * __restrict__ p)
{
    typedef typename KrylovGroup<T>::type G;
    constexpr int W = 16 / (int) sizeof(T);
    constexpr int GROUPS = kKrylovChunk / W;
    constexpr int PER_LANE = GROUPS / kWave, U = HASM ? 2 : 4; // six or eight loads in flight per lane (three arrays x 4 spill)
    static_assert(PER_LANE % U == 0, "whole passes");
    const int wave = __builtin_amdgcn_readfirstlane((int) threadIdx.x >> 6);
    const long long chunk = (long long) blockIdx.x * 4 + wave;
    if (chunk * kKrylovChunk >= n)
        return;
    const int lane = (int) threadIdx.x & (kWave - 1);
    const double b = num[0] / den[0];
    const G * rg = reinterpret_cast<const G *>(r);
    const G * mg = reinterpret_cast<const G *>(minv);
    G * pg = reinterpret_cast<G *>(p);
    const long long g0 = chunk * GROUPS + lane;
    if ((chunk + 1) * kKrylovChunk <= n) {
#pragma unroll 1
        for (int j = 0; j < PER_LANE; j += U) {
            G vr[U], vp[U], vm[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long long g = g0 + (long long) (j + u) * kWave;
                vr[u] = rg[g];
                vp[u] = pg[g];
                if (HASM)
                    vm[u] = mg[g];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int c = 0; c < W; ++c)
                    vp[u][c] = cg_direction_element<T, HASM>(b, vr[u][c], HASM ? vm[u][c] : (T) 0, vp[u][c]);
                pg[g0 + (long long) (j + u) * kWave] = vp[u];
            }
        }
    } else {
        const long long ngroups = n / W;
        for (int j = 0; j < PER_LANE; ++j) {
            const long long g = g0 + (long long) j * kWave;
            if (g < ngroups) {
                const G vr = rg[g];
                G vp = pg[g], vm = vr;
                if (HASM)
                    vm = mg[g];
#pragma unroll
                for (int c = 0; c < W; ++c)
                    vp[c] = cg_direction_element<T, HASM>(b, vr[c], vm[c], vp[c]);
                pg[g] = vp;
            }
        }
        const long long t = ngroups * W + lane;
        if (t < n)
            p[t] = cg_direction_element<T, HASM>(b, r[t], HASM ? minv[t] : (T) 0, p[t]);
    }
}

} // namespace spmv
