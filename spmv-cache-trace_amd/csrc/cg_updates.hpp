// cg_updates.hpp -- the vector updates of a conjugate-gradient iteration with their scalar read from device memory
// (include/spmv_hip_krylov.h): element-wise kernels over the cut of krylov_stream.hpp.  The step keeps its two sums in registers
// and stores them in the slot of its chunk.
#pragma once

#include "krylov_stream.hpp"

namespace spmv {

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
    const KrylovWave at = krylov_wave(n);
    if (!at.any)
        return;
    const double a = num[0] / den[0];
    double sums[2] = {0.0, 0.0};
    const T * const arrays[] = {p, q, x, r, minv};
    // U = 2 groups of each of the four or five arrays in flight per lane
    krylov_stream<T, 2, false, kKrylovRead, kKrylovRead, kKrylovUpdate, kKrylovUpdate, HASM ? kKrylovRead : kKrylovAbsent>(
        n, at, arrays, [&](T * e) { cg_step_element<T, HASM>(a, e[0], e[1], e[4], e[2], e[3], sums); });
    store_wave_dots(slots, (int) at.chunk, sums); // every lane of the wave is active again
}

// p <- z + b p, z = m r or r: no sums
template <class T, bool HASM>
__global__ __launch_bounds__(256, 8) void cg_direction_kernel(long long n, const double * __restrict__ num, const double * __restrict__ den,
                                                              const T * __restrict__ r, const T * __restrict__ minv, T * __restrict__ p)
{
    const KrylovWave at = krylov_wave(n);
    if (!at.any)
        return;
    const double b = num[0] / den[0];
    const T * const arrays[] = {r, p, minv};
    // six or eight loads in flight per lane (three arrays x 4 spill)
    krylov_stream<T, HASM ? 2 : 4, false, kKrylovRead, kKrylovUpdate, HASM ? kKrylovRead : kKrylovAbsent>(
        n, at, arrays, [&](T * e) { e[1] = cg_direction_element<T, HASM>(b, e[0], e[2], e[1]); });
}

} // namespace spmv
