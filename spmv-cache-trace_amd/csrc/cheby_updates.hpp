// cheby_updates.hpp -- the Chebyshev polynomial preconditioner (include/spmv_hip_cheby.h).
//
// cheby_step_kernel<T, HASM, MODE> is an element-wise kernel over the cut of krylov_stream.hpp: d <- c d + e (m u), z <- z + d with
// the pair {c, e} read from the table in device memory.  MODE says which of the four arrays d and z are read and stored and whether
// r is read for the sums: an array a mode does not need has no load and no store (kKrylovAbsent).  The sums are kept as the
// conjugate-gradient step keeps them and go to the slot of the chunk (store_wave_dots).  No LDS, no barrier, no atomics.
//
// cheby_bound_kernel and cheby_coeffs_kernel are one-time code.  The bound gives a row to a lane, which adds the row's |a_ij| in
// stored order; the maximum of these non-negative doubles is the integer maximum of their bit patterns (a NaN, made the positive
// quiet one, is above +Inf): a butterfly over the wave, then one integer atomic per wave of a bounded grid onto the double that
// cheby_zero_kernel zeroed on the stream.  The coefficients are one lane's sequential recurrence.
#pragma once

#include "cg_updates.hpp"

namespace spmv {

constexpr int kChebyMaxDegree = 16; // SPMV_HIP_CHEBY_MAX_DEGREE

// first: j == 0 of several steps; middle: 0 < j < degree - 1; last: j == degree - 1 > 0; sole: degree == 1
enum ChebyMode { kChebyFirst = 0, kChebyMiddle = 1, kChebyLast = 2, kChebyLastDots = 3, kChebySole = 4, kChebySoleDots = 5 };

constexpr bool cheby_starts(int mode) { return mode == kChebyFirst || mode == kChebySole || mode == kChebySoleDots; } // j == 0
constexpr bool cheby_dots(int mode) { return mode == kChebyLastDots || mode == kChebySoleDots; }
constexpr int cheby_d_access(int mode)
{
    return mode == kChebyFirst ? kKrylovWrite : mode == kChebyMiddle ? kKrylovUpdate : cheby_starts(mode) ? kKrylovAbsent : kKrylovRead;
}

// one element: what is stored in d and z, and z's two products onto the lane's sums
template <class T, bool HASM, int MODE>
__device__ __forceinline__ void cheby_element(double c, double e, T uv, T mv, T & dv, T & zv, T rv, double * sums)
{
    const double s = HASM ? (double) mv * (double) uv : (double) uv;
    double d = e * s;
    if (!cheby_starts(MODE))
        d = c * (double) dv + d;
    if (cheby_d_access(MODE) & kKrylovWrite)
        dv = (T) d;
    zv = cheby_starts(MODE) ? (T) d : (T) ((double) zv + d);
    if (cheby_dots(MODE)) {
        const double z = (double) zv;
        sums[0] += z * (double) rv;
        sums[1] += z * z;
    }
}

// pair = the table from entry j on: {coef[2j], coef[2j + 1]}.  u and r may be one array (both are only read).
template <class T, bool HASM, int MODE>
__global__ __launch_bounds__(256, 8) void cheby_step_kernel(long long n, const double * __restrict__ pair, const T * u, const T * __restrict__ minv,
                                                            T * __restrict__ d, T * __restrict__ z, const T * r, v2d * __restrict__ slots)
{
    const KrylovWave at = krylov_wave(n);
    if (!at.any)
        return;
    const double c = cheby_starts(MODE) ? 0.0 : pair[0];
    const double e = pair[1];
    double sums[2] = {0.0, 0.0};
    const T * const arrays[] = {u, minv, d, z, r};
    constexpr int D = cheby_d_access(MODE), Z = cheby_starts(MODE) ? kKrylovWrite : kKrylovUpdate;
    // arrays a pass loads: four groups of each in flight per lane up to two arrays, two beyond (cg_direction_kernel: three x 4 spill)
    constexpr int LOADS = 1 + (HASM ? 1 : 0) + (D & kKrylovRead ? 1 : 0) + (Z & kKrylovRead ? 1 : 0) + (cheby_dots(MODE) ? 1 : 0);
    krylov_stream<T, LOADS <= 2 ? 4 : 2, false, kKrylovRead, HASM ? kKrylovRead : kKrylovAbsent, D, Z, cheby_dots(MODE) ? kKrylovRead : kKrylovAbsent>(
        n, at, arrays, [&](T * v) { cheby_element<T, HASM, MODE>(c, e, v[0], v[1], v[2], v[3], v[4], sums); });
    if (cheby_dots(MODE))
        store_wave_dots(slots, (int) at.chunk, sums); // every lane of the wave is active again
}

// lambda <- +0.0: the integer maximum starts from the smallest bit pattern
__global__ void cheby_zero_kernel(unsigned long long * __restrict__ lambda)
{
    if (threadIdx.x == 0)
        lambda[0] = 0ULL;
}

constexpr int kChebyBoundBlocks = 1024; // the bound's grid at the most: 4096 atomics onto lambda

// every lane of the grid takes the rows i, i + the grid's lanes, ...; all lanes reach the butterfly
template <class T, bool HASM>
__global__ __launch_bounds__(256) void cheby_bound_kernel(int rows, const int * __restrict__ row_ptr, const double * __restrict__ value,
                                                          const T * __restrict__ minv, unsigned long long * lambda)
{
    const long long stride = (long long) gridDim.x * 256;
    unsigned long long bits = 0ULL;
    for (long long i = (long long) blockIdx.x * 256 + (int) threadIdx.x; i < rows; i += stride) {
        double s = 0.0;
        const long long end = row_ptr[i + 1];
        for (long long k = row_ptr[i]; k < end; ++k)
            s += fabs(value[k]);
        const double v = HASM ? fabs((double) minv[i]) * s : s;
        const unsigned long long b = v != v ? 0x7ff8000000000000ULL : (unsigned long long) __double_as_longlong(v); // v >= +0.0 otherwise
        bits = b > bits ? b : bits;
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
        const unsigned long long other = __shfl_xor(bits, off, kWave);
        bits = other > bits ? other : bits;
    }
    if (((int) threadIdx.x & (kWave - 1)) == 0 && bits != 0ULL)
        atomicMax(lambda, bits);
}

// the table of include/spmv_hip_cheby.h, every operation rounded on its own
__global__ __launch_bounds__(64) void cheby_coeffs_kernel(int degree, const double * __restrict__ lambda, double scale, double ratio,
                                                          double * __restrict__ coef)
{
    if (threadIdx.x != 0)
        return;
    const double lmax = scale * lambda[0];
    const double lmin = lmax / ratio;
    const double theta = (lmax + lmin) * 0.5, delta = (lmax - lmin) * 0.5;
    const double sigma = theta / delta, twice = 2.0 * sigma;
    double rho = 1.0 / sigma;
    coef[0] = 0.0;
    coef[1] = 1.0 / theta;
    for (int j = 1; j < degree; ++j) {
        const double next = 1.0 / (twice - rho);
        coef[2 * j] = next * rho;
        coef[2 * j + 1] = (2.0 * next) / delta;
        rho = next;
    }
}

} // namespace spmv
