// csr_dots.hpp -- the scaled multiplies with ||y_out||^2 and w' y_out in the same launch (include/spmv_hip_dots.h): a third
// epilogue for f32_tile, ScaledDotRows, which stores what ScaledRows stores and adds the row's two products -- of the value AS
// STORED -- to a pair of sums that the storing lane keeps in registers.  When the wave's tile is done the 64 pairs are added by
// one butterfly (group_sum<64>: all lanes are active again behind f32_tile) and lane 0 writes the tile's pair into slot `tile`
// of the caller's workspace with one 16-byte vector store.  No atomics, no counters, no workgroup barrier and no LDS beyond the
// sibling's in the tile kernels; dots_reduce_kernel, launched behind them, adds the slots in an order that their number fixes.
#pragma once

#include "csr_f32values.hpp"

namespace spmv {

constexpr int kDotsChunk = 2048; // slots per workgroup of dots_reduce_kernel's first stage

// sums points at the storing lane's {sum of v v, sum of w v}: locals of the kernel, registers once the tile is inlined
template <class T, bool BETA0, bool HASW>
struct ScaledDotRows {
    double alpha, beta;
    const T * y_in;
    T * y_out;
    const T * w;
    double * sums;
    __device__ __forceinline__ double old(int i) const
    {
        if (BETA0)
            return 0.0;
        return (double) y_in[i];
    }
    __device__ __forceinline__ void store(int i, double yv, double z) const
    {
        T stored;
        if (BETA0)
            stored = (T) (alpha * z);
        else
            stored = (T) (alpha * z + beta * yv);
        y_out[i] = stored;
        const double v = (double) stored;
        sums[0] += v * v;
        if (HASW)
            sums[1] += (double) w[i] * v;
    }
};

// the wave's pair into its slot; every lane of the wave is active here
__device__ __forceinline__ void store_wave_dots(v2d * __restrict__ slots, int slot, const double * sums)
{
    const double vv = group_sum<kWave>(sums[0]), wv = group_sum<kWave>(sums[1]);
    if ((int) __lane_id() == 0)
        slots[slot] = v2d{vv, wv};
}

template <bool BETA0, bool HASW>
__global__ __launch_bounds__(256, 8) void csr_f32values_scaled_dots_kernel(int ntiles, const int4 * __restrict__ desc, const int32_t * __restrict__ p,
                                                                           const int32_t * __restrict__ j, const float * __restrict__ a,
                                                                           const double * __restrict__ x, double alpha, double beta,
                                                                           const double * y_in, double * y_out, const double * dw,
                                                                           v2d * __restrict__ slots, int exact_order)
{
    __shared__ __attribute__((aligned(16))) double prod_all[4][kF32Tile + 4];
    const int wave = __builtin_amdgcn_readfirstlane((int) threadIdx.x >> 6);
    const int w = (int) blockIdx.x * 4 + wave;
    if (w >= ntiles)
        return; // whole wave leaves; no workgroup barrier in this kernel
    double sums[2] = {0.0, 0.0};
    f32_tile<true>(prod_all[wave], load_f32_tile(desc, w), WideSource{j}, p, a, x,
                   ScaledDotRows<double, BETA0, HASW>{alpha, beta, y_in, y_out, dw, sums}, exact_order);
    store_wave_dots(slots, w, sums);
}

// scaled_rows_only_kernel (csr_f32values.hpp) with the dots of what it stores: a lane per row, a slot per wave (64 rows)
template <class T, bool BETA0, bool ZTERM, bool HASW>
__global__ __launch_bounds__(256) void scaled_rows_only_dots_kernel(int rows, double alpha, double beta, const T * y_in, T * y_out, const T * dw,
                                                                    v2d * __restrict__ slots)
{
    const long long i = (long long) blockIdx.x * 256 + (int) threadIdx.x;
    double sums[2] = {0.0, 0.0};
    if (i < rows) {
        double r = 0.0;
        if (ZTERM)
            r = alpha * 0.0;
        if (!BETA0)
            r = ZTERM ? r + beta * (double) y_in[i] : beta * (double) y_in[i];
        const T stored = (T) r;
        y_out[i] = stored;
        const double v = (double) stored;
        sums[0] += v * v;
        if (HASW)
            sums[1] += (double) dw[i] * v;
    }
    if ((i & ~63LL) < rows) // wave-uniform: the waves behind the last row have no slot
        store_wave_dots(slots, (int) (i >> 6), sums);
}

// The sum of in[b * per_block, min(n, (b + 1) * per_block)) for workgroup b: thread t adds the elements t, t + 256, ... in that
// order, a butterfly per wave, and thread 0 adds the four waves left to right and is the one thread that holds the result.  The
// order depends on n and per_block alone.  One workgroup with per_block >= n is the whole sum (n == 0: +0.0, +0.0).
template <int THREADS>
__device__ __forceinline__ v2d dots_reduce_block(int n, int per_block, const v2d * __restrict__ in, long long b)
{
    static_assert(THREADS == 256, "four waves");
    __shared__ v2d part[THREADS / kWave];
    const long long first = b * per_block;
    const long long rest = (long long) n - first;
    const int count = (int) (rest < per_block ? rest : per_block);
    const v2d * src = in + first;
    double sums[2] = {0.0, 0.0};
    for (int k = (int) threadIdx.x; k < count; k += THREADS) {
        const v2d s = src[k];
        sums[0] += s.x;
        sums[1] += s.y;
    }
    const double a = group_sum<kWave>(sums[0]), c = group_sum<kWave>(sums[1]);
    if (((int) threadIdx.x & (kWave - 1)) == 0)
        part[threadIdx.x >> 6] = v2d{a, c};
    __syncthreads();
    v2d total = v2d{0.0, 0.0};
    if (threadIdx.x == 0) {
        total = part[0];
        for (int q = 1; q < THREADS / kWave; ++q) {
            total.x += part[q].x;
            total.y += part[q].y;
        }
    }
    return total;
}

// out[b] = dots_reduce_block of workgroup b
template <int THREADS>
__global__ __launch_bounds__(THREADS) void dots_reduce_kernel(int n, int per_block, const v2d * __restrict__ in, v2d * __restrict__ out)
{
    const v2d total = dots_reduce_block<THREADS>(n, per_block, in, (long long) blockIdx.x);
    if (threadIdx.x == 0)
        out[blockIdx.x] = total;
}

} // namespace spmv
