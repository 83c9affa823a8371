// csr_multivec.hpp -- Y += A X for K vectors in one pass over the matrix (include/spmv_hip_multivec.h, multivec.hip).
//
// X (cols x ldx) and Y (rows x ldy) are row-major: the K values of row i sit side by side, so one gathered column index
// brings K contiguous doubles of X.  Every lane keeps K fp64 accumulators.
//
// Wave tiles: the plan cuts consecutive rows into tiles of at most 64 / L rows, where L (lanes per row, a power of two) is
// the largest of the tile's rows' own choice (multivec.hip: mv_lanes_for).  The L lanes of a row walk its entries with
// stride L, in order, and meet in the butterfly of group_sum<L>; the first lane adds the K sums to Y.  Rows longer than
// kMvLongRow entries are left out of the tiles: one workgroup each (csr_mv_long_kernel), waves reduced by group_sum<64>
// and then added in wave order.  The order of every sum therefore comes from row lengths alone, never from K, the leading
// dimensions or the other vectors: a K-wide multiply gives, column for column, the bits of K one-wide ones, and no
// atomics touch Y.  With L = 1 (SPMV_HIP_FLAG_EXACT_ORDER: every tile, long rows included) a row is summed left to right
// by one lane, the reference's order.
#pragma once

#include "wave_ops.hpp"

#include <cstdint>

namespace spmv {

constexpr int kMvBlock = 256;                       // four waves per workgroup, each striding the tile list
constexpr int kMvWaves = kMvBlock / kWave;
constexpr int kMvLongBlock = 256;                   // one workgroup per long row
constexpr int kMvEntriesPerLane = 4;                // a row asks for the fewest lanes that leave at most this many entries each
                                                    // (few per lane: the lanes of a row read 4 * L contiguous bytes of columns)
constexpr int kMvLongRow = 4096;                    // rows longer than this get a workgroup (non-exact plans)
constexpr int kMvExactTileEntries = 1024;           // EXACT_ORDER tiles: entries beyond the first row

// tile descriptor: {first row, rows | log2(lanes per row) << 8}
__host__ __device__ constexpr int mv_tile_code(int nrows, int log2_lanes) { return nrows | (log2_lanes << 8); }

// K doubles at p: 16-byte loads when VEC (p 16-byte aligned), 8-byte loads otherwise
template <int K, bool VEC>
__device__ __forceinline__ void mv_load(const double * __restrict__ p, double (&v)[K])
{
    if constexpr (VEC) {
#pragma unroll
        for (int q = 0; q + 1 < K; q += 2) {
            const double2 t = *reinterpret_cast<const double2 *>(p + q);
            v[q] = t.x;
            v[q + 1] = t.y;
        }
        if constexpr (K & 1)
            v[K - 1] = p[K - 1];
    } else {
#pragma unroll
        for (int q = 0; q < K; ++q)
            v[q] = p[q];
    }
}

template <int K, bool VEC>
__device__ __forceinline__ void mv_add_to(double * __restrict__ p, const double (&s)[K])
{
    double v[K];
    mv_load<K, VEC>(p, v);
    if constexpr (VEC) {
#pragma unroll
        for (int q = 0; q + 1 < K; q += 2)
            *reinterpret_cast<double2 *>(p + q) = make_double2(v[q] + s[q], v[q + 1] + s[q + 1]);
        if constexpr (K & 1)
            p[K - 1] = v[K - 1] + s[K - 1];
    } else {
#pragma unroll
        for (int q = 0; q < K; ++q)
            p[q] = v[q] + s[q];
    }
}

template <int K>
__device__ __forceinline__ void mv_zero(double (&v)[K])
{
#pragma unroll
    for (int q = 0; q < K; ++q)
        v[q] = 0.0;
}

// the entries k, k + L, k + 2 L, ... below k1 of one row, U of them per trip: the U column / value loads and the U gathers of
// X are issued before the adds, which keep the entry order
template <int K, bool VEC, int U>
__device__ __forceinline__ void mv_row_part(int k, int k1, int L, const int32_t * __restrict__ j, const double * __restrict__ a,
                                            const double * __restrict__ X, long long ldx, double (&acc)[K])
{
    for (; k < k1; k += U * L) {
        int c[U];
        double v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int e = k + u * L;
            const bool in = e < k1;
            c[u] = in ? __builtin_nontemporal_load(j + e) : 0;
            v[u] = in ? __builtin_nontemporal_load(a + e) : 0.0;
        }
        double xv[U][K];
#pragma unroll
        for (int u = 0; u < U; ++u)
            mv_load<K, VEC>(X + (long long) c[u] * ldx, xv[u]);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (k + u * L < k1) {
#pragma unroll
                for (int q = 0; q < K; ++q)
                    acc[q] += v[u] * xv[u][q];
            }
        }
    }
}

template <int L, int K>
__device__ __forceinline__ void mv_group_sum(double (&acc)[K])
{
#pragma unroll
    for (int q = 0; q < K; ++q)
        acc[q] = group_sum<L>(acc[q]);
}

template <int K>
constexpr int mv_unroll() { return K <= 4 ? 4 : 2; }

template <int K, bool VEC>
__device__ __forceinline__ void mv_tile(int2 d, const int32_t * __restrict__ p, const int32_t * __restrict__ j,
                                        const double * __restrict__ a, const double * __restrict__ X, long long ldx,
                                        double * __restrict__ Y, long long ldy)
{
    const int nrows = d.y & 0xFF;
    const int lg = (d.y >> 8) & 7;
    const int L = 1 << lg;
    const int lane = (int) (threadIdx.x & (kWave - 1));
    const int sub = lane >> lg;
    const int l = lane & (L - 1);
    const bool valid = sub < nrows;
    const int row = d.x + sub;
    int k0 = 0, k1 = 0;
    if (valid) {
        k0 = p[row];
        k1 = p[row + 1];
    }
    double acc[K];
    mv_zero(acc);
    mv_row_part<K, VEC, mv_unroll<K>()>(k0 + l, k1, L, j, a, X, ldx, acc);
    switch (lg) { // uniform over the wave: every lane takes part in the butterfly
    case 0: break;
    case 1: mv_group_sum<2>(acc); break;
    case 2: mv_group_sum<4>(acc); break;
    case 3: mv_group_sum<8>(acc); break;
    case 4: mv_group_sum<16>(acc); break;
    case 5: mv_group_sum<32>(acc); break;
    default: mv_group_sum<64>(acc); break;
    }
    if (valid && l == 0)
        mv_add_to<K, VEC>(Y + (long long) row * ldy, acc);
}

// Needs cols >= 1 when the tile holds entries (masked lanes gather row 0 of X).
template <int K, bool VEC>
__global__ __launch_bounds__(kMvBlock) void csr_mv_tile_kernel(int ntiles, const int2 * __restrict__ tiles, const int32_t * __restrict__ p,
                                                             const int32_t * __restrict__ j, const double * __restrict__ a,
                                                             const double * __restrict__ X, long long ldx, double * __restrict__ Y,
                                                             long long ldy)
{
    // waves stride the tile list (a tile is a few hundred entries: one wave per tile would spend its life starting up)
    for (int t = (int) blockIdx.x * kMvWaves + (int) (threadIdx.x / kWave); t < ntiles; t += (int) gridDim.x * kMvWaves)
        mv_tile<K, VEC>(tiles[t], p, j, a, X, ldx, Y, ldy);
}

// one workgroup per row of long_rows[]: threads stride the row, waves reduce by butterfly, then wave 0's sum + wave 1's + ...
template <int K, bool VEC>
__global__ __launch_bounds__(kMvLongBlock) void csr_mv_long_kernel(const int32_t * __restrict__ long_rows, const int32_t * __restrict__ p,
                                                                 const int32_t * __restrict__ j, const double * __restrict__ a,
                                                                 const double * __restrict__ X, long long ldx, double * __restrict__ Y,
                                                                 long long ldy)
{
    __shared__ double part[kMvLongBlock / kWave][K];
    const int row = long_rows[blockIdx.x];
    const int k0 = p[row], k1 = p[row + 1];
    double acc[K];
    mv_zero(acc);
    mv_row_part<K, VEC, mv_unroll<K>()>(k0 + (int) threadIdx.x, k1, kMvLongBlock, j, a, X, ldx, acc);
    mv_group_sum<kWave>(acc);
    const int w = (int) (threadIdx.x / kWave);
    if ((threadIdx.x & (kWave - 1)) == 0) {
#pragma unroll
        for (int q = 0; q < K; ++q)
            part[w][q] = acc[q];
    }
    __syncthreads();
    if ((int) threadIdx.x < K) {
        const int q = (int) threadIdx.x;
        double s = part[0][q];
        for (int v = 1; v < kMvLongBlock / kWave; ++v)
            s += part[v][q];
        double * yq = Y + (long long) row * ldy + q;
        *yq = *yq + s;
    }
}

} // namespace spmv
