// csr_compact.hpp -- y += fl32(A) x with 16-bit column codes (include/spmv_hip_compact.h): the tile of csr_f32values.hpp
// (f32_tile) over the column stream of a COMPACT tile at 2 bytes per entry.  Only the column source differs: per lane and quad
// ONE 8-byte load of four codes beside the 16-byte load of four floats, both quads of a lane issued before anything waits, and
//     column = base[code >> 13] + (code & 0x1FFF)
// with the tile's eight window bases in a per-wave LDS table (one 32-byte vector load and one LDS write per tile).  A tile
// whose columns fit ONE window -- every 2-D mesh, stencil and band -- adds its base to the scalar x pointer instead and gathers
// at the code itself: no table read, no add.  The wave-uniform compact bit of the descriptor sends WIDE tiles to the caller's
// 32-bit columns (WideSource).  No atomics, no workgroup barrier.
//
// csr_compact_f64_kernel is y += A x: the same tile over the caller's fp64 values (ValueQuad<double>: a quad is two
// 16-byte loads, so per lane four value loads and two code loads go out before anything waits; nothing is widened).
//
// csr_compact_f32xy_kernel is y <- fl32(y + fl32(A) x) on FLOAT x and y (include/spmv_hip_compact_f32xy.h): the same tile with
// the vector element type T = float.  A gather is a 4-byte load widened to fp64, the one-window base goes onto a const float *,
// and a row's sum is rounded once where it is stored; the products and the LDS slice are doubles as everywhere.
#pragma once

#include "csr_dots.hpp"

namespace spmv {

// descriptor {first row, first entry, meta, first code quad}: csr_f32values_kernel's meta plus two bits that no kTileMeta*
// constant of tile_common.hpp uses (bits 21 and 23)
constexpr int kC16MetaCompact = 1 << 21;   // the tile's columns are codes; otherwise it is wide
constexpr int kC16MetaOneWindow = 1 << 23; // compact, and every column lies in window 0
constexpr int kC16OffsetBits = 13;
constexpr unsigned kC16OffsetMask = (1u << kC16OffsetBits) - 1;

typedef unsigned v2c __attribute__((ext_vector_type(2)));

// the codes of a compact tile: the stored quad is an 8-byte load of four codes.  ONE: the tile has one window and the caller
// gathers from x + base[0]: the code is the column.  (A tile's slots in front of its first entry and behind its last hold code
// 0: the tile's smallest column.)
template <bool ONE>
struct CodeColumns {
    typedef v2c quad;
    const uint16_t * __restrict__ c;
    const int * tab;
    __device__ __forceinline__ int decode(unsigned code) const
    {
        if (ONE)
            return (int) code;
        return tab[code >> kC16OffsetBits] + (int) (code & kC16OffsetMask);
    }
    __device__ __forceinline__ quad load(int o) const { return *reinterpret_cast<const v2c *>(c + o); }
    __device__ __forceinline__ v4i columns(quad q) const
    {
        return v4i{decode(q.x & 0xFFFFu), decode(q.x >> 16), decode(q.y & 0xFFFFu), decode(q.y >> 16)};
    }
    __device__ __forceinline__ int at(int k) const { return decode(c[k]); }
};

// csr_compact_kernel's source for one tile: its codes (cz[k]: the code of entry k) or, for a wide tile, the caller's columns.
// The choice is wave-uniform and is made around the loops that read quads, nowhere else.
struct CompactSource {
    bool compact, one;
    const uint16_t * __restrict__ cz;
    const int * tab;
    int base0;
    WideSource wide;

    __device__ __forceinline__ int at(int k) const { return compact ? CodeColumns<false>{cz, tab}.at(k) : wide.at(k); }

    template <int QUADS, bool X32, class V, class T>
    __device__ __forceinline__ void products(double * prod, const V * __restrict__ at, const T * __restrict__ x, int kb,
                                             int last, int lane) const
    {
        if (!compact)
            wide.products<QUADS, X32>(prod, at, x, kb, last, lane);
        else if (one)
            quad_products<QUADS, X32>(prod, CodeColumns<true>{cz + kb, tab}, at, x + base0, last, lane);
        else
            quad_products<QUADS, X32>(prod, CodeColumns<false>{cz + kb, tab}, at, x, last, lane);
    }
    template <bool X32, class V, class T>
    __device__ __forceinline__ double long_row(const V * __restrict__ a, const T * __restrict__ x, int k0, int k1, int lane) const
    {
        return compact ? long_row_sum_f32<X32>(CodeColumns<false>{cz, tab}, a, x, k0, k1, lane) : wide.long_row<X32>(a, x, k0, k1, lane);
    }
};

// One wave of any kernel below: its tile's window table into the wave's LDS slot, then the tile over V values and T vectors.
template <bool X32, class V, class T, class Rows>
__device__ __forceinline__ void compact_wave(int ntiles, const int4 * __restrict__ desc, const int * __restrict__ bases,
                                             const uint16_t * __restrict__ codes, const int32_t * __restrict__ p,
                                             const int32_t * __restrict__ j, const V * __restrict__ a, const T * __restrict__ x,
                                             const Rows out, int exact_order)
{
    __shared__ __attribute__((aligned(16))) double prod_all[4][kF32Tile + 4];
    __shared__ int tab_all[4][8];
    const int wave = __builtin_amdgcn_readfirstlane((int) threadIdx.x >> 6);
    const int lane = (int) __lane_id();
    const int w = (int) blockIdx.x * 4 + wave;
    if (w >= ntiles)
        return; // whole wave leaves; no workgroup barrier in this kernel
    const F32Tile t = load_f32_tile(desc, w);
    int * tab = tab_all[wave];
    const bool compact = (t.meta & kC16MetaCompact) != 0; // wave-uniform
    int base0 = 0;
    if (compact) {
        const int b = bases[8 * (size_t) w + (lane & 7)];
        if (lane < 8)
            tab[lane] = b;
        base0 = __builtin_amdgcn_readfirstlane(b);
        wave_lds_fence();
    }
    // the tile's codes start at quad t.w with the slot of entry k0 & ~3
    const CompactSource src{compact, (t.meta & kC16MetaOneWindow) != 0, codes + 4 * (size_t) (unsigned) t.w - (t.k0 & ~3), tab, base0, WideSource{j}};
    f32_tile<X32>(prod_all[wave], t, src, p, a, x, out, exact_order);
}

template <bool X32>
__global__ __launch_bounds__(256, 8) void csr_compact_kernel(int ntiles, const int4 * __restrict__ desc, const int * __restrict__ bases,
                                                             const uint16_t * __restrict__ codes, const int32_t * __restrict__ p,
                                                             const int32_t * __restrict__ j, const float * __restrict__ a,
                                                             const double * __restrict__ x, double * y, int exact_order)
{
    compact_wave<X32>(ntiles, desc, bases, codes, p, j, a, x, AccumulateRows<double>{y}, exact_order);
}

// y += A x: the fp64 values of the caller beside the codes
template <bool X32>
__global__ __launch_bounds__(256, 8) void csr_compact_f64_kernel(int ntiles, const int4 * __restrict__ desc, const int * __restrict__ bases,
                                                                 const uint16_t * __restrict__ codes, const int32_t * __restrict__ p,
                                                                 const int32_t * __restrict__ j, const double * __restrict__ a,
                                                                 const double * __restrict__ x, double * y, int exact_order)
{
    compact_wave<X32>(ntiles, desc, bases, codes, p, j, a, x, AccumulateRows<double>{y}, exact_order);
}

// y <- fl32(y + fl32(A) x): float x and y beside the float values and the codes; X32: cols * 4 < 2^32
template <bool X32>
__global__ __launch_bounds__(256, 8) void csr_compact_f32xy_kernel(int ntiles, const int4 * __restrict__ desc, const int * __restrict__ bases,
                                                                   const uint16_t * __restrict__ codes, const int32_t * __restrict__ p,
                                                                   const int32_t * __restrict__ j, const float * __restrict__ a,
                                                                   const float * __restrict__ x, float * y, int exact_order)
{
    compact_wave<X32>(ntiles, desc, bases, codes, p, j, a, x, AccumulateRows<float>{y}, exact_order);
}

// ---- y_out <- alpha A x + beta y_in (include/spmv_hip_scaled.h): the three kernels above with the scaled epilogue of
// csr_f32values.hpp (ScaledRows); BETA0: beta == 0, y_in is not loaded.  The LDS is the sibling's: compact_wave's.
#define SPMV_C16_SCALED_KERNEL(NAME, V, T)                                                                                                  \
    template <bool X32, bool BETA0>                                                                                                        \
    __global__ __launch_bounds__(256, 8) void NAME(int ntiles, const int4 * __restrict__ desc, const int * __restrict__ bases,            \
                                                   const uint16_t * __restrict__ codes, const int32_t * __restrict__ p,                    \
                                                   const int32_t * __restrict__ j, const V * __restrict__ a, const T * __restrict__ x,     \
                                                   double alpha, double beta, const T * y_in, T * y_out, int exact_order)                  \
    {                                                                                                                                      \
        compact_wave<X32>(ntiles, desc, bases, codes, p, j, a, x, ScaledRows<T, BETA0>{alpha, beta, y_in, y_out}, exact_order);            \
    }
SPMV_C16_SCALED_KERNEL(csr_compact_scaled_kernel, float, double)
SPMV_C16_SCALED_KERNEL(csr_compact_f64_scaled_kernel, double, double)
SPMV_C16_SCALED_KERNEL(csr_compact_f32xy_scaled_kernel, float, float)
#undef SPMV_C16_SCALED_KERNEL

// ---- ... and with the two dots of y_out (include/spmv_hip_dots.h): the epilogue of csr_dots.hpp, then the wave's pair into its
// tile's slot.  compact_wave returns where the wave has no tile; such a wave has no slot either.  HASW: d_w is not null.
#define SPMV_C16_DOTS_KERNEL(NAME, V, T)                                                                                                    \
    template <bool BETA0, bool HASW>                                                                                                       \
    __global__ __launch_bounds__(256, 8) void NAME(int ntiles, const int4 * __restrict__ desc, const int * __restrict__ bases,            \
                                                   const uint16_t * __restrict__ codes, const int32_t * __restrict__ p,                    \
                                                   const int32_t * __restrict__ j, const V * __restrict__ a, const T * __restrict__ x,     \
                                                   double alpha, double beta, const T * y_in, T * y_out, const T * dw,                     \
                                                   v2d * __restrict__ slots, int exact_order)                                              \
    {                                                                                                                                      \
        double sums[2] = {0.0, 0.0};                                                                                                       \
        compact_wave<true>(ntiles, desc, bases, codes, p, j, a, x, ScaledDotRows<T, BETA0, HASW>{alpha, beta, y_in, y_out, dw, sums},      \
                           exact_order);                                                                                                   \
        const int w = (int) blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int) threadIdx.x >> 6);                                      \
        if (w < ntiles)                                                                                                                    \
            store_wave_dots(slots, w, sums);                                                                                               \
    }
SPMV_C16_DOTS_KERNEL(csr_compact_scaled_dots_kernel, float, double)
SPMV_C16_DOTS_KERNEL(csr_compact_f64_scaled_dots_kernel, double, double)
SPMV_C16_DOTS_KERNEL(csr_compact_f32xy_scaled_dots_kernel, float, float)
#undef SPMV_C16_DOTS_KERNEL

// spmv_hip_c16_plan_verify: a wave per tile; every entry of a compact tile decoded and compared with the caller's column
static __global__ __launch_bounds__(256) void c16_verify_kernel(int ntiles, const int4 * __restrict__ desc, const int * __restrict__ bases,
                                                                const uint16_t * __restrict__ codes, const int32_t * __restrict__ j,
                                                                unsigned long long * mismatches)
{
    const int w = (int) blockIdx.x * 4 + ((int) threadIdx.x >> 6);
    const int lane = (int) threadIdx.x & 63;
    if (w >= ntiles)
        return;
    const int4 d0 = desc[w], d1 = desc[w + 1];
    if (!(d0.z & kC16MetaCompact))
        return;
    const int k0 = d0.y, k1 = d1.y, kb = k0 & ~3;
    const uint16_t * ct = codes + 4 * (size_t) (unsigned) d0.w;
    const int * b = bases + 8 * (size_t) w;
    unsigned long long n = 0;
    for (int k = k0 + lane; k < k1; k += kWave) {
        const unsigned code = ct[k - kb];
        n += (b[code >> kC16OffsetBits] + (int) (code & kC16OffsetMask)) != j[k];
    }
    if (n)
        atomicAdd(mismatches, n);
}

} // namespace spmv
