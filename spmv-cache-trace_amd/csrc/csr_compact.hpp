// csr_compact.hpp -- y += fl32(A) x with 16-bit column codes (include/spmv_hip_compact.h): csr_f32values_kernel with the column
// stream of a COMPACT tile at 2 bytes per entry.  The tiles, the lanes per row, the products, their LDS parking and the row sums
// are those of csr_f32values.hpp; only where a column comes from differs: per lane and quad ONE 8-byte load of four codes beside
// the 16-byte load of four floats, both quads of a lane issued before anything waits, and
//     column = base[code >> 13] + (code & 0x1FFF)
// with the tile's eight window bases in a per-wave LDS table (one 32-byte vector load and one LDS write per tile).  A tile
// whose columns fit ONE window -- every 2-D mesh, stencil and band -- adds its base to the scalar x pointer instead and gathers
// at the code itself: no table read, no add.  The wave-uniform compact bit of the descriptor sends WIDE tiles down the fp32
// path unchanged (tile_products_f32, long_row_sum_f32 on the caller's 32-bit columns).  No atomics, no workgroup barrier.
#pragma once

#include "csr_f32values.hpp"

namespace spmv {

// descriptor {first row, first entry, meta, first code quad}: csr_f32values_kernel's meta plus two bits that no kTileMeta*
// constant of tile_common.hpp uses (bits 21 and 23)
constexpr int kC16MetaCompact = 1 << 21;   // the tile's columns are codes; otherwise it is wide
constexpr int kC16MetaOneWindow = 1 << 23; // compact, and every column lies in window 0
constexpr int kC16OffsetBits = 13;
constexpr unsigned kC16OffsetMask = (1u << kC16OffsetBits) - 1;

typedef unsigned v2c __attribute__((ext_vector_type(2)));

// ONE: the tile has one window and the caller gathers from x + base[0]: the code is the column
template <bool ONE>
__device__ __forceinline__ int decode(const int * tab, unsigned code)
{
    if (ONE)
        return (int) code;
    return tab[code >> kC16OffsetBits] + (int) (code & kC16OffsetMask);
}

template <bool X32>
__device__ __forceinline__ double gather_code(const double * __restrict__ x, const int * tab, unsigned code)
{
    return gather_x<X32>(x, decode<false>(tab, code));
}

// tile_products_f32 with the four columns of a quad from four codes; ct is the tile's first code quad (its slots in front of
// the tile's first entry and behind its last hold code 0: the tile's smallest column)
template <int QUADS, bool ONE, bool X32>
__device__ __forceinline__ void tile_products_c16(double * prod, const uint16_t * __restrict__ ct, const float * __restrict__ at,
                                                  const double * __restrict__ x, const int * tab, int last, int lane)
{
    v2c c[QUADS];
    v4f v[QUADS];
#pragma unroll
    for (int q = 0; q < QUADS; ++q) {
        int o = 256 * q + 4 * lane;
        o = o < last ? o : last;
        c[q] = *reinterpret_cast<const v2c *>(ct + o);
        v[q] = *reinterpret_cast<const v4f *>(at + o);
    }
#pragma unroll
    for (int q = 0; q < QUADS; ++q) {
        const int o = 256 * q + 4 * lane;
        // every lane decodes (the lanes past the tile's end hold its last quad's codes); only the gathers are predicated
        const int c0 = decode<ONE>(tab, c[q].x & 0xFFFFu), c1 = decode<ONE>(tab, c[q].x >> 16);
        const int c2 = decode<ONE>(tab, c[q].y & 0xFFFFu), c3 = decode<ONE>(tab, c[q].y >> 16);
        if (o <= last) {
            const double q0 = (double) v[q].x * gather_x<X32>(x, c0);
            const double q1 = (double) v[q].y * gather_x<X32>(x, c1);
            const double q2 = (double) v[q].z * gather_x<X32>(x, c2);
            const double q3 = (double) v[q].w * gather_x<X32>(x, c3);
            v2d * dst = reinterpret_cast<v2d *>(prod + o);
            dst[0] = v2d{q0, q1};
            dst[1] = v2d{q2, q3};
        }
    }
}

// long_row_sum_f32 with the columns from codes; cz[k] is the code of entry k (k0 <= k < k1)
template <bool X32>
__device__ __forceinline__ double long_row_sum_c16(const uint16_t * __restrict__ cz, const int * tab, const float * __restrict__ a,
                                                   const double * __restrict__ x, int k0, int k1, int lane)
{
    double z0 = 0.0, z1 = 0.0, z2 = 0.0, z3 = 0.0;
    const int ka = (k0 + 3) & ~3, kz = k1 & ~3;
    if (ka >= kz) {
        for (int k = k0 + lane; k < k1; k += kWave)
            z0 += (double) a[k] * gather_code<false>(x, tab, cz[k]);
        return group_sum<kWave>(z0);
    }
    if (lane < ka - k0)
        z0 += (double) a[k0 + lane] * gather_code<false>(x, tab, cz[k0 + lane]);
    if (lane >= 4 && lane - 4 < k1 - kz)
        z1 += (double) a[kz + lane - 4] * gather_code<false>(x, tab, cz[kz + lane - 4]);
    for (int o = ka + 4 * lane; o < kz; o += 2 * 4 * kWave) {
        const bool two = o + 4 * kWave < kz;
        const int o2 = two ? o + 4 * kWave : o;
        const v2c ca = *reinterpret_cast<const v2c *>(cz + o), cb = *reinterpret_cast<const v2c *>(cz + o2);
        const v4f va = *reinterpret_cast<const v4f *>(a + o), vb = *reinterpret_cast<const v4f *>(a + o2);
        const double xa0 = gather_code<X32>(x, tab, ca.x & 0xFFFFu), xa1 = gather_code<X32>(x, tab, ca.x >> 16);
        const double xa2 = gather_code<X32>(x, tab, ca.y & 0xFFFFu), xa3 = gather_code<X32>(x, tab, ca.y >> 16);
        const double xb0 = gather_code<X32>(x, tab, cb.x & 0xFFFFu), xb1 = gather_code<X32>(x, tab, cb.x >> 16);
        const double xb2 = gather_code<X32>(x, tab, cb.y & 0xFFFFu), xb3 = gather_code<X32>(x, tab, cb.y >> 16);
        z0 += (double) va.x * xa0;
        z1 += (double) va.y * xa1;
        z2 += (double) va.z * xa2;
        z3 += (double) va.w * xa3;
        if (two) {
            z0 += (double) vb.x * xb0;
            z1 += (double) vb.y * xb1;
            z2 += (double) vb.z * xb2;
            z3 += (double) vb.w * xb3;
        }
    }
    return group_sum<kWave>((z0 + z1) + (z2 + z3));
}

template <bool X32>
__global__ __launch_bounds__(256, 8) void csr_compact_kernel(int ntiles, const int4 * __restrict__ desc, const int * __restrict__ bases,
                                                             const uint16_t * __restrict__ codes, const int32_t * __restrict__ p,
                                                             const int32_t * __restrict__ j, const float * __restrict__ a,
                                                             const double * __restrict__ x, double * y, int exact_order)
{
    constexpr int TILE = kF32Tile, QUADS = TILE / 256;
    __shared__ __attribute__((aligned(16))) double prod_all[4][TILE + 4];
    __shared__ int tab_all[4][8];
    const int wave = __builtin_amdgcn_readfirstlane((int) threadIdx.x >> 6);
    const int lane = (int) __lane_id();
    const int w = (int) blockIdx.x * 4 + wave;
    if (w >= ntiles)
        return; // whole wave leaves; no workgroup barrier in this kernel
    double * prod = prod_all[wave];
    int * tab = tab_all[wave];
    const TilePair dp = load_tile_pair(desc, w);
    const int r0 = __builtin_amdgcn_readfirstlane(dp.d0.x);
    const int k0 = __builtin_amdgcn_readfirstlane(dp.d0.y);
    const int meta = __builtin_amdgcn_readfirstlane(dp.d0.z);
    const unsigned quad = (unsigned) __builtin_amdgcn_readfirstlane(dp.d0.w);
    const int r1 = __builtin_amdgcn_readfirstlane(dp.d1.x);
    const int k1 = __builtin_amdgcn_readfirstlane(dp.d1.y);
    const int nrows = r1 - r0;
    const int kb = k0 & ~3;
    const int maxlen = meta & 0xFFFF;
    const int lanes_log2 = (meta >> kTileMetaLanesShift) & 0x7;
    const bool compact = (meta & kC16MetaCompact) != 0; // wave-uniform
    const bool one = (meta & kC16MetaOneWindow) != 0;
    const uint16_t * ct = codes + 4 * (size_t) quad; // the code of entry k is ct[k - kb]
    int base0 = 0;
    if (compact) {
        const int b = bases[8 * (size_t) w + (lane & 7)];
        if (lane < 8)
            tab[lane] = b;
        base0 = __builtin_amdgcn_readfirstlane(b);
        // same-wave LDS operations execute in order; the fences only pin the compiler
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }

    if (meta & kTileMetaFast) {
        // ---- stream tile: rows << lanes_log2 <= 64, not empty, its last quad inside the arrays ----
        const int sub = lane >> lanes_log2;
        const int part = lane & ((1 << lanes_log2) - 1);
        const int rowi = sub < nrows ? sub : nrows - 1;
        int ps, pe;
        if (meta & kTileMetaUniform) { // all rows equally long: row_ptr is not read
            ps = k0 + rowi * maxlen;
            pe = ps + maxlen;
        } else {
            const int32_t * pt = p + r0;
            ps = pt[rowi];
            pe = pt[rowi + 1];
        }
        const double yv = y[r0 + rowi];
        const int last = (k1 - 1 - kb) & ~3;
        if (!compact)
            tile_products_f32<QUADS, X32>(prod, j + kb, a + kb, x, last, lane);
        else if (one)
            tile_products_c16<QUADS, true, X32>(prod, ct, a + kb, x + base0, tab, last, lane);
        else
            tile_products_c16<QUADS, false, X32>(prod, ct, a + kb, x, tab, last, lane);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const int s = ps - kb, e_row = pe - kb;
        double z;
        if (lanes_log2 == 0) { // one lane per row, left to right: the reference's order
            z = tile_row_sum<1>(prod, s, e_row, 0, maxlen);
        } else {
            const int trips = (maxlen + (1 << lanes_log2) - 1) >> lanes_log2;
            switch (lanes_log2) {
            case 1: z = tile_row_sum<2>(prod, s, e_row, part, trips); break;
            case 2: z = tile_row_sum<4>(prod, s, e_row, part, trips); break;
            case 3: z = tile_row_sum<8>(prod, s, e_row, part, trips); break;
            case 4: z = tile_row_sum<16>(prod, s, e_row, part, trips); break;
            case 5: z = tile_row_sum<32>(prod, s, e_row, part, trips); break;
            default: z = tile_row_sum<64>(prod, s, e_row, part, trips); break;
            }
        }
        if (sub < nrows && part == 0)
            y[r0 + sub] = yv + z;
    } else if (k1 - kb <= TILE) {
        // ---- a tile of empty rows, or the tile whose last quad is not whole (the ragged end of the arrays): entry by entry,
        // one lane per row, left to right
        for (int k = k0 + lane; k < k1; k += kWave)
            prod[k - kb] = (double) a[k] * (compact ? gather_code<false>(x, tab, ct[k - kb]) : x[j[k]]);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int r = lane; r < nrows; r += kWave) {
            const int s = p[r0 + r] - kb, e_row = p[r0 + r + 1] - kb;
            double z = 0.0;
            for (int k = s; k < e_row; ++k)
                z += prod[k];
            y[r0 + r] = y[r0 + r] + z;
        }
    } else if (!exact_order) {
        // ---- one row longer than a tile: the whole wave, in registers ----
        const double z = compact ? long_row_sum_c16<X32>(ct - kb, tab, a, x, k0, k1, lane) : long_row_sum_f32<X32>(j, a, x, k0, k1, lane);
        if (lane == 0)
            y[r0] = y[r0] + z;
    } else {
        // ---- ... in the reference's order: lane 0 adds tiles of products left to right ----
        double z = 0.0;
        for (int t0 = k0; t0 < k1; t0 += TILE) {
            const int t1 = (t0 + TILE < k1) ? t0 + TILE : k1;
            for (int k = t0 + lane; k < t1; k += kWave)
                prod[k - t0] = (double) a[k] * (compact ? gather_code<false>(x, tab, ct[k - kb]) : x[j[k]]);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            if (lane == 0)
                for (int k = 0; k < t1 - t0; ++k)
                    z += prod[k];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        if (lane == 0)
            y[r0] = y[r0] + z;
    }
}

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
