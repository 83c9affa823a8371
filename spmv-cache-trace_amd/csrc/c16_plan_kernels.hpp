// c16_plan_kernels.hpp -- the compact plan of include/spmv_hip_compact.h made from DEVICE columns (include/spmv_hip_compact_device.h):
// the window bases and the codes of every tile, one wave per tile and four waves to a workgroup as in the multiply, from the
// descriptors the host cut out of row_ptr.  Integer work only; no LDS, no scratch, no atomic but the count of columns outside
// [0, cols).  A column is data here and never an address: it is compared, subtracted from and stored in its own entry's slot.
//
// c16_windows_kernel: base[0] is the wave's smallest column, base[w + 1] the smallest column with column - base[w] >= 8192 (a
// difference of two columns in [0, 2^31 - 2]: it cannot overflow).  No sort: at most nine wave minima say whether the tile is
// compact.  A tile of at most kF32Tile entries keeps them in registers, eight to a lane, loaded once and coalesced; a longer one
// is a single row of any length and is read again for every minimum, 64 consecutive entries a trip.
//
// c16_codes_kernel: a lane per quad of four slots, stored as one 8-byte word; the slots of a tile in front of its first entry
// and behind its last are 0, as the multiply's quad loads expect.
#pragma once

#include "csr_compact.hpp"
#include "spmv_hip_compact.h"

namespace spmv {

constexpr int kC16NoColumn = 0x7FFFFFFF; // cols is at most 2^31 - 1, so this is no column of any matrix
constexpr int kC16Span = 1 << kC16OffsetBits;

// a tile's entries in registers: entry k0 + 64 i + lane in c[i]; columns outside [0, cols) are counted and dropped
struct C16RegisterColumns {
    int c[kF32Tile / kWave];
    unsigned bad = 0;
    __device__ __forceinline__ C16RegisterColumns(const int32_t * __restrict__ j, int k0, int k1, int cols, int lane)
    {
#pragma unroll
        for (int i = 0; i < kF32Tile / kWave; ++i) {
            const int o = kWave * i + lane; // (k0 + o is formed only where it is an entry of the tile)
            const bool in_tile = o < k1 - k0;
            const int v = in_tile ? j[k0 + o] : 0;
            const bool out = (unsigned) v >= (unsigned) cols;
            bad += in_tile && out;
            c[i] = in_tile && !out ? v : kC16NoColumn;
        }
    }
    // this lane's smallest column (first), or its smallest with column - base >= 8192
    __device__ __forceinline__ int least(bool first, int base)
    {
        int m = kC16NoColumn;
#pragma unroll
        for (int i = 0; i < kF32Tile / kWave; ++i)
            m = min(m, first || c[i] - base >= kC16Span ? c[i] : kC16NoColumn);
        return m;
    }
};

// a long row: read again on every call, in trips of 64 consecutive entries; the first call counts the columns outside [0, cols)
struct C16RowColumns {
    const int32_t * __restrict__ j;
    int k0, k1, cols, lane;
    unsigned bad = 0;
    __device__ __forceinline__ int least(bool first, int base)
    {
        int m = kC16NoColumn;
        for (unsigned o = (unsigned) lane, n = (unsigned) (k1 - k0); o < n; o += kWave) { // (unsigned: a row may end near 2^31)
            const int v = j[(size_t) k0 + o];
            const bool in = (unsigned) v < (unsigned) cols;
            bad += first && !in;
            m = min(m, in && (first || v - base >= kC16Span) ? v : kC16NoColumn);
        }
        return m;
    }
};

// The windows of one tile: lane w < 8 returns base[w] (a base past the last window repeats the last one), `windows` the number
// the tile needs, 9 standing for more than eight.  A tile without a column in range needs none: windows = 0.
template <class Columns>
__device__ __forceinline__ int c16_tile_windows(Columns & col, int lane, int & windows)
{
    int mine = 0, last = 0, nw = 0;
    int base = __builtin_amdgcn_readfirstlane(wave_min(col.least(true, 0)));
    while (base != kC16NoColumn) { // wave-uniform
        if (nw == SPMV_HIP_C16_WINDOWS) {
            ++nw; // a ninth window: the tile is wide
            break;
        }
        if (lane == nw)
            mine = base;
        last = base;
        ++nw;
        base = __builtin_amdgcn_readfirstlane(wave_min(col.least(false, base)));
    }
    windows = nw;
    return lane < nw ? mine : last;
}

__global__ __launch_bounds__(256) void c16_windows_kernel(int ntiles, const int4 * __restrict__ desc, const int32_t * __restrict__ j,
                                                                 int cols, int * __restrict__ bases, int * __restrict__ windows,
                                                                 unsigned long long * out_of_range)
{
    const int w = (int) blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int) threadIdx.x >> 6);
    const int lane = (int) __lane_id();
    if (w >= ntiles)
        return; // the whole wave leaves
    const int k0 = desc[w].y, k1 = desc[w + 1].y;
    int nw, base;
    unsigned bad;
    if (k1 - k0 <= kF32Tile) { // wave-uniform
        C16RegisterColumns col(j, k0, k1, cols, lane);
        base = c16_tile_windows(col, lane, nw);
        bad = col.bad;
    } else {
        C16RowColumns col{j, k0, k1, cols, lane};
        base = c16_tile_windows(col, lane, nw);
        bad = col.bad;
    }
    // a tile without entries is compact with one window and bases 0; a wide tile's bases are 0 too
    const bool compact = nw <= SPMV_HIP_C16_WINDOWS;
    if (lane < SPMV_HIP_C16_WINDOWS)
        bases[8 * (size_t) w + lane] = compact && nw > 0 ? base : 0;
    if (lane == 0)
        windows[w] = compact ? max(nw, 1) : 0;
    if (bad)
        atomicAdd(out_of_range, (unsigned long long) bad);
}

// the code of `column` among bases that ascend up to the last window and repeat it from there on
__device__ __forceinline__ unsigned c16_code(const int (&b)[SPMV_HIP_C16_WINDOWS], int column)
{
    int win = 0, base = b[0];
#pragma unroll
    for (int i = 1; i < SPMV_HIP_C16_WINDOWS; ++i)
        if (b[i] > b[i - 1] && column >= b[i]) {
            win = i;
            base = b[i];
        }
    return ((unsigned) win << kC16OffsetBits) | (unsigned) (column - base);
}

// desc: the finished descriptors (the compact bit and the first code quad); codes: the plan's stream, 8-byte aligned
__global__ __launch_bounds__(256) void c16_codes_kernel(int ntiles, const int4 * __restrict__ desc, const int * __restrict__ bases,
                                                               const int32_t * __restrict__ j, uint16_t * __restrict__ codes)
{
    const int w = (int) blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int) threadIdx.x >> 6);
    const int lane = (int) __lane_id();
    if (w >= ntiles)
        return;
    const int4 d0 = desc[w];
    const int k0 = d0.y, k1 = desc[w + 1].y, kb = k0 & ~3;
    if (!(d0.z & kC16MetaCompact) || k1 == k0)
        return;
    int b[SPMV_HIP_C16_WINDOWS];
#pragma unroll
    for (int i = 0; i < SPMV_HIP_C16_WINDOWS; ++i)
        b[i] = bases[8 * (size_t) w + i]; // wave-uniform
    v2c * out = reinterpret_cast<v2c *>(codes + 4 * (size_t) (unsigned) d0.w);
    const int quads = ((k1 - 1 - kb) >> 2) + 1;
    for (int q = lane; q < quads; q += kWave) {
        unsigned c[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int k = kb + 4 * q + s;
            c[s] = k >= k0 && k < k1 ? c16_code(b, j[k]) : 0u;
        }
        out[q] = v2c{c[0] | (c[1] << 16), c[2] | (c[3] << 16)};
    }
}

} // namespace spmv
