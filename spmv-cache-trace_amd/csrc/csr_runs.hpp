// csr_runs.hpp -- stencil row runs: every row of a structured grid that follows one 5-entry pattern, fully or as a subset, in
// chunks of 128 rows, a wave per chunk, the values landing in the wave's LDS by LDS-DMA.  One launch for Poisson.
//
// The tiles this replaces (csr_wavetile.hpp: `stencil_values` -- shifted, uniform, one lane per row, values read as doubles -- and
// the masked stencil tiles of csr_stenciltile.hpp) cost a wave each too, but one of ~102 rows on 64 lanes, found through a
// descriptor PAIR, with its values parked in LDS through VGPRs and ds_write.  The plan (plan_csr.hip, build_stencil_runs) picks
// the 5-entry pattern P of most run rows, takes every such tile whose rows' columns are a subset of {row + P[p]}, and cuts the
// ranges of consecutive taken tiles at absolute multiples of 128 rows; every other tile goes to the LIST variant of
// csr_wavetile_kernel in a second launch (none for Poisson).
//
// Per chunk a lane owns two ADJACENT rows (2l, 2l + 1) as tile_rows_pairs_constant does: x, old y and new y move as one 16-byte
// access per lane and position.  The chunk's values go global -> LDS with 6 `global_load_lds_dwordx4` (128 doubles each, from the
// 16-byte-aligned entry in front of the chunk: a lead of 0 or 1), so they take no VGPRs while in flight and no ds_write.  A full
// chunk's lane reads its rows' values back at `lead + row * 5 + p`; a chunk that holds a row with missing positions has a byte mask
// per row (plan-time side array) and a lane finds its rows' values from a prefix of the mask counts (one DPP scan).  Missing
// positions are skipped, never multiplied by 0; x is read clamped into [0, cols) where a neighbour does not exist.
//
// Sums: z = 0; z += v_p * x_p in column order over the stored positions, then y_in + z -- the plain and masked tiles' expression,
// bit for bit.
//
// P comes as a kernel argument.  NT: the value loads carry `nt` (the values are read once per step, a step moves 4x the
// Infinity Cache; 169 -> 156 us on Poisson 4096^2).  DENSE (chunk c is rows [128 c, 128 c + 128) for every c, and the plan asked
// for it): a wave issues its x and y_in loads before its descriptor returns and only the value stream waits for the first entry --
// measured no faster (155.7 against 155.6 us), so plans leave it off.
//
// A grid of resident waves that each walk many chunks was slower (212 against 180 us on Poisson 4096^2): the dispatcher's refill of
// finished waves hides a chunk's vmcnt(0) better than a fixed set of waves.
#pragma once

#include "csr_wavetile.hpp"

namespace spmv {

constexpr int kRunChunkRows = 128;
constexpr int kRunWaves = 4; // waves per workgroup
constexpr int kRunLen = 5;   // positions of the run pattern
// doubles per wave slot: the lead and 128 rows of 5, in whole LDS-DMA instructions of 128 doubles
constexpr int kRunSlot = (kRunLen + 1) * 128;

// the run pattern by value: row + rel[p] is position p's column, rel ascending
struct RunPattern {
    int rel[kRunLen];
};

// A chunk: {first row, first entry, rows (2 ... 128) | entries << 8, mask slot or -1}; its entries are [first entry, + entries),
// a full chunk's columns rel[p] + row.  A masked chunk's row masks are bytes masks[128 * slot + row] (bit p: position p stored).
__device__ __forceinline__ int4 scalar_load_i4(const int4 * p)
{
    typedef const v4i __attribute__((address_space(4))) * const_ptr;
    const v4i v = *reinterpret_cast<const_ptr>(reinterpret_cast<uintptr_t>(p));
    return make_int4(v[0], v[1], v[2], v[3]);
}

// x[c], x[c + 1] for a lane's two rows; clamped into [0, cols) where either does not exist (the value is then never used)
__device__ __forceinline__ v2d_a8 run_x_pair(const double * __restrict__ x, int c, int cols)
{
    if (c >= 0 && c + 1 < cols)
        return *reinterpret_cast<const v2d_a8 *>(x + c);
    const int top = cols - 1;
    const int ca = c < 0 ? 0 : (c > top ? top : c), cb = c + 1 < 0 ? 0 : (c + 1 > top ? top : c + 1);
    return v2d_a8{x[ca], x[cb]};
}

template <bool NT>
__device__ __forceinline__ void run_values_lds(unsigned slot, const double * __restrict__ a, int e0, int entries, int lane)
{
    const int kb = e0 & ~1;
    const int lastpair = (e0 + entries - 1) & ~1; // lanes past the chunk re-read its last pair into slots nobody reads
#pragma unroll
    for (int i = 0; i <= kRunLen; ++i) {
        const double * src = a + min(kb + 128 * i + 2 * lane, lastpair);
        unsigned keep;
        if (NT)
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off nt\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(src), "s"(slot + 1024u * i) : "memory");
        else
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(src), "s"(slot + 1024u * i) : "memory");
    }
}

// A wave per chunk.  The compiler cannot count the LDS-DMA loads (inline asm), so the wave waits for them with vmcnt(0).
template <bool DENSE, bool NT>
__global__ __launch_bounds__(256) void csr_runs_kernel(int nchunks, int rows, int cols, const int4 * __restrict__ chunks,
                                                       const uint8_t * __restrict__ masks, RunPattern pat, const double * __restrict__ a,
                                                       const double * __restrict__ x, const double * y_in, double * y)
{
    __shared__ __attribute__((aligned(16))) double slots[kRunWaves][kRunSlot];
    const int wave = __builtin_amdgcn_readfirstlane((int) threadIdx.x >> 6);
    const int lane = (int) __lane_id();
    const int c = (int) blockIdx.x * kRunWaves + wave;
    if (c >= nchunks)
        return;
    const double * slot = slots[wave];
    const unsigned lds = __builtin_amdgcn_readfirstlane((unsigned) reinterpret_cast<uintptr_t>((const __attribute__((address_space(3))) double *) slot));
    const int4 d = scalar_load_i4(chunks + c);
    // DENSE: the rows follow from the chunk's number, and x and y_in are on their way before the descriptor is back
    const int row0 = DENSE ? c * kRunChunkRows : d.x;
    const int n = DENSE ? min(kRunChunkRows, rows - row0) : (d.z & 0xFF);
    const int base = min(2 * lane, n - 2);
    v2d_a8 xv[kRunLen];
#pragma unroll
    for (int p = 0; p < kRunLen; ++p)
        xv[p] = run_x_pair(x, row0 + base + pat.rel[p], cols);
    const v2d_a8 yv = __builtin_nontemporal_load(reinterpret_cast<const v2d_a8 *>(y_in + row0 + base));
    const int e0 = d.y, entries = d.z >> 8, mslot = d.w;
    run_values_lds<NT>(lds, a, e0, entries, lane);
    const int lead = e0 & 1;
    double zA = 0.0, zB = 0.0;
    if (mslot < 0) { // every row holds all five positions
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const double * v = slot + lead + base * kRunLen;
#pragma unroll
        for (int p = 0; p < kRunLen; ++p) {
            zA += v[p] * xv[p].x;
            zB += v[kRunLen + p] * xv[p].y;
        }
    } else {
        // rows 2l, 2l + 1 of the lane (none past the chunk); where a row's values start: a prefix of the rows' counts
        const uint8_t * mk = masks + (size_t) mslot * kRunChunkRows;
        const unsigned m0 = 2 * lane < n ? mk[2 * lane] : 0u, m1 = 2 * lane + 1 < n ? mk[2 * lane + 1] : 0u;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int cnt = __builtin_popcount(m0) + __builtin_popcount(m1);
        const int before = wave_inclusive_scan(cnt) - cnt;
        // (an odd chunk's last lane holds rows n - 2, n - 1 and owns only n - 1 = 2l: its row B)
        const bool own_pair = 2 * lane <= n - 2;
        const unsigned mA = own_pair ? m0 : 0u, mB = own_pair ? m1 : m0;
        int kA = lead + before, kB = lead + before + (own_pair ? __builtin_popcount(m0) : 0);
#pragma unroll
        for (int p = 0; p < kRunLen; ++p) {
            if ((mA >> p) & 1u) {
                zA += slot[kA] * xv[p].x;
                ++kA;
            }
            if ((mB >> p) & 1u) {
                zB += slot[kB] * xv[p].y;
                ++kB;
            }
        }
    }
    if (2 * lane <= n - 2) {
        const v2d_a8 out = {yv.x + zA, yv.y + zB};
        __builtin_nontemporal_store(out, reinterpret_cast<v2d_a8 *>(y + row0 + base));
    } else if (2 * lane == n - 1) {
        __builtin_nontemporal_store(yv.y + zB, y + row0 + base + 1);
    }
}

} // namespace spmv
