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
// access per lane and position.  The chunk's values go global -> LDS with 5 `global_load_lds_dwordx4` (128 doubles each, from the
// 16-byte-aligned entry in front of the chunk: a lead of 0 or 1), so they take no VGPRs while in flight and no ds_write.  The
// 640 doubles of a slot hold every entry but the last of a full chunk of 128 rows with a lead of 1; a full chunk's last entry
// comes as one 8-byte load instead, so 4 slots are 20 KiB and 8 workgroups (8 waves per SIMD) fit a CU.  A full chunk's lane
// reads its rows' values back at `lead + row * 5 + p`; a chunk that holds a row with missing positions has a byte mask per row
// (plan-time side array) and a lane finds its rows' values from a prefix of the mask counts (one DPP scan).  Missing positions
// are skipped, never multiplied by 0.
//
// One memory round trip per chunk: once the descriptor is back, the wave issues every load of the chunk -- the value LDS-DMA,
// y_in, the five x pairs, then the last entry or the mask bytes -- from inline asm, with no wait between them, and waits once
// (vmcnt(0)).  Left to hipcc the x loads sat on divergent clamp branches whose waits chained them two by two, and the values went
// out behind them.  x is read as the pair at clamp(c, 0, cols - 2), and the lanes whose column c or c + 1 does
// not exist take the other half of the pair for it: the value a clamp of each column into [0, cols) reads, never used.
//
// Sums: z = 0; z += v_p * x_p in column order over the stored positions, then y_in + z -- the plain and masked tiles' expression,
// bit for bit.
//
// P comes as a kernel argument.  NT: the value loads carry `nt` (the values are read once per step, a step moves 4x the
// Infinity Cache; 169 -> 156 us on Poisson 4096^2).  DENSE (chunk c is rows [128 c, 128 c + 128) for every c, and the plan asked
// for it): the rows follow from the chunk's number, not from the descriptor -- measured no faster, so plans leave it off.
//
// Sweep (round 10): x and y (the next step's y_in) are what a step leaves in the 256 MiB Infinity Cache.  A plan's odd launches
// take the chunks backwards (RunPattern::mirror: whole groups of 8 workgroups mirrored, so a chunk stays on its XCD), and a step
// starts on the rows the step before touched last; with every sweep forward an LRU-like cache that is a little too small holds
// nothing of them by the time they are needed.  YIN_NT / YOUT_NT: `nt` on the y_in load and the y store, the plan's choice.
//
// A grid of resident waves that each walk many chunks was slower (212 against 180 us on Poisson 4096^2): the dispatcher's refill of
// finished waves hides a chunk's vmcnt(0) better than a fixed set of waves.
#pragma once

#include "csr_wavetile.hpp"

namespace spmv {

constexpr int kRunChunkRows = 128;
constexpr int kRunWaves = 4; // waves per workgroup
constexpr int kRunLen = 5;   // positions of the run pattern
// doubles per wave slot: 128 rows of 5 in whole LDS-DMA instructions of 128 doubles (with a lead of 1 a full chunk's last entry
// lies past them: csr_runs_kernel loads it into a register)
constexpr int kRunSlot = kRunLen * 128;

// the run pattern by value: row + rel[p] is position p's column, rel ascending
// `mirror`: 0, or the number G of groups of 8 workgroups in the grid -- workgroup b then takes the chunks of workgroup
// ((G - 1 - (b >> 3)) << 3) | (b & 7): the sweep backwards, every chunk on the XCD (b mod 8) it has in the forward sweep
struct RunPattern {
    int rel[kRunLen];
    int mirror;
};

// A chunk: {first row, first entry, rows (2 ... 128) | entries << 8, mask slot or -1}; its entries are [first entry, + entries),
// a full chunk's columns rel[p] + row.  A masked chunk's row masks are bytes masks[128 * slot + row] (bit p: position p stored).
__device__ __forceinline__ int4 scalar_load_i4(const int4 * p)
{
    typedef const v4i __attribute__((address_space(4))) * const_ptr;
    const v4i v = *reinterpret_cast<const_ptr>(reinterpret_cast<uintptr_t>(p));
    return make_int4(v[0], v[1], v[2], v[3]);
}

// The 5 value LDS-DMA loads: base `ak` (wave-uniform), byte offset o[i] per lane, destination LDS byte address lds[i].  No wait:
// the caller's run_issue_* waits for them.  (s_nop 4: an SGPR operand may come fresh from a VALU readfirstlane.)
template <bool NT>
__device__ __forceinline__ void run_values_lds(const unsigned (&lds)[kRunLen], const double * ak, const unsigned (&o)[kRunLen])
{
    unsigned keep;
#define SPMV_RUN_DMA5(NTS)                                                                                                     \
    "s_nop 4\n\ts_mov_b32 %0, m0\n\t"                                                                                          \
    "s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %6, %11" NTS "\n\t"                                                \
    "s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %7, %11" NTS "\n\t"                                                \
    "s_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %8, %11" NTS "\n\t"                                                \
    "s_mov_b32 m0, %4\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %9, %11" NTS "\n\t"                                                \
    "s_mov_b32 m0, %5\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %10, %11" NTS "\n\t"                                               \
    "s_mov_b32 m0, %0"
    if (NT)
        asm volatile(SPMV_RUN_DMA5(" nt") : "=&s"(keep) : "s"(lds[0]), "s"(lds[1]), "s"(lds[2]), "s"(lds[3]), "s"(lds[4]), "v"(o[0]),
                     "v"(o[1]), "v"(o[2]), "v"(o[3]), "v"(o[4]), "s"(ak) : "memory");
    else
        asm volatile(SPMV_RUN_DMA5("") : "=&s"(keep) : "s"(lds[0]), "s"(lds[1]), "s"(lds[2]), "s"(lds[3]), "s"(lds[4]), "v"(o[0]),
                     "v"(o[1]), "v"(o[2]), "v"(o[3]), "v"(o[4]), "s"(ak) : "memory");
#undef SPMV_RUN_DMA5
}

// y_in, the five x pairs and one more load (`global_load_dwordx2` of a full chunk's last entry, or `global_load_ushort` of a masked
// chunk's two row masks) behind the value loads, then the chunk's one wait: loads and wait in one statement, so hipcc neither waits
// between them nor touches the destinations before the data is there.
#define SPMV_RUN_ISSUE(YNT, LAST)                                                                                                \
    "s_nop 4\n\t"                                                                                                              \
    "global_load_dwordx4 %0, %7, %8" YNT "\n\t"                                                                                 \
    "global_load_dwordx4 %1, %9, %14\n\t"                                                                                      \
    "global_load_dwordx4 %2, %10, %14\n\t"                                                                                     \
    "global_load_dwordx4 %3, %11, %14\n\t"                                                                                     \
    "global_load_dwordx4 %4, %12, %14\n\t"                                                                                     \
    "global_load_dwordx4 %5, %13, %14\n\t" LAST " %6, %15, %16\n\t"                                                            \
    "s_waitcnt vmcnt(0)"
#define SPMV_RUN_ISSUE_FULL(YNT)                                                                                               \
    asm volatile(SPMV_RUN_ISSUE(YNT, "global_load_dwordx2")                                                                    \
                 : "=&v"(yv), "=&v"(xv[0]), "=&v"(xv[1]), "=&v"(xv[2]), "=&v"(xv[3]), "=&v"(xv[4]), "=&v"(last)                \
                 : "v"(yo), "s"(yb), "v"(xo[0]), "v"(xo[1]), "v"(xo[2]), "v"(xo[3]), "v"(xo[4]), "s"(x), "v"(lo), "s"(ak)      \
                 : "memory")
#define SPMV_RUN_ISSUE_MASKED(YNT)                                                                                             \
    asm volatile(SPMV_RUN_ISSUE(YNT, "global_load_ushort")                                                                     \
                 : "=&v"(yv), "=&v"(xv[0]), "=&v"(xv[1]), "=&v"(xv[2]), "=&v"(xv[3]), "=&v"(xv[4]), "=&v"(m2)                  \
                 : "v"(yo), "s"(yb), "v"(xo[0]), "v"(xo[1]), "v"(xo[2]), "v"(xo[3]), "v"(xo[4]), "s"(x), "v"(mo), "s"(mk)      \
                 : "memory")
// YIN_NT: the y_in load carries `nt` (x never does: it is the stream that is to stay in the Infinity Cache)
template <bool YIN_NT>
__device__ __forceinline__ void run_issue_full(v2d_a8 & yv, v2d_a8 (&xv)[kRunLen], double & last, unsigned yo, const double * yb,
                                               const unsigned (&xo)[kRunLen], const double * x, unsigned lo, const double * ak)
{
    if (YIN_NT)
        SPMV_RUN_ISSUE_FULL(" nt");
    else
        SPMV_RUN_ISSUE_FULL("");
}
template <bool YIN_NT>
__device__ __forceinline__ void run_issue_masked(v2d_a8 & yv, v2d_a8 (&xv)[kRunLen], unsigned & m2, unsigned yo, const double * yb,
                                                 const unsigned (&xo)[kRunLen], const double * x, unsigned mo, const uint8_t * mk)
{
    if (YIN_NT)
        SPMV_RUN_ISSUE_MASKED(" nt");
    else
        SPMV_RUN_ISSUE_MASKED("");
}
#undef SPMV_RUN_ISSUE_MASKED
#undef SPMV_RUN_ISSUE_FULL
#undef SPMV_RUN_ISSUE

// A wave per chunk.  hipcc counts none of the chunk's loads (inline asm): run_issue_* waits for all of them at once.
// YIN_NT, YOUT_NT: the y_in load and the y store carry `nt` (round 10's A/B).
template <bool DENSE, bool NT, bool YIN_NT = true, bool YOUT_NT = true>
__global__ __launch_bounds__(256) void csr_runs_kernel(int nchunks, int rows, int cols, const int4 * __restrict__ chunks,
                                                       const uint8_t * __restrict__ masks, RunPattern pat, const double * __restrict__ a,
                                                       const double * __restrict__ x, const double * y_in, double * y)
{
    __shared__ __attribute__((aligned(16))) double slots[kRunWaves][kRunSlot];
    const int wave = __builtin_amdgcn_readfirstlane((int) threadIdx.x >> 6);
    const int lane = (int) __lane_id();
    // (the asm below holds the arguments; the mirrored workgroup number costs three scalar instructions)
    // every kernel argument in one scalar round trip (else hipcc loads them next to their first uses, one wait each)
    asm volatile("" ::"s"(nchunks), "s"(rows), "s"(cols), "s"(chunks), "s"(masks), "s"(pat.rel[0]), "s"(pat.rel[1]), "s"(pat.rel[2]),
                 "s"(pat.rel[3]), "s"(pat.rel[4]), "s"(pat.mirror), "s"(a), "s"(x), "s"(y_in), "s"(y));
    const int b = (int) blockIdx.x;
    const int c = (pat.mirror ? ((pat.mirror - 1 - (b >> 3)) << 3) | (b & 7) : b) * kRunWaves + wave;
    if (c >= nchunks)
        return;
    const double * slot = slots[wave];
    const unsigned lds = __builtin_amdgcn_readfirstlane((unsigned) reinterpret_cast<uintptr_t>((const __attribute__((address_space(3))) double *) slot));
    const int4 d = scalar_load_i4(chunks + c);
    const int row0 = DENSE ? c * kRunChunkRows : d.x;
    const int n = DENSE ? min(kRunChunkRows, rows - row0) : (d.z & 0xFF);
    const int e0 = d.y, entries = d.z >> 8, mslot = d.w;
    const int base = min(2 * lane, n - 2);
    // every address before the first load: the values from the 16-byte-aligned entry kb in front of the chunk (lanes past the
    // chunk re-read its last pair into slots nobody reads) ...
    const int kb = e0 & ~1, lead = e0 & 1;
    const int lastpair = ((e0 + entries - 1) & ~1) - kb;
    unsigned ldsi[kRunLen], vo[kRunLen];
#pragma unroll
    for (int i = 0; i < kRunLen; ++i) {
        ldsi[i] = lds + 1024u * i;
        vo[i] = 8u * (unsigned) min(128 * i + 2 * lane, lastpair);
    }
    // ... and the x pairs at clamp(c, 0, cols - 2) (the plan leaves cols < 2 without runs)
    int cx[kRunLen];
    unsigned xo[kRunLen];
#pragma unroll
    for (int p = 0; p < kRunLen; ++p) {
        cx[p] = row0 + base + pat.rel[p];
        xo[p] = 8u * (unsigned) min(max(cx[p], 0), cols - 2);
    }
    const double * ak = a + kb;
    run_values_lds<NT>(ldsi, ak, vo);
    v2d_a8 yv, xl[kRunLen];
    double zA = 0.0, zB = 0.0;
    if (mslot < 0) { // every row holds all five positions
        double last;
        // (a full chunk's rows hold all five columns: every pair lies inside [0, cols), as loaded)
        run_issue_full<YIN_NT>(yv, xl, last, 8u * (unsigned) base, y_in + row0, xo, x, 8u * (unsigned) (lead + entries - 1), ak);
        const double * v = slot + lead + base * kRunLen;
        // the chunk's last entry is the last row's position 4 (slot index lead + 5 n - 1, past the slot when n = 128, lead = 1)
        const double vlast = base == n - 2 ? last : slot[min(lead + base * kRunLen + 2 * kRunLen - 1, kRunSlot - 1)];
#pragma unroll
        for (int p = 0; p < kRunLen; ++p) {
            zA += v[p] * xl[p].x;
            zB += (p == kRunLen - 1 ? vlast : v[kRunLen + p]) * xl[p].y;
        }
    } else {
        // rows 2l, 2l + 1 of the lane: one 2-byte load (a slot's masks past the chunk's rows are 0)
        unsigned m2;
        run_issue_masked<YIN_NT>(yv, xl, m2, 8u * (unsigned) base, y_in + row0, xo, x, 2u * (unsigned) lane, masks + (size_t) mslot * kRunChunkRows);
        v2d_a8 xv[kRunLen];
#pragma unroll
        for (int p = 0; p < kRunLen; ++p) // a missing column is never used
            xv[p] = v2d_a8{cx[p] > cols - 2 ? xl[p].y : xl[p].x, cx[p] < 0 ? xl[p].x : xl[p].y};
        const unsigned m0 = m2 & 0xFFu, m1 = (m2 >> 8) & 0xFFu;
        const int cnt = __builtin_popcount(m0) + __builtin_popcount(m1);
        const int before = wave_inclusive_scan(cnt) - cnt;
        // (an odd chunk's last lane holds rows n - 2, n - 1 and owns only n - 1 = 2l: its row B)
        const bool own_pair = 2 * lane <= n - 2;
        const unsigned mA = own_pair ? m0 : 0u, mB = own_pair ? m1 : m0;
        int kA = lead + before, kB = lead + before + (own_pair ? __builtin_popcount(m0) : 0);
        // every LDS read at once, one wait (a skipped position's read is in bounds and unused; the empty asm keeps hipcc from
        // sinking the reads into the branches of their sums)
        double vA[kRunLen], vB[kRunLen];
#pragma unroll
        for (int p = 0; p < kRunLen; ++p) {
            vA[p] = slot[min(kA, kRunSlot - 1)];
            vB[p] = slot[min(kB, kRunSlot - 1)];
            kA += (mA >> p) & 1u;
            kB += (mB >> p) & 1u;
        }
        asm volatile("" : "+v"(vA[0]), "+v"(vA[1]), "+v"(vA[2]), "+v"(vA[3]), "+v"(vA[4]), "+v"(vB[0]), "+v"(vB[1]), "+v"(vB[2]), "+v"(vB[3]),
                     "+v"(vB[4]));
#pragma unroll
        for (int p = 0; p < kRunLen; ++p) {
            if ((mA >> p) & 1u)
                zA += vA[p] * xv[p].x;
            if ((mB >> p) & 1u)
                zB += vB[p] * xv[p].y;
        }
    }
    if (2 * lane <= n - 2) {
        const v2d_a8 out = {yv.x + zA, yv.y + zB};
        if (YOUT_NT)
            __builtin_nontemporal_store(out, reinterpret_cast<v2d_a8 *>(y + row0 + base));
        else
            *reinterpret_cast<v2d_a8 *>(y + row0 + base) = out;
    } else if (2 * lane == n - 1) {
        if (YOUT_NT)
            __builtin_nontemporal_store(yv.y + zB, y + row0 + base + 1);
        else
            y[row0 + base + 1] = yv.y + zB;
    }
}

} // namespace spmv
