// csr_runs.hpp -- stencil row runs: the interior of a structured grid in chunks of 128 rows, a wave per chunk, the values
// landing in the wave's LDS by LDS-DMA.
//
// The tiles this replaces (csr_wavetile.hpp, `stencil_values`: shifted, uniform, one lane per row, values read as doubles)
// cost a wave each too, but one of ~102 rows on 64 lanes, found through a descriptor PAIR, with its values parked in LDS
// through VGPRs and ds_write.  The plan (plan_csr.hip, build_stencil_runs) merges maximal runs of such tiles that share
// their row length and pattern record and cuts them into chunks of up to 128 rows; every other tile goes to the LIST
// variant of csr_wavetile_kernel in a second launch.
//
// Per chunk a lane owns two ADJACENT rows (2l, 2l + 1) as tile_rows_pairs_constant does: x, old y and new y move as one
// 16-byte access per lane and position.  The chunk's values go global -> LDS with L + 1 `global_load_lds_dwordx4` (128
// doubles each, from the 16-byte-aligned entry in front of the chunk: a lead of 0 or 1), so they take no VGPRs while in
// flight and no ds_write.  The LDS image is lane-linear; a lane reads its rows' values back at `lead + row * L + p`.
//
// Sums: z = 0; z += v_p * x_p in column order, then y_in + z -- the plain tile's expression, bit for bit.
//
// Measured on Poisson 4096^2 (values as doubles): 180 us against 188 for the tiles.  A grid of resident waves that each walk
// many chunks (wave w takes w, w + G, ...) was slower, 212 us: the compiler's own LDS-DMA builtin makes it drain every load in
// flight before each LDS read, so with the inline-asm form below each wave still retires a chunk with vmcnt(0) before the
// next, and the dispatcher's refill of finished waves hides that better than a fixed set of waves.
#pragma once

#include "csr_wavetile.hpp"

namespace spmv {

constexpr int kRunChunkRows = 128;
constexpr int kRunWaves = 4; // waves per workgroup
// doubles per wave slot: the lead and 128 rows of L, in whole LDS-DMA instructions of 128 doubles
template <int L>
constexpr int kRunSlot = (L + 1) * 128;

// A chunk: {first row, first entry, rows (2 ... 128), pattern record}; its entries are [first entry, + rows * L), its
// columns pattern[p] + row.  Fast tiles only (their last quad lies inside the arrays), so every 16-byte pair that holds
// one of the chunk's entries lies inside the value array.
__device__ __forceinline__ int4 scalar_load_i4(const int4 * p)
{
    typedef const v4i __attribute__((address_space(4))) * const_ptr;
    const v4i v = *reinterpret_cast<const_ptr>(reinterpret_cast<uintptr_t>(p));
    return make_int4(v[0], v[1], v[2], v[3]);
}

template <int L>
struct RunStage {
    v2d_a8 xv[L];
    v2d_a8 yv;
    int row0, lead, n;
};

template <int L>
__device__ __forceinline__ void run_chunk_issue(RunStage<L> & st, unsigned slot, const int4 * __restrict__ chunks, int c,
                                                const int32_t * __restrict__ patterns, const double * __restrict__ a,
                                                const double * __restrict__ x, const double * y_in, int lane)
{
    const int4 d = scalar_load_i4(chunks + c);
    const int row0 = d.x, e0 = d.y, n = d.z;
    const int kb = e0 & ~1;
    const int lastpair = (e0 + n * L - 1) & ~1; // lanes past the chunk re-read its last pair into slots nobody reads
#pragma unroll
    for (int i = 0; i <= L; ++i) {
        const double * src = a + min(kb + 128 * i + 2 * lane, lastpair);
        unsigned keep;
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(src), "s"(slot + 1024u * i) : "memory");
    }
    const int base = min(2 * lane, n - 2);
    const int32_t * pat = patterns + (size_t) d.w * kPatStride + kPatRel;
#pragma unroll
    for (int p = 0; p < L; ++p) {
        const int col = scalar_load_i32(pat + p) + row0 + base;
        st.xv[p] = *reinterpret_cast<const v2d_a8 *>(x + col);
    }
    st.yv = __builtin_nontemporal_load(reinterpret_cast<const v2d_a8 *>(y_in + row0 + base));
    st.row0 = row0;
    st.lead = e0 - kb;
    st.n = n;
}

template <int L>
__device__ __forceinline__ void run_chunk_finish(const RunStage<L> & st, const double * slot, double * y, int lane)
{
    const int n = st.n;
    const int base = min(2 * lane, n - 2);
    const double * v = slot + st.lead + base * L;
    double zA = 0.0, zB = 0.0;
#pragma unroll
    for (int p = 0; p < L; ++p) {
        zA += v[p] * st.xv[p].x;
        zB += v[L + p] * st.xv[p].y;
    }
    if (2 * lane <= n - 2) {
        const v2d_a8 out = {st.yv.x + zA, st.yv.y + zB};
        __builtin_nontemporal_store(out, reinterpret_cast<v2d_a8 *>(y + st.row0 + base));
    } else if (2 * lane == n - 1) {
        __builtin_nontemporal_store(st.yv.y + zB, y + st.row0 + base + 1);
    }
}

// A wave per chunk (the loop covers a grid smaller than the chunk list as well).  The compiler cannot count the LDS-DMA loads
// (inline asm), so the wave retires its chunk with vmcnt(0).
template <int L>
__global__ __launch_bounds__(256) void csr_wavetile_kernel_runs(int nchunks, const int4 * __restrict__ chunks,
                                                                const int32_t * __restrict__ patterns, const double * __restrict__ a,
                                                                const double * __restrict__ x, const double * y_in, double * y)
{
    __shared__ __attribute__((aligned(16))) double slots[kRunWaves][kRunSlot<L>];
    const int wave = __builtin_amdgcn_readfirstlane((int) threadIdx.x >> 6);
    const int lane = (int) __lane_id();
    const int G = (int) gridDim.x * kRunWaves;
    const double * slot = slots[wave];
    const unsigned lds = __builtin_amdgcn_readfirstlane((unsigned) reinterpret_cast<uintptr_t>((const __attribute__((address_space(3))) double *) slot));
    for (int c = (int) blockIdx.x * kRunWaves + wave; c < nchunks; c += G) {
        RunStage<L> st;
        run_chunk_issue<L>(st, lds, chunks, c, patterns, a, x, y_in, lane);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        run_chunk_finish<L>(st, slot, y, lane);
        // (the next chunk overwrites the slot only after these reads: same-wave LDS operations execute in order; the fences
        // pin the compiler)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

} // namespace spmv
