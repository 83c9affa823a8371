// graph_rounds.hpp -- the device side of the Luby-style rounds over a CSR pattern that the colouring (mcgs_kernels.hpp) and the
// two aggregations (agg_kernels.hpp) run: the key of a row, the mark of the undecided, the walk over a row's neighbours, the
// neighbour with the largest key, a count per wave and the distance-1 mark kernel.  The host side of a round -- counter, copy,
// synchronisation, the refusal of a round that decided nothing -- is graph_rounds() in krylov_check.hpp.
//
// The key of row i under a seed is (fmix32(i ^ seed), i), compared in that order.  In a round a row wins when no undecided
// neighbour has a larger key; the largest remaining key always wins, so every round decides a row.
#pragma once

#include "cg_updates.hpp"

namespace spmv {

constexpr int kUndecided = -1; // what colour[] and state[] hold for a row that no round has decided

// the murmur3 finaliser in 32 bits
__device__ __forceinline__ unsigned fmix32(unsigned h)
{
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return h;
}

// whether the key of row a (its hash ha) is above the key of row b
__device__ __forceinline__ bool key_above(unsigned ha, int a, unsigned hb, int b)
{
    return ha > hb || (ha == hb && a > b);
}

// The pattern whose rows are walked; a kernel fills it from its own __restrict__ parameters.  Without thresh (the colouring, or
// theta = 0) every stored entry beside the diagonal makes its column a neighbour, and value is not read.
struct Neighbours {
    const int * row_ptr, * column_index;
    const double * value, * thresh;
};

// visit(j) for the stored entries of row i whose column j is not i and that are strong: |a_ij| >= thresh[i], the threshold of the
// row that is walked, never of the column's row.  The walk ends behind the first visit that returns false.
template <class F>
__device__ __forceinline__ void for_neighbours(const Neighbours & g, int i, F visit)
{
    const int end = g.row_ptr[i + 1];
    bool go = true;
    for (int e = g.row_ptr[i]; e < end && go; ++e) {
        const int j = g.column_index[e];
        __builtin_assume(j >= 0); // (a column of a CSR matrix: lets a candidate "j or -1" fold into its condition)
        if (j != i && (!g.thresh || __builtin_fabs(g.value[e]) >= g.thresh[i]))
            go = visit(j);
    }
}

// the row with the largest key among `first` (-1: none) and candidate(j) of the neighbours j of row i, where candidate gives a
// row or -1; -1 where there is none at all
template <class M>
__device__ __forceinline__ int best_by_key(const Neighbours & g, unsigned seed, int i, int first, M candidate)
{
    int best = first;
    unsigned hb = fmix32((unsigned) first ^ seed);
    for_neighbours(g, i, [&](int j) {
        const int q = candidate(j);
        if (q >= 0) {
            const unsigned hq = fmix32((unsigned) q ^ seed);
            if (best < 0 || key_above(hq, q, hb, best)) {
                best = q;
                hb = hq;
            }
        }
        return true;
    });
    return best;
}

// the number of lanes with `yes`, added to *counter by one of them; called by every lane of the wave that has not returned
__device__ __forceinline__ void wave_count(bool yes, int * __restrict__ counter)
{
    const unsigned long long m = __ballot(yes);
    if (m != 0 && ((int) threadIdx.x & (kWave - 1)) == (int) __builtin_ctzll(m))
        atomicAdd(counter, __popcll(m));
}

// mark[i] <- 1 where row i is undecided and its key is above the key of every undecided neighbour; with COUNT, *winners += their
// number, and without it winners is null.  (A template because two translation units launch it: mcgs.hip counts, agg.hip counts
// in its assign kernel.)
template <bool COUNT>
__global__ __launch_bounds__(256) void rounds_mark_kernel(int rows, unsigned seed, const int * __restrict__ row_ptr,
                                                          const int * __restrict__ column_index, const double * __restrict__ value,
                                                          const double * __restrict__ thresh, const int * __restrict__ state,
                                                          unsigned char * __restrict__ mark, int * __restrict__ winners)
{
    const long long i = (long long) blockIdx.x * 256 + (int) threadIdx.x;
    if (i >= rows)
        return;
    bool win = state[i] == kUndecided;
    if (win) {
        const unsigned hi = fmix32((unsigned) i ^ seed);
        for_neighbours({row_ptr, column_index, value, thresh}, (int) i, [&](int j) {
            if (state[j] == kUndecided && key_above(fmix32((unsigned) j ^ seed), j, hi, (int) i))
                win = false;
            return win;
        });
    }
    mark[i] = win ? 1 : 0;
    if (COUNT)
        wave_count(win, winners);
}

} // namespace spmv
