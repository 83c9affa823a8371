// agg_kernels.hpp -- one level of a plain aggregation multigrid (include/spmv_hip_agg.h).
//
// agg_prolong_kernel<T> and agg_restrict_kernel<T> are the hot path.  The prolongation runs over the cut of krylov_stream.hpp --
// chunk c of 1024 elements belongs to wave c -- but not on its driver: that driver hands a kernel the scalars of ONE element of
// arrays of ONE type, and here an element's second operand is e_c[agg[i]], found through an int32 array.  A lane takes four
// consecutive elements: one 16-byte load of agg, 16 (floats) or 2 x 16 (doubles) bytes of x, four gathers of e_c; the loads of U
// such pieces are issued before anything is used.  Aggregates are mesh neighbours, so the gathers of a wave fall into few lines.
// The restriction gives a lane an aggregate: the pair member_ptr[I], member_ptr[I + 1] in one 8-byte load, the members four at a
// time in one 16-byte load, their four gathers of r in flight together, added in member order (the contract) with a test per
// member -- a member of the next aggregate that the quad brought along is never added, and not even read.  Two aggregates per
// lane are in flight; members beyond the fourth run in a rolled loop of such quads.  agg, member_ptr and member are only 4-byte
// aligned by contract, so their wide loads are typed aligned(4): gfx950 reads such a load at any dword address.  No LDS, no
// barrier, no atomics, no scratch.
//
// The aggregation, the member lists and the Galerkin product are one-time code: a lane per row or per entry, integer atomics for
// the counters only.  The key of a row, the walk over its strong neighbours, the largest key among them, the count per wave and
// the marks of a distance-1 round (rounds_mark_kernel, which does not count here) are graph_rounds.hpp's, shared with the
// colouring of mcgs_kernels.hpp.
//
// include/spmv_hip_agg_mis2.h adds, at the end of this file, agg_restrict_group_kernel<T, G> -- G = 2 ... 64 lanes per aggregate
// that stride its member list and meet in group_sum<G> -- and the six one-time kernels of the aggregation by a distance-2
// independent set: four per round (the nearest undecided key, the marks, who is beside a mark, the states) and the two passes in
// which rows join roots, all on the walk of graph_rounds.hpp.
#pragma once

#include "graph_rounds.hpp"

namespace spmv {

constexpr int kAggCovered = -2, kAggRoot = -3; // beside kUndecided
constexpr int kAggRestrictChunk = 256; // aggregates per wave in the restriction

typedef int agg_i4 __attribute__((ext_vector_type(4), aligned(4)));
typedef int agg_i2 __attribute__((ext_vector_type(2), aligned(4)));
typedef double agg_d4 __attribute__((ext_vector_type(4), aligned(16)));
typedef float agg_f4 __attribute__((ext_vector_type(4), aligned(16)));

template <class T>
struct AggQuad;
template <>
struct AggQuad<double> {
    typedef agg_d4 type;
};
template <>
struct AggQuad<float> {
    typedef agg_f4 type;
};

// ---- the aggregation -------------------------------------------------------------------------------------------------------------

// state <- undecided, status <- {0, 0, 0, 0}, thresh[i] <- fl(theta max_{k != i} |a_ik|) where there is one
__global__ __launch_bounds__(256) void agg_init_kernel(int rows, const int * __restrict__ row_ptr, const int * __restrict__ column_index,
                                                       const double * __restrict__ value, double theta, int * __restrict__ state,
                                                       double * __restrict__ thresh, int * __restrict__ status)
{
    const long long i = (long long) blockIdx.x * 256 + (int) threadIdx.x;
    if (i < 4)
        status[i] = 0;
    if (i >= rows)
        return;
    state[i] = kUndecided;
    if (!thresh)
        return;
    double m = 0.0;
    const int end = row_ptr[i + 1];
    for (int e = row_ptr[i]; e < end; ++e) {
        const double a = __builtin_fabs(value[e]);
        if (column_index[e] != (int) i && a > m)
            m = a;
    }
    thresh[i] = theta * m;
}

// A marked row becomes a root; an undecided row that is not marked and has a neighbour that is a root or marked becomes covered.
// What a row reads of another does not depend on whether that row has been written yet: a marked row counts by its mark, and a
// row that is not marked is no root before this launch and none behind it.  *decided += the rows that left the undecided.
__global__ __launch_bounds__(256) void agg_assign_kernel(int rows, const int * __restrict__ row_ptr, const int * __restrict__ column_index,
                                                         const double * __restrict__ value, const double * __restrict__ thresh, int * state,
                                                         const unsigned char * __restrict__ mark, int * __restrict__ decided)
{
    const long long i = (long long) blockIdx.x * 256 + (int) threadIdx.x;
    int to = 0;
    if (i < rows && state[i] == kUndecided) {
        if (mark[i]) {
            to = kAggRoot;
        } else {
            for_neighbours({row_ptr, column_index, value, thresh}, (int) i, [&](int j) {
                if (mark[j] || state[j] == kAggRoot)
                    to = kAggCovered;
                return to == 0;
            });
        }
        if (to != 0)
            state[i] = to;
    }
    wave_count(to != 0, decided);
}

// flag[i] <- 1 for a root, flag[rows] <- 0: its exclusive prefix sums are the roots' numbers, and the aggregates behind the last
__global__ __launch_bounds__(256) void agg_flag_kernel(int rows, const int * __restrict__ state, int * __restrict__ flag)
{
    const long long i = (long long) blockIdx.x * 256 + (int) threadIdx.x;
    if (i <= rows)
        flag[i] = i < rows && state[i] == kAggRoot;
}

// the root that row i joins at distance 1: itself, or the root among its neighbours with the largest key; -1 without one
__device__ __forceinline__ int agg_root_beside(const Neighbours & g, unsigned seed, const int * __restrict__ state, int i)
{
    if (state[i] == kAggRoot)
        return i;
    return best_by_key(g, seed, i, -1, [&](int j) { return state[j] == kAggRoot ? j : -1; });
}

// agg[i] <- the number of the root row i joins (agg_root_beside); count[agg[i]] += 1
__global__ __launch_bounds__(256) void agg_join_kernel(int rows, unsigned seed, const int * __restrict__ row_ptr, const int * __restrict__ column_index,
                                                       const double * __restrict__ value, const double * __restrict__ thresh,
                                                       const int * __restrict__ state, const int * __restrict__ rank, int * __restrict__ agg,
                                                       int * __restrict__ count)
{
    const long long i = (long long) blockIdx.x * 256 + (int) threadIdx.x;
    if (i >= rows)
        return;
    const int root = agg_root_beside({row_ptr, column_index, value, thresh}, seed, state, (int) i);
    const int a = root >= 0 ? rank[root] : 0; // (a covered row has a root beside it)
    agg[i] = a;
    atomicAdd(count + a, 1);
}

// status <- {aggregates, rounds, the largest count, the counts that are 1}
__global__ __launch_bounds__(256) void agg_status_kernel(int rows, int rounds, const int * __restrict__ rank, const int * __restrict__ count,
                                                         int * __restrict__ status)
{
    const long long i = (long long) blockIdx.x * 256 + (int) threadIdx.x;
    const int aggregates = rank[rows];
    if (i == 0) {
        status[0] = aggregates;
        status[1] = rounds;
    }
    int c = i < aggregates ? count[i] : 0;
    wave_count(c == 1, status + 3);
#pragma unroll
    for (int d = kWave / 2; d >= 1; d >>= 1)
        c = max(c, __shfl_xor(c, d));
    if (((int) threadIdx.x & (kWave - 1)) == 0 && c > 0)
        atomicMax(status + 2, c);
}

// ---- the member lists ----------------------------------------------------------------------------------------------------------------

// count[agg[i]] += 1, idx[i] <- i; *bad += the rows whose aggregate is outside 0 ... aggregates - 1 (they are counted nowhere)
__global__ __launch_bounds__(256) void agg_count_kernel(int rows, int aggregates, const int * __restrict__ agg, int * __restrict__ count,
                                                        int * __restrict__ idx, int * __restrict__ bad)
{
    const long long i = (long long) blockIdx.x * 256 + (int) threadIdx.x;
    bool off = false;
    if (i < rows) {
        const int a = agg[i];
        idx[i] = (int) i;
        off = a < 0 || a >= aggregates;
        if (!off)
            atomicAdd(count + a, 1);
    }
    wave_count(off, bad);
}

// ---- the Galerkin product ----------------------------------------------------------------------------------------------------------

// key[e] <- agg[row of e] aggregates + agg[column of e], idx[e] <- e: 16 lanes per row
__global__ __launch_bounds__(256) void agg_key_kernel(int rows, int aggregates, const int * __restrict__ row_ptr, const int * __restrict__ column_index,
                                                      const int * __restrict__ agg, unsigned long long * __restrict__ key, int * __restrict__ idx)
{
    const long long i = (long long) blockIdx.x * 16 + ((int) threadIdx.x >> 4);
    if (i >= rows)
        return;
    const unsigned long long high = (unsigned long long) agg[i] * (unsigned) aggregates;
    const int end = row_ptr[i + 1];
    for (int e = row_ptr[i] + ((int) threadIdx.x & 15); e < end; e += 16) {
        key[e] = high + (unsigned) agg[column_index[e]];
        idx[e] = e;
    }
}

// flag[k] <- 1 where the sorted key k begins a run, flag[nnz] <- 0
__global__ __launch_bounds__(256) void agg_head_kernel(int nnz, const unsigned long long * __restrict__ key, int * __restrict__ flag)
{
    const long long k = (long long) blockIdx.x * 256 + (int) threadIdx.x;
    if (k <= nnz)
        flag[k] = k < nnz && (k == 0 || key[k] != key[k - 1]);
}

// at[k] = the exclusive prefix sums of the flags: the head of coarse entry e = at[k] stores entry_ptr[e] and the entry's column,
// and the row pointers of the coarse rows that begin between its predecessor and it; the lane behind the last key closes them
__global__ __launch_bounds__(256) void agg_pattern_kernel(int nnz, int aggregates, const unsigned long long * __restrict__ key,
                                                          const int * __restrict__ at, int * __restrict__ coarse_row_ptr,
                                                          int * __restrict__ coarse_column_index, int * __restrict__ entry_ptr,
                                                          int * __restrict__ status)
{
    const long long k = (long long) blockIdx.x * 256 + (int) threadIdx.x;
    if (k > nnz)
        return;
    const int e = at[k];
    const unsigned a = (unsigned) (aggregates > 0 ? aggregates : 1);
    const long long before = k == 0 ? -1 : (long long) (key[k - 1] / a);
    if (k == nnz) {
        entry_ptr[e] = nnz;
        status[0] = e;
        for (long long row = before + 1; row <= aggregates; ++row)
            coarse_row_ptr[row] = e;
        return;
    }
    const unsigned long long mine = key[k];
    if (k != 0 && mine == key[k - 1])
        return;
    entry_ptr[e] = (int) k;
    coarse_column_index[e] = (int) (mine % a);
    for (long long row = before + 1; row <= (long long) (mine / a); ++row)
        coarse_row_ptr[row] = e;
}

// coarse_value[e] <- the fine values of the entry's run, added left to right from +0.0
__global__ __launch_bounds__(256) void agg_numeric_kernel(int nnz_c, const int * __restrict__ entry_order, const int * __restrict__ entry_ptr,
                                                          const double * __restrict__ value, double * __restrict__ coarse_value)
{
    const long long e = (long long) blockIdx.x * 256 + (int) threadIdx.x;
    if (e >= nnz_c)
        return;
    double s = 0.0;
    const int end = entry_ptr[e + 1];
    for (int k = entry_ptr[e]; k < end; ++k)
        s += value[entry_order[k]];
    coarse_value[e] = s;
}

// ---- the prolongation ----------------------------------------------------------------------------------------------------------------

template <class T>
__global__ __launch_bounds__(256, 8) void agg_prolong_kernel(long long n, double omega, const int * __restrict__ agg, const T * __restrict__ ec,
                                                             T * __restrict__ x)
{
    typedef typename AggQuad<T>::type Q;
    constexpr int W = 4;                            // elements of a lane's piece
    constexpr int PIECES = kKrylovChunk / (W * kWave);
    constexpr int U = 2;                            // pieces in flight
    static_assert(PIECES % U == 0, "whole passes");
    const KrylovWave at = krylov_wave(n);
    if (!at.any)
        return;
    const int lane = at.lane();
    const long long base = at.chunk * kKrylovChunk;
    if (base + kKrylovChunk <= n) {
#pragma unroll 1
        for (int j = 0; j < PIECES; j += U) {
            agg_i4 a[U];
            Q xv[U];
            T e[U][W];
#pragma unroll
            for (int u = 0; u < U; ++u)
                a[u] = *reinterpret_cast<const agg_i4 *>(agg + base + ((long long) (j + u) * kWave + lane) * W);
#pragma unroll
            for (int u = 0; u < U; ++u)
                xv[u] = *reinterpret_cast<const Q *>(x + base + ((long long) (j + u) * kWave + lane) * W);
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int c = 0; c < W; ++c)
                    e[u][c] = ec[a[u][c]];
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int c = 0; c < W; ++c)
                    xv[u][c] = (T) ((double) xv[u][c] + omega * (double) e[u][c]);
                *reinterpret_cast<Q *>(x + base + ((long long) (j + u) * kWave + lane) * W) = xv[u];
            }
        }
        return;
    }
    // the last chunk of a vector that does not fill it: an element at a time
    for (long long i = base + lane; i < n; i += kWave)
        x[i] = (T) ((double) x[i] + omega * (double) ec[agg[i]]);
}

// ---- the restriction -----------------------------------------------------------------------------------------------------------------

// the members k ... k + 3 of the list: one 16-byte load where the list has them all; a position behind the list is row 0
__device__ __forceinline__ agg_i4 agg_members(const int * __restrict__ member, int k, int rows)
{
    agg_i4 m = {0, 0, 0, 0};
    if (k + 4 <= rows) {
        m = *reinterpret_cast<const agg_i4 *>(member + k);
    } else {
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (k + t < rows)
                m[t] = member[k + t];
    }
    return m;
}

template <class T>
__global__ __launch_bounds__(256, 8) void agg_restrict_kernel(int aggregates, int rows, const int * __restrict__ member_ptr,
                                                              const int * __restrict__ member, const T * __restrict__ r, T * __restrict__ rc)
{
    constexpr int U = 2; // aggregates of a lane in flight
    constexpr int PASSES = kAggRestrictChunk / kWave;
    static_assert(PASSES % U == 0, "whole passes");
    const int wave = __builtin_amdgcn_readfirstlane((int) threadIdx.x >> 6);
    const long long base = ((long long) blockIdx.x * 4 + wave) * kAggRestrictChunk;
    if (base >= aggregates)
        return; // the whole wave
    const int lane = (int) threadIdx.x & (kWave - 1);
#pragma unroll 1
    for (int j = 0; j < PASSES; j += U) {
        long long I[U];
        int k[U], end[U];
        agg_i4 m[U];
        double v[U][4], s[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            I[u] = base + (long long) (j + u) * kWave + lane;
            k[u] = end[u] = 0;
            if (I[u] < aggregates) {
                const agg_i2 p = *reinterpret_cast<const agg_i2 *>(member_ptr + I[u]);
                k[u] = p[0];
                end[u] = p[1];
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            m[u] = agg_members(member, k[u], rows);
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                v[u][t] = 0.0;
                if (k[u] + t < end[u])
                    v[u][t] = (double) r[m[u][t]];
            }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            s[u] = 0.0;
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (k[u] + t < end[u])
                    s[u] += v[u][t];
        }
        // aggregates of more than four rows
#pragma unroll
        for (int u = 0; u < U; ++u)
            for (int q = k[u] + 4; q < end[u]; q += 4) {
                const agg_i4 mq = agg_members(member, q, rows);
                double w[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    w[t] = 0.0;
                    if (q + t < end[u])
                        w[t] = (double) r[mq[t]];
                }
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    if (q + t < end[u])
                        s[u] += w[t];
            }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (I[u] < aggregates)
                rc[I[u]] = (T) s[u];
    }
}

// ---- the restriction by a group of lanes per aggregate (include/spmv_hip_agg_mis2.h) -----------------------------------------------

// G lanes per aggregate, 64 / G aggregates per pass of the wave, kAggGroupPasses passes per wave, all four in flight.  Every
// lane of a group loads its aggregate's member_ptr pair in one 8-byte load (one address per group: one fetch); lane l takes the
// members l, l + G, ... -- a lane's own members lie G apart, which is why its loads are 4 bytes wide, and the G lanes of a group
// read G consecutive words -- two of them with their gathers of r in flight per aggregate, added in that order (the contract) with
// a test per member; members beyond the first 2 G run in a rolled loop of such pairs.  The loops end per lane; behind them every
// lane of the wave is active again, a lane without a member (or without an aggregate) holding +0.0, and the group's sums meet in
// group_sum<G>: p += p[lane ^ step], step = 1 ... G / 2.  The group's first lane stores.
constexpr int kAggGroupPasses = 4;

template <class T, int G>
__global__ __launch_bounds__(256, 8) void agg_restrict_group_kernel(int aggregates, const int * __restrict__ member_ptr,
                                                                    const int * __restrict__ member, const T * __restrict__ r, T * __restrict__ rc)
{
    static_assert(G >= 2, "a group of one lane is agg_restrict_kernel");
    constexpr int PER = kWave / G; // aggregates of one pass of the wave
    constexpr int U = 4;           // passes in flight
    constexpr int V = 2;           // members of a lane in flight per aggregate
    static_assert(kAggGroupPasses % U == 0, "whole passes");
    const int wave = __builtin_amdgcn_readfirstlane((int) threadIdx.x >> 6);
    const long long base = ((long long) blockIdx.x * 4 + wave) * (kAggGroupPasses * PER);
    if (base >= aggregates)
        return; // the whole wave
    const int lane = (int) threadIdx.x & (kWave - 1);
    const int l = lane & (G - 1), g = lane / G;
#pragma unroll 1
    for (int j = 0; j < kAggGroupPasses; j += U) {
        long long I[U];
        int k[U], end[U], m[U][V];
        double v[U][V], s[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            I[u] = base + (long long) (j + u) * PER + g;
            k[u] = end[u] = 0;
            if (I[u] < aggregates) {
                const agg_i2 p = *reinterpret_cast<const agg_i2 *>(member_ptr + I[u]);
                k[u] = p[0] + l;
                end[u] = p[1];
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int t = 0; t < V; ++t) {
                m[u][t] = 0;
                if (k[u] + t * G < end[u])
                    m[u][t] = member[k[u] + t * G];
            }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int t = 0; t < V; ++t) {
                v[u][t] = 0.0;
                if (k[u] + t * G < end[u])
                    v[u][t] = (double) r[m[u][t]];
            }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            s[u] = 0.0;
#pragma unroll
            for (int t = 0; t < V; ++t)
                if (k[u] + t * G < end[u])
                    s[u] += v[u][t];
        }
        // aggregates of more than 2 G rows
#pragma unroll
        for (int u = 0; u < U; ++u)
            for (int q = k[u] + V * G; q < end[u]; q += V * G) {
                int mq[V];
                double w[V];
#pragma unroll
                for (int t = 0; t < V; ++t) {
                    mq[t] = 0;
                    if (q + t * G < end[u])
                        mq[t] = member[q + t * G];
                }
#pragma unroll
                for (int t = 0; t < V; ++t) {
                    w[t] = 0.0;
                    if (q + t * G < end[u])
                        w[t] = (double) r[mq[t]];
                }
#pragma unroll
                for (int t = 0; t < V; ++t)
                    if (q + t * G < end[u])
                        s[u] += w[t];
            }
#pragma unroll
        for (int u = 0; u < U; ++u)
            s[u] = group_sum<G>(s[u]); // every lane of the wave is active again
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (l == 0 && I[u] < aggregates)
                rc[I[u]] = (T) s[u];
    }
}

// ---- the aggregation by a distance-2 independent set (include/spmv_hip_agg_mis2.h) -------------------------------------------------

// near[i] <- the undecided row of {i} + N(i) with the largest key, -1 without one: every row relays, whatever its state
__global__ __launch_bounds__(256) void agg_mis2_near_kernel(int rows, unsigned seed, const int * __restrict__ row_ptr,
                                                            const int * __restrict__ column_index, const double * __restrict__ value,
                                                            const double * __restrict__ thresh, const int * __restrict__ state,
                                                            int * __restrict__ near)
{
    const long long i = (long long) blockIdx.x * 256 + (int) threadIdx.x;
    if (i >= rows)
        return;
    near[i] = best_by_key({row_ptr, column_index, value, thresh}, seed, (int) i, state[i] == kUndecided ? (int) i : -1,
                          [&](int j) { return state[j] == kUndecided ? j : -1; });
}

// mark[i] <- 1 where row i is undecided and no near[j], j in {i} + N(i), has a key above its own: the largest within two steps
__global__ __launch_bounds__(256) void agg_mis2_mark_kernel(int rows, unsigned seed, const int * __restrict__ row_ptr,
                                                            const int * __restrict__ column_index, const double * __restrict__ value,
                                                            const double * __restrict__ thresh, const int * __restrict__ state,
                                                            const int * __restrict__ near, unsigned char * __restrict__ mark)
{
    const long long i = (long long) blockIdx.x * 256 + (int) threadIdx.x;
    if (i >= rows)
        return;
    bool win = state[i] == kUndecided && near[i] == (int) i;
    if (win) {
        const unsigned hi = fmix32((unsigned) i ^ seed);
        for_neighbours({row_ptr, column_index, value, thresh}, (int) i, [&](int j) {
            const int n = near[j];
            if (n >= 0 && key_above(fmix32((unsigned) n ^ seed), n, hi, (int) i))
                win = false;
            return win;
        });
    }
    mark[i] = win ? 1 : 0;
}

// beside[i] <- 1 where row i or one of its neighbours is marked
__global__ __launch_bounds__(256) void agg_mis2_beside_kernel(int rows, const int * __restrict__ row_ptr, const int * __restrict__ column_index,
                                                              const double * __restrict__ value, const double * __restrict__ thresh,
                                                              const unsigned char * __restrict__ mark, unsigned char * __restrict__ beside)
{
    const long long i = (long long) blockIdx.x * 256 + (int) threadIdx.x;
    if (i >= rows)
        return;
    bool yes = mark[i] != 0;
    if (!yes)
        for_neighbours({row_ptr, column_index, value, thresh}, (int) i, [&](int j) {
            yes = mark[j] != 0;
            return !yes;
        });
    beside[i] = yes ? 1 : 0;
}

// A marked row becomes a root; an undecided row that is not marked and has beside[j] for a j of {i} + N(i) becomes covered.  A
// lane reads the state of its own row alone, and the marks and `beside` of the others.  *decided += the rows that left the undecided.
__global__ __launch_bounds__(256) void agg_mis2_assign_kernel(int rows, const int * __restrict__ row_ptr, const int * __restrict__ column_index,
                                                              const double * __restrict__ value, const double * __restrict__ thresh, int * state,
                                                              const unsigned char * __restrict__ mark, const unsigned char * __restrict__ beside,
                                                              int * __restrict__ decided)
{
    const long long i = (long long) blockIdx.x * 256 + (int) threadIdx.x;
    int to = 0;
    if (i < rows && state[i] == kUndecided) {
        if (mark[i]) {
            to = kAggRoot;
        } else if (beside[i]) {
            to = kAggCovered;
        } else {
            for_neighbours({row_ptr, column_index, value, thresh}, (int) i, [&](int j) {
                if (beside[j])
                    to = kAggCovered;
                return to == 0;
            });
        }
        if (to != 0)
            state[i] = to;
    }
    wave_count(to != 0, decided);
}

// pass 1: joined[i] <- i for a root, the root among the neighbours with the largest key for a row beside one, else -1
__global__ __launch_bounds__(256) void agg_mis2_join1_kernel(int rows, unsigned seed, const int * __restrict__ row_ptr,
                                                             const int * __restrict__ column_index, const double * __restrict__ value,
                                                             const double * __restrict__ thresh, const int * __restrict__ state,
                                                             int * __restrict__ joined)
{
    const long long i = (long long) blockIdx.x * 256 + (int) threadIdx.x;
    if (i >= rows)
        return;
    joined[i] = agg_root_beside({row_ptr, column_index, value, thresh}, seed, state, (int) i);
}

// pass 2: a row that joined nobody in pass 1 joins the root that one of its neighbours joined in pass 1 (a neighbour that is no
// root itself), the largest key among those roots; agg[i] <- the number of the row's root, count[agg[i]] += 1; *missing += the
// rows that found none (they are counted in aggregate 0).  `joined` is read only: what pass 2 finds is stored in agg alone.
__global__ __launch_bounds__(256) void agg_mis2_join2_kernel(int rows, unsigned seed, const int * __restrict__ row_ptr,
                                                             const int * __restrict__ column_index, const double * __restrict__ value,
                                                             const double * __restrict__ thresh, const int * __restrict__ state,
                                                             const int * __restrict__ joined, const int * __restrict__ rank,
                                                             int * __restrict__ agg, int * __restrict__ count, int * __restrict__ missing)
{
    const long long i = (long long) blockIdx.x * 256 + (int) threadIdx.x;
    bool none = false;
    if (i < rows) {
        int root = joined[i];
        if (root < 0)
            root = best_by_key({row_ptr, column_index, value, thresh}, seed, (int) i, -1, [&](int j) {
                if (state[j] == kAggRoot)
                    return -1;
                const int q = joined[j];
                return q >= 0 && q < rows ? q : -1;
            });
        none = root < 0;
        const int a = none ? 0 : rank[root];
        agg[i] = a;
        atomicAdd(count + a, 1);
    }
    wave_count(none, missing);
}

} // namespace spmv
