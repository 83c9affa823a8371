// mcgs_kernels.hpp -- the multicolour Gauss-Seidel / SSOR preconditioner (include/spmv_hip_mcgs.h).
//
// mcgs_sweep_kernel<T, G> is the hot path: one launch per colour over the colour-major copy of the matrix.  A group of G lanes
// owns a row, a wave 64 / G rows per pass and kMcgsPasses passes at once: the row bounds, the row's b, minv and x and the first
// G entries of all its passes are loaded before anything is used, so a lane has kMcgsPasses gathers of x in flight.  Rows of a
// wave's pass are consecutive rows of the copy and lane l of a group takes the entries l, l + G, ... (the contract: the order of
// the sum), so one column load of the wave is a contiguous run of 4-byte words and one value load a run of 8-byte words with
// holes only where a row is shorter than G: every line of a colour is fetched once.  A lane's own entries lie G apart, which
// is why its loads are 4 and 8 bytes wide and not 16.  Entries beyond the first G of a row run in a rolled loop.  The group's
// sums meet in a butterfly from step G / 2 down to 1; the first lane of the group stores x_i.  x is neither const nor
// restrict: it is written by this launch, by other rows' lanes.  No LDS, no barrier, no atomics, no scratch.
//
// The colouring, the counting sort and the copy are one-time code: a lane per row (a wave per 1024 rows in the sort), integer
// atomics for the counters only.  The colouring's key, its walk over a row's neighbours and the marks of a round are
// graph_rounds.hpp's, shared with the aggregations of agg_kernels.hpp.
#pragma once

#include "graph_rounds.hpp"

namespace spmv {

constexpr int kMcgsMaxColours = 64; // SPMV_HIP_MCGS_MAX_COLOURS
constexpr int kMcgsPasses = 4;      // rows per group in flight in the sweep
constexpr int kMcgsChunk = 1024;    // rows per wave in the counting sort and the scan

// ---- the colouring ---------------------------------------------------------------------------------------------------------------

// colour <- undecided, status <- {0, 0, 0, 0}
__global__ __launch_bounds__(256) void mcgs_init_kernel(int rows, int * __restrict__ colour, int * __restrict__ status)
{
    const long long i = (long long) blockIdx.x * 256 + (int) threadIdx.x;
    if (i < rows)
        colour[i] = kUndecided;
    if (i < 4)
        status[i] = 0;
}

// (the marks of a round are rounds_mark_kernel's, counted there: graph_rounds.hpp)

// the marked rows take the smallest colour that no neighbour which is NOT marked holds: those rows are not written in this launch
__global__ __launch_bounds__(256) void mcgs_assign_kernel(int rows, const int * __restrict__ row_ptr, const int * __restrict__ column_index, int * colour,
                                                          const unsigned char * __restrict__ mark, int * __restrict__ status)
{
    const long long i = (long long) blockIdx.x * 256 + (int) threadIdx.x;
    if (i >= rows || !mark[i])
        return;
    unsigned long long held = 0;
    for_neighbours({row_ptr, column_index, nullptr, nullptr}, (int) i, [&](int j) {
        const int c = mark[j] ? -1 : colour[j]; // (the colour of a marked row is not even read)
        if (c >= 0)
            held |= 1ULL << (c & 63);
        return true;
    });
    int c = kMcgsMaxColours - 1;
    if (~held == 0)
        atomicAdd(status + 3, 1);
    else
        c = __builtin_ctzll(~held);
    colour[i] = c;
}

// status[0] <- the largest colour + 1, status[1] <- rounds, status[2] <- the stored entries (i, j), j != i, of one colour
__global__ __launch_bounds__(256) void mcgs_check_kernel(int rows, const int * __restrict__ row_ptr, const int * __restrict__ column_index,
                                                         const int * __restrict__ colour, int rounds, int * __restrict__ status)
{
    const long long i = (long long) blockIdx.x * 256 + (int) threadIdx.x;
    if (i == 0)
        status[1] = rounds;
    int mine = -1, same = 0;
    if (i < rows) {
        mine = colour[i];
        for_neighbours({row_ptr, column_index, nullptr, nullptr}, (int) i, [&](int j) {
            same += colour[j] == mine;
            return true;
        });
    }
    // one atomic per wave and counter (a single address takes about 10^8 a second)
#pragma unroll
    for (int d = kWave / 2; d >= 1; d >>= 1) {
        same += __shfl_xor(same, d);
        mine = max(mine, __shfl_xor(mine, d));
    }
    if (((int) threadIdx.x & (kWave - 1)) == 0) {
        if (same)
            atomicAdd(status + 2, same);
        if (mine >= 0)
            atomicMax(status, mine + 1);
    }
}

// ---- the colour-major order: a stable counting sort on six bits, a wave per kMcgsChunk rows ---------------------------------------

__device__ __forceinline__ int mcgs_wave_scan(int v, int lane) // inclusive
{
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const int u = __shfl_up(v, d);
        if (lane >= d)
            v += u;
    }
    return v;
}

// the colour of row i as a bin: 0 ... 63 whatever the array holds, 64 behind the last row
__device__ __forceinline__ int mcgs_bin(const int * __restrict__ colour, long long i, int rows) { return i < rows ? colour[i] & 63 : 64; }

// hist[chunk][c] <- the rows of colour c in the chunk (lane c counts colour c)
__global__ __launch_bounds__(256) void mcgs_hist_kernel(int rows, const int * __restrict__ colour, int * __restrict__ hist)
{
    const int lane = (int) threadIdx.x & (kWave - 1);
    const long long chunk = (long long) blockIdx.x * 4 + ((int) threadIdx.x >> 6);
    if (chunk * kMcgsChunk >= rows)
        return;
    int count = 0;
    for (int pass = 0; pass < kMcgsChunk / kWave; ++pass) {
        const int c = mcgs_bin(colour, chunk * kMcgsChunk + pass * kWave + lane, rows);
        for (int q = 0; q < kMcgsMaxColours; ++q) {
            const unsigned long long m = __ballot(c == q);
            if (lane == q)
                count += __popcll(m);
        }
    }
    hist[chunk * kMcgsMaxColours + lane] = count;
}

// one wave: hist[chunk][c] <- the position of the chunk's first row of colour c; cptr[c] <- the colour's first position
__global__ __launch_bounds__(64) void mcgs_offsets_kernel(int chunks, int * __restrict__ hist, int * __restrict__ cptr)
{
    const int lane = (int) threadIdx.x;
    int run = 0;
    for (int ch = 0; ch < chunks; ++ch)
        run += hist[(long long) ch * kMcgsMaxColours + lane];
    const int incl = mcgs_wave_scan(run, lane);
    int at = incl - run;
    cptr[lane] = at;
    if (lane == kWave - 1)
        cptr[kMcgsMaxColours] = incl;
    for (int ch = 0; ch < chunks; ++ch) {
        const int t = hist[(long long) ch * kMcgsMaxColours + lane];
        hist[(long long) ch * kMcgsMaxColours + lane] = at;
        at += t;
    }
}

// order[position] <- row, and the row's length behind it in the copy's row_ptr (mcgs_row_scan_kernel adds them up)
__global__ __launch_bounds__(256) void mcgs_scatter_kernel(int rows, const int * __restrict__ colour, const int * __restrict__ row_ptr,
                                                           const int * __restrict__ hist, int * __restrict__ order, int * __restrict__ perm_row_ptr)
{
    const int lane = (int) threadIdx.x & (kWave - 1);
    const long long chunk = (long long) blockIdx.x * 4 + ((int) threadIdx.x >> 6);
    if (chunk * kMcgsChunk >= rows)
        return;
    if (chunk == 0 && lane == 0)
        perm_row_ptr[0] = 0;
    int base = hist[chunk * kMcgsMaxColours + lane]; // of colour `lane`
    for (int pass = 0; pass < kMcgsChunk / kWave; ++pass) {
        const long long i = chunk * kMcgsChunk + pass * kWave + lane;
        const int c = mcgs_bin(colour, i, rows);
        unsigned long long mine = 0;
        int add = 0;
        for (int q = 0; q < kMcgsMaxColours; ++q) {
            const unsigned long long m = __ballot(c == q);
            if (c == q)
                mine = m;
            if (lane == q)
                add = __popcll(m);
        }
        const int first = __shfl(base, c & 63);
        if (i < rows) {
            const int at = first + __popcll(mine & ((1ULL << lane) - 1));
            order[at] = (int) i;
            perm_row_ptr[at + 1] = row_ptr[i + 1] - row_ptr[i];
        }
        base += add;
    }
}

// sums[chunk] <- the sum of a[1 + chunk kMcgsChunk ...], kMcgsChunk elements of a[1 ... rows]
__global__ __launch_bounds__(256) void mcgs_chunk_sum_kernel(int rows, const int * __restrict__ a, int * __restrict__ sums)
{
    const int lane = (int) threadIdx.x & (kWave - 1);
    const long long chunk = (long long) blockIdx.x * 4 + ((int) threadIdx.x >> 6);
    if (chunk * kMcgsChunk >= rows)
        return;
    int sum = 0;
    for (int pass = 0; pass < kMcgsChunk / kWave; ++pass) {
        const long long k = chunk * kMcgsChunk + pass * kWave + lane;
        sum += k < rows ? a[1 + k] : 0;
    }
    sum = mcgs_wave_scan(sum, lane);
    if (lane == kWave - 1)
        sums[chunk] = sum;
}

// one wave: sums <- its exclusive prefix sums
__global__ __launch_bounds__(64) void mcgs_chunk_scan_kernel(int chunks, int * __restrict__ sums)
{
    const int lane = (int) threadIdx.x;
    int carry = 0;
    for (int base = 0; base < chunks; base += kWave) { // wave-uniform
        const int v = base + lane < chunks ? sums[base + lane] : 0;
        const int incl = mcgs_wave_scan(v, lane);
        if (base + lane < chunks)
            sums[base + lane] = carry + incl - v;
        carry += __shfl(incl, kWave - 1);
    }
}

// a[1 ... rows] <- its inclusive prefix sums, in place (an element is read and written by the same lane)
__global__ __launch_bounds__(256) void mcgs_row_scan_kernel(int rows, int * __restrict__ a, const int * __restrict__ sums)
{
    const int lane = (int) threadIdx.x & (kWave - 1);
    const long long chunk = (long long) blockIdx.x * 4 + ((int) threadIdx.x >> 6);
    if (chunk * kMcgsChunk >= rows)
        return;
    int carry = sums[chunk];
    for (int pass = 0; pass < kMcgsChunk / kWave; ++pass) {
        const long long k = chunk * kMcgsChunk + pass * kWave + lane;
        const int v = k < rows ? a[1 + k] : 0;
        const int incl = mcgs_wave_scan(v, lane);
        if (k < rows)
            a[1 + k] = carry + incl;
        carry += __shfl(incl, kWave - 1);
    }
}

// the entries of row order[k] to row k of the copy, in stored order: 16 lanes per row
__global__ __launch_bounds__(256) void mcgs_copy_kernel(int rows, const int * __restrict__ order, const int * __restrict__ row_ptr,
                                                        const int * __restrict__ column_index, const double * __restrict__ value,
                                                        const int * __restrict__ perm_row_ptr, int * __restrict__ perm_column_index,
                                                        double * __restrict__ perm_value)
{
    const long long k = (long long) blockIdx.x * 16 + ((int) threadIdx.x >> 4);
    if (k >= rows)
        return;
    const int i = order[k];
    const long long from = row_ptr[i], to = perm_row_ptr[k];
    const int n = row_ptr[i + 1] - (int) from;
    for (int e = (int) threadIdx.x & 15; e < n; e += 16) {
        perm_column_index[to + e] = column_index[from + e];
        perm_value[to + e] = value[from + e];
    }
}

// ---- the sweep ---------------------------------------------------------------------------------------------------------------------

// p += p[lane ^ step] for step = G / 2 ... 1: every lane of a group ends with the group's sum
template <int G>
__device__ __forceinline__ double mcgs_butterfly(double p)
{
    static_assert(G == 1 || G == 2 || G == 4 || G == 8 || G == 16 || G == 32 || G == 64, "a power of two up to the wave");
    if (G >= 64) p += bpermute_xor32(p);
    if (G >= 32) p += swizzle_xor<16>(p);
    if (G >= 16) p += swizzle_xor<8>(p);
    if (G >= 8) p += swizzle_xor<4>(p);
    if (G >= 4) p += dpp_move<kDppQuadXor2>(p);
    if (G >= 2) p += dpp_move<kDppQuadXor1>(p);
    return p;
}

// rows [k0, k1) of the copy: one colour
template <class T, int G>
__global__ __launch_bounds__(256) void mcgs_sweep_kernel(int k0, int k1, const int * __restrict__ order, const int * __restrict__ row_ptr,
                                                         const int * __restrict__ column_index, const double * __restrict__ value, double omega,
                                                         double keep, const T * __restrict__ b, const T * __restrict__ minv, T * x)
{
    constexpr int ROWS = kWave / G; // rows of one pass of the wave
    constexpr int R = kMcgsPasses;
    const int wave = __builtin_amdgcn_readfirstlane((int) threadIdx.x >> 6);
    const long long first = k0 + ((long long) blockIdx.x * 4 + wave) * (ROWS * R);
    if (first >= k1)
        return; // the whole wave
    const int lane = (int) threadIdx.x & (kWave - 1);
    const int l = lane & (G - 1), g = lane / G;
    int row[R], at[R], end[R];
    // Lane t of the wave looks after row first + t: its place in x, its bounds, its b, minv and x -- one load of each per wave --
    // and hands the first three to the lanes of the row's group in its pass.  (Groups of one or two lanes are 256 or 128 rows a
    // wave: there every lane of a group loads its passes' rows itself.)  A row behind the colour's last looks at that row and
    // has no entry.
    constexpr bool SHARED = ROWS * R <= kWave;
    const long long mine = first + (SHARED ? lane : 0);
    const bool mine_live = SHARED && lane < ROWS * R && mine < k1;
    int my_row = 0, my_at = 0, my_end = 0;
    T my_b = (T) 0, my_m = (T) 0, my_x = (T) 0;
    T bv[R], mv[R], xv[R];
    bool live[R];
    if (SHARED) {
        const int kk = (int) (mine < k1 ? mine : k1 - 1);
        my_row = order[kk];
        my_at = row_ptr[kk];
        my_end = mine_live ? row_ptr[kk + 1] : 0;
        my_b = b[my_row];
        my_m = minv[my_row];
        my_x = x[my_row];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int src = r * ROWS + g;
            row[r] = __shfl(my_row, src);
            at[r] = __shfl(my_at, src) + l;
            end[r] = __shfl(my_end, src);
        }
    } else {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const long long k = first + r * ROWS + g;
            live[r] = k < k1;
            const int kk = (int) (live[r] ? k : k1 - 1);
            row[r] = order[kk];
            at[r] = row_ptr[kk] + l;
            end[r] = live[r] ? row_ptr[kk + 1] : 0;
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            bv[r] = b[row[r]];
            mv[r] = minv[row[r]];
            xv[r] = x[row[r]];
        }
    }
    // the first G entries of every pass: columns and values, then the gathers, then the products
    int c[R];
    double a[R], xg[R], p[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        c[r] = row[r];
        a[r] = 0.0;
        if (at[r] < end[r]) {
            c[r] = column_index[at[r]];
            a[r] = value[at[r]];
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        xg[r] = 0.0;
        if (c[r] != row[r])
            xg[r] = (double) x[c[r]];
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        p[r] = 0.0;
        if (c[r] != row[r])
            p[r] += a[r] * xg[r];
    }
    // rows of more than G entries
#pragma unroll
    for (int r = 0; r < R; ++r)
        for (int e = at[r] + G; e < end[r]; e += G) {
            const int j = column_index[e];
            if (j != row[r])
                p[r] += value[e] * (double) x[j];
        }
    double sum[R];
#pragma unroll
    for (int r = 0; r < R; ++r)
        sum[r] = mcgs_butterfly<G>(p[r]); // every lane of the wave is active again
    if (SHARED) {
        // the row's sum back to the lane that looks after it: from the first lane of group t % ROWS, of pass t / ROWS
        double s = 0.0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const double from = __shfl(sum[r], (lane & (ROWS - 1)) * G);
            if (lane / ROWS == r)
                s = from;
        }
        if (mine_live) {
            const double t = omega * ((double) my_m * ((double) my_b - s));
            x[my_row] = (T) (keep * (double) my_x + t);
        }
    } else {
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (l == 0 && live[r]) {
                const double t = omega * ((double) mv[r] * ((double) bv[r] - sum[r]));
                x[row[r]] = (T) (keep * (double) xv[r] + t);
            }
    }
}

// ---- the dots behind the last colour ---------------------------------------------------------------------------------------------

// slots[chunk] = {sum z r, sum z z} over the chunk, in the cut of krylov_stream.hpp
template <class T>
__global__ __launch_bounds__(256, 8) void mcgs_dots_kernel(long long n, const T * __restrict__ r, const T * __restrict__ z, v2d * __restrict__ slots)
{
    const KrylovWave at = krylov_wave(n);
    if (!at.any)
        return;
    double sums[2] = {0.0, 0.0};
    const T * const arrays[] = {r, z};
    krylov_stream<T, 4, false, kKrylovRead, kKrylovRead>(n, at, arrays, [&](T * e) {
        const double zv = (double) e[1];
        sums[0] += zv * (double) e[0];
        sums[1] += zv * zv;
    });
    store_wave_dots(slots, (int) at.chunk, sums); // every lane of the wave is active again
}

} // namespace spmv
