// coarse_kernels.hpp -- the dense coarsest-level solve (include/spmv_hip_coarse.h).
//
// coarse_apply_kernel<T> is the call of every cycle: one wave per row of the inverse, lane l taking the elements l, l + 64, ... of
// the row (consecutive lanes read consecutive elements: a wave's load is one run of 64 elements), the products added in that
// order in fp64, then the butterfly of wave_ops.hpp and one store by lane 0.  No LDS, no atomics, no scratch; r comes from the
// vector cache, which the waves of the workgroup share.
//
// The setup is one-time code over the workspace W = [B | I]: n rows of 2 ld doubles (ld = n rounded up to a multiple of 4: a row
// starts 32-byte aligned and holds whole pairs of doubles), B in the columns 0 ... n - 1 and I in ld ... ld + n - 1, and behind it
// the vector f of ld doubles.  The launches, all on one stream, each reading only what an EARLIER launch wrote or what its own
// thread (its own workgroup behind a barrier, in the pivot kernel) wrote:
//     coarse_init_kernel       W <- [0 | I], status <- {0, -1, 0}
//     coarse_densify_kernel    a lane per row adds the row's entries in stored order; the entries skipped are counted
//     for c = 0 ... n - 1:
//         coarse_pivot_kernel<<<1>>>    the search down column c, f <- column c as it stands behind the swap, then the swap of the
//                                       rows c and p fused with the scaling of the new row c; a zero pivot sets status[0] instead
//         coarse_update_kernel          every row i != c: W[i][j] <- W[i][j] - f[i] W[c][j]
//     coarse_store_kernel<T>   the right half, or the identity, rounded to T; the padding columns +0.0
// Every launch behind a zero pivot tests status[0] and does nothing.
//
// Column c of B is not read again behind the copy into f, and the columns in front of it have not been since their own steps:
// both kernels of step c work on the columns from c & ~1 on (whole pairs).  Every element that is ever read again sees exactly
// the operations of the header in their order; the padding columns of W take part in the row operations and are never stored.
//
// Why no launch reads what another workgroup of the same launch writes.  The pivot kernel is ONE workgroup.  Its reads of column
// c (the search, the copy into f, the pivot into LDS) all precede a barrier, its writes of the rows c and p follow it, and a
// value that has been stored on, or compared, has been loaded; behind the barrier a thread reads and writes its own columns of
// the two rows alone.  The update kernel writes the rows i != c from column c & ~1 on, each element by the one thread that read
// it; beside its own element a thread reads f and row c, which no thread of this launch writes (f exists for this: W[i][c] is
// overwritten by whichever thread owns it).
#pragma once

#include "wave_ops.hpp"

namespace spmv {

constexpr int kCoarseMaxN = 2048; // SPMV_HIP_COARSE_MAX_N
constexpr int kCoarseRows = 16;   // rows of one workgroup of the update: 4 of each of its 4 waves
constexpr int kCoarsePivotThreads = 256;

// the elements of a row of the inverse, and half the doubles of a row of W
__host__ __device__ constexpr int coarse_ld(int n) { return n <= 0 ? 0 : (n + 3) & ~3; }

template <class T>
__global__ __launch_bounds__(256, 8) void coarse_apply_kernel(int n, int ld, const T * __restrict__ inv, const T * __restrict__ r, T * __restrict__ z)
{
    const int i = (int) (blockIdx.x * 4 + threadIdx.x / kWave); // wave-uniform: a wave leaves whole
    if (i >= n)
        return;
    const int lane = (int) (threadIdx.x % kWave);
    const T * row = inv + (size_t) i * ld;
    double s = 0.0;
#pragma unroll 4
    for (int j = lane; j < n; j += kWave)
        s += (double) row[j] * (double) r[j];
    s = group_sum<kWave>(s); // every lane of the wave is active
    if (lane == 0)
        z[i] = (T) s;
}

// W <- [0 | I] over n rows of 2 ld doubles; status <- {not singular, no column, nothing skipped}
__global__ __launch_bounds__(256) void coarse_init_kernel(int n, int ld, double * __restrict__ w, int * __restrict__ status)
{
    const long long e = (long long) blockIdx.x * 256 + threadIdx.x;
    if (e < 3)
        status[e] = e == 1 ? -1 : 0;
    if (e < (long long) n * 2 * ld) {
        const int i = (int) (e / (2 * ld)), j = (int) (e % (2 * ld));
        w[e] = j == ld + i ? 1.0 : 0.0;
    }
}

// a lane per row: its entries in stored order; a column outside 0 ... n - 1 is counted, not followed
__global__ __launch_bounds__(256) void coarse_densify_kernel(int n, int ld, const int * __restrict__ row_ptr, const int * __restrict__ column_index,
                                                             const double * __restrict__ value, double * __restrict__ w, int * __restrict__ status)
{
    const int i = (int) (blockIdx.x * 256 + threadIdx.x);
    if (i >= n)
        return;
    double * row = w + (size_t) i * 2 * ld;
    int skipped = 0;
    for (long long at = row_ptr[i], end = row_ptr[i + 1]; at < end; ++at) {
        const int col = column_index[at];
        if (col < 0 || col >= n)
            ++skipped;
        else
            row[col] += value[at];
    }
    if (skipped)
        atomicAdd(status + 2, skipped);
}

// step c, one workgroup: the pivot row, f, the swap and the scaling (the file's head has the order of its reads and writes)
__global__ __launch_bounds__(kCoarsePivotThreads) void coarse_pivot_kernel(int n, int ld, int c, double * __restrict__ w, double * __restrict__ f,
                                                                          int * __restrict__ status)
{
    __shared__ double best_of[kCoarsePivotThreads];
    __shared__ int row_of[kCoarsePivotThreads];
    __shared__ double pivot_value;
    if (status[0] != 0) // a zero pivot in front of this column: every thread alike
        return;
    const int t = (int) threadIdx.x;
    const size_t stride = (size_t) 2 * ld;
    // the first row >= c with the largest |.|: a NaN is no candidate, and a NaN in row c itself keeps row c
    double best = -1.0;
    int p = n;
    for (int i = c + t; i < n; i += kCoarsePivotThreads) {
        const double a = fabs(w[i * stride + c]);
        if (a > best) { // rows ascending inside a thread: the first of equals stays
            best = a;
            p = i;
        }
    }
    best_of[t] = best;
    row_of[t] = p;
    __syncthreads();
    for (int half = kCoarsePivotThreads / 2; half > 0; half /= 2) {
        if (t < half) {
            const double b2 = best_of[t + half];
            const int p2 = row_of[t + half];
            if (b2 > best_of[t] || (b2 == best_of[t] && p2 < row_of[t])) {
                best_of[t] = b2;
                row_of[t] = p2;
            }
        }
        __syncthreads();
    }
    if (t == 0) {
        const double own = w[c * stride + c];
        if (own != own)
            row_of[0] = c;
        pivot_value = w[row_of[0] * stride + c];
    }
    __syncthreads();
    p = row_of[0];
    const double pivot = pivot_value;
    if (pivot == 0.0) {
        if (t == 0) {
            status[0] = 1;
            status[1] = c;
        }
        return;
    }
    // f <- column c behind the swap (f[c] is not read)
    for (int i = t; i < n; i += kCoarsePivotThreads)
        if (i != c)
            f[i] = w[(i == p ? c : i) * stride + c];
    __syncthreads();
    const double scale = 1.0 / pivot;
    double2 * rc = reinterpret_cast<double2 *>(w + c * stride);
    double2 * rp = reinterpret_cast<double2 *>(w + p * stride);
    for (int g = (c >> 1) + t; g < ld; g += kCoarsePivotThreads) { // pairs from column c & ~1 to 2 ld
        const double2 old = rc[g], e = rp[g];
        if (p != c)
            rp[g] = old;
        rc[g] = double2{e.x * scale, e.y * scale};
    }
}

// step c, the rows i != c: a thread takes one pair of columns (from c & ~1 on) of 4 rows, the pair of the pivot row in registers
__global__ __launch_bounds__(256) void coarse_update_kernel(int n, int ld, int c, double * __restrict__ w, const double * __restrict__ f,
                                                            const int * __restrict__ status)
{
    if (status[0] != 0)
        return;
    const int g = (c >> 1) + (int) (blockIdx.x * kWave + threadIdx.x % kWave);
    if (g >= ld)
        return;
    const size_t stride = (size_t) ld; // in pairs
    double2 * wp = reinterpret_cast<double2 *>(w);
    const double2 e = wp[c * stride + g];
    const int i0 = (int) (blockIdx.y * kCoarseRows + threadIdx.x / kWave * (kCoarseRows / 4));
#pragma unroll
    for (int k = 0; k < kCoarseRows / 4; ++k) {
        const int i = i0 + k;
        if (i < n && i != c) {
            const double fi = f[i];
            const double2 v = wp[i * stride + g];
            wp[i * stride + g] = double2{v.x - fi * e.x, v.y - fi * e.y};
        }
    }
}

// inv <- the right half of W rounded to T, or the identity behind a zero pivot; the padding columns +0.0
template <class T>
__global__ __launch_bounds__(256) void coarse_store_kernel(int n, int ld, const double * __restrict__ w, const int * __restrict__ status,
                                                           T * __restrict__ inv)
{
    const int e = (int) (blockIdx.x * 256 + threadIdx.x);
    if (e >= n * ld)
        return;
    const int i = e / ld, j = e % ld;
    const bool singular = status[0] != 0;
    inv[e] = j >= n ? (T) 0.0 : singular ? (T) (i == j ? 1.0 : 0.0) : (T) w[(size_t) i * 2 * ld + ld + j];
}

} // namespace spmv
