// bjacobi_kernels.hpp -- the point-block Jacobi preconditioner (include/spmv_hip_bjacobi.h).
//
// bjacobi_apply_kernel<T, B, MODE> is a streaming kernel over the cut of krylov_stream.hpp.  Row i of the block-diagonal inverse
// is the B elements at inv + i B, so a lane's share of the inverse for one group of the vector is exactly B aligned 16-byte
// groups, and the wave's share for 64 groups is 64 B consecutive ones: the dominant stream is 16-byte loads of which every byte
// of every line is used.  A block's r entries straddle lanes, groups and chunks (1024 is no multiple of 3, 5, 6 or 7): unless
// the block lies in the lane's own group (B == 1, 2, and 4 in floats) they are loaded by address -- as 16-byte groups where a
// block is whole groups, as scalars otherwise -- and come from the vector cache, which neighbouring lanes and the lane's own
// group load have just filled: r leaves HBM once.  B is a template parameter: i / B is a multiplication and every register array
// is indexed statically.  No LDS, no barrier, no atomics; offsets into the inverse are 64-bit.
// MODE 0: z <- M^-1 r; MODE 1: ... with slots[chunk] = {sum z r, sum z z} of z as stored (store_wave_dots); MODE 2: z <- z + M^-1 r.
//
// bjacobi_setup_kernel<T> is one-time code: one wave (a workgroup of 64) per block.  The wave scans each of the block's rows 64
// entries at a time, adds the entries inside the block in stored order (one ballot per pass, then the hits in lane order), and
// inverts [B | I] in LDS by Gauss-Jordan with partial pivoting, lane l owning column l; the pivot search is done by every lane
// alike.  A zero pivot stores the identity and counts the block with integer atomics.
#pragma once

#include "cg_updates.hpp"

namespace spmv {

constexpr int kBJacobiMaxBlock = 8; // SPMV_HIP_BJACOBI_MAX_BLOCK

// the B entries of r from element kb on (kb a multiple of B): whole 16-byte groups where a block is, scalars otherwise
template <class T, int B>
__device__ __forceinline__ void bjacobi_load_block(const T * __restrict__ r, unsigned kb, T * out)
{
    typedef typename KrylovGroup<T>::type G;
    constexpr int W = 16 / (int) sizeof(T);
    if constexpr (B % W == 0) {
        const G * rg = reinterpret_cast<const G *>(r + kb);
#pragma unroll
        for (int q = 0; q < B / W; ++q) {
            const G v = rg[q];
#pragma unroll
            for (int c = 0; c < W; ++c)
                out[q * W + c] = v[c];
        }
    } else {
        const T * rp = r + kb; // one address, B immediate offsets
#pragma unroll
        for (int j = 0; j < B; ++j)
            out[j] = rp[j];
    }
}

// An entry of the inverse or of r as a double.  A float is converted where it is used, in program order: left to itself the compiler
// converts a group's W B floats as soon as they arrive, which takes twice their registers and spills.
__device__ __forceinline__ double bjacobi_wide(double v) { return v; }
__device__ __forceinline__ double bjacobi_wide(float v)
{
    asm volatile("" : "+v"(v));
    return (double) v;
}

// what is stored for one element, and its two products onto the lane's sums
template <class T, int MODE>
__device__ __forceinline__ T bjacobi_element(double s, T rv, T old, double * sums)
{
    const T stored = MODE == 2 ? (T) ((double) old + s) : (T) s;
    if (MODE == 1) {
        const double z = (double) stored;
        sums[0] += z * (double) rv;
        sums[1] += z * z;
    }
    return stored;
}

// one 16-byte group of the vector: W rows of the inverse (B groups), the r entries of their blocks, W elements stored.  Row c of
// the lane's share is its elements [c B, (c + 1) B), element e of the share being vi[e / W][e % W]; the sum is formed over j
// ascending from the first product on, every operand converted where it is used.
template <class T, int B, int MODE>
__device__ __forceinline__ void bjacobi_group(long long g, const typename KrylovGroup<T>::type * __restrict__ ig, const T * __restrict__ r,
                                              typename KrylovGroup<T>::type * zg, double * sums)
{
    typedef typename KrylovGroup<T>::type G;
    constexpr int W = 16 / (int) sizeof(T);
    G vi[B];
#pragma unroll
    for (int t = 0; t < B; ++t)
        vi[t] = ig[g * B + t];
    const G own = reinterpret_cast<const G *>(r)[g];
    G out;
    if (MODE == 2)
        out = zg[g];
    const unsigned e0 = (unsigned) g * W; // n sizeof(T) < 2^32: an element index is 32-bit
    // the r entries of the group's blocks: the lane's own group where a block lies in it (B divides W); one block where the group
    // lies in one (W divides B); the blocks of the first and of the last element where B > W otherwise (W consecutive elements
    // touch two blocks at the most; an element in between takes the one it belongs to); a block per element for B = 3 in floats
    constexpr bool OWN = W % B == 0, ONE = !OWN && B % W == 0, TWO = !OWN && !ONE && B > W;
    constexpr int NB = OWN ? 1 : ONE ? 1 : TWO ? 2 : W;
    T rb[NB][B];
    const unsigned last = (e0 + W - 1) / B * B;
    if constexpr (ONE) {
        bjacobi_load_block<T, B>(r, e0 / B * B, rb[0]);
    } else if constexpr (TWO) {
        bjacobi_load_block<T, B>(r, e0 / B * B, rb[0]);
        bjacobi_load_block<T, B>(r, last, rb[1]);
    } else if constexpr (!OWN) {
#pragma unroll
        for (int c = 0; c < W; ++c)
            bjacobi_load_block<T, B>(r, (e0 + c) / B * B, rb[c]);
    }
#pragma unroll
    for (int c = 0; c < W; ++c) {
        T rc[B];
#pragma unroll
        for (int j = 0; j < B; ++j) {
            if constexpr (OWN)
                rc[j] = own[c / B * B + j];
            else if constexpr (ONE)
                rc[j] = rb[0][j];
            else if constexpr (TWO)
                rc[j] = c == 0 ? rb[0][j] : c == W - 1 ? rb[1][j] : e0 + c >= last ? rb[1][j] : rb[0][j];
            else
                rc[j] = rb[c][j];
        }
        double s = bjacobi_wide(vi[c * B / W][c * B % W]) * bjacobi_wide(rc[0]);
#pragma unroll
        for (int j = 1; j < B; ++j)
            s += bjacobi_wide(vi[(c * B + j) / W][(c * B + j) % W]) * bjacobi_wide(rc[j]);
        out[c] = bjacobi_element<T, MODE>(s, own[c], MODE == 2 ? out[c] : (T) 0, sums);
    }
    zg[g] = out;
}

// waves per SIMD the registers are budgeted for: 8 as the conjugate-gradient kernels, but 7 (72 registers) for B = 7, 8 and for
// B = 6 in floats, and 6 (80) for B = 7 in floats: B 16-byte groups of the inverse, two blocks of r and the lane's own group are
// 60 registers and more before the first address.  These have six to eight 16-byte loads in flight per lane as it is.
template <class T, int B>
constexpr int bjacobi_waves()
{
    return B == 7 && sizeof(T) == 4 ? 6 : B >= 7 || (B == 6 && sizeof(T) == 4) ? 7 : 8;
}

template <class T, int B, int MODE>
__global__ __launch_bounds__(256, (bjacobi_waves<T, B>())) void bjacobi_apply_kernel(long long n, const T * __restrict__ inv, const T * __restrict__ r, T * z,
                                                               v2d * __restrict__ slots)
{
    typedef typename KrylovGroup<T>::type G;
    constexpr int W = 16 / (int) sizeof(T);
    constexpr int GROUPS = kKrylovChunk / W;
    constexpr int PER_LANE = GROUPS / kWave;
    const KrylovWave at = krylov_wave(n);
    if (!at.any)
        return;
    const long long chunk = at.chunk;
    const int lane = at.lane();
    const G * ig = reinterpret_cast<const G *>(inv);
    G * zg = reinterpret_cast<G *>(z);
    const long long g0 = chunk * GROUPS + lane;
    double sums[2] = {0.0, 0.0};
    if ((chunk + 1) * kKrylovChunk <= n) {
#pragma unroll 1
        for (int j = 0; j < PER_LANE; ++j)
            bjacobi_group<T, B, MODE>(g0 + (long long) j * kWave, ig, r, zg, sums);
    } else { // the last chunk of a vector that does not fill it: whole groups below n, then the elements behind them
        const long long ngroups = n / W;
        for (int j = 0; j < PER_LANE; ++j) {
            const long long g = g0 + (long long) j * kWave;
            if (g < ngroups)
                bjacobi_group<T, B, MODE>(g, ig, r, zg, sums);
        }
        const long long t = ngroups * W + lane; // fewer than W elements: lanes 0 ... W - 2 at the most
        if (t < n) {
            const unsigned kb = (unsigned) t / B * B;
            double s = (double) inv[t * B] * (double) r[kb];
#pragma unroll
            for (int j = 1; j < B; ++j)
                s += (double) inv[t * B + j] * (double) r[kb + j];
            z[t] = bjacobi_element<T, MODE>(s, r[t], MODE == 2 ? z[t] : (T) 0, sums);
        }
    }
    if (MODE == 1)
        store_wave_dots(slots, (int) chunk, sums); // every lane of the wave is active again
}

// status <- {0, -1}: no singular block yet
__global__ void bjacobi_status_kernel(int * __restrict__ status)
{
    if (threadIdx.x == 0) {
        status[0] = 0;
        status[1] = -1;
    }
}

template <class T>
__global__ __launch_bounds__(64) void bjacobi_setup_kernel(int b, const int * __restrict__ row_ptr, const int * __restrict__ column_index,
                                                           const double * __restrict__ value, T * __restrict__ inv, int * __restrict__ status)
{
    __shared__ double m[kBJacobiMaxBlock][2 * kBJacobiMaxBlock]; // [B | I]
    __shared__ int singular;
    const int lane = (int) threadIdx.x;
    const long long k = blockIdx.x;
    const long long kb = k * b;
    for (int e = lane; e < kBJacobiMaxBlock * 2 * kBJacobiMaxBlock; e += kWave) {
        const int i = e / (2 * kBJacobiMaxBlock), l = e % (2 * kBJacobiMaxBlock);
        m[i][l] = l == b + i ? 1.0 : 0.0;
    }
    if (lane == 0)
        singular = 0;
    __syncthreads();
    // extraction: the entries of each row inside the block, in stored order
    for (int i = 0; i < b; ++i) {
        const int begin = row_ptr[kb + i], end = row_ptr[kb + i + 1];
        for (long long base = begin; base < end; base += kWave) { // wave-uniform
            const long long at = base + lane;
            long long col = -1;
            double v = 0.0;
            if (at < end) {
                col = column_index[at];
                v = value[at];
            }
            const bool inside = col >= kb && col < kb + b;
            unsigned long long hits = __ballot(inside);
            while (hits) {
                const int src = __builtin_ctzll(hits);
                hits &= hits - 1;
                const int c = (int) (__shfl((int) (col - kb), src));
                const double add = __shfl(v, src);
                if (lane == 0)
                    m[i][c] += add;
            }
        }
    }
    __syncthreads();
    // Gauss-Jordan with partial pivoting, lane l owning column l of [B | I]
    for (int c = 0; c < b; ++c) {
        int p = c;
        double best = fabs(m[c][c]);
        for (int i = c + 1; i < b; ++i) {
            const double a = fabs(m[i][c]);
            if (a > best) {
                best = a;
                p = i;
            }
        }
        __syncthreads();
        if (lane < 2 * b && p != c) {
            const double u = m[c][lane];
            m[c][lane] = m[p][lane];
            m[p][lane] = u;
        }
        __syncthreads();
        const double pivot = m[c][c];
        if (pivot == 0.0) { // every lane alike
            if (lane == 0)
                singular = 1;
            break;
        }
        double f[kBJacobiMaxBlock];
#pragma unroll
        for (int i = 0; i < kBJacobiMaxBlock; ++i)
            f[i] = i < b ? m[i][c] : 0.0;
        __syncthreads();
        if (lane < 2 * b) {
            const double t = 1.0 / pivot;
            const double ec = m[c][lane] * t;
            m[c][lane] = ec;
#pragma unroll
            for (int i = 0; i < kBJacobiMaxBlock; ++i)
                if (i < b && i != c)
                    m[i][lane] = m[i][lane] - f[i] * ec;
        }
        __syncthreads();
    }
    __syncthreads();
    const bool bad = singular != 0;
    if (lane < b * b) {
        const int i = lane / b, j = lane % b;
        inv[kb * b + lane] = bad ? (T) (i == j ? 1.0 : 0.0) : (T) m[i][b + j];
    }
    if (bad && lane == 0) {
        atomicAdd(status, 1);
        atomicMin(reinterpret_cast<unsigned *>(status) + 1, (unsigned) k);
    }
}

} // namespace spmv
