// gmres_updates.hpp -- the kernels of restarted GMRES with classical Gram-Schmidt applied twice (include/spmv_hip_gmres.h), over
// the cut of krylov_stream.hpp.
//
//   project   h[j] = V_j' w, h[k] = w' w.  The basis is blocked in registers, at most kGmresBlock vectors at a time: the chunk is the outer
//             loop and the block the inner one, so every V_j is streamed once and the chunk's w (8 KiB, 4 KiB of floats) is read
//             again from cache.  w itself is vector k of the last block.  A lane keeps one sum per vector of the block; at the
//             block's end each is added over the wave by one butterfly and stored in the slot of (vector, chunk).  What a sum
//             holds is the same whichever block its vector falls in.
//   axpys     one running value per element, V_j streamed with j ascending and its coefficient in scalar registers: the update
//             (w -= sum h_j V_j in place, with the sum of the squares of w as stored in the slot of its chunk) and the
//             correction (x += u or x += m u, u = sum y_j V_j).  A lane keeps the running values of its WHOLE share of the chunk
//             (16 elements) and reads a vector's 8 KiB of the chunk in one go, two vectors in flight: passes of a quarter of the
//             chunk over all vectors, returning to every vector four times, ran a quarter slower at k = 16.
//   scale     v *= scale[0] in place and, with minv, vhat = m v: element-wise, on krylov_stream.
//   reduce    dots_reduce_block (csr_dots.hpp) over the slots of each pair of vectors: the order of dots_reduce for that many slots.
//   start, column, solve   the Hessenberg bookkeeping of one cycle, one workgroup each.
//
// No atomics and no counters; no LDS in project, axpys and scale; every offset is 64-bit (in project's whole chunks: a 64-bit
// wave-uniform base per vector and chunk, and the lane's byte offset inside the chunk).
#pragma once

#include "cg_updates.hpp"

namespace spmv {

constexpr int kGmresBlock = 8;     // vectors of the basis whose sums a lane keeps at once
constexpr int kGmresMaxBasis = 32; // SPMV_HIP_GMRES_MAX_BASIS

// vector j of the extended basis of a projection: V_j for j < k, w itself for j == k
template <class T>
__device__ __forceinline__ const T * gmres_vector(const T * V, long long ldv, const T * w, int k, int j)
{
    return j < k ? V + (long long) j * ldv : w;
}

// the sums of NB vectors, the first of them vector j0, over one chunk; every lane of the wave arrives at the butterflies
template <class T, int NB>
__device__ __forceinline__ void gmres_project_block(long long n, long long chunk, int lane, int k, int j0, const T * V, long long ldv, const T * w,
                                                    double * __restrict__ slots, long long stride)
{
    typedef typename KrylovGroup<T>::type G;
    constexpr int W = 16 / (int) sizeof(T);
    constexpr int GROUPS = kKrylovChunk / W;
    constexpr int PER_LANE = GROUPS / kWave;
    const G * wg = reinterpret_cast<const G *>(w);
    const G * vg[NB];
    const T * ve[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        ve[b] = gmres_vector(V, ldv, w, k, j0 + b);
        vg[b] = reinterpret_cast<const G *>(ve[b]);
    }
    const long long g0 = chunk * GROUPS + lane;
    double sums[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b)
        sums[b] = 0.0;
    if ((chunk + 1) * kKrylovChunk <= n) {
        // the chunk's first byte of every vector is wave-uniform (64-bit, scalar registers); what a lane adds lies inside the chunk
        const long long first = chunk * kKrylovChunk * (long long) sizeof(T);
        const char * wb = reinterpret_cast<const char *>(w) + first;
        const char * vb[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b)
            vb[b] = reinterpret_cast<const char *>(ve[b]) + first;
        const unsigned lo = (unsigned) lane * 16u;
#pragma unroll 1
        for (int j = 0; j < PER_LANE; ++j) {
            const unsigned at = lo + (unsigned) j * (16u * kWave);
            G vv[NB];
#pragma unroll
            for (int b = 0; b < NB; ++b)
                vv[b] = *reinterpret_cast<const G *>(vb[b] + at);
            const G vw = *reinterpret_cast<const G *>(wb + at);
#pragma unroll
            for (int b = 0; b < NB; ++b)
#pragma unroll
                for (int c = 0; c < W; ++c)
                    sums[b] += (double) vv[b][c] * (double) vw[c];
        }
    } else { // the last chunk of a vector that does not fill it: whole groups below n, then the elements behind them
        const long long ngroups = n / W;
        for (int j = 0; j < PER_LANE; ++j) {
            const long long g = g0 + (long long) j * kWave;
            if (g < ngroups) {
                const G vw = wg[g];
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    const G vv = vg[b][g];
#pragma unroll
                    for (int c = 0; c < W; ++c)
                        sums[b] += (double) vv[c] * (double) vw[c];
                }
            }
        }
        const long long t = ngroups * W + lane; // fewer than W elements: lanes 0 ... W - 2 at the most
        if (t < n) {
            const double wv = (double) w[t];
#pragma unroll
            for (int b = 0; b < NB; ++b)
                sums[b] += (double) ve[b][t] * wv;
        }
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const double total = group_sum<kWave>(sums[b]);
        const int v = j0 + b;
        if (lane == 0) {
            double * slot = slots + ((long long) (v >> 1) * stride + chunk) * 2;
            slot[v & 1] = total;
            if (v == k && (v & 1) == 0)
                slot[1] = 0.0; // w' w alone in the last pair: the reduction adds both halves of a slot
        }
    }
}

// slots: for the pair of vectors (2 q, 2 q + 1) `stride` 16-byte slots, of which slot c holds the two sums of chunk c
template <class T>
__global__ __launch_bounds__(256) void gmres_project_kernel(long long n, int k, const T * V, long long ldv, const T * w, double * __restrict__ slots,
                                                            long long stride)
{
    const KrylovWave at = krylov_wave(n);
    if (!at.any)
        return;
    const long long chunk = at.chunk;
    const int lane = at.lane();
    // k + 1 vectors (w itself the last) in the fewest blocks of at most kGmresBlock, of equal size but for one vector: no
    // block of one or two vectors behind whole ones, whose few loads would leave the wave waiting on every pass
    const int total = k + 1, nblocks = (total + kGmresBlock - 1) / kGmresBlock;
    const int size = total / nblocks, larger = total % nblocks;
    int j0 = 0;
    for (int b = 0; b < nblocks; ++b) {
        const int nb = size + (b < larger ? 1 : 0);
        switch (nb) {
        case 1: gmres_project_block<T, 1>(n, chunk, lane, k, j0, V, ldv, w, slots, stride); break;
        case 2: gmres_project_block<T, 2>(n, chunk, lane, k, j0, V, ldv, w, slots, stride); break;
        case 3: gmres_project_block<T, 3>(n, chunk, lane, k, j0, V, ldv, w, slots, stride); break;
        case 4: gmres_project_block<T, 4>(n, chunk, lane, k, j0, V, ldv, w, slots, stride); break;
        case 5: gmres_project_block<T, 5>(n, chunk, lane, k, j0, V, ldv, w, slots, stride); break;
        case 6: gmres_project_block<T, 6>(n, chunk, lane, k, j0, V, ldv, w, slots, stride); break;
        case 7: gmres_project_block<T, 7>(n, chunk, lane, k, j0, V, ldv, w, slots, stride); break;
        default: gmres_project_block<T, kGmresBlock>(n, chunk, lane, k, j0, V, ldv, w, slots, stride); break;
        }
        j0 += nb;
    }
}

// Workgroup (b, q) adds a run of the slots of pair q.  h null: a first stage, its sum goes to slot out_first + b of the pair.
// h given: the last stage (one workgroup per pair), its two sums are h[2 q] and h[2 q + 1] where those lie below count.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void gmres_reduce_kernel(int n, int per_block, v2d * work, long long stride, long long in_first,
                                                               long long out_first, double * h, int count)
{
    const long long q = (long long) blockIdx.y;
    v2d * pair = work + q * stride;
    const v2d total = dots_reduce_block<THREADS>(n, per_block, pair + in_first, (long long) blockIdx.x);
    if (threadIdx.x != 0)
        return;
    if (!h) {
        pair[out_first + blockIdx.x] = total;
        return;
    }
    if (2 * q < count)
        h[2 * q] = total.x;
    if (2 * q + 1 < count)
        h[2 * q + 1] = total.y;
}

enum GmresAxpys { kGmresUpdate = 0, kGmresCorrect = 1, kGmresCorrectM = 2 };

// the running value of one element after vector j: the update starts from w, the correction from its first product
template <int MODE>
__device__ __forceinline__ double gmres_axpy_element(int j, double run, double coef, double v)
{
    if (MODE == kGmresUpdate)
        return run - coef * v;
    return j == 0 ? coef * v : run + coef * v;
}

template <class T, int MODE>
__device__ __forceinline__ T gmres_axpys_finish(double run, T old, T mv)
{
    if (MODE == kGmresUpdate)
        return (T) run;
    if (MODE == kGmresCorrect)
        return (T) ((double) old + run);
    return (T) ((double) old + (double) mv * run);
}

// MODE kGmresUpdate: y is w, in place, coef is h, and slots[chunk] = {sum of the squares of w as stored, +0.0}
// MODE kGmresCorrect, kGmresCorrectM: y is x, coef is y of the solve, k > 0
template <class T, int MODE>
__global__ __launch_bounds__(256, 4) void gmres_axpys_kernel(long long n, int k, const T * __restrict__ V, long long ldv,
                                                             const double * __restrict__ coef, T * __restrict__ y, const T * __restrict__ minv,
                                                             v2d * __restrict__ slots)
{
    typedef typename KrylovGroup<T>::type G;
    constexpr int W = 16 / (int) sizeof(T);
    constexpr int GROUPS = kKrylovChunk / W;
    constexpr int PER_LANE = GROUPS / kWave, U = PER_LANE, JU = 2; // the lane's whole share of the chunk, of JU vectors at a time
    static_assert(PER_LANE % U == 0, "whole passes");
    const KrylovWave at = krylov_wave(n);
    if (!at.any)
        return;
    const long long chunk = at.chunk;
    const int lane = at.lane();
    G * yg = reinterpret_cast<G *>(y);
    const G * mg = reinterpret_cast<const G *>(minv);
    const long long g0 = chunk * GROUPS + lane;
    double sums[2] = {0.0, 0.0};
    if ((chunk + 1) * kKrylovChunk <= n) {
#pragma unroll 1
        for (int p = 0; p < PER_LANE; p += U) {
            double run[U][W]; // the update's w; the correction starts from its first product, and reads x and m last
#pragma unroll
            for (int u = 0; u < U; ++u) {
                G vw = G{};
                if (MODE == kGmresUpdate)
                    vw = yg[g0 + (long long) (p + u) * kWave];
#pragma unroll
                for (int c = 0; c < W; ++c)
                    run[u][c] = (double) vw[c];
            }
            int j = 0;
#pragma unroll 1
            for (; j + JU <= k; j += JU) {
                G vv[JU][U];
#pragma unroll
                for (int b = 0; b < JU; ++b) {
                    const G * vg = reinterpret_cast<const G *>(V + (long long) (j + b) * ldv);
#pragma unroll
                    for (int u = 0; u < U; ++u)
                        vv[b][u] = vg[g0 + (long long) (p + u) * kWave];
                }
#pragma unroll
                for (int b = 0; b < JU; ++b) {
                    const double cj = coef[j + b];
#pragma unroll
                    for (int u = 0; u < U; ++u)
#pragma unroll
                        for (int c = 0; c < W; ++c)
                            run[u][c] = gmres_axpy_element<MODE>(j + b, run[u][c], cj, (double) vv[b][u][c]);
                }
            }
#pragma unroll 1
            for (; j < k; ++j) {
                const G * vg = reinterpret_cast<const G *>(V + (long long) j * ldv);
                const double cj = coef[j];
                G vv[U];
#pragma unroll
                for (int u = 0; u < U; ++u)
                    vv[u] = vg[g0 + (long long) (p + u) * kWave];
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int c = 0; c < W; ++c)
                        run[u][c] = gmres_axpy_element<MODE>(j, run[u][c], cj, (double) vv[u][c]);
            }
            G vy[U], vm[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long long g = g0 + (long long) (p + u) * kWave;
                if (MODE != kGmresUpdate)
                    vy[u] = yg[g];
                if (MODE == kGmresCorrectM)
                    vm[u] = mg[g];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int c = 0; c < W; ++c) {
                    const T stored = gmres_axpys_finish<T, MODE>(run[u][c], MODE != kGmresUpdate ? vy[u][c] : (T) 0,
                                                                 MODE == kGmresCorrectM ? vm[u][c] : (T) 0);
                    vy[u][c] = stored;
                    if (MODE == kGmresUpdate)
                        sums[0] += (double) stored * (double) stored;
                }
                yg[g0 + (long long) (p + u) * kWave] = vy[u];
            }
        }
    } else { // the last chunk of a vector that does not fill it: whole groups below n, then the elements behind them
        const long long ngroups = n / W;
        for (int p = 0; p < PER_LANE; ++p) {
            const long long g = g0 + (long long) p * kWave;
            if (g < ngroups) {
                G vy = yg[g], vm = vy;
                if (MODE == kGmresCorrectM)
                    vm = mg[g];
                double run[W];
#pragma unroll
                for (int c = 0; c < W; ++c)
                    run[c] = (double) vy[c];
                for (int j = 0; j < k; ++j) {
                    const G vv = reinterpret_cast<const G *>(V + (long long) j * ldv)[g];
                    const double cj = coef[j];
#pragma unroll
                    for (int c = 0; c < W; ++c)
                        run[c] = gmres_axpy_element<MODE>(j, run[c], cj, (double) vv[c]);
                }
#pragma unroll
                for (int c = 0; c < W; ++c) {
                    const T stored = gmres_axpys_finish<T, MODE>(run[c], vy[c], vm[c]);
                    vy[c] = stored;
                    if (MODE == kGmresUpdate)
                        sums[0] += (double) stored * (double) stored;
                }
                yg[g] = vy;
            }
        }
        const long long t = ngroups * W + lane; // fewer than W elements: lanes 0 ... W - 2 at the most
        if (t < n) {
            const T old = y[t];
            double run = (double) old;
            for (int j = 0; j < k; ++j)
                run = gmres_axpy_element<MODE>(j, run, coef[j], (double) V[(long long) j * ldv + t]);
            const T stored = gmres_axpys_finish<T, MODE>(run, old, MODE == kGmresCorrectM ? minv[t] : (T) 0);
            y[t] = stored;
            if (MODE == kGmresUpdate)
                sums[0] += (double) stored * (double) stored;
        }
    }
    if (MODE == kGmresUpdate)
        store_wave_dots(slots, (int) chunk, sums); // every lane of the wave is active again
}

template <class T, bool HASM>
__device__ __forceinline__ void gmres_scale_element(double s, T mv, T & v, T & vhat)
{
    v = (T) ((double) v * s);
    if (HASM)
        vhat = (T) ((double) mv * (double) v);
}

// v <- v scale[0] in place; with minv: vhat <- m v, v as stored
template <class T, bool HASM>
__global__ __launch_bounds__(256, 8) void gmres_scale_kernel(long long n, const double * __restrict__ scale, T * __restrict__ v,
                                                             const T * __restrict__ minv, T * __restrict__ vhat)
{
    const KrylovWave at = krylov_wave(n);
    if (!at.any)
        return;
    const double s = scale[0];
    const T * const arrays[] = {v, minv, vhat};
    krylov_stream<T, HASM ? 2 : 4, false, kKrylovUpdate, HASM ? kKrylovRead : kKrylovAbsent, HASM ? kKrylovWrite : kKrylovAbsent>(
        n, at, arrays, [&](T * e) { gmres_scale_element<T, HASM>(s, e[1], e[0], e[2]); });
}

// ---- the state of one cycle (include/spmv_hip_gmres.h documents the layout) --------------------------------------------------------

__host__ __device__ constexpr int gmres_state_g(int) { return 2; }
__host__ __device__ constexpr int gmres_state_c(int m) { return 3 + m; }
__host__ __device__ constexpr int gmres_state_s(int m) { return 3 + 2 * m; }
__host__ __device__ constexpr int gmres_state_r(int m) { return 3 + 3 * m; }
__host__ __device__ constexpr int gmres_state_doubles(int m) { return (3 + 3 * m + m * (m + 1) / 2 + 1) & ~1; }

// g = beta e_1, state[0] = beta, state[1] = 1 / beta
__global__ __launch_bounds__(64) void gmres_start_kernel(int m, const double * __restrict__ nrm2, double * __restrict__ state)
{
    const int t = (int) threadIdx.x;
    const double beta = sqrt(nrm2[0]);
    if (t == 0) {
        state[0] = beta;
        state[1] = 1.0 / beta;
    }
    if (t <= m)
        state[gmres_state_g(m) + t] = t == 0 ? beta : 0.0;
}

// column k of the Hessenberg matrix through the k stored rotations and a new one; the sequential part is thread 0's
__global__ __launch_bounds__(64) void gmres_column_kernel(int k, int m, const double * __restrict__ h1, const double * __restrict__ h2,
                                                          const double * nrm2, double * state)
{
    __shared__ double h[kGmresMaxBasis + 1];
    const int t = (int) threadIdx.x;
    if (t <= k)
        h[t] = h1[t] + h2[t];
    __syncthreads();
    if (t != 0)
        return;
    double * g = state + gmres_state_g(m);
    double * cs = state + gmres_state_c(m);
    double * sn = state + gmres_state_s(m);
    double * col = state + gmres_state_r(m) + k * (k + 1) / 2;
    const double below = sqrt(nrm2[0]);
    for (int i = 0; i < k; ++i) {
        const double c = cs[i], s = sn[i], a = h[i], b = h[i + 1];
        h[i] = c * a + s * b;
        h[i + 1] = c * b - s * a;
    }
    const double a = h[k];
    const double d = sqrt(a * a + below * below);
    const double c = a / d, s = below / d;
    cs[k] = c;
    sn[k] = s;
    h[k] = c * a + s * below;
    for (int i = 0; i <= k; ++i)
        col[i] = h[i];
    const double gk = g[k];
    const double next = -(s * gk);
    g[k] = c * gk;
    g[k + 1] = next;
    state[0] = fabs(next);
    state[1] = 1.0 / below;
}

// y = R[0:k, 0:k]^-1 g[0:k]: one thread, rows from k - 1 down, columns ascending
__global__ __launch_bounds__(64) void gmres_solve_kernel(int k, int m, const double * __restrict__ state, double * __restrict__ y)
{
    if (threadIdx.x != 0)
        return;
    const double * g = state + gmres_state_g(m);
    const double * R = state + gmres_state_r(m);
    for (int i = k - 1; i >= 0; --i) {
        double acc = g[i];
        for (int j = i + 1; j < k; ++j)
            acc -= R[j * (j + 1) / 2 + i] * y[j];
        y[i] = acc / R[i * (i + 1) / 2 + i];
    }
}

} // namespace spmv
