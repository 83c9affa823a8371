// krylov_stream.hpp -- the cut of a vector that every Krylov update kernel streams over (cg_updates.hpp, bicgstab_updates.hpp,
// gmres_updates.hpp, bjacobi_kernels.hpp, cheby_updates.hpp, the dots pass of mcgs_kernels.hpp), written once.  The kernels are shaped as triad_kernel is -- 16-byte loads and stores,
// several independent loads per lane in flight -- over a FIXED cut: chunk c = elements [c kKrylovChunk, (c + 1) kKrylovChunk)
// belongs to wave c of the grid (four to a workgroup), and lane l of that wave takes the 16-byte groups l, l + 64, ... of the
// chunk in that order.  Whole chunks run in unrolled passes of U groups per array without a bounds test; the last chunk of a
// vector that does not fill it runs in a tested loop, and the up to 3 elements behind the vector's last whole group go last, to
// lanes 0, 1, 2 of that chunk.  A kernel with sums keeps them in registers -- groups in that order, the elements of a group
// ascending, the tail element last -- adds the 64 lanes by one butterfly and stores them in slot c (store_wave_dots,
// csr_dots.hpp: every lane of the wave is active again by then); dots_reduce_kernel adds the slots behind it.  No LDS, no
// barrier, no atomics; every offset is 64-bit.
//
// krylov_wave is the prologue of all ten kernels.  krylov_stream is the whole body of the element-wise ones: it owns the arrays,
// the vector registers and the three paths, and calls the kernel's function on the SCALARS of one element (functors
// over structs of whole vectors spill).
#pragma once

#include "csr_dots.hpp"

namespace spmv {

constexpr int kKrylovChunk = 1024; // SPMV_HIP_KRYLOV_CHUNK: elements per wave and per slot

template <class T>
struct KrylovGroup;
template <>
struct KrylovGroup<double> {
    typedef v2d type;
};
template <>
struct KrylovGroup<float> {
    typedef v4f type;
};

// The wave's chunk, whether the chunk has an element -- a wave without one returns whole: no slot behind the last element -- and
// the lane, which is formed where it is asked for, behind that return (bjacobi_apply_kernel's pinned registers depend on it).
struct KrylovWave {
    long long chunk;
    bool any;
    __device__ __forceinline__ int lane() const { return (int) threadIdx.x & (kWave - 1); }
};

__device__ __forceinline__ KrylovWave krylov_wave(long long n)
{
    const int wave = __builtin_amdgcn_readfirstlane((int) threadIdx.x >> 6);
    const long long chunk = (long long) blockIdx.x * 4 + wave;
    return KrylovWave{chunk, chunk * kKrylovChunk < n};
}

// what krylov_stream does with an array: an absent one (a null minv, the output that goes with it) has no load and no store
enum KrylovAccess { kKrylovAbsent = 0, kKrylovRead = 1, kKrylovWrite = 2, kKrylovUpdate = 3 };

// UU groups of every array, kWave apart from group g on: all loads, then f on each element's scalars, then the stores
template <class T, int UU, int... ACCESS, class F>
__device__ __forceinline__ void krylov_groups(const T * const (&array)[sizeof...(ACCESS)], long long g, const F & f)
{
    typedef typename KrylovGroup<T>::type G;
    constexpr int W = 16 / (int) sizeof(T); // elements of a group
    constexpr int N = sizeof...(ACCESS), access[] = {ACCESS...};
    G v[N][UU];
#pragma unroll
    for (int u = 0; u < UU; ++u)
#pragma unroll
        for (int k = 0; k < N; ++k)
            if (access[k] & kKrylovRead)
                v[k][u] = reinterpret_cast<const G *>(array[k])[g + (long long) u * kWave];
#pragma unroll
    for (int u = 0; u < UU; ++u) {
#pragma unroll
        for (int c = 0; c < W; ++c) {
            T e[N];
#pragma unroll
            for (int k = 0; k < N; ++k)
                e[k] = access[k] & kKrylovRead ? v[k][u][c] : (T) 0;
            f(e);
#pragma unroll
            for (int k = 0; k < N; ++k)
                if (access[k] & kKrylovWrite)
                    v[k][u][c] = e[k];
        }
#pragma unroll
        for (int k = 0; k < N; ++k)
            if (access[k] & kKrylovWrite)
                reinterpret_cast<G *>(const_cast<T *>(array[k]))[g + (long long) u * kWave] = v[k][u];
    }
}

// The wave's chunk of an element-wise update.  array: the kernel's vectors in the order a pass loads them, ACCESS what is done
// with each; f(e) takes the scalars of one element, e[k] of array k ((T) 0 where it is not read), leaves what is to be stored in
// them and may add to the lane's sums.  ROLLED: the tested loop of the last chunk is not unrolled.
template <class T, int U, bool ROLLED, int... ACCESS, class F>
__device__ __forceinline__ void krylov_stream(long long n, const KrylovWave & at, const T * const (&array)[sizeof...(ACCESS)], const F & f)
{
    constexpr int W = 16 / (int) sizeof(T);
    constexpr int GROUPS = kKrylovChunk / W; // groups of a chunk
    constexpr int PER_LANE = GROUPS / kWave;
    constexpr int N = sizeof...(ACCESS), access[] = {ACCESS...};
    static_assert(PER_LANE % U == 0, "whole passes");
    const long long g0 = at.chunk * GROUPS + at.lane();
    if ((at.chunk + 1) * kKrylovChunk <= n) {
#pragma unroll 1
        for (int j = 0; j < PER_LANE; j += U)
            krylov_groups<T, U, ACCESS...>(array, g0 + (long long) j * kWave, f);
        return;
    }
    // the last chunk of a vector that does not fill it: whole groups below n, then the elements behind them
    const long long ngroups = n / W;
    auto tested = [&](int j) {
        const long long g = g0 + (long long) j * kWave;
        if (g < ngroups)
            krylov_groups<T, 1, ACCESS...>(array, g, f);
    };
    if constexpr (ROLLED) {
#pragma unroll 1
        for (int j = 0; j < PER_LANE; ++j)
            tested(j);
    } else {
        for (int j = 0; j < PER_LANE; ++j)
            tested(j);
    }
    const long long t = ngroups * W + at.lane(); // fewer than W elements: lanes 0 ... W - 2 at the most
    if (t < n) {
        T e[N];
#pragma unroll
        for (int k = 0; k < N; ++k)
            e[k] = access[k] & kKrylovRead ? array[k][t] : (T) 0;
        f(e);
#pragma unroll
        for (int k = 0; k < N; ++k)
            if (access[k] & kKrylovWrite)
                const_cast<T *>(array[k])[t] = e[k];
    }
}

} // namespace spmv
