// krylov_check.hpp -- what bicgstab.hip, gmres.hip, bjacobi.hip, cheby.hip, mcgs.hip and agg.hip take from krylov.hip: the workspace rule of a step's dots, the
// table-driven check of the arrays of one call and the launch over the chunk grid of krylov_stream.hpp
// (include/spmv_hip_krylov.h, include/spmv_hip_bicgstab.h, include/spmv_hip_gmres.h, include/spmv_hip_bjacobi.h, include/spmv_hip_cheby.h,
// include/spmv_hip_mcgs.h, include/spmv_hip_agg.h).  Behind them, what the one-time setup code of mcgs.hip and agg.hip shares: the
// rounding of a workspace piece, the grid of a lane per row, the dispatch on a lane group and the host side of the rounds of
// graph_rounds.hpp.
#pragma once

#include "f32_plan.hpp"

#include <type_traits>

namespace spmvi {

// one 16-byte slot per chunk of SPMV_HIP_KRYLOV_CHUNK elements ...
long long krylov_slots(long long n);
// ... then one per workgroup of the reduction's first stage: spmv_hip_krylov_workspace
size_t krylov_bytes(long long n);

// one array of a call: a null one is neither aligned nor compared
struct KrylovArray {
    const void * p;
    unsigned long long bytes;
    bool written;
    int align;
    const char * name;
};

// what the updates refuse, in the order of spmv_hip_dots.h: null, (the workspace's size: the caller), alignment, 4 GiB, overlaps
int krylov_check_arrays(int32_t n, size_t elem, const KrylovArray * arrays, int count);

// the workspace's size, where the caller looks at it: "work_bytes is ... and <what> needs ... (<rule>)", rule the function that tells
int krylov_check_work(size_t work_bytes, size_t need, const char * what, const char * rule);

// workgroups of four waves, a wave per chunk and slot
inline unsigned krylov_blocks(long long slots) { return (unsigned) ((slots + 3) / 4); }

// one launch of `kernel` over the chunk grid on s, every argument converted to its parameter's type; no slot, no launch
template <class... P, class... A>
int krylov_launch(void (*kernel)(P...), long long slots, hipStream_t s, A... args)
{
    if (slots == 0)
        return SPMV_HIP_OK;
    hipLaunchKernelGGL(kernel, dim3(krylov_blocks(slots)), dim3(256), 0, s, static_cast<P>(args)...);
    HIP_TRY(hipGetLastError());
    return SPMV_HIP_OK;
}

// ---- what the one-time setup code of mcgs.hip and agg.hip shares ------------------------------------------------------------------

inline size_t up16(size_t b) { return (b + 15) & ~(size_t) 15; }
inline unsigned blocks_of(long long threads) { return (unsigned) ((threads + 255) / 256); }

// f(std::integral_constant<int, G>()) for the power of two G = group in 1 ... 64 (the caller has refused every other group)
template <class F>
void dispatch_group(int group, F f)
{
    switch (group) {
    case 1: f(std::integral_constant<int, 1>()); break;
    case 2: f(std::integral_constant<int, 2>()); break;
    case 4: f(std::integral_constant<int, 4>()); break;
    case 8: f(std::integral_constant<int, 8>()); break;
    case 16: f(std::integral_constant<int, 16>()); break;
    case 32: f(std::integral_constant<int, 32>()); break;
    default: f(std::integral_constant<int, 64>()); break;
    }
}

// The host side of the rounds of graph_rounds.hpp until every one of `rows` rows is decided: a round zeroes *d_counter, launches
// its kernels (launch_round(), which returns a code), copies the counter back and synchronises.  The largest remaining key
// always wins, so a round that decided no row, or more than were left, saw arrays that changed under the call or are not a CSR
// matrix: SPMV_HIP_ERR_STATE with `message`.  *rounds <- their number.
template <class F>
int graph_rounds(long long rows, int * d_counter, hipStream_t s, const char * message, F launch_round, int * rounds)
{
    *rounds = 0;
    for (long long left = rows; left > 0; ++*rounds) {
        HIP_TRY(hipMemsetAsync(d_counter, 0, 4, s));
        const int rc = launch_round();
        if (rc != 0)
            return rc;
        int got = 0;
        HIP_TRY(hipMemcpyAsync(&got, d_counter, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (got <= 0 || got > left)
            return fail(SPMV_HIP_ERR_STATE, message);
        left -= got;
    }
    return SPMV_HIP_OK;
}

} // namespace spmvi
