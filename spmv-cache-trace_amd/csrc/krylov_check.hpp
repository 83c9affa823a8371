// krylov_check.hpp -- what bicgstab.hip, gmres.hip, bjacobi.hip, cheby.hip, mcgs.hip and agg.hip take from krylov.hip: the workspace rule of a step's dots, the
// table-driven check of the arrays of one call and the launch over the chunk grid of krylov_stream.hpp
// (include/spmv_hip_krylov.h, include/spmv_hip_bicgstab.h, include/spmv_hip_gmres.h, include/spmv_hip_bjacobi.h, include/spmv_hip_cheby.h,
// include/spmv_hip_mcgs.h, include/spmv_hip_agg.h).
#pragma once

#include "f32_plan.hpp"

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

} // namespace spmvi
