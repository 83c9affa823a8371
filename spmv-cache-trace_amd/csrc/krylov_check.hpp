// krylov_check.hpp -- what bicgstab.hip takes from krylov.hip: the workspace rule of a step's dots and the table-driven check of
// the arrays of one call (include/spmv_hip_krylov.h, include/spmv_hip_bicgstab.h).
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

} // namespace spmvi
