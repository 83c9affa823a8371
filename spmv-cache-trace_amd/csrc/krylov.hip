// krylov.hip -- include/spmv_hip_krylov.h: the step and the direction of a conjugate-gradient iteration over caller-owned device
// vectors, their scalar a quotient of two doubles in device memory.  The kernels are cg_updates.hpp; the reduction of the step's
// slots is the one of the multiplies with dots (f32_plan.hpp: dots_reduce).  The workspace rule, the check of a call's arrays and
// the launch over the chunk grid are shared with bicgstab.hip, gmres.hip, bjacobi.hip and cheby.hip (krylov_check.hpp).
#include "spmv_hip_krylov.h"

#include "krylov_check.hpp"
#include "cg_updates.hpp"

#include <cstdio>

using namespace spmvi;

static_assert(spmv::kKrylovChunk == SPMV_HIP_KRYLOV_CHUNK, "the header documents the chunk");

namespace spmvi {

long long krylov_slots(long long n) { return (n + spmv::kKrylovChunk - 1) / spmv::kKrylovChunk; }

// one slot per chunk, then one per workgroup of the reduction's first stage
size_t krylov_bytes(long long n) { return dots_workspace_bytes((int) krylov_slots(n), 0); }

int krylov_check_arrays(int32_t n, size_t elem, const KrylovArray * arrays, int count)
{
    char text[160];
    for (int i = 0; i < count; ++i)
        if ((reinterpret_cast<uintptr_t>(arrays[i].p) & (uintptr_t) (arrays[i].align - 1)) != 0) {
            std::snprintf(text, sizeof text, "%s must be %d-byte aligned", arrays[i].name, arrays[i].align);
            return fail(SPMV_HIP_ERR_ALIGN, text);
        }
    if ((unsigned long long) n * elem >= (1ULL << 32))
        return fail(SPMV_HIP_ERR_INVALID, "the vectors span 4 GiB or more: the updates have no kernel for such vectors");
    for (int i = 0; i < count; ++i)
        for (int j = i + 1; j < count; ++j)
            if ((arrays[i].written || arrays[j].written) && overlap(arrays[i].p, arrays[i].bytes, arrays[j].p, arrays[j].bytes)) {
                std::snprintf(text, sizeof text, "%s and %s overlap, and one of them is written", arrays[i].name, arrays[j].name);
                return fail(SPMV_HIP_ERR_INVALID, text);
            }
    return SPMV_HIP_OK;
}

int krylov_check_work(size_t work_bytes, size_t need, const char * what, const char * rule)
{
    if (work_bytes >= need)
        return SPMV_HIP_OK;
    char text[160];
    std::snprintf(text, sizeof text, "work_bytes is %zu and %s needs %zu (%s)", work_bytes, what, need, rule);
    return fail(SPMV_HIP_ERR_INVALID, text);
}

} // namespace spmvi

namespace {

template <class T>
int cg_step(int32_t n, const double * d_num, const double * d_den, const T * d_p, const T * d_q, T * d_x, T * d_r, const T * d_minv, double * d_dots,
            void * d_work, size_t work_bytes, void * stream)
{
    if (n < 0)
        return fail(SPMV_HIP_ERR_INVALID, "n < 0");
    if (!d_num || !d_den || !d_p || !d_q || !d_x || !d_r || !d_dots || !d_work)
        return fail(SPMV_HIP_ERR_INVALID, "null device pointer (only d_minv may be null)");
    const size_t need = krylov_bytes(n);
    int rc = krylov_check_work(work_bytes, need, "n", "spmv_hip_krylov_workspace");
    if (rc != 0)
        return rc;
    const unsigned long long vec = (unsigned long long) n * sizeof(T);
    const KrylovArray arrays[] = {{d_p, vec, false, 16, "d_p"},       {d_q, vec, false, 16, "d_q"},       {d_x, vec, true, 16, "d_x"},
                                  {d_r, vec, true, 16, "d_r"},        {d_minv, vec, false, 16, "d_minv"}, {d_dots, 16, true, 16, "d_dots"},
                                  {d_work, need, true, 16, "d_work"}, {d_num, 8, false, 8, "d_num"},      {d_den, 8, false, 8, "d_den"}};
    rc = krylov_check_arrays(n, sizeof(T), arrays, (int) (sizeof arrays / sizeof arrays[0]));
    if (rc != 0)
        return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long long slots = krylov_slots(n);
    rc = krylov_launch(d_minv ? spmv::cg_step_kernel<T, true> : spmv::cg_step_kernel<T, false>, slots, s, n, d_num, d_den, d_p, d_q, d_x, d_r,
                       d_minv, d_work);
    if (rc != 0)
        return rc;
    return dots_reduce(DotsArgs{nullptr, d_dots, d_work, work_bytes}, (int) slots, s);
}

template <class T>
int cg_direction(int32_t n, const double * d_num, const double * d_den, const T * d_r, const T * d_minv, T * d_p, void * stream)
{
    if (n < 0)
        return fail(SPMV_HIP_ERR_INVALID, "n < 0");
    if (!d_num || !d_den || !d_r || !d_p)
        return fail(SPMV_HIP_ERR_INVALID, "null device pointer (only d_minv may be null)");
    const unsigned long long vec = (unsigned long long) n * sizeof(T);
    const KrylovArray arrays[] = {{d_r, vec, false, 16, "d_r"}, {d_minv, vec, false, 16, "d_minv"}, {d_p, vec, true, 16, "d_p"},
                                  {d_num, 8, false, 8, "d_num"}, {d_den, 8, false, 8, "d_den"}};
    const int rc = krylov_check_arrays(n, sizeof(T), arrays, (int) (sizeof arrays / sizeof arrays[0]));
    if (rc != 0)
        return rc;
    return krylov_launch(d_minv ? spmv::cg_direction_kernel<T, true> : spmv::cg_direction_kernel<T, false>, krylov_slots(n),
                         static_cast<hipStream_t>(stream), n, d_num, d_den, d_r, d_minv, d_p);
}

} // namespace

extern "C" {

int spmv_hip_krylov_workspace(int32_t n, size_t * bytes)
{
    if (n < 0 || !bytes)
        return fail(SPMV_HIP_ERR_INVALID, "n < 0, or bytes is null");
    *bytes = krylov_bytes(n);
    return SPMV_HIP_OK;
}

int spmv_hip_cg_step_f64(int32_t n, const double * d_num, const double * d_den, const double * d_p, const double * d_q, double * d_x, double * d_r,
                         const double * d_minv, double * d_dots, void * d_work, size_t work_bytes, void * stream)
{
    return cg_step(n, d_num, d_den, d_p, d_q, d_x, d_r, d_minv, d_dots, d_work, work_bytes, stream);
}

int spmv_hip_cg_step_f32(int32_t n, const double * d_num, const double * d_den, const float * d_p, const float * d_q, float * d_x, float * d_r,
                         const float * d_minv, double * d_dots, void * d_work, size_t work_bytes, void * stream)
{
    return cg_step(n, d_num, d_den, d_p, d_q, d_x, d_r, d_minv, d_dots, d_work, work_bytes, stream);
}

int spmv_hip_cg_direction_f64(int32_t n, const double * d_num, const double * d_den, const double * d_r, const double * d_minv, double * d_p,
                              void * stream)
{
    return cg_direction(n, d_num, d_den, d_r, d_minv, d_p, stream);
}

int spmv_hip_cg_direction_f32(int32_t n, const double * d_num, const double * d_den, const float * d_r, const float * d_minv, float * d_p,
                              void * stream)
{
    return cg_direction(n, d_num, d_den, d_r, d_minv, d_p, stream);
}

} // extern "C"
