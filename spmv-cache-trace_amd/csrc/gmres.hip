// gmres.hip -- include/spmv_hip_gmres.h: the updates of restarted GMRES with classical Gram-Schmidt applied twice over a
// caller-owned basis, every scalar in device memory.  The kernels are gmres_updates.hpp; the workspace rule of one vector's slots
// and the check of a call's arrays (krylov_check.hpp) are those of krylov.hip, the update's reduction is dots_reduce
// (f32_plan.hpp) and the projection's is the same workgroup code (csr_dots.hpp: dots_reduce_block) over one pair of vectors each.
#include "spmv_hip_gmres.h"

#include "krylov_check.hpp"
#include "gmres_updates.hpp"

using namespace spmvi;

static_assert(spmv::kGmresMaxBasis == SPMV_HIP_GMRES_MAX_BASIS, "the header documents the largest basis");

namespace {

// pairs of sums that a projection over k vectors (and w itself) reduces
long long project_pairs(int k) { return (k + 2) / 2; }

// the 16-byte slots of one pair: those of a step over n elements (krylov_bytes: at least one)
long long pair_stride(long long n) { return (long long) (krylov_bytes(n) / 16); }

size_t project_bytes(long long n, int k) { return (size_t) project_pairs(k) * krylov_bytes(n); }

// n, k and the basis of a call; basis_bytes is what its k vectors span
template <class T>
int basis_check(int32_t n, int32_t k, const T * d_V, long long ldv, unsigned long long * basis_bytes)
{
    if (n < 0)
        return fail(SPMV_HIP_ERR_INVALID, "n < 0");
    if (k < 0 || k > SPMV_HIP_GMRES_MAX_BASIS)
        return fail(SPMV_HIP_ERR_INVALID, "k is outside 0 ... SPMV_HIP_GMRES_MAX_BASIS");
    if (k > 0 && !d_V)
        return fail(SPMV_HIP_ERR_INVALID, "d_V is null and k > 0");
    if (ldv < n)
        return fail(SPMV_HIP_ERR_INVALID, "ldv < n");
    if (((unsigned long long) ldv * sizeof(T)) % 16 != 0)
        return fail(SPMV_HIP_ERR_INVALID, "ldv * sizeof(T) is no multiple of 16");
    *basis_bytes = k > 0 ? ((unsigned long long) (k - 1) * (unsigned long long) ldv + (unsigned long long) n) * sizeof(T) : 0;
    return SPMV_HIP_OK;
}

int work_check(size_t work_bytes, size_t need) { return krylov_check_work(work_bytes, need, "the call", "spmv_hip_gmres_workspace"); }

template <class T>
int gmres_project(int32_t n, int32_t k, const T * d_V, long long ldv, const T * d_w, double * d_h, void * d_work, size_t work_bytes, void * stream)
{
    unsigned long long basis = 0;
    int rc = basis_check(n, k, d_V, ldv, &basis);
    if (rc != 0)
        return rc;
    if (!d_w || !d_h || !d_work)
        return fail(SPMV_HIP_ERR_INVALID, "null device pointer (only d_V where k == 0 may be null)");
    const size_t need = project_bytes(n, k);
    const KrylovArray arrays[] = {{k > 0 ? d_V : nullptr, basis, false, 16, "d_V"},
                                  {d_w, (unsigned long long) n * sizeof(T), false, 16, "d_w"},
                                  {d_h, 8ULL * (unsigned long long) (k + 1), true, 16, "d_h"},
                                  {d_work, need, true, 16, "d_work"}};
    rc = krylov_check_arrays(n, sizeof(T), arrays, (int) (sizeof arrays / sizeof arrays[0]));
    if (rc != 0)
        return rc;
    rc = work_check(work_bytes, need);
    if (rc != 0)
        return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long long slots = krylov_slots(n), stride = pair_stride(n);
    const unsigned pairs = (unsigned) project_pairs(k);
    spmv::v2d * work = static_cast<spmv::v2d *>(d_work);
    rc = krylov_launch(spmv::gmres_project_kernel<T>, slots, s, n, k, d_V, ldv, d_w, d_work, stride);
    if (rc != 0)
        return rc;
    // dots_reduce's stages, for every pair at once
    const long long blocks = reduce_blocks(slots);
    if (blocks > 1) {
        hipLaunchKernelGGL(spmv::gmres_reduce_kernel<256>, dim3((unsigned) blocks, pairs), dim3(256), 0, s, (int) slots, spmv::kDotsChunk, work, stride,
                           0LL, slots, (double *) nullptr, 0);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(spmv::gmres_reduce_kernel<256>, dim3(1, pairs), dim3(256), 0, s, (int) blocks, (int) blocks, work, stride, slots, 0LL, d_h,
                           (int) k + 1);
    } else
        hipLaunchKernelGGL(spmv::gmres_reduce_kernel<256>, dim3(1, pairs), dim3(256), 0, s, (int) slots, spmv::kDotsChunk, work, stride, 0LL, 0LL, d_h,
                           (int) k + 1);
    HIP_TRY(hipGetLastError());
    return SPMV_HIP_OK;
}

template <class T>
int gmres_update(int32_t n, int32_t k, const T * d_V, long long ldv, const double * d_h, T * d_w, double * d_dots, void * d_work, size_t work_bytes,
                 void * stream)
{
    unsigned long long basis = 0;
    int rc = basis_check(n, k, d_V, ldv, &basis);
    if (rc != 0)
        return rc;
    if (!d_h || !d_w || !d_dots || !d_work)
        return fail(SPMV_HIP_ERR_INVALID, "null device pointer (only d_V where k == 0 may be null)");
    const size_t need = krylov_bytes(n);
    const KrylovArray arrays[] = {{k > 0 ? d_V : nullptr, basis, false, 16, "d_V"},
                                  {d_h, 8ULL * (unsigned long long) k, false, 16, "d_h"},
                                  {d_w, (unsigned long long) n * sizeof(T), true, 16, "d_w"},
                                  {d_dots, 16, true, 16, "d_dots"},
                                  {d_work, need, true, 16, "d_work"}};
    rc = krylov_check_arrays(n, sizeof(T), arrays, (int) (sizeof arrays / sizeof arrays[0]));
    if (rc != 0)
        return rc;
    rc = work_check(work_bytes, need);
    if (rc != 0)
        return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long long slots = krylov_slots(n);
    rc = krylov_launch(spmv::gmres_axpys_kernel<T, spmv::kGmresUpdate>, slots, s, n, k, d_V, ldv, d_h, d_w, nullptr, d_work);
    if (rc != 0)
        return rc;
    return dots_reduce(DotsArgs{nullptr, d_dots, d_work, work_bytes}, (int) slots, s);
}

template <class T>
int gmres_scale(int32_t n, const double * d_scale, T * d_v, const T * d_minv, T * d_vhat, void * stream)
{
    if (n < 0)
        return fail(SPMV_HIP_ERR_INVALID, "n < 0");
    if (!d_scale || !d_v)
        return fail(SPMV_HIP_ERR_INVALID, "null device pointer (only d_minv and d_vhat may be null)");
    if (!d_minv != !d_vhat)
        return fail(SPMV_HIP_ERR_INVALID, "d_minv and d_vhat are both null or both given");
    const unsigned long long vec = (unsigned long long) n * sizeof(T);
    const KrylovArray arrays[] = {{d_v, vec, true, 16, "d_v"},
                                  {d_minv, vec, false, 16, "d_minv"},
                                  {d_vhat, vec, true, 16, "d_vhat"},
                                  {d_scale, 8, false, 8, "d_scale"}};
    const int rc = krylov_check_arrays(n, sizeof(T), arrays, (int) (sizeof arrays / sizeof arrays[0]));
    if (rc != 0)
        return rc;
    return krylov_launch(d_minv ? spmv::gmres_scale_kernel<T, true> : spmv::gmres_scale_kernel<T, false>, krylov_slots(n),
                         static_cast<hipStream_t>(stream), n, d_scale, d_v, d_minv, d_vhat);
}

template <class T>
int gmres_correct(int32_t n, int32_t k, const T * d_V, long long ldv, const double * d_y, const T * d_minv, T * d_x, void * stream)
{
    unsigned long long basis = 0;
    int rc = basis_check(n, k, d_V, ldv, &basis);
    if (rc != 0)
        return rc;
    if (!d_y || !d_x)
        return fail(SPMV_HIP_ERR_INVALID, "null device pointer (only d_minv, and d_V where k == 0, may be null)");
    const unsigned long long vec = (unsigned long long) n * sizeof(T);
    const KrylovArray arrays[] = {{k > 0 ? d_V : nullptr, basis, false, 16, "d_V"},
                                  {d_y, 8ULL * (unsigned long long) k, false, 16, "d_y"},
                                  {d_minv, vec, false, 16, "d_minv"},
                                  {d_x, vec, true, 16, "d_x"}};
    rc = krylov_check_arrays(n, sizeof(T), arrays, (int) (sizeof arrays / sizeof arrays[0]));
    if (rc != 0)
        return rc;
    if (k == 0)
        return SPMV_HIP_OK;
    return krylov_launch(d_minv ? spmv::gmres_axpys_kernel<T, spmv::kGmresCorrectM> : spmv::gmres_axpys_kernel<T, spmv::kGmresCorrect>,
                         krylov_slots(n), static_cast<hipStream_t>(stream), n, k, d_V, ldv, d_y, d_x, d_minv, nullptr);
}

bool basis_size(int32_t m) { return m >= 1 && m <= SPMV_HIP_GMRES_MAX_BASIS; }

} // namespace

extern "C" {

int spmv_hip_gmres_workspace(int32_t n, int32_t k_max, size_t * bytes)
{
    if (n < 0 || k_max < 0 || k_max > SPMV_HIP_GMRES_MAX_BASIS || !bytes)
        return fail(SPMV_HIP_ERR_INVALID, "n < 0, k_max outside 0 ... SPMV_HIP_GMRES_MAX_BASIS, or bytes is null");
    *bytes = project_bytes(n, k_max);
    return SPMV_HIP_OK;
}

int spmv_hip_gmres_state_doubles(int32_t m)
{
    if (!basis_size(m))
        return fail(SPMV_HIP_ERR_INVALID, "m is outside 1 ... SPMV_HIP_GMRES_MAX_BASIS");
    return spmv::gmres_state_doubles(m);
}

int spmv_hip_gmres_project_f64(int32_t n, int32_t k, const double * d_V, int64_t ldv, const double * d_w, double * d_h, void * d_work,
                               size_t work_bytes, void * stream)
{
    return gmres_project(n, k, d_V, (long long) ldv, d_w, d_h, d_work, work_bytes, stream);
}

int spmv_hip_gmres_project_f32(int32_t n, int32_t k, const float * d_V, int64_t ldv, const float * d_w, double * d_h, void * d_work,
                               size_t work_bytes, void * stream)
{
    return gmres_project(n, k, d_V, (long long) ldv, d_w, d_h, d_work, work_bytes, stream);
}

int spmv_hip_gmres_update_f64(int32_t n, int32_t k, const double * d_V, int64_t ldv, const double * d_h, double * d_w, double * d_dots,
                              void * d_work, size_t work_bytes, void * stream)
{
    return gmres_update(n, k, d_V, (long long) ldv, d_h, d_w, d_dots, d_work, work_bytes, stream);
}

int spmv_hip_gmres_update_f32(int32_t n, int32_t k, const float * d_V, int64_t ldv, const double * d_h, float * d_w, double * d_dots,
                              void * d_work, size_t work_bytes, void * stream)
{
    return gmres_update(n, k, d_V, (long long) ldv, d_h, d_w, d_dots, d_work, work_bytes, stream);
}

int spmv_hip_gmres_scale_f64(int32_t n, const double * d_scale, double * d_v, const double * d_minv, double * d_vhat, void * stream)
{
    return gmres_scale(n, d_scale, d_v, d_minv, d_vhat, stream);
}

int spmv_hip_gmres_scale_f32(int32_t n, const double * d_scale, float * d_v, const float * d_minv, float * d_vhat, void * stream)
{
    return gmres_scale(n, d_scale, d_v, d_minv, d_vhat, stream);
}

int spmv_hip_gmres_correct_f64(int32_t n, int32_t k, const double * d_V, int64_t ldv, const double * d_y, const double * d_minv, double * d_x,
                               void * stream)
{
    return gmres_correct(n, k, d_V, (long long) ldv, d_y, d_minv, d_x, stream);
}

int spmv_hip_gmres_correct_f32(int32_t n, int32_t k, const float * d_V, int64_t ldv, const double * d_y, const float * d_minv, float * d_x,
                               void * stream)
{
    return gmres_correct(n, k, d_V, (long long) ldv, d_y, d_minv, d_x, stream);
}

int spmv_hip_gmres_start(int32_t m, const double * d_nrm2, double * d_state, void * stream)
{
    if (!basis_size(m))
        return fail(SPMV_HIP_ERR_INVALID, "m is outside 1 ... SPMV_HIP_GMRES_MAX_BASIS");
    if (!d_nrm2 || !d_state)
        return fail(SPMV_HIP_ERR_INVALID, "null device pointer");
    const KrylovArray arrays[] = {{d_state, 8ULL * (unsigned long long) spmv::gmres_state_doubles(m), true, 16, "d_state"},
                                  {d_nrm2, 8, false, 8, "d_nrm2"}};
    const int rc = krylov_check_arrays(0, 8, arrays, 2);
    if (rc != 0)
        return rc;
    hipLaunchKernelGGL(spmv::gmres_start_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), (int) m, d_nrm2, d_state);
    HIP_TRY(hipGetLastError());
    return SPMV_HIP_OK;
}

int spmv_hip_gmres_column(int32_t k, int32_t m, const double * d_h1, const double * d_h2, const double * d_nrm2, double * d_state, void * stream)
{
    if (!basis_size(m) || k < 0 || k >= m)
        return fail(SPMV_HIP_ERR_INVALID, "m is outside 1 ... SPMV_HIP_GMRES_MAX_BASIS, or k outside 0 ... m - 1");
    if (!d_h1 || !d_h2 || !d_nrm2 || !d_state)
        return fail(SPMV_HIP_ERR_INVALID, "null device pointer");
    const unsigned long long col = 8ULL * (unsigned long long) (k + 1);
    const KrylovArray arrays[] = {{d_h1, col, false, 16, "d_h1"},
                                  {d_h2, col, false, 16, "d_h2"},
                                  {d_state, 8ULL * (unsigned long long) spmv::gmres_state_doubles(m), true, 16, "d_state"},
                                  {d_nrm2, 8, false, 8, "d_nrm2"}};
    const int rc = krylov_check_arrays(0, 8, arrays, 4);
    if (rc != 0)
        return rc;
    hipLaunchKernelGGL(spmv::gmres_column_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), (int) k, (int) m, d_h1, d_h2, d_nrm2,
                       d_state);
    HIP_TRY(hipGetLastError());
    return SPMV_HIP_OK;
}

int spmv_hip_gmres_solve(int32_t k, int32_t m, const double * d_state, double * d_y, void * stream)
{
    if (!basis_size(m) || k < 0 || k > m)
        return fail(SPMV_HIP_ERR_INVALID, "m is outside 1 ... SPMV_HIP_GMRES_MAX_BASIS, or k outside 0 ... m");
    if (!d_state || !d_y)
        return fail(SPMV_HIP_ERR_INVALID, "null device pointer");
    const KrylovArray arrays[] = {{d_state, 8ULL * (unsigned long long) spmv::gmres_state_doubles(m), false, 16, "d_state"},
                                  {d_y, 8ULL * (unsigned long long) k, true, 16, "d_y"}};
    const int rc = krylov_check_arrays(0, 8, arrays, 2);
    if (rc != 0)
        return rc;
    if (k == 0)
        return SPMV_HIP_OK;
    hipLaunchKernelGGL(spmv::gmres_solve_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), (int) k, (int) m, d_state, d_y);
    HIP_TRY(hipGetLastError());
    return SPMV_HIP_OK;
}

} // extern "C"
