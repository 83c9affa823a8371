// coarse.hip -- include/spmv_hip_coarse.h: the dense inverse of a multigrid's coarsest level over caller-owned device arrays, and
// its application.  The kernels and the order of their launches are coarse_kernels.hpp; the check of a call's arrays is the
// conjugate-gradient step's (krylov_check.hpp).
#include "spmv_hip_coarse.h"

#include "krylov_check.hpp"
#include "coarse_kernels.hpp"

using namespace spmvi;

static_assert(spmv::kCoarseMaxN == SPMV_HIP_COARSE_MAX_N, "the header documents the largest matrix");

namespace {

// [B | I]: n rows of 2 ld doubles, and the column f: ld doubles
size_t coarse_bytes(int32_t n)
{
    const size_t ld = (size_t) spmv::coarse_ld(n);
    const size_t bytes = ((size_t) n * 2 * ld + ld) * sizeof(double);
    return bytes < 16 ? 16 : bytes;
}

int check_n(int32_t n)
{
    if (n < 0)
        return fail(SPMV_HIP_ERR_INVALID, "n < 0");
    if (n > SPMV_HIP_COARSE_MAX_N)
        return fail(SPMV_HIP_ERR_INVALID, "n is above SPMV_HIP_COARSE_MAX_N");
    return SPMV_HIP_OK;
}

template <class T>
int coarse_setup(int32_t n, const int32_t * d_row_ptr, const int32_t * d_column_index, const double * d_value, T * d_inv, int32_t * d_status,
                 void * d_work, size_t work_bytes, void * stream)
{
    const int rc0 = check_n(n);
    if (rc0 != 0)
        return rc0;
    if (!d_row_ptr || !d_column_index || !d_value || !d_inv || !d_status || !d_work)
        return fail(SPMV_HIP_ERR_INVALID, "null device pointer");
    const int ld = spmv::coarse_ld(n);
    const size_t need = coarse_bytes(n);
    const KrylovArray arrays[] = {{d_row_ptr, ((unsigned long long) n + 1) * 4, false, 4, "d_row_ptr"},
                                  {d_column_index, 4, false, 4, "d_column_index"},
                                  {d_value, 8, false, 8, "d_value"},
                                  {d_inv, (unsigned long long) n * ld * sizeof(T), true, 16, "d_inv"},
                                  {d_status, 12, true, 4, "d_status"},
                                  {d_work, need, true, 16, "d_work"}};
    int rc = krylov_check_arrays(n, sizeof(T), arrays, (int) (sizeof arrays / sizeof arrays[0]));
    if (rc != 0)
        return rc;
    // looked at last: a call refused for this alone has passed every other check
    rc = krylov_check_work(work_bytes, need, "n", "spmv_hip_coarse_workspace");
    if (rc != 0)
        return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    double * w = static_cast<double *>(d_work);
    double * f = w + (size_t) n * 2 * ld;
    const long long elements = (long long) n * 2 * ld;
    hipLaunchKernelGGL(spmv::coarse_init_kernel, dim3(elements ? blocks_of(elements) : 1), dim3(256), 0, s, (int) n, ld, w, d_status);
    HIP_TRY(hipGetLastError());
    if (n == 0)
        return SPMV_HIP_OK;
    hipLaunchKernelGGL(spmv::coarse_densify_kernel, dim3(blocks_of(n)), dim3(256), 0, s, (int) n, ld, d_row_ptr, d_column_index, d_value, w, d_status);
    HIP_TRY(hipGetLastError());
    const unsigned row_blocks = (unsigned) ((n + spmv::kCoarseRows - 1) / spmv::kCoarseRows);
    for (int c = 0; c < n; ++c) {
        hipLaunchKernelGGL(spmv::coarse_pivot_kernel, dim3(1), dim3(spmv::kCoarsePivotThreads), 0, s, (int) n, ld, c, w, f, d_status);
        HIP_TRY(hipGetLastError());
        const unsigned pair_blocks = (unsigned) ((ld - (c >> 1) + spmv::kWave - 1) / spmv::kWave); // the pairs from column c & ~1 on
        hipLaunchKernelGGL(spmv::coarse_update_kernel, dim3(pair_blocks, row_blocks), dim3(256), 0, s, (int) n, ld, c, w, f, d_status);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(spmv::coarse_store_kernel<T>, dim3(blocks_of((long long) n * ld)), dim3(256), 0, s, (int) n, ld, w, d_status, d_inv);
    HIP_TRY(hipGetLastError());
    return SPMV_HIP_OK;
}

template <class T>
int coarse_apply(int32_t n, const T * d_inv, const T * d_r, T * d_z, void * stream)
{
    const int rc0 = check_n(n);
    if (rc0 != 0)
        return rc0;
    if (!d_inv || !d_r || !d_z)
        return fail(SPMV_HIP_ERR_INVALID, "null device pointer");
    const int ld = spmv::coarse_ld(n);
    const unsigned long long vec = (unsigned long long) n * sizeof(T);
    const KrylovArray arrays[] = {{d_inv, vec * ld, false, 16, "d_inv"}, {d_r, vec, false, 16, "d_r"}, {d_z, vec, true, 16, "d_z"}};
    const int rc = krylov_check_arrays(n, sizeof(T), arrays, (int) (sizeof arrays / sizeof arrays[0]));
    if (rc != 0)
        return rc;
    if (n == 0)
        return SPMV_HIP_OK;
    // a wave per row, four to a workgroup
    hipLaunchKernelGGL(spmv::coarse_apply_kernel<T>, dim3((unsigned) ((n + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), (int) n, ld,
                       d_inv, d_r, d_z);
    HIP_TRY(hipGetLastError());
    return SPMV_HIP_OK;
}

} // namespace

extern "C" {

int32_t spmv_hip_coarse_ld(int32_t n) { return spmv::coarse_ld(n); }

int spmv_hip_coarse_workspace(int32_t n, size_t * bytes)
{
    if (!bytes)
        return fail(SPMV_HIP_ERR_INVALID, "bytes is null");
    const int rc = check_n(n);
    if (rc != 0)
        return rc;
    *bytes = coarse_bytes(n);
    return SPMV_HIP_OK;
}

int spmv_hip_coarse_setup_f64(int32_t n, const int32_t * d_row_ptr, const int32_t * d_column_index, const double * d_value, double * d_inv,
                              int32_t * d_status, void * d_work, size_t work_bytes, void * stream)
{
    return coarse_setup(n, d_row_ptr, d_column_index, d_value, d_inv, d_status, d_work, work_bytes, stream);
}

int spmv_hip_coarse_setup_f32(int32_t n, const int32_t * d_row_ptr, const int32_t * d_column_index, const double * d_value, float * d_inv,
                              int32_t * d_status, void * d_work, size_t work_bytes, void * stream)
{
    return coarse_setup(n, d_row_ptr, d_column_index, d_value, d_inv, d_status, d_work, work_bytes, stream);
}

int spmv_hip_coarse_apply_f64(int32_t n, const double * d_inv, const double * d_r, double * d_z, void * stream)
{
    return coarse_apply(n, d_inv, d_r, d_z, stream);
}

int spmv_hip_coarse_apply_f32(int32_t n, const float * d_inv, const float * d_r, float * d_z, void * stream)
{
    return coarse_apply(n, d_inv, d_r, d_z, stream);
}

} // extern "C"
