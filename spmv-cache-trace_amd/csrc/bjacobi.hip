// bjacobi.hip -- include/spmv_hip_bjacobi.h: the point-block Jacobi preconditioner over caller-owned device arrays.  The kernels
// are bjacobi_kernels.hpp; the cut, the workspace rule, the check of a call's arrays and the launch are the conjugate-gradient
// step's (krylov_check.hpp), the reduction of the apply's slots is the one of the multiplies with dots (f32_plan.hpp: dots_reduce).
#include "spmv_hip_bjacobi.h"

#include "krylov_check.hpp"
#include "bjacobi_kernels.hpp"

using namespace spmvi;

static_assert(spmv::kBJacobiMaxBlock == SPMV_HIP_BJACOBI_MAX_BLOCK, "the header documents the largest block");

namespace {

// n >= 0, 1 <= b <= 8, n % b == 0
int check_block(int32_t n, int32_t b)
{
    if (n < 0)
        return fail(SPMV_HIP_ERR_INVALID, "n < 0");
    if (b < 1 || b > SPMV_HIP_BJACOBI_MAX_BLOCK)
        return fail(SPMV_HIP_ERR_INVALID, "the block size b is outside 1 ... 8");
    if (n % b != 0)
        return fail(SPMV_HIP_ERR_INVALID, "n is not a multiple of the block size b");
    return SPMV_HIP_OK;
}

template <class T, int MODE>
int launch_apply(int b, long long slots, hipStream_t s, int32_t n, const T * inv, const T * r, T * z, void * work)
{
    void (*kernel)(long long, const T *, const T *, T *, spmv::v2d *) = nullptr;
    switch (b) {
    case 1: kernel = spmv::bjacobi_apply_kernel<T, 1, MODE>; break;
    case 2: kernel = spmv::bjacobi_apply_kernel<T, 2, MODE>; break;
    case 3: kernel = spmv::bjacobi_apply_kernel<T, 3, MODE>; break;
    case 4: kernel = spmv::bjacobi_apply_kernel<T, 4, MODE>; break;
    case 5: kernel = spmv::bjacobi_apply_kernel<T, 5, MODE>; break;
    case 6: kernel = spmv::bjacobi_apply_kernel<T, 6, MODE>; break;
    case 7: kernel = spmv::bjacobi_apply_kernel<T, 7, MODE>; break;
    default: kernel = spmv::bjacobi_apply_kernel<T, 8, MODE>; break;
    }
    return krylov_launch(kernel, slots, s, n, inv, r, z, work);
}

template <class T>
int bjacobi_setup(int32_t rows, int32_t b, const int32_t * d_row_ptr, const int32_t * d_column_index, const double * d_value, T * d_inv,
                  int32_t * d_status, void * stream)
{
    const int rc0 = check_block(rows, b);
    if (rc0 != 0)
        return rc0;
    if (!d_row_ptr || !d_column_index || !d_value || !d_inv || !d_status)
        return fail(SPMV_HIP_ERR_INVALID, "null device pointer");
    const unsigned long long inv_bytes = (unsigned long long) rows * b * sizeof(T);
    const KrylovArray arrays[] = {{d_row_ptr, ((unsigned long long) rows + 1) * 4, false, 4, "d_row_ptr"},
                                  {d_column_index, 4, false, 4, "d_column_index"},
                                  {d_value, 8, false, 8, "d_value"},
                                  {d_inv, inv_bytes, true, 16, "d_inv"},
                                  {d_status, 8, true, 4, "d_status"}};
    const int rc = krylov_check_arrays(rows, sizeof(T), arrays, (int) (sizeof arrays / sizeof arrays[0]));
    if (rc != 0)
        return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(spmv::bjacobi_status_kernel, dim3(1), dim3(64), 0, s, d_status);
    HIP_TRY(hipGetLastError());
    if (rows > 0) {
        hipLaunchKernelGGL(spmv::bjacobi_setup_kernel<T>, dim3((unsigned) (rows / b)), dim3(64), 0, s, (int) b, d_row_ptr, d_column_index, d_value,
                           d_inv, d_status);
        HIP_TRY(hipGetLastError());
    }
    return SPMV_HIP_OK;
}

template <class T>
int bjacobi_apply(int32_t n, int32_t b, const T * d_inv, const T * d_r, T * d_z, double * d_dots, void * d_work, size_t work_bytes, void * stream)
{
    const int rc0 = check_block(n, b);
    if (rc0 != 0)
        return rc0;
    if (!d_inv || !d_r || !d_z)
        return fail(SPMV_HIP_ERR_INVALID, "null device pointer (only d_dots and d_work may be null, and only together)");
    if ((d_dots == nullptr) != (d_work == nullptr))
        return fail(SPMV_HIP_ERR_INVALID, "d_dots and d_work are given together or not at all");
    const size_t need = d_dots ? krylov_bytes(n) : 0;
    const unsigned long long vec = (unsigned long long) n * sizeof(T);
    const KrylovArray arrays[] = {{d_inv, vec * b, false, 16, "d_inv"},
                                  {d_r, vec, false, 16, "d_r"},
                                  {d_z, vec, true, 16, "d_z"},
                                  {d_dots, 16, true, 16, "d_dots"},
                                  {d_work, need, true, 16, "d_work"}};
    int rc = krylov_check_arrays(n, sizeof(T), arrays, (int) (sizeof arrays / sizeof arrays[0]));
    if (rc != 0)
        return rc;
    // looked at last: a call refused for this alone has passed every other check
    rc = krylov_check_work(work_bytes, need, "n", "spmv_hip_krylov_workspace");
    if (rc != 0)
        return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long long slots = krylov_slots(n);
    if (!d_dots)
        return launch_apply<T, 0>(b, slots, s, n, d_inv, d_r, d_z, nullptr);
    rc = launch_apply<T, 1>(b, slots, s, n, d_inv, d_r, d_z, d_work);
    if (rc != 0)
        return rc;
    return dots_reduce(DotsArgs{nullptr, d_dots, d_work, work_bytes}, (int) slots, s);
}

template <class T>
int bjacobi_apply_add(int32_t n, int32_t b, const T * d_inv, const T * d_u, T * d_x, void * stream)
{
    const int rc0 = check_block(n, b);
    if (rc0 != 0)
        return rc0;
    if (!d_inv || !d_u || !d_x)
        return fail(SPMV_HIP_ERR_INVALID, "null device pointer");
    const unsigned long long vec = (unsigned long long) n * sizeof(T);
    const KrylovArray arrays[] = {{d_inv, vec * b, false, 16, "d_inv"}, {d_u, vec, false, 16, "d_u"}, {d_x, vec, true, 16, "d_x"}};
    const int rc = krylov_check_arrays(n, sizeof(T), arrays, (int) (sizeof arrays / sizeof arrays[0]));
    if (rc != 0)
        return rc;
    return launch_apply<T, 2>(b, krylov_slots(n), static_cast<hipStream_t>(stream), n, d_inv, d_u, d_x, nullptr);
}

} // namespace

extern "C" {

int spmv_hip_bjacobi_setup_f64(int32_t rows, int32_t b, const int32_t * d_row_ptr, const int32_t * d_column_index, const double * d_value,
                               double * d_inv, int32_t * d_status, void * stream)
{
    return bjacobi_setup(rows, b, d_row_ptr, d_column_index, d_value, d_inv, d_status, stream);
}

int spmv_hip_bjacobi_setup_f32(int32_t rows, int32_t b, const int32_t * d_row_ptr, const int32_t * d_column_index, const double * d_value,
                               float * d_inv, int32_t * d_status, void * stream)
{
    return bjacobi_setup(rows, b, d_row_ptr, d_column_index, d_value, d_inv, d_status, stream);
}

int spmv_hip_bjacobi_apply_f64(int32_t n, int32_t b, const double * d_inv, const double * d_r, double * d_z, double * d_dots, void * d_work,
                               size_t work_bytes, void * stream)
{
    return bjacobi_apply(n, b, d_inv, d_r, d_z, d_dots, d_work, work_bytes, stream);
}

int spmv_hip_bjacobi_apply_f32(int32_t n, int32_t b, const float * d_inv, const float * d_r, float * d_z, double * d_dots, void * d_work,
                               size_t work_bytes, void * stream)
{
    return bjacobi_apply(n, b, d_inv, d_r, d_z, d_dots, d_work, work_bytes, stream);
}

int spmv_hip_bjacobi_apply_add_f64(int32_t n, int32_t b, const double * d_inv, const double * d_u, double * d_x, void * stream)
{
    return bjacobi_apply_add(n, b, d_inv, d_u, d_x, stream);
}

int spmv_hip_bjacobi_apply_add_f32(int32_t n, int32_t b, const float * d_inv, const float * d_u, float * d_x, void * stream)
{
    return bjacobi_apply_add(n, b, d_inv, d_u, d_x, stream);
}

} // extern "C"
