// cheby.hip -- include/spmv_hip_cheby.h: the Chebyshev polynomial preconditioner over caller-owned device arrays.  The kernels are
// cheby_updates.hpp; the cut, the workspace rule, the check of a call's arrays and the launch are the conjugate-gradient step's
// (krylov_check.hpp), the reduction of the last step's slots is the one of the multiplies with dots (f32_plan.hpp: dots_reduce).
#include "spmv_hip_cheby.h"

#include "krylov_check.hpp"
#include "cheby_updates.hpp"

#include <cmath>

using namespace spmvi;

static_assert(spmv::kChebyMaxDegree == SPMV_HIP_CHEBY_MAX_DEGREE, "the header documents the largest degree");

namespace {

int check_degree(int32_t degree)
{
    if (degree < 1 || degree > SPMV_HIP_CHEBY_MAX_DEGREE)
        return fail(SPMV_HIP_ERR_INVALID, "the degree is outside 1 ... SPMV_HIP_CHEBY_MAX_DEGREE");
    return SPMV_HIP_OK;
}

template <class T, bool HASM>
int launch_step(int mode, long long slots, hipStream_t s, int32_t n, const double * pair, const T * u, const T * minv, T * d, T * z, const T * r,
                void * work)
{
    void (*kernel)(long long, const double *, const T *, const T *, T *, T *, const T *, spmv::v2d *) = nullptr;
    switch (mode) {
    case spmv::kChebyFirst: kernel = spmv::cheby_step_kernel<T, HASM, spmv::kChebyFirst>; break;
    case spmv::kChebyMiddle: kernel = spmv::cheby_step_kernel<T, HASM, spmv::kChebyMiddle>; break;
    case spmv::kChebyLast: kernel = spmv::cheby_step_kernel<T, HASM, spmv::kChebyLast>; break;
    case spmv::kChebyLastDots: kernel = spmv::cheby_step_kernel<T, HASM, spmv::kChebyLastDots>; break;
    case spmv::kChebySole: kernel = spmv::cheby_step_kernel<T, HASM, spmv::kChebySole>; break;
    default: kernel = spmv::cheby_step_kernel<T, HASM, spmv::kChebySoleDots>; break;
    }
    return krylov_launch(kernel, slots, s, n, pair, u, minv, d, z, r, work);
}

template <class T>
int cheby_bound(int32_t rows, const int32_t * d_row_ptr, const double * d_value, const T * d_minv, double * d_lambda, void * stream)
{
    if (rows < 0)
        return fail(SPMV_HIP_ERR_INVALID, "rows < 0");
    if (!d_row_ptr || !d_value || !d_lambda)
        return fail(SPMV_HIP_ERR_INVALID, "null device pointer (only d_minv may be null)");
    const KrylovArray arrays[] = {{d_row_ptr, ((unsigned long long) rows + 1) * 4, false, 4, "d_row_ptr"},
                                  {d_value, 8, false, 8, "d_value"},
                                  {d_minv, (unsigned long long) rows * sizeof(T), false, 16, "d_minv"},
                                  {d_lambda, 8, true, 8, "d_lambda"}};
    const int rc = krylov_check_arrays(rows, sizeof(T), arrays, (int) (sizeof arrays / sizeof arrays[0]));
    if (rc != 0)
        return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    unsigned long long * bits = reinterpret_cast<unsigned long long *>(d_lambda);
    hipLaunchKernelGGL(spmv::cheby_zero_kernel, dim3(1), dim3(64), 0, s, bits);
    HIP_TRY(hipGetLastError());
    if (rows > 0) {
        const long long blocks = ((long long) rows + 255) / 256;
        const dim3 grid((unsigned) (blocks < spmv::kChebyBoundBlocks ? blocks : spmv::kChebyBoundBlocks));
        if (d_minv)
            hipLaunchKernelGGL((spmv::cheby_bound_kernel<T, true>), grid, dim3(256), 0, s, (int) rows, d_row_ptr, d_value, d_minv, bits);
        else
            hipLaunchKernelGGL((spmv::cheby_bound_kernel<T, false>), grid, dim3(256), 0, s, (int) rows, d_row_ptr, d_value, d_minv, bits);
        HIP_TRY(hipGetLastError());
    }
    return SPMV_HIP_OK;
}

template <class T>
int cheby_step(int32_t n, int32_t degree, int32_t j, const double * d_coef, const T * d_u, const T * d_minv, T * d_d, T * d_z, const T * d_r,
               double * d_dots, void * d_work, size_t work_bytes, void * stream)
{
    if (n < 0)
        return fail(SPMV_HIP_ERR_INVALID, "n < 0");
    const int rc0 = check_degree(degree);
    if (rc0 != 0)
        return rc0;
    if (j < 0 || j >= degree)
        return fail(SPMV_HIP_ERR_INVALID, "the step j is outside 0 ... degree - 1");
    if (degree == 1)
        d_d = nullptr; // neither read nor stored: not an array of this call
    if (!d_coef || !d_u || !d_z || (degree > 1 && !d_d))
        return fail(SPMV_HIP_ERR_INVALID, "null device pointer (only d_minv, the three d_r, d_dots, d_work, and d_d at degree 1 may be null)");
    const int given = (d_r != nullptr) + (d_dots != nullptr) + (d_work != nullptr);
    if (given != 0 && given != 3)
        return fail(SPMV_HIP_ERR_INVALID, "d_r, d_dots and d_work are given together or not at all");
    const bool dots = given == 3, last = j == degree - 1;
    if (dots && !last)
        return fail(SPMV_HIP_ERR_INVALID, "the dots are formed by the last step alone (j == degree - 1)");
    const size_t need = dots ? krylov_bytes(n) : 0;
    const unsigned long long vec = (unsigned long long) n * sizeof(T);
    const KrylovArray arrays[] = {{d_u, vec, false, 16, "d_u"},
                                  {d_minv, vec, false, 16, "d_minv"},
                                  {d_d, vec, !last, 16, "d_d"},
                                  {d_z, vec, true, 16, "d_z"},
                                  {d_r, vec, false, 16, "d_r"},
                                  {d_dots, 16, true, 16, "d_dots"},
                                  {d_work, need, true, 16, "d_work"},
                                  {d_coef, 16ULL * (unsigned long long) degree, false, 8, "d_coef"}};
    int rc = krylov_check_arrays(n, sizeof(T), arrays, (int) (sizeof arrays / sizeof arrays[0]));
    if (rc != 0)
        return rc;
    // looked at last: a call refused for this alone has passed every other check
    rc = krylov_check_work(work_bytes, need, "n", "spmv_hip_krylov_workspace");
    if (rc != 0)
        return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long long slots = krylov_slots(n);
    const int mode = degree == 1 ? (dots ? spmv::kChebySoleDots : spmv::kChebySole)
                     : j == 0    ? spmv::kChebyFirst
                     : !last     ? spmv::kChebyMiddle
                                 : (dots ? spmv::kChebyLastDots : spmv::kChebyLast);
    const double * pair = d_coef + 2 * j;
    rc = d_minv ? launch_step<T, true>(mode, slots, s, n, pair, d_u, d_minv, d_d, d_z, d_r, d_work)
                : launch_step<T, false>(mode, slots, s, n, pair, d_u, d_minv, d_d, d_z, d_r, d_work);
    if (rc != 0 || !dots)
        return rc;
    return dots_reduce(DotsArgs{nullptr, d_dots, d_work, work_bytes}, (int) slots, s);
}

} // namespace

extern "C" {

int spmv_hip_cheby_bound_f64(int32_t rows, const int32_t * d_row_ptr, const double * d_value, const double * d_minv, double * d_lambda,
                             void * stream)
{
    return cheby_bound(rows, d_row_ptr, d_value, d_minv, d_lambda, stream);
}

int spmv_hip_cheby_bound_f32(int32_t rows, const int32_t * d_row_ptr, const double * d_value, const float * d_minv, double * d_lambda,
                             void * stream)
{
    return cheby_bound(rows, d_row_ptr, d_value, d_minv, d_lambda, stream);
}

int spmv_hip_cheby_coeffs(int32_t degree, const double * d_lambda, double scale, double ratio, double * d_coef, void * stream)
{
    const int rc0 = check_degree(degree);
    if (rc0 != 0)
        return rc0;
    if (!std::isfinite(scale) || !std::isfinite(ratio) || !(scale > 0.0) || !(ratio > 1.0))
        return fail(SPMV_HIP_ERR_INVALID, "scale and ratio are finite, scale > 0 and ratio > 1");
    if (!d_lambda || !d_coef)
        return fail(SPMV_HIP_ERR_INVALID, "null device pointer");
    const KrylovArray arrays[] = {{d_coef, 16ULL * (unsigned long long) degree, true, 8, "d_coef"}, {d_lambda, 8, false, 8, "d_lambda"}};
    const int rc = krylov_check_arrays(0, 8, arrays, 2);
    if (rc != 0)
        return rc;
    hipLaunchKernelGGL(spmv::cheby_coeffs_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), (int) degree, d_lambda, scale, ratio,
                       d_coef);
    HIP_TRY(hipGetLastError());
    return SPMV_HIP_OK;
}

int spmv_hip_cheby_step_f64(int32_t n, int32_t degree, int32_t j, const double * d_coef, const double * d_u, const double * d_minv, double * d_d,
                            double * d_z, const double * d_r, double * d_dots, void * d_work, size_t work_bytes, void * stream)
{
    return cheby_step(n, degree, j, d_coef, d_u, d_minv, d_d, d_z, d_r, d_dots, d_work, work_bytes, stream);
}

int spmv_hip_cheby_step_f32(int32_t n, int32_t degree, int32_t j, const double * d_coef, const float * d_u, const float * d_minv, float * d_d,
                            float * d_z, const float * d_r, double * d_dots, void * d_work, size_t work_bytes, void * stream)
{
    return cheby_step(n, degree, j, d_coef, d_u, d_minv, d_d, d_z, d_r, d_dots, d_work, work_bytes, stream);
}

} // extern "C"
