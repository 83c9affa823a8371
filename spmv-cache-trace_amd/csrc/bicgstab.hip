// bicgstab.hip -- include/spmv_hip_bicgstab.h: the three vector updates of a BiCGStab iteration over caller-owned device vectors,
// their scalars quotients of doubles in device memory.  The kernels are bicgstab_updates.hpp; the workspace rule, the check of a
// call's arrays, the launch (krylov_check.hpp) and the reduction of the step's slots (f32_plan.hpp: dots_reduce) are those of krylov.hip.
#include "spmv_hip_bicgstab.h"

#include "krylov_check.hpp"
#include "bicgstab_updates.hpp"

using namespace spmvi;

namespace {

template <class T>
int bicgstab_s(int32_t n, const double * d_num, const double * d_den, const T * d_v, T * d_r, const T * d_minv, T * d_shat, void * stream)
{
    if (n < 0)
        return fail(SPMV_HIP_ERR_INVALID, "n < 0");
    if (!d_num || !d_den || !d_v || !d_r)
        return fail(SPMV_HIP_ERR_INVALID, "null device pointer (only d_minv and d_shat may be null)");
    if (!d_minv != !d_shat)
        return fail(SPMV_HIP_ERR_INVALID, "d_minv and d_shat are both null or both given");
    const unsigned long long vec = (unsigned long long) n * sizeof(T);
    const KrylovArray arrays[] = {{d_v, vec, false, 16, "d_v"},          {d_r, vec, true, 16, "d_r"},   {d_minv, vec, false, 16, "d_minv"},
                                  {d_shat, vec, true, 16, "d_shat"},     {d_num, 8, false, 8, "d_num"}, {d_den, 8, false, 8, "d_den"}};
    const int rc = krylov_check_arrays(n, sizeof(T), arrays, (int) (sizeof arrays / sizeof arrays[0]));
    if (rc != 0)
        return rc;
    return krylov_launch(d_minv ? spmv::bicgstab_s_kernel<T, true> : spmv::bicgstab_s_kernel<T, false>, krylov_slots(n),
                         static_cast<hipStream_t>(stream), n, d_num, d_den, d_v, d_r, d_minv, d_shat);
}

template <class T>
int bicgstab_step(int32_t n, const double * d_num_a, const double * d_den_a, const double * d_num_w, const double * d_den_w, const T * d_phat,
                  const T * d_shat, const T * d_t, const T * d_rhat, T * d_x, T * d_r, double * d_dots, void * d_work, size_t work_bytes,
                  void * stream)
{
    if (n < 0)
        return fail(SPMV_HIP_ERR_INVALID, "n < 0");
    if (!d_num_a || !d_den_a || !d_num_w || !d_den_w || !d_phat || !d_t || !d_rhat || !d_x || !d_r || !d_dots || !d_work)
        return fail(SPMV_HIP_ERR_INVALID, "null device pointer (only d_shat may be null)");
    const size_t need = krylov_bytes(n);
    const unsigned long long vec = (unsigned long long) n * sizeof(T);
    const KrylovArray arrays[] = {{d_phat, vec, false, 16, "d_phat"},     {d_shat, vec, false, 16, "d_shat"},   {d_t, vec, false, 16, "d_t"},
                                  {d_rhat, vec, false, 16, "d_rhat"},     {d_x, vec, true, 16, "d_x"},          {d_r, vec, true, 16, "d_r"},
                                  {d_dots, 16, true, 16, "d_dots"},       {d_work, need, true, 16, "d_work"},   {d_num_a, 8, false, 8, "d_num_a"},
                                  {d_den_a, 8, false, 8, "d_den_a"},      {d_num_w, 8, false, 8, "d_num_w"},    {d_den_w, 8, false, 8, "d_den_w"}};
    int rc = krylov_check_arrays(n, sizeof(T), arrays, (int) (sizeof arrays / sizeof arrays[0]));
    if (rc != 0)
        return rc;
    // looked at last: a call refused for this alone has arrays that may be launched over
    rc = krylov_check_work(work_bytes, need, "n", "spmv_hip_krylov_workspace");
    if (rc != 0)
        return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long long slots = krylov_slots(n);
    rc = krylov_launch(d_shat ? spmv::bicgstab_step_kernel<T, true> : spmv::bicgstab_step_kernel<T, false>, slots, s, n, d_num_a, d_den_a,
                       d_num_w, d_den_w, d_phat, d_shat, d_t, d_rhat, d_x, d_r, d_work);
    if (rc != 0)
        return rc;
    return dots_reduce(DotsArgs{nullptr, d_dots, d_work, work_bytes}, (int) slots, s);
}

template <class T>
int bicgstab_direction(int32_t n, const double * d_num_r, const double * d_den_r, const double * d_num_a, const double * d_den_a,
                       const double * d_num_w, const double * d_den_w, const T * d_r, const T * d_v, T * d_p, const T * d_minv, T * d_phat,
                       void * stream)
{
    if (n < 0)
        return fail(SPMV_HIP_ERR_INVALID, "n < 0");
    if (!d_num_r || !d_den_r || !d_num_a || !d_den_a || !d_num_w || !d_den_w || !d_r || !d_v || !d_p)
        return fail(SPMV_HIP_ERR_INVALID, "null device pointer (only d_minv and d_phat may be null)");
    if (!d_minv != !d_phat)
        return fail(SPMV_HIP_ERR_INVALID, "d_minv and d_phat are both null or both given");
    const unsigned long long vec = (unsigned long long) n * sizeof(T);
    const KrylovArray arrays[] = {{d_r, vec, false, 16, "d_r"},           {d_v, vec, false, 16, "d_v"},         {d_p, vec, true, 16, "d_p"},
                                  {d_minv, vec, false, 16, "d_minv"},     {d_phat, vec, true, 16, "d_phat"},    {d_num_r, 8, false, 8, "d_num_r"},
                                  {d_den_r, 8, false, 8, "d_den_r"},      {d_num_a, 8, false, 8, "d_num_a"},    {d_den_a, 8, false, 8, "d_den_a"},
                                  {d_num_w, 8, false, 8, "d_num_w"},      {d_den_w, 8, false, 8, "d_den_w"}};
    const int rc = krylov_check_arrays(n, sizeof(T), arrays, (int) (sizeof arrays / sizeof arrays[0]));
    if (rc != 0)
        return rc;
    return krylov_launch(d_minv ? spmv::bicgstab_direction_kernel<T, true> : spmv::bicgstab_direction_kernel<T, false>, krylov_slots(n),
                         static_cast<hipStream_t>(stream), n, d_num_r, d_den_r, d_num_a, d_den_a, d_num_w, d_den_w, d_r, d_v, d_p, d_minv, d_phat);
}

} // namespace

extern "C" {

int spmv_hip_bicgstab_s_f64(int32_t n, const double * d_num, const double * d_den, const double * d_v, double * d_r, const double * d_minv,
                            double * d_shat, void * stream)
{
    return bicgstab_s(n, d_num, d_den, d_v, d_r, d_minv, d_shat, stream);
}

int spmv_hip_bicgstab_s_f32(int32_t n, const double * d_num, const double * d_den, const float * d_v, float * d_r, const float * d_minv,
                            float * d_shat, void * stream)
{
    return bicgstab_s(n, d_num, d_den, d_v, d_r, d_minv, d_shat, stream);
}

int spmv_hip_bicgstab_step_f64(int32_t n, const double * d_num_a, const double * d_den_a, const double * d_num_w, const double * d_den_w,
                               const double * d_phat, const double * d_shat, const double * d_t, const double * d_rhat, double * d_x, double * d_r,
                               double * d_dots, void * d_work, size_t work_bytes, void * stream)
{
    return bicgstab_step(n, d_num_a, d_den_a, d_num_w, d_den_w, d_phat, d_shat, d_t, d_rhat, d_x, d_r, d_dots, d_work, work_bytes, stream);
}

int spmv_hip_bicgstab_step_f32(int32_t n, const double * d_num_a, const double * d_den_a, const double * d_num_w, const double * d_den_w,
                               const float * d_phat, const float * d_shat, const float * d_t, const float * d_rhat, float * d_x, float * d_r,
                               double * d_dots, void * d_work, size_t work_bytes, void * stream)
{
    return bicgstab_step(n, d_num_a, d_den_a, d_num_w, d_den_w, d_phat, d_shat, d_t, d_rhat, d_x, d_r, d_dots, d_work, work_bytes, stream);
}

int spmv_hip_bicgstab_direction_f64(int32_t n, const double * d_num_r, const double * d_den_r, const double * d_num_a, const double * d_den_a,
                                    const double * d_num_w, const double * d_den_w, const double * d_r, const double * d_v, double * d_p,
                                    const double * d_minv, double * d_phat, void * stream)
{
    return bicgstab_direction(n, d_num_r, d_den_r, d_num_a, d_den_a, d_num_w, d_den_w, d_r, d_v, d_p, d_minv, d_phat, stream);
}

int spmv_hip_bicgstab_direction_f32(int32_t n, const double * d_num_r, const double * d_den_r, const double * d_num_a, const double * d_den_a,
                                    const double * d_num_w, const double * d_den_w, const float * d_r, const float * d_v, float * d_p,
                                    const float * d_minv, float * d_phat, void * stream)
{
    return bicgstab_direction(n, d_num_r, d_den_r, d_num_a, d_den_a, d_num_w, d_den_w, d_r, d_v, d_p, d_minv, d_phat, stream);
}

} // extern "C"
