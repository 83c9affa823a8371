// tile_front.hpp -- the host side of a float-tile multiply (formats 7 to 10), once: with_bools, which turns run-time bools into
// a template instantiation, and tile_multiply, the refusals of spmv_hip_f32values.h / spmv_hip_compact*.h / spmv_hip_scaled.h /
// spmv_hip_dots.h in the order they are documented and the three launch shapes (plain, scaled, scaled with dots).  f32values.hip
// and compact.hip describe their family to it (below) and instantiate their own kernels through it.
#pragma once

#include "f32_plan.hpp"

#include <type_traits>

namespace spmvi {

// f(std::bool_constant<b>...) for the run-time bools b...: f returns kernel<B(), ...>, every combination is instantiated
template <class F>
auto with_bools(F f)
{
    return f();
}

template <class F, class... Rest>
auto with_bools(F f, bool b, Rest... rest)
{
    return b ? with_bools([f](auto... c) { return f(std::true_type{}, c...); }, rest...)
             : with_bools([f](auto... c) { return f(std::false_type{}, c...); }, rest...);
}

// One multiply of a family over values V and vectors T.  A Family holds
//   pl                      the plan (rows, cols, nnz, ntiles, flags; null is refused here, before anything else looks at it)
//   null_columns()          the refusal of a null d_column_index, or null where that is one more "null device pointer"
//   columns_read()          ... and whether this plan reads the array at all
//   plain(x32), scaled(x32, beta0), dots(beta0, hasw)    the kernel of a launch shape
//   launch(kernel, grid, s, args...)                     the launch, with the family's leading kernel arguments in front of args
// scale null: y += A x on d_y; otherwise d_y is y_out; dots only with a scale.
template <class V, class T, class Family>
int tile_multiply(const Family & f, const int32_t * d_row_ptr, const int32_t * d_column_index, const V * d_value, const T * d_x, T * d_y,
                  void * stream, const ScaledArgs<T> * scale, const DotsArgs * dots)
{
    constexpr bool float_vectors = std::is_same<T, float>::value;
    const auto * pl = f.pl;
    if (!pl)
        return fail(SPMV_HIP_ERR_INVALID, "plan is null");
    if (d_x && (const void *) d_x == (const void *) d_y)
        return fail(SPMV_HIP_ERR_INVALID, "d_x and d_y must be different arrays");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (scale) {
        int rc = scaled_vectors_check(pl->rows, sizeof(T), scale->beta, scale->y_in, d_y);
        if (rc == 0 && dots)
            rc = dots_check(*dots, pl->ntiles, pl->rows, pl->cols, pl->nnz, sizeof(T), sizeof(V), d_row_ptr, d_column_index, d_value, d_x,
                            scale->beta, scale->y_in, d_y);
        if (rc != 0)
            return rc;
        if (pl->rows == 0)
            return dots ? dots_reduce(*dots, 0, s) : SPMV_HIP_OK;
        if (scale->alpha == 0.0 || pl->ntiles == 0) { // the beta part alone: neither the matrix nor x is read
            if (dots)
                return scaled_rows_only_dots(pl->rows, float_vectors, scale->alpha != 0.0, scale->alpha, scale->beta, scale->y_in, d_y, *dots, s);
            return scaled_rows_only(pl->rows, float_vectors, scale->alpha != 0.0, scale->alpha, scale->beta, scale->y_in, d_y, s);
        }
    }
    if (pl->ntiles == 0) // rows, cols or nnz of zero
        return SPMV_HIP_OK;
    if (!d_row_ptr || !d_value || !d_x || !d_y || (!d_column_index && !f.null_columns()))
        return fail(SPMV_HIP_ERR_INVALID, "null device pointer");
    if (!d_column_index && f.columns_read())
        return fail(SPMV_HIP_ERR_INVALID, f.null_columns());
    if (!aligned16(d_column_index) || !aligned16(d_value))
        return fail(SPMV_HIP_ERR_ALIGN, "column / value arrays must be 16-byte aligned");
    if constexpr (float_vectors) // (the kernel reads and writes x and y one element at a time)
        if ((reinterpret_cast<uintptr_t>(d_x) | reinterpret_cast<uintptr_t>(d_y)) & 3u)
            return fail(SPMV_HIP_ERR_ALIGN, "d_x and d_y must be 4-byte aligned");
    const dim3 grid((unsigned) ((pl->ntiles + 3) / 4));
    const int exact = (pl->flags & SPMV_HIP_FLAG_EXACT_ORDER) ? 1 : 0;
    const bool x32 = (long long) pl->cols * (long long) sizeof(T) < (1LL << 32);
    if (dots) // (x32 holds: dots_check)
        f.launch(f.dots(scale->beta == 0.0, dots->w != nullptr), grid, s, d_row_ptr, d_column_index, d_value, d_x, scale->alpha, scale->beta,
                 scale->y_in, d_y, static_cast<const T *>(dots->w), static_cast<spmv::v2d *>(dots->work), exact);
    else if (scale)
        f.launch(f.scaled(x32, scale->beta == 0.0), grid, s, d_row_ptr, d_column_index, d_value, d_x, scale->alpha, scale->beta, scale->y_in,
                 d_y, exact);
    else
        f.launch(f.plain(x32), grid, s, d_row_ptr, d_column_index, d_value, d_x, d_y, exact);
    HIP_TRY(hipGetLastError());
    return dots ? dots_reduce(*dots, pl->ntiles, s) : SPMV_HIP_OK;
}

} // namespace spmvi
