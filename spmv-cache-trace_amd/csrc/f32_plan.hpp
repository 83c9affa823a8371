// f32_plan.hpp -- what compact.hip takes from f32values.hip: the tiling rule of the fp32-value multiplies (one rule: the compact
// plan's descriptors ARE the fp32-value plan's, with its own bits added) and the narrowing of the values to float.
#pragma once

#include "internal.hpp"

struct spmv_hip_f32_plan {
    int32_t rows = 0, cols = 0, nnz = 0;
    unsigned flags = 0;
    int ntiles = 0, long_tiles = 0, uniform_tiles = 0, scalar_tiles = 0, longest = 0;
    long long streamed_bytes = 0;
    size_t device_bytes = 0;
    int4 * d_desc = nullptr; // ntiles + 1 records
};

namespace spmvi {

// what the preview and the plan share: every number of plan_info and the descriptors (ntiles + 1 records, or none)
struct F32HostPlan {
    spmv_hip_f32_plan numbers;
    std::vector<int4> desc;
};

// rows, cols, row_ptr and the flags (0 or SPMV_HIP_FLAG_EXACT_ORDER), refused in that order
int f32_check_host(int32_t rows, int32_t cols, const int32_t * row_ptr, unsigned flags);
// the tiles of checked arguments; throws std::bad_alloc
void f32_plan_host(F32HostPlan & hp, int32_t rows, int32_t cols, const int32_t * row_ptr, unsigned flags);

struct NarrowResult {
    long long inexact = 0, overflow = 0, first_inexact = -1, first_overflow = -1;
    double max_rel = 0.0;
};

// out[k] = (float) value[k], and what that changed
NarrowResult narrow_host(int64_t n, const double * value, float * out);
// what an upload refuses: finite values that are infinite as floats, and -- unless allow_rounding -- values that are not floats
int narrow_refusal(NarrowResult const & c, int allow_rounding);

// ---- y_out <- alpha A x + beta y_in (include/spmv_hip_scaled.h): what the four scaled multiplies share -------------------------------

// the scale of one call; a multiply without one (y += A x) passes none
template <class T>
struct ScaledArgs {
    double alpha, beta;
    const T * y_in;
};

// y_in and y_out of a scaled call over `rows` elements of `elem` bytes: y_out null, y_in null where it is read (beta != 0), the
// two overlapping without being the same array, or float vectors off their 4-byte alignment
int scaled_vectors_check(int32_t rows, size_t elem, double beta, const void * y_in, const void * y_out);
// the call where no tile runs (alpha == 0, or a plan without tiles: zterm says that alpha * +0.0 is still added): one vector kernel
int scaled_rows_only(int32_t rows, bool float_vectors, bool zterm, double alpha, double beta, const void * y_in, void * y_out, hipStream_t s);

} // namespace spmvi
