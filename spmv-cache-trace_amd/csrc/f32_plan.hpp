// f32_plan.hpp -- what compact.hip and the Krylov files take from f32values.hip: the tiling rule of the fp32-value multiplies (one
// rule: the compact plan's descriptors ARE the fp32-value plan's, with its own bits added), the narrowing of the values to float,
// the checks and the tile-free path of the scaled multiplies and their dots (the ladder that calls them is tile_front.hpp's), and
// the two Level-1 entries of formats 7 to 10 that compact.hip defines for both plans.
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
// the two in one call that throws nothing: what the preview, the plan and the upload use (each with its own text for bad_alloc)
int f32_plan_host_guarded(F32HostPlan & hp, int32_t rows, int32_t cols, const int32_t * row_ptr, unsigned flags,
                          const char * out_of_memory = "fp32-value plan: host memory");
// the host plan onto the current device
int f32_build_plan(spmv_hip_f32_plan ** out, F32HostPlan const & hp, hipStream_t s);
// every column in [0, cols)
int check_columns(int32_t nnz, const int32_t * column_index, int32_t cols);
// the four ints that open a tile-table row of either preview (first row, first entry, rows, log2 lanes per row) from the tile's
// descriptor d[0] and the next one
void tile_table_row(int32_t * t, const int4 * d);

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

// ---- ... with the two dots of y_out (include/spmv_hip_dots.h) ----------------------------------------------------------------------

// the dots of one call: w (null: no second dot), where the two doubles go, and the caller's workspace
struct DotsArgs {
    const void * w;
    double * dots;
    void * work;
    size_t work_bytes;
};

// do [a, a + abytes) and [b, b + bbytes) share a byte?  A null or empty array overlaps nothing.
bool overlap(const void * a, unsigned long long abytes, const void * b, unsigned long long bbytes);
// Workspace of a plan with `ntiles` tiles over `rows` rows: one 16-byte slot per tile or, where no tile runs, per 64 rows, then
// one per workgroup of the reduction's first stage; at least 16 bytes.
size_t dots_workspace_bytes(int ntiles, int32_t rows);
// What only a call with dots refuses, after scaled_vectors_check has passed: the list of spmv_hip_dots.h.  elem is sizeof(T),
// value_elem the size of a stored value; null arrays are not compared.
int dots_check(const DotsArgs & d, int ntiles, int32_t rows, int32_t cols, int32_t nnz, size_t elem, size_t value_elem, const void * row_ptr,
               const void * column_index, const void * value, const void * x, double beta, const void * y_in, const void * y_out);
// the workgroups of the reduction's first stage over n slots (one: a single stage): dots_reduce's rule, for gmres.hip to share
long long reduce_blocks(long long n);
// dots <- the sum of the first n slots of the workspace, in one or two launches on s (n == 0: +0.0, +0.0)
int dots_reduce(const DotsArgs & d, int n, hipStream_t s);
// scaled_rows_only with the dots of what it stores
int scaled_rows_only_dots(int32_t rows, bool float_vectors, bool zterm, double alpha, double beta, const void * y_in, void * y_out,
                          const DotsArgs & d, hipStream_t s);

// spmv_hip_csr_spmv_f32 and its scaled forms (scale, dots: null, or as for tile_front.hpp's tile_multiply)
int f32_multiply(const spmv_hip_f32_plan * pl, const int32_t * d_row_ptr, const int32_t * d_column_index, const float * d_value,
                 const double * d_x, double * d_y, void * stream, const ScaledArgs<double> * scale, const DotsArgs * dots);

// ---- Level 1 of formats 7 to 10 (compact.hip, beside internal.hpp's ctx_tile_multiply) ------------------------------------------------

// The upload of `format`: the values narrowed to float (allow_rounding as in spmv_hip_f32values.h) or kept as doubles, x and y
// doubles or floats; `multi` is what a multi-GPU context is told.  Refuses before anything of the previous matrix is freed.
int upload_float_tile(spmv_hip_ctx * c, int format, const char * multi, int32_t rows, int32_t cols, int32_t nnz, const int32_t * row_ptr,
                      const int32_t * column_index, const double * value, bool narrow_values, int allow_rounding, bool float_vectors);

} // namespace spmvi
