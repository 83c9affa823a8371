// mcgs.hip -- include/spmv_hip_mcgs.h: the multicolour Gauss-Seidel / SSOR preconditioner over caller-owned device arrays.  The
// kernels are mcgs_kernels.hpp; the check of a call's arrays, the cut and the workspace rule of the apply's dots are the
// conjugate-gradient step's (krylov_check.hpp), their reduction is the one of the multiplies with dots (f32_plan.hpp: dots_reduce).
// The rounds of the colouring are those of graph_rounds.hpp, driven by graph_rounds() of krylov_check.hpp.
#include "spmv_hip_mcgs.h"

#include "krylov_check.hpp"
#include "mcgs_kernels.hpp"

#include <cmath>

using namespace spmvi;

static_assert(spmv::kMcgsMaxColours == SPMV_HIP_MCGS_MAX_COLOURS, "the header documents the number of colours");

namespace {

constexpr int C = SPMV_HIP_MCGS_MAX_COLOURS;

long long mcgs_chunks(long long rows) { return (rows + spmv::kMcgsChunk - 1) / spmv::kMcgsChunk; }

// The workspace of colour and permute, cut the same way by both: [counter 16][colour_ptr (C + 1) ints][marks: rows bytes]
// [chunk sums: chunks ints][histograms: chunks x C ints]
struct Work {
    size_t counter, cptr, marks, sums, hist, bytes;
};
Work work_of(long long rows)
{
    const long long chunks = mcgs_chunks(rows);
    Work w;
    w.counter = 0;
    w.cptr = 16;
    w.marks = w.cptr + up16((C + 1) * 4);
    w.sums = w.marks + up16((size_t) rows);
    w.hist = w.sums + up16((size_t) chunks * 4);
    w.bytes = w.hist + up16((size_t) chunks * C * 4);
    return w;
}

unsigned chunk_blocks(long long rows) { return (unsigned) ((mcgs_chunks(rows) + 3) / 4); }

int mcgs_colour(int32_t rows, const int32_t * d_row_ptr, const int32_t * d_column_index, uint32_t seed, int32_t * d_colour, int32_t * d_status,
                void * d_work, size_t work_bytes, void * stream)
{
    if (rows < 0)
        return fail(SPMV_HIP_ERR_INVALID, "rows < 0");
    if (!d_row_ptr || !d_column_index || !d_colour || !d_status || !d_work)
        return fail(SPMV_HIP_ERR_INVALID, "null device pointer");
    const Work w = work_of(rows);
    const KrylovArray arrays[] = {{d_row_ptr, ((unsigned long long) rows + 1) * 4, false, 4, "d_row_ptr"},
                                  {d_column_index, 4, false, 4, "d_column_index"},
                                  {d_colour, (unsigned long long) rows * 4, true, 4, "d_colour"},
                                  {d_status, 16, true, 4, "d_status"},
                                  {d_work, w.bytes, true, 16, "d_work"}};
    int rc = krylov_check_arrays(rows, 4, arrays, (int) (sizeof arrays / sizeof arrays[0]));
    if (rc != 0)
        return rc;
    rc = krylov_check_work(work_bytes, w.bytes, "rows", "spmv_hip_mcgs_workspace");
    if (rc != 0)
        return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    char * work = static_cast<char *>(d_work);
    int * winners = reinterpret_cast<int *>(work + w.counter);
    unsigned char * mark = reinterpret_cast<unsigned char *>(work + w.marks);
    const unsigned grid = blocks_of(rows > 4 ? rows : 4);
    hipLaunchKernelGGL(spmv::mcgs_init_kernel, dim3(grid), dim3(256), 0, s, (int) rows, d_colour, d_status);
    HIP_TRY(hipGetLastError());
    int rounds = 0;
    rc = graph_rounds(rows, winners, s, "a colouring round without a winner: the arrays are not those of a CSR matrix", [&]() -> int {
        hipLaunchKernelGGL(spmv::rounds_mark_kernel<true>, dim3(grid), dim3(256), 0, s, (int) rows, (unsigned) seed, d_row_ptr, d_column_index,
                           (const double *) nullptr, (const double *) nullptr, d_colour, mark, winners);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(spmv::mcgs_assign_kernel, dim3(grid), dim3(256), 0, s, (int) rows, d_row_ptr, d_column_index, d_colour, mark, d_status);
        HIP_TRY(hipGetLastError());
        return SPMV_HIP_OK;
    }, &rounds);
    if (rc != 0)
        return rc;
    hipLaunchKernelGGL(spmv::mcgs_check_kernel, dim3(grid), dim3(256), 0, s, (int) rows, d_row_ptr, d_column_index, d_colour, rounds, d_status);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    return SPMV_HIP_OK;
}

// the smallest power of two >= nnz / rows, clamped to 4 ... 64
int default_group(long long rows, long long nnz)
{
    int g = 4;
    while (g < 64 && (long long) g * rows < nnz)
        g *= 2;
    return g;
}

int mcgs_permute(int32_t rows, int32_t nnz, const int32_t * d_row_ptr, const int32_t * d_column_index, const double * d_value, const int32_t * d_colour,
                 const int32_t * d_status, int32_t * d_order, int32_t * d_perm_row_ptr, int32_t * d_perm_column_index, double * d_perm_value,
                 spmv_hip_mcgs_plan * plan, void * d_work, size_t work_bytes, void * stream)
{
    if (rows < 0 || nnz < 0)
        return fail(SPMV_HIP_ERR_INVALID, "rows < 0 or nnz < 0");
    if (!d_row_ptr || !d_column_index || !d_value || !d_colour || !d_status || !d_order || !d_perm_row_ptr || !d_perm_column_index || !d_perm_value ||
        !plan || !d_work)
        return fail(SPMV_HIP_ERR_INVALID, "null pointer");
    const Work w = work_of(rows);
    const unsigned long long n4 = (unsigned long long) nnz * 4, n8 = (unsigned long long) nnz * 8, r4 = (unsigned long long) rows * 4;
    const KrylovArray arrays[] = {{d_row_ptr, r4 + 4, false, 4, "d_row_ptr"},
                                  {d_column_index, n4, false, 4, "d_column_index"},
                                  {d_value, n8, false, 8, "d_value"},
                                  {d_colour, r4, false, 4, "d_colour"},
                                  {d_status, 16, false, 4, "d_status"},
                                  {d_order, r4, true, 4, "d_order"},
                                  {d_perm_row_ptr, r4 + 4, true, 4, "d_perm_row_ptr"},
                                  {d_perm_column_index, n4, true, 4, "d_perm_column_index"},
                                  {d_perm_value, n8, true, 8, "d_perm_value"},
                                  {d_work, w.bytes, true, 16, "d_work"}};
    int rc = krylov_check_arrays(rows, 4, arrays, (int) (sizeof arrays / sizeof arrays[0]));
    if (rc != 0)
        return rc;
    rc = krylov_check_work(work_bytes, w.bytes, "rows", "spmv_hip_mcgs_workspace");
    if (rc != 0)
        return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    char * work = static_cast<char *>(d_work);
    int * cptr = reinterpret_cast<int *>(work + w.cptr);
    int * sums = reinterpret_cast<int *>(work + w.sums);
    int * hist = reinterpret_cast<int *>(work + w.hist);
    const int chunks = (int) mcgs_chunks(rows);
    int32_t status[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(status, d_status, sizeof status, hipMemcpyDeviceToHost, s));
    int32_t host_ptr[C + 1];
    for (int c = 0; c <= C; ++c)
        host_ptr[c] = 0;
    if (rows > 0) {
        const unsigned cb = chunk_blocks(rows);
        hipLaunchKernelGGL(spmv::mcgs_hist_kernel, dim3(cb), dim3(256), 0, s, (int) rows, d_colour, hist);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(spmv::mcgs_offsets_kernel, dim3(1), dim3(64), 0, s, chunks, hist, cptr);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(spmv::mcgs_scatter_kernel, dim3(cb), dim3(256), 0, s, (int) rows, d_colour, d_row_ptr, hist, d_order, d_perm_row_ptr);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(spmv::mcgs_chunk_sum_kernel, dim3(cb), dim3(256), 0, s, (int) rows, d_perm_row_ptr, sums);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(spmv::mcgs_chunk_scan_kernel, dim3(1), dim3(64), 0, s, chunks, sums);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(spmv::mcgs_row_scan_kernel, dim3(cb), dim3(256), 0, s, (int) rows, d_perm_row_ptr, sums);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(spmv::mcgs_copy_kernel, dim3((unsigned) (((long long) rows + 15) / 16)), dim3(256), 0, s, (int) rows, d_order, d_row_ptr,
                           d_column_index, d_value, d_perm_row_ptr, d_perm_column_index, d_perm_value);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(host_ptr, cptr, sizeof host_ptr, hipMemcpyDeviceToHost, s));
    } else {
        HIP_TRY(hipMemsetAsync(d_perm_row_ptr, 0, 4, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    if (status[0] < 0 || status[0] > C)
        return fail(SPMV_HIP_ERR_INVALID, "d_status[0] is outside 0 ... 64: not the status of spmv_hip_mcgs_colour");
    plan->rows = rows;
    plan->colours = status[0];
    plan->conflicts = status[2];
    plan->group = default_group(rows, nnz);
    for (int c = 0; c <= C; ++c)
        plan->colour_ptr[c] = host_ptr[c];
    plan->d_order = d_order;
    plan->d_row_ptr = d_perm_row_ptr;
    plan->d_column_index = d_perm_column_index;
    plan->d_value = d_perm_value;
    return SPMV_HIP_OK;
}

int check_omega(double omega)
{
    if (!std::isfinite(omega) || !(omega > 0.0) || !(omega < 2.0))
        return fail(SPMV_HIP_ERR_INVALID, "omega is not inside (0, 2)");
    return SPMV_HIP_OK;
}

// what every call refuses in a plan, before any of its arrays is looked at
int check_plan(const spmv_hip_mcgs_plan * plan)
{
    if (!plan)
        return fail(SPMV_HIP_ERR_INVALID, "null plan");
    if (plan->rows < 0)
        return fail(SPMV_HIP_ERR_INVALID, "plan->rows < 0");
    if (!plan->d_order || !plan->d_row_ptr || !plan->d_column_index || !plan->d_value)
        return fail(SPMV_HIP_ERR_INVALID, "null device pointer in the plan");
    if (plan->colours < 0 || plan->colours > C)
        return fail(SPMV_HIP_ERR_INVALID, "plan->colours is outside 0 ... 64");
    const int g = plan->group;
    if (g < 1 || g > 64 || (g & (g - 1)) != 0)
        return fail(SPMV_HIP_ERR_INVALID, "plan->group is not a power of two in 1 ... 64");
    if (plan->conflicts != 0)
        return fail(SPMV_HIP_ERR_INVALID, "plan->conflicts != 0: rows of one colour couple and would race");
    if (plan->colour_ptr[0] != 0 || plan->colour_ptr[plan->colours] != plan->rows)
        return fail(SPMV_HIP_ERR_INVALID, "plan->colour_ptr does not run from 0 to rows");
    for (int c = 0; c < plan->colours; ++c)
        if (plan->colour_ptr[c] > plan->colour_ptr[c + 1])
            return fail(SPMV_HIP_ERR_INVALID, "plan->colour_ptr decreases");
    return SPMV_HIP_OK;
}

// the arrays of a sweep (x written) or of an apply (z, dots and the workspace written)
template <class T>
int check_arrays(const spmv_hip_mcgs_plan * plan, const T * d_b, const T * d_minv, T * d_x, double * d_dots, void * d_work, size_t need)
{
    const unsigned long long vec = (unsigned long long) plan->rows * sizeof(T), r4 = (unsigned long long) plan->rows * 4;
    const KrylovArray arrays[] = {{plan->d_order, r4, false, 4, "plan->d_order"},
                                  {plan->d_row_ptr, r4 + 4, false, 4, "plan->d_row_ptr"},
                                  {plan->d_column_index, 4, false, 4, "plan->d_column_index"},
                                  {plan->d_value, 8, false, 8, "plan->d_value"},
                                  {d_b, vec, false, 16, "d_b (d_r)"},
                                  {d_minv, vec, false, 16, "d_minv"},
                                  {d_x, vec, true, 16, "d_x (d_z)"},
                                  {d_dots, 16, true, 16, "d_dots"},
                                  {d_work, need, true, 16, "d_work"}};
    return krylov_check_arrays(plan->rows, sizeof(T), arrays, (int) (sizeof arrays / sizeof arrays[0]));
}

template <class T, int G>
void launch_colour(const spmv_hip_mcgs_plan * plan, int k0, int k1, double omega, const T * b, const T * minv, T * x, hipStream_t s)
{
    const long long per_wave = (long long) (64 / G) * spmv::kMcgsPasses;
    const long long waves = ((long long) k1 - k0 + per_wave - 1) / per_wave;
    hipLaunchKernelGGL((spmv::mcgs_sweep_kernel<T, G>), dim3((unsigned) ((waves + 3) / 4)), dim3(256), 0, s, k0, k1, plan->d_order, plan->d_row_ptr,
                       plan->d_column_index, plan->d_value, omega, 1.0 - omega, b, minv, x);
}

// the colours first ... last in turn; everything has been checked
template <class T>
int sweep_colours(const spmv_hip_mcgs_plan * plan, int first, int last, double omega, const T * b, const T * minv, T * x, hipStream_t s)
{
    const int step = last < first ? -1 : 1;
    for (int c = first;; c += step) {
        const int k0 = plan->colour_ptr[c], k1 = plan->colour_ptr[c + 1];
        if (k1 > k0) {
            dispatch_group(plan->group, [&](auto G) { launch_colour<T, G()>(plan, k0, k1, omega, b, minv, x, s); });
            HIP_TRY(hipGetLastError());
        }
        if (c == last)
            break;
    }
    return SPMV_HIP_OK;
}

template <class T>
int mcgs_sweep(const spmv_hip_mcgs_plan * plan, int32_t first, int32_t last, double omega, const T * d_b, const T * d_minv, T * d_x, void * stream)
{
    int rc = check_plan(plan);
    if (rc != 0)
        return rc;
    rc = check_omega(omega);
    if (rc != 0)
        return rc;
    const int top = plan->colours > 0 ? plan->colours : 1; // a plan without a colour: colour 0 is its empty range
    if (first < 0 || first >= top || last < 0 || last >= top)
        return fail(SPMV_HIP_ERR_INVALID, "a colour index outside the plan");
    if (!d_b || !d_minv || !d_x)
        return fail(SPMV_HIP_ERR_INVALID, "null device pointer");
    rc = check_arrays<T>(plan, d_b, d_minv, d_x, nullptr, nullptr, 0);
    if (rc != 0)
        return rc;
    return sweep_colours<T>(plan, first, last, omega, d_b, d_minv, d_x, static_cast<hipStream_t>(stream));
}

template <class T>
int mcgs_apply(const spmv_hip_mcgs_plan * plan, double omega, const T * d_r, const T * d_minv, T * d_z, double * d_dots, void * d_work,
               size_t work_bytes, void * stream)
{
    int rc = check_plan(plan);
    if (rc != 0)
        return rc;
    rc = check_omega(omega);
    if (rc != 0)
        return rc;
    if (!d_r || !d_minv || !d_z)
        return fail(SPMV_HIP_ERR_INVALID, "null device pointer (only d_dots and d_work may be null, and only together)");
    if ((d_dots == nullptr) != (d_work == nullptr))
        return fail(SPMV_HIP_ERR_INVALID, "d_dots and d_work are given together or not at all");
    const int32_t n = plan->rows;
    const size_t need = d_dots ? krylov_bytes(n) : 0;
    rc = check_arrays<T>(plan, d_r, d_minv, d_z, d_dots, d_work, need);
    if (rc != 0)
        return rc;
    // looked at last: a call refused for this alone has passed every other check
    rc = krylov_check_work(work_bytes, need, "rows", "spmv_hip_krylov_workspace");
    if (rc != 0)
        return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n > 0) {
        HIP_TRY(hipMemsetAsync(d_z, 0, (size_t) n * sizeof(T), s));
        if (plan->colours > 0) {
            rc = sweep_colours<T>(plan, 0, plan->colours - 1, omega, d_r, d_minv, d_z, s);
            if (rc != 0)
                return rc;
            rc = sweep_colours<T>(plan, plan->colours - 1, 0, omega, d_r, d_minv, d_z, s);
            if (rc != 0)
                return rc;
        }
    }
    if (!d_dots)
        return SPMV_HIP_OK;
    const long long slots = krylov_slots(n);
    rc = krylov_launch(spmv::mcgs_dots_kernel<T>, slots, s, n, d_r, d_z, d_work);
    if (rc != 0)
        return rc;
    return dots_reduce(DotsArgs{nullptr, d_dots, d_work, work_bytes}, (int) slots, s);
}

} // namespace

extern "C" {

int spmv_hip_mcgs_workspace(int32_t rows, size_t * bytes)
{
    if (rows < 0 || !bytes)
        return fail(SPMV_HIP_ERR_INVALID, "rows < 0, or bytes is null");
    *bytes = work_of(rows).bytes;
    return SPMV_HIP_OK;
}

int spmv_hip_mcgs_colour(int32_t rows, const int32_t * d_row_ptr, const int32_t * d_column_index, uint32_t seed, int32_t * d_colour,
                         int32_t * d_status, void * d_work, size_t work_bytes, void * stream)
{
    return mcgs_colour(rows, d_row_ptr, d_column_index, seed, d_colour, d_status, d_work, work_bytes, stream);
}

int spmv_hip_mcgs_permute(int32_t rows, int32_t nnz, const int32_t * d_row_ptr, const int32_t * d_column_index, const double * d_value,
                          const int32_t * d_colour, const int32_t * d_status, int32_t * d_order, int32_t * d_perm_row_ptr,
                          int32_t * d_perm_column_index, double * d_perm_value, spmv_hip_mcgs_plan * plan, void * d_work, size_t work_bytes,
                          void * stream)
{
    return mcgs_permute(rows, nnz, d_row_ptr, d_column_index, d_value, d_colour, d_status, d_order, d_perm_row_ptr, d_perm_column_index, d_perm_value,
                        plan, d_work, work_bytes, stream);
}

int spmv_hip_mcgs_sweep_f64(const spmv_hip_mcgs_plan * plan, int32_t first, int32_t last, double omega, const double * d_b, const double * d_minv,
                            double * d_x, void * stream)
{
    return mcgs_sweep(plan, first, last, omega, d_b, d_minv, d_x, stream);
}

int spmv_hip_mcgs_sweep_f32(const spmv_hip_mcgs_plan * plan, int32_t first, int32_t last, double omega, const float * d_b, const float * d_minv,
                            float * d_x, void * stream)
{
    return mcgs_sweep(plan, first, last, omega, d_b, d_minv, d_x, stream);
}

int spmv_hip_mcgs_apply_f64(const spmv_hip_mcgs_plan * plan, double omega, const double * d_r, const double * d_minv, double * d_z, double * d_dots,
                            void * d_work, size_t work_bytes, void * stream)
{
    return mcgs_apply(plan, omega, d_r, d_minv, d_z, d_dots, d_work, work_bytes, stream);
}

int spmv_hip_mcgs_apply_f32(const spmv_hip_mcgs_plan * plan, double omega, const float * d_r, const float * d_minv, float * d_z, double * d_dots,
                            void * d_work, size_t work_bytes, void * stream)
{
    return mcgs_apply(plan, omega, d_r, d_minv, d_z, d_dots, d_work, work_bytes, stream);
}

} // extern "C"
