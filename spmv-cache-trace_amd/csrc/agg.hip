// agg.hip -- include/spmv_hip_agg.h and include/spmv_hip_agg_mis2.h (the aggregates of a distance-2 independent set, the restriction by
// a group of lanes per aggregate): one level of a plain aggregation multigrid over caller-owned device arrays.  The kernels are
// agg_kernels.hpp; the check of a call's arrays is the conjugate-gradient step's (krylov_check.hpp); the stable sorts are
// hipCUB's radix sort and the prefix sums spmv_hip_internal_exclusive_scan_i32 (coo_sort.hip), whose temporary memory is
// allocated and freed inside the three calls that synchronise anyway.  The rounds of both aggregations are those of
// graph_rounds.hpp, driven by graph_rounds() of krylov_check.hpp, inside one body for the two entry points.
#include "spmv_hip_agg_mis2.h"

#include "krylov_check.hpp"
#include "agg_kernels.hpp"

#include <hipcub/hipcub.hpp>

#include <cmath>

using namespace spmvi;

namespace {

typedef struct spmv_hip_agg_plan Plan;

// The workspace, cut the same way by the three setup calls: [counters 16: decided, missing][marks: rows bytes][four arrays of
// rows + 1 ints: the state / the sorted keys, the flags / the row numbers, the ranks, the counts][thresholds: rows doubles] and,
// for the Galerkin product, [keys: nnz + 2 of 8 bytes, behind the sort the flags and their sums][sorted keys: nnz of 8 bytes]
// [positions: nnz ints].  The distance-2 aggregation (spmv_hip_agg_mis2_workspace) has [beside: rows bytes] behind the marks, and
// in the second of the four arrays the nearest keys, then the flags, then the roots joined in pass 1.
struct Work {
    size_t counter, marks, beside, ints[4], thresh, key, sorted, idx, bytes;
};
Work work_of(long long rows, long long nnz, bool mis2 = false)
{
    Work w;
    w.counter = 0;
    w.marks = 16;
    w.beside = w.marks + up16((size_t) rows);
    size_t at = w.beside + (mis2 ? up16((size_t) rows) : 0);
    for (int k = 0; k < 4; ++k) {
        w.ints[k] = at;
        at += up16(((size_t) rows + 1) * 4);
    }
    w.thresh = at;
    at += up16((size_t) rows * 8);
    w.key = at;
    if (nnz > 0)
        at += up16(((size_t) nnz + 2) * 8);
    w.sorted = at;
    if (nnz > 0)
        at += up16((size_t) nnz * 8);
    w.idx = at;
    if (nnz > 0)
        at += up16((size_t) nnz * 4);
    w.bytes = at;
    return w;
}

// out <- the exclusive prefix sums of the n ints of in
int scan(const int * in, int * out, long long n, hipStream_t s, const char * what)
{
    return spmv_hip_internal_exclusive_scan_i32(in, out, n, s) != 0 ? fail(SPMV_HIP_ERR_HIP, what) : SPMV_HIP_OK;
}

// bits that hold every key below `keys`
int bits_of(unsigned long long keys)
{
    int bits = 1;
    while (bits < 64 && (1ULL << bits) < keys)
        ++bits;
    return bits;
}

// hipCUB's stable radix sort of n pairs with its temporary memory allocated and freed here
template <class K>
int sort_pairs(const K * key_in, K * key_out, const int * value_in, int * value_out, int n, int bits, hipStream_t s)
{
    void * temp = nullptr;
    size_t temp_bytes = 0;
    hipError_t e = hipcub::DeviceRadixSort::SortPairs(nullptr, temp_bytes, key_in, key_out, value_in, value_out, n, 0, bits, s);
    if (e == hipSuccess)
        e = hipMalloc(&temp, temp_bytes ? temp_bytes : 16);
    if (e == hipSuccess)
        e = hipcub::DeviceRadixSort::SortPairs(temp, temp_bytes, key_in, key_out, value_in, value_out, n, 0, bits, s);
    if (e == hipSuccess)
        e = hipStreamSynchronize(s);
    if (temp)
        (void) hipFree(temp);
    return e == hipSuccess ? SPMV_HIP_OK : fail_hip(e, "the radix sort of the aggregation");
}

// spmv_hip_agg_aggregate and, with mis2, spmv_hip_agg_aggregate_mis2: the two differ in the workspace's rule, in the kernels of a
// round and in how the rows join the roots; the missing counter and its error are the distance-2 call's alone
int agg_aggregate(bool mis2, int32_t rows, const int32_t * d_row_ptr, const int32_t * d_column_index, const double * d_value, double theta,
                  uint32_t seed, int32_t * d_agg, int32_t * d_status, void * d_work, size_t work_bytes, void * stream)
{
    if (rows < 0)
        return fail(SPMV_HIP_ERR_INVALID, "rows < 0");
    if (!d_row_ptr || !d_column_index || !d_agg || !d_status || !d_work)
        return fail(SPMV_HIP_ERR_INVALID, "null device pointer (only d_value may be null)");
    if (!std::isfinite(theta) || !(theta >= 0.0) || !(theta <= 1.0))
        return fail(SPMV_HIP_ERR_INVALID, "theta is not inside [0, 1]");
    const Work w = work_of(rows, 0, mis2);
    const KrylovArray arrays[] = {{d_row_ptr, ((unsigned long long) rows + 1) * 4, false, 4, "d_row_ptr"},
                                  {d_column_index, 4, false, 4, "d_column_index"},
                                  {d_value, 8, false, 8, "d_value"},
                                  {d_agg, (unsigned long long) rows * 4, true, 4, "d_agg"},
                                  {d_status, 16, true, 4, "d_status"},
                                  {d_work, w.bytes, true, 16, "d_work"}};
    int rc = krylov_check_arrays(rows, 4, arrays, (int) (sizeof arrays / sizeof arrays[0]));
    if (rc != 0)
        return rc;
    rc = krylov_check_work(work_bytes, w.bytes, "rows", mis2 ? "spmv_hip_agg_mis2_workspace(rows)" : "spmv_hip_agg_workspace(rows, 0)");
    if (rc != 0)
        return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (rows == 0) {
        HIP_TRY(hipMemsetAsync(d_status, 0, 16, s));
        HIP_TRY(hipStreamSynchronize(s));
        return SPMV_HIP_OK;
    }
    char * work = static_cast<char *>(d_work);
    int * decided = reinterpret_cast<int *>(work + w.counter);
    int * missing = decided + 1;
    unsigned char * mark = reinterpret_cast<unsigned char *>(work + w.marks);
    unsigned char * beside = reinterpret_cast<unsigned char *>(work + w.beside);
    int * state = reinterpret_cast<int *>(work + w.ints[0]);
    int * near = reinterpret_cast<int *>(work + w.ints[1]); // in the rounds; then the flags of the roots; then the roots joined in pass 1
    int * flag = near, * joined = near;
    int * rank = reinterpret_cast<int *>(work + w.ints[2]);
    int * count = reinterpret_cast<int *>(work + w.ints[3]);
    const double * thresh = d_value && theta > 0.0 ? reinterpret_cast<double *>(work + w.thresh) : nullptr;
    const dim3 g(blocks_of(rows > 4 ? rows : 4)), b(256);
    const int n = rows;
    const unsigned key = seed;
    hipLaunchKernelGGL(spmv::agg_init_kernel, g, b, 0, s, n, d_row_ptr, d_column_index, d_value, theta, state, const_cast<double *>(thresh), d_status);
    HIP_TRY(hipGetLastError());
    int rounds = 0;
    rc = graph_rounds(rows, decided, s, "an aggregation round that decided no row: the arrays are not those of a CSR matrix", [&]() -> int {
        if (mis2) {
            hipLaunchKernelGGL(spmv::agg_mis2_near_kernel, g, b, 0, s, n, key, d_row_ptr, d_column_index, d_value, thresh, state, near);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(spmv::agg_mis2_mark_kernel, g, b, 0, s, n, key, d_row_ptr, d_column_index, d_value, thresh, state, near, mark);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(spmv::agg_mis2_beside_kernel, g, b, 0, s, n, d_row_ptr, d_column_index, d_value, thresh, mark, beside);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(spmv::agg_mis2_assign_kernel, g, b, 0, s, n, d_row_ptr, d_column_index, d_value, thresh, state, mark, beside, decided);
        } else {
            hipLaunchKernelGGL(spmv::rounds_mark_kernel<false>, g, b, 0, s, n, key, d_row_ptr, d_column_index, d_value, thresh, state, mark, (int *) nullptr);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(spmv::agg_assign_kernel, g, b, 0, s, n, d_row_ptr, d_column_index, d_value, thresh, state, mark, decided);
        }
        HIP_TRY(hipGetLastError());
        return SPMV_HIP_OK;
    }, &rounds);
    if (rc != 0)
        return rc;
    hipLaunchKernelGGL(spmv::agg_flag_kernel, dim3(blocks_of((long long) rows + 1)), b, 0, s, n, state, flag);
    HIP_TRY(hipGetLastError());
    rc = scan(flag, rank, (long long) rows + 1, s, "the prefix sum over the roots");
    if (rc != 0)
        return rc;
    HIP_TRY(hipMemsetAsync(count, 0, (size_t) rows * 4, s));
    if (mis2) {
        HIP_TRY(hipMemsetAsync(missing, 0, 4, s));
        hipLaunchKernelGGL(spmv::agg_mis2_join1_kernel, g, b, 0, s, n, key, d_row_ptr, d_column_index, d_value, thresh, state, joined);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(spmv::agg_mis2_join2_kernel, g, b, 0, s, n, key, d_row_ptr, d_column_index, d_value, thresh, state, joined, rank, d_agg, count,
                           missing);
    } else {
        hipLaunchKernelGGL(spmv::agg_join_kernel, g, b, 0, s, n, key, d_row_ptr, d_column_index, d_value, thresh, state, rank, d_agg, count);
    }
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(spmv::agg_status_kernel, g, b, 0, s, n, rounds, rank, count, d_status);
    HIP_TRY(hipGetLastError());
    int none = 0;
    if (mis2)
        HIP_TRY(hipMemcpyAsync(&none, missing, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (none != 0)
        return fail(SPMV_HIP_ERR_STATE, "a covered row without a neighbour that joined a root: the arrays changed under the call");
    return SPMV_HIP_OK;
}

int agg_plan(int32_t rows, const int32_t * d_agg, const int32_t * d_status, int32_t * d_member_ptr, int32_t * d_member, Plan * plan, void * d_work,
             size_t work_bytes, void * stream)
{
    if (rows < 0)
        return fail(SPMV_HIP_ERR_INVALID, "rows < 0");
    if (!d_agg || !d_status || !d_member_ptr || !d_member || !plan || !d_work)
        return fail(SPMV_HIP_ERR_INVALID, "null pointer");
    const Work w = work_of(rows, 0);
    const unsigned long long r4 = (unsigned long long) rows * 4;
    // (d_member_ptr holds aggregates + 1 <= rows + 1 elements; before the status is read, one is known)
    const KrylovArray arrays[] = {{d_agg, r4, false, 4, "d_agg"},
                                  {d_status, 16, false, 4, "d_status"},
                                  {d_member_ptr, 4, true, 4, "d_member_ptr"},
                                  {d_member, r4, true, 4, "d_member"},
                                  {d_work, w.bytes, true, 16, "d_work"}};
    int rc = krylov_check_arrays(rows, 4, arrays, (int) (sizeof arrays / sizeof arrays[0]));
    if (rc != 0)
        return rc;
    rc = krylov_check_work(work_bytes, w.bytes, "rows", "spmv_hip_agg_workspace(rows, 0)");
    if (rc != 0)
        return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int32_t status[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(status, d_status, sizeof status, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const int aggregates = status[0];
    if (aggregates < 0 || aggregates > rows || (aggregates == 0 && rows > 0))
        return fail(SPMV_HIP_ERR_INVALID, "d_status[0] is outside 1 ... rows: not the status of spmv_hip_agg_aggregate");
    if (overlap(d_member_ptr, ((unsigned long long) aggregates + 1) * 4, d_member, r4) ||
        overlap(d_member_ptr, ((unsigned long long) aggregates + 1) * 4, d_agg, r4) ||
        overlap(d_member_ptr, ((unsigned long long) aggregates + 1) * 4, d_work, w.bytes))
        return fail(SPMV_HIP_ERR_INVALID, "d_member_ptr overlaps another array of the call");
    if (rows > 0) {
        char * work = static_cast<char *>(d_work);
        int * bad = reinterpret_cast<int *>(work + w.counter);
        int * sorted = reinterpret_cast<int *>(work + w.ints[0]);
        int * idx = reinterpret_cast<int *>(work + w.ints[1]);
        int * count = reinterpret_cast<int *>(work + w.ints[3]);
        HIP_TRY(hipMemsetAsync(bad, 0, 4, s));
        HIP_TRY(hipMemsetAsync(count, 0, ((size_t) aggregates + 1) * 4, s));
        hipLaunchKernelGGL(spmv::agg_count_kernel, dim3(blocks_of(rows)), dim3(256), 0, s, (int) rows, aggregates, d_agg, count, idx, bad);
        HIP_TRY(hipGetLastError());
        int off = 0;
        HIP_TRY(hipMemcpyAsync(&off, bad, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (off != 0)
            return fail(SPMV_HIP_ERR_STATE, "d_agg holds a number outside 0 ... aggregates - 1");
        rc = scan(count, d_member_ptr, (long long) aggregates + 1, s, "the prefix sum over the aggregates");
        if (rc != 0)
            return rc;
        rc = sort_pairs<int>(d_agg, sorted, idx, d_member, rows, bits_of((unsigned long long) aggregates), s);
        if (rc != 0)
            return rc;
    } else {
        HIP_TRY(hipMemsetAsync(d_member_ptr, 0, 4, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    plan->rows = rows;
    plan->aggregates = aggregates;
    plan->largest = status[2];
    plan->d_agg = d_agg;
    plan->d_member_ptr = d_member_ptr;
    plan->d_member = d_member;
    return SPMV_HIP_OK;
}

// what every call refuses in a plan, before any of its arrays is looked at
int check_plan(const Plan * plan)
{
    if (!plan)
        return fail(SPMV_HIP_ERR_INVALID, "null plan");
    if (plan->rows < 0)
        return fail(SPMV_HIP_ERR_INVALID, "plan->rows < 0");
    if (!plan->d_agg || !plan->d_member_ptr || !plan->d_member)
        return fail(SPMV_HIP_ERR_INVALID, "null device pointer in the plan");
    if (plan->aggregates < 0 || plan->aggregates > plan->rows || (plan->aggregates == 0 && plan->rows > 0))
        return fail(SPMV_HIP_ERR_INVALID, "plan->aggregates is outside 1 ... rows (0 without rows)");
    return SPMV_HIP_OK;
}

int agg_symbolic(const Plan * plan, int32_t nnz, const int32_t * d_row_ptr, const int32_t * d_column_index, int32_t * d_coarse_row_ptr,
                 int32_t * d_coarse_column_index, int32_t * d_entry_order, int32_t * d_entry_ptr, int32_t * d_status, void * d_work,
                 size_t work_bytes, void * stream)
{
    int rc = check_plan(plan);
    if (rc != 0)
        return rc;
    if (nnz < 0)
        return fail(SPMV_HIP_ERR_INVALID, "nnz < 0");
    if (!d_row_ptr || !d_column_index || !d_coarse_row_ptr || !d_coarse_column_index || !d_entry_order || !d_entry_ptr || !d_status || !d_work)
        return fail(SPMV_HIP_ERR_INVALID, "null device pointer");
    const int rows = plan->rows, aggregates = plan->aggregates;
    const Work w = work_of(rows, nnz);
    const unsigned long long n4 = (unsigned long long) nnz * 4, r4 = (unsigned long long) rows * 4;
    const KrylovArray arrays[] = {{plan->d_agg, r4, false, 4, "plan->d_agg"},
                                  {d_row_ptr, r4 + 4, false, 4, "d_row_ptr"},
                                  {d_column_index, n4, false, 4, "d_column_index"},
                                  {d_coarse_row_ptr, ((unsigned long long) aggregates + 1) * 4, true, 4, "d_coarse_row_ptr"},
                                  {d_coarse_column_index, n4, true, 4, "d_coarse_column_index"},
                                  {d_entry_order, n4, true, 4, "d_entry_order"},
                                  {d_entry_ptr, n4 + 4, true, 4, "d_entry_ptr"},
                                  {d_status, 4, true, 4, "d_status"},
                                  {d_work, w.bytes, true, 16, "d_work"}};
    rc = krylov_check_arrays(rows, 4, arrays, (int) (sizeof arrays / sizeof arrays[0]));
    if (rc != 0)
        return rc;
    rc = krylov_check_work(work_bytes, w.bytes, "(rows, nnz)", "spmv_hip_agg_workspace(plan->rows, nnz)");
    if (rc != 0)
        return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    char * work = static_cast<char *>(d_work);
    unsigned long long * key = reinterpret_cast<unsigned long long *>(work + w.key);
    unsigned long long * sorted = reinterpret_cast<unsigned long long *>(work + w.sorted);
    int * idx = reinterpret_cast<int *>(work + w.idx);
    int * flag = reinterpret_cast<int *>(key); // behind the sort: nnz + 1 flags, then their nnz + 1 sums
    int * at = flag + nnz + 1;
    if (nnz > 0) {
        hipLaunchKernelGGL(spmv::agg_key_kernel, dim3((unsigned) (((long long) rows + 15) / 16)), dim3(256), 0, s, rows, aggregates, d_row_ptr,
                           d_column_index, plan->d_agg, key, idx);
        HIP_TRY(hipGetLastError());
        rc = sort_pairs<unsigned long long>(key, sorted, idx, d_entry_order, nnz, bits_of((unsigned long long) aggregates * (unsigned) aggregates), s);
        if (rc != 0)
            return rc;
        hipLaunchKernelGGL(spmv::agg_head_kernel, dim3(blocks_of((long long) nnz + 1)), dim3(256), 0, s, nnz, sorted, flag);
        HIP_TRY(hipGetLastError());
        rc = scan(flag, at, (long long) nnz + 1, s, "the prefix sum over the coarse entries");
        if (rc != 0)
            return rc;
        hipLaunchKernelGGL(spmv::agg_pattern_kernel, dim3(blocks_of((long long) nnz + 1)), dim3(256), 0, s, nnz, aggregates, sorted, at,
                           d_coarse_row_ptr, d_coarse_column_index, d_entry_ptr, d_status);
        HIP_TRY(hipGetLastError());
    } else {
        HIP_TRY(hipMemsetAsync(d_coarse_row_ptr, 0, ((size_t) aggregates + 1) * 4, s));
        HIP_TRY(hipMemsetAsync(d_entry_ptr, 0, 4, s));
        HIP_TRY(hipMemsetAsync(d_status, 0, 4, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    return SPMV_HIP_OK;
}

int agg_numeric(int32_t nnz, int32_t nnz_c, const int32_t * d_entry_order, const int32_t * d_entry_ptr, const double * d_value,
                double * d_coarse_value, void * stream)
{
    if (nnz < 0 || nnz_c < 0 || nnz_c > nnz)
        return fail(SPMV_HIP_ERR_INVALID, "nnz < 0, or nnz_c outside 0 ... nnz");
    if (!d_entry_order || !d_entry_ptr || !d_value || !d_coarse_value)
        return fail(SPMV_HIP_ERR_INVALID, "null device pointer");
    const KrylovArray arrays[] = {{d_entry_order, (unsigned long long) nnz * 4, false, 4, "d_entry_order"},
                                  {d_entry_ptr, ((unsigned long long) nnz_c + 1) * 4, false, 4, "d_entry_ptr"},
                                  {d_value, (unsigned long long) nnz * 8, false, 8, "d_value"},
                                  {d_coarse_value, (unsigned long long) nnz_c * 8, true, 8, "d_coarse_value"}};
    const int rc = krylov_check_arrays(0, 8, arrays, (int) (sizeof arrays / sizeof arrays[0]));
    if (rc != 0)
        return rc;
    if (nnz_c == 0)
        return SPMV_HIP_OK;
    hipLaunchKernelGGL(spmv::agg_numeric_kernel, dim3(blocks_of(nnz_c)), dim3(256), 0, static_cast<hipStream_t>(stream), nnz_c, d_entry_order,
                       d_entry_ptr, d_value, d_coarse_value);
    HIP_TRY(hipGetLastError());
    return SPMV_HIP_OK;
}

// the arrays of a restriction (r_c written) or a prolongation (x written): `fine` has rows, `coarse` aggregates elements
template <class T>
int check_vectors(const Plan * plan, const T * fine, bool fine_written, const T * coarse, const char * fine_name, const char * coarse_name)
{
    const unsigned long long r4 = (unsigned long long) plan->rows * 4;
    const KrylovArray arrays[] = {{plan->d_agg, r4, false, 4, "plan->d_agg"},
                                  {plan->d_member_ptr, ((unsigned long long) plan->aggregates + 1) * 4, false, 4, "plan->d_member_ptr"},
                                  {plan->d_member, r4, false, 4, "plan->d_member"},
                                  {fine, (unsigned long long) plan->rows * sizeof(T), fine_written, 16, fine_name},
                                  {coarse, (unsigned long long) plan->aggregates * sizeof(T), !fine_written, 16, coarse_name}};
    return krylov_check_arrays(plan->rows, sizeof(T), arrays, (int) (sizeof arrays / sizeof arrays[0]));
}

template <class T>
int agg_restrict(const Plan * plan, const T * d_r, T * d_rc, void * stream)
{
    int rc = check_plan(plan);
    if (rc != 0)
        return rc;
    if (!d_r || !d_rc)
        return fail(SPMV_HIP_ERR_INVALID, "null device pointer");
    rc = check_vectors<T>(plan, d_r, false, d_rc, "d_r", "d_rc");
    if (rc != 0)
        return rc;
    if (plan->rows == 0)
        return SPMV_HIP_OK;
    const long long waves = ((long long) plan->aggregates + spmv::kAggRestrictChunk - 1) / spmv::kAggRestrictChunk;
    hipLaunchKernelGGL(spmv::agg_restrict_kernel<T>, dim3(krylov_blocks(waves)), dim3(256), 0, static_cast<hipStream_t>(stream), plan->aggregates,
                       plan->rows, plan->d_member_ptr, plan->d_member, d_r, d_rc);
    HIP_TRY(hipGetLastError());
    return SPMV_HIP_OK;
}

// ---- include/spmv_hip_agg_mis2.h ---------------------------------------------------------------------------------------------------

bool group_ok(int32_t group) { return group >= 1 && group <= spmv::kWave && (group & (group - 1)) == 0; }

template <class T, int G>
void launch_group(const Plan * plan, const T * d_r, T * d_rc, hipStream_t s)
{
    const long long per_wave = (long long) spmv::kAggGroupPasses * (spmv::kWave / G);
    const long long waves = (plan->aggregates + per_wave - 1) / per_wave;
    hipLaunchKernelGGL((spmv::agg_restrict_group_kernel<T, G>), dim3(krylov_blocks(waves)), dim3(256), 0, s, plan->aggregates, plan->d_member_ptr,
                       plan->d_member, d_r, d_rc);
}

template <class T>
int agg_restrict_group(const Plan * plan, int32_t group, const T * d_r, T * d_rc, void * stream)
{
    int rc = check_plan(plan);
    if (rc != 0)
        return rc;
    if (!group_ok(group))
        return fail(SPMV_HIP_ERR_INVALID, "group is not a power of two in 1 ... 64");
    if (group == 1)
        return agg_restrict(plan, d_r, d_rc, stream); // the same sums by contract: the same kernel
    if (!d_r || !d_rc)
        return fail(SPMV_HIP_ERR_INVALID, "null device pointer");
    rc = check_vectors<T>(plan, d_r, false, d_rc, "d_r", "d_rc");
    if (rc != 0)
        return rc;
    if (plan->rows == 0)
        return SPMV_HIP_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    dispatch_group(group, [&](auto G) {
        if constexpr (G() >= 2) // (a group of one lane went to agg_restrict above)
            launch_group<T, G()>(plan, d_r, d_rc, s);
    });
    HIP_TRY(hipGetLastError());
    return SPMV_HIP_OK;
}

template <class T>
int agg_prolong_add(const Plan * plan, double omega, const T * d_ec, T * d_x, void * stream)
{
    int rc = check_plan(plan);
    if (rc != 0)
        return rc;
    if (!std::isfinite(omega))
        return fail(SPMV_HIP_ERR_INVALID, "omega is not finite");
    if (!d_ec || !d_x)
        return fail(SPMV_HIP_ERR_INVALID, "null device pointer");
    rc = check_vectors<T>(plan, d_x, true, d_ec, "d_x", "d_ec");
    if (rc != 0)
        return rc;
    return krylov_launch(spmv::agg_prolong_kernel<T>, krylov_slots(plan->rows), static_cast<hipStream_t>(stream), plan->rows, omega, plan->d_agg, d_ec,
                         d_x);
}

} // namespace

extern "C" {

int spmv_hip_agg_workspace(int32_t rows, int32_t nnz, size_t * bytes)
{
    if (rows < 0 || nnz < 0 || !bytes)
        return fail(SPMV_HIP_ERR_INVALID, "rows < 0, nnz < 0, or bytes is null");
    *bytes = work_of(rows, nnz).bytes;
    return SPMV_HIP_OK;
}

int spmv_hip_agg_aggregate(int32_t rows, const int32_t * d_row_ptr, const int32_t * d_column_index, const double * d_value, double theta,
                           uint32_t seed, int32_t * d_agg, int32_t * d_status, void * d_work, size_t work_bytes, void * stream)
{
    return agg_aggregate(false, rows, d_row_ptr, d_column_index, d_value, theta, seed, d_agg, d_status, d_work, work_bytes, stream);
}

int spmv_hip_agg_plan(int32_t rows, const int32_t * d_agg, const int32_t * d_status, int32_t * d_member_ptr, int32_t * d_member,
                      struct spmv_hip_agg_plan * plan, void * d_work, size_t work_bytes, void * stream)
{
    return agg_plan(rows, d_agg, d_status, d_member_ptr, d_member, plan, d_work, work_bytes, stream);
}

int spmv_hip_agg_galerkin_symbolic(const struct spmv_hip_agg_plan * plan, int32_t nnz, const int32_t * d_row_ptr, const int32_t * d_column_index,
                                   int32_t * d_coarse_row_ptr, int32_t * d_coarse_column_index, int32_t * d_entry_order, int32_t * d_entry_ptr,
                                   int32_t * d_status, void * d_work, size_t work_bytes, void * stream)
{
    return agg_symbolic(plan, nnz, d_row_ptr, d_column_index, d_coarse_row_ptr, d_coarse_column_index, d_entry_order, d_entry_ptr, d_status, d_work,
                        work_bytes, stream);
}

int spmv_hip_agg_galerkin_numeric(int32_t nnz, int32_t nnz_c, const int32_t * d_entry_order, const int32_t * d_entry_ptr, const double * d_value,
                                  double * d_coarse_value, void * stream)
{
    return agg_numeric(nnz, nnz_c, d_entry_order, d_entry_ptr, d_value, d_coarse_value, stream);
}

int spmv_hip_agg_restrict_f64(const struct spmv_hip_agg_plan * plan, const double * d_r, double * d_rc, void * stream)
{
    return agg_restrict(plan, d_r, d_rc, stream);
}

int spmv_hip_agg_restrict_f32(const struct spmv_hip_agg_plan * plan, const float * d_r, float * d_rc, void * stream)
{
    return agg_restrict(plan, d_r, d_rc, stream);
}

int spmv_hip_agg_prolong_add_f64(const struct spmv_hip_agg_plan * plan, double omega, const double * d_ec, double * d_x, void * stream)
{
    return agg_prolong_add(plan, omega, d_ec, d_x, stream);
}

int spmv_hip_agg_prolong_add_f32(const struct spmv_hip_agg_plan * plan, double omega, const float * d_ec, float * d_x, void * stream)
{
    return agg_prolong_add(plan, omega, d_ec, d_x, stream);
}

int spmv_hip_agg_mis2_workspace(int32_t rows, size_t * bytes)
{
    if (rows < 0 || !bytes)
        return fail(SPMV_HIP_ERR_INVALID, "rows < 0, or bytes is null");
    *bytes = work_of(rows, 0, true).bytes;
    return SPMV_HIP_OK;
}

int spmv_hip_agg_aggregate_mis2(int32_t rows, const int32_t * d_row_ptr, const int32_t * d_column_index, const double * d_value, double theta,
                                uint32_t seed, int32_t * d_agg, int32_t * d_status, void * d_work, size_t work_bytes, void * stream)
{
    return agg_aggregate(true, rows, d_row_ptr, d_column_index, d_value, theta, seed, d_agg, d_status, d_work, work_bytes, stream);
}

int spmv_hip_agg_restrict_group_f64(const struct spmv_hip_agg_plan * plan, int32_t group, const double * d_r, double * d_rc, void * stream)
{
    return agg_restrict_group(plan, group, d_r, d_rc, stream);
}

int spmv_hip_agg_restrict_group_f32(const struct spmv_hip_agg_plan * plan, int32_t group, const float * d_r, float * d_rc, void * stream)
{
    return agg_restrict_group(plan, group, d_r, d_rc, stream);
}

int32_t spmv_hip_agg_group(const struct spmv_hip_agg_plan * plan)
{
    if (!plan || plan->rows <= 0 || plan->aggregates <= 0)
        return 1;
    int32_t g = 1;
    while (g < spmv::kWave && (long long) g * plan->aggregates < plan->rows)
        g *= 2;
    return g;
}

} // extern "C"
