// transpose.hip -- include/spmv_hip_transpose.h: y += A' x from the CSR arrays of A as the caller holds them.  The ranges, each
// range's LDS windows of y and their table are window_plan.hpp (shared with symmetric.hip: here no window is implied, the
// targets are columns, and the exact cover is tried first); the kernel is csr_transpose.hpp.
#include "internal.hpp"
#include "csr_transpose.hpp"
#include "window_plan.hpp"

using namespace spmvi;

struct spmv_hip_tr_plan {
    int32_t rows = 0, cols = 0, nnz = 0;
    WindowPlan win; // the table holds max_windows windows per range
    long long most_entries = 0;
};

namespace {

// row_ptr and the window arguments already checked; the columns are checked here
int plan_host(HostPlan<spmv_hip_tr_plan> & hp, int32_t rows, int32_t cols, const int32_t * rp, const int32_t * col, int max_windows,
              int window_doubles)
{
    spmv_hip_tr_plan & pl = hp.numbers;
    WindowPlan & w = pl.win;
    const int32_t nnz = rp[rows];
    if (nnz > 0 && !col)
        return fail(SPMV_HIP_ERR_INVALID, "column_index is null");
    bool bad = false;
    for (int32_t e = 0; e < nnz; ++e)
        bad |= col[e] < 0 || col[e] >= cols;
    if (bad)
        return fail(SPMV_HIP_ERR_INVALID, "column index out of range [0, cols)");
    pl.rows = rows;
    pl.cols = cols;
    pl.nnz = nnz;
    w.max_windows = w.stride = max_windows > 0 ? max_windows : kWinAutoWindows;
    w.kw = w.stride <= 1 ? 1 : w.stride <= 2 ? 2 : w.stride <= 4 ? 4 : 8;
    w.R = std::max(1, std::min(kWinRows, window_doubles > 0 ? window_doubles : kWinRows));
    w.ranges = rows > 0 && cols > 0 && nnz > 0 ? (int) ((rows + (long long) w.R - 1) / w.R) : 0;
    // LDS: windows (doubles) + R + 1 ints of row_ptr
    const int budget_all = (int) ((kWinLdsBytes - 4 * ((size_t) w.R + 1)) / 8) / kWinBucket * kWinBucket;
    const int budget = window_doubles > 0 ? (int) std::min((long long) budget_all, (long long) w.stride * window_doubles) : budget_all;
    const int cap = window_doubles > 0 ? window_doubles : budget;
    plan_windows(w, hp.table, CoverRule{/*own_rows=*/false, /*exact_first=*/true}, rows, cols, rp, col, cap, budget);
    w.lds_bytes = w.ranges > 0 ? 8 * (size_t) w.slots + 4 * ((size_t) w.R + 1) : 0;
    for (int b = 0; b < w.ranges; ++b) {
        const int r0 = b * w.R;
        pl.most_entries = std::max(pl.most_entries, (long long) rp[r0 + std::min(w.R, rows - r0)] - rp[r0]);
    }
    return SPMV_HIP_OK;
}

void plan_numbers(const spmv_hip_tr_plan & pl, int64_t * out, int n)
{
    const int64_t v[SPMV_HIP_TR_INFO] = {pl.win.ranges,
                                         pl.win.R,
                                         pl.win.max_windows,
                                         pl.win.windows_used,
                                         (int64_t) pl.win.lds_bytes,
                                         pl.win.spilled,
                                         8 * (pl.win.window_slots + pl.win.spilled),
                                         pl.nnz,
                                         pl.rows,
                                         pl.cols,
                                         (int64_t) pl.win.device_bytes,
                                         12LL * pl.nnz + 4LL * (pl.rows + 1LL) + 8LL * pl.rows,
                                         pl.win.window_slots,
                                         pl.most_entries};
    for (int i = 0; i < n && i < SPMV_HIP_TR_INFO; ++i)
        out[i] = v[i];
}

template <class F>
auto with_tr_kernel(int kw, F && f)
{
    return with_kw<1, 2, 4, 8>(kw, [&](auto k) { return f(spmv::csr_spmv_t_kernel<decltype(k)::value>); });
}

int build_tr_plan(spmv_hip_tr_plan ** out, HostPlan<spmv_hip_tr_plan> const & hp)
{
    return build_plan(out, hp, "transposed", [](int kw) { return with_tr_kernel(kw, [](auto kernel) { return allow_window_lds(kernel); }); });
}

} // namespace

extern "C" {

int spmv_hip_tr_plan_preview(int32_t rows, int32_t cols, const int32_t * host_row_ptr, const int32_t * host_column_index,
                             int max_windows, int window_doubles, int64_t * out, int n, int32_t * window_table,
                             int64_t window_table_ints)
{
    if (!out || n < 0 || window_table_ints < 0)
        return fail(SPMV_HIP_ERR_INVALID, "out is null, or a negative count");
    int rc;
    if ((rc = check_csr_row_ptr(rows, cols, host_row_ptr)) != 0 || (rc = check_windows_args(max_windows, window_doubles)) != 0)
        return rc;
    HostPlan<spmv_hip_tr_plan> hp;
    try {
        if ((rc = plan_host(hp, rows, cols, host_row_ptr, host_column_index, max_windows, window_doubles)) != 0)
            return rc;
    } catch (std::bad_alloc const &) {
        return fail(SPMV_HIP_ERR_ALLOC, "transposed plan: host memory");
    }
    if (window_table) {
        if ((int64_t) (2 * hp.table.size()) > window_table_ints)
            return fail(SPMV_HIP_ERR_INVALID, "window_table is too small: it takes 2 * ranges * windows per range int32 values");
        for (size_t k = 0; k < hp.table.size(); ++k) {
            window_table[2 * k] = hp.table[k].x;
            window_table[2 * k + 1] = hp.table[k].y;
        }
    }
    plan_numbers(hp.numbers, out, n);
    return SPMV_HIP_OK;
}

int spmv_hip_tr_plan_csr(spmv_hip_tr_plan ** plan, int32_t rows, int32_t cols, const int32_t * host_row_ptr,
                         const int32_t * d_column_index, int max_windows, int window_doubles, void * stream)
{
    if (!plan)
        return fail(SPMV_HIP_ERR_INVALID, "plan is null");
    *plan = nullptr;
    int rc;
    if ((rc = check_csr_row_ptr(rows, cols, host_row_ptr)) != 0 || (rc = check_windows_args(max_windows, window_doubles)) != 0)
        return rc;
    const int32_t nnz = host_row_ptr[rows];
    if (nnz > 0 && !d_column_index)
        return fail(SPMV_HIP_ERR_INVALID, "d_column_index is null");
    std::vector<int32_t> col;
    HostPlan<spmv_hip_tr_plan> hp;
    try {
        if ((rc = read_back_columns(col, nnz, d_column_index, stream)) != 0)
            return rc;
        if ((rc = plan_host(hp, rows, cols, host_row_ptr, col.data(), max_windows, window_doubles)) != 0)
            return rc;
    } catch (std::bad_alloc const &) {
        return fail(SPMV_HIP_ERR_ALLOC, "transposed plan: host memory");
    }
    return build_tr_plan(plan, hp);
}

int spmv_hip_csr_spmv_t(const spmv_hip_tr_plan * pl, const int32_t * d_row_ptr, const int32_t * d_column_index,
                        const double * d_value, const double * d_x, double * d_y, void * stream)
{
    if (!pl)
        return fail(SPMV_HIP_ERR_INVALID, "plan is null");
    if (d_x && (const void *) d_x == (const void *) d_y)
        return fail(SPMV_HIP_ERR_INVALID, "d_x and d_y must be different arrays");
    if (pl->win.ranges == 0) // rows, cols or nnz of zero
        return SPMV_HIP_OK;
    int rc = check_multiply_arrays(d_row_ptr, d_column_index, d_value, d_x, d_y);
    if (rc != 0)
        return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    WindowPlan const & w = pl->win;
    with_tr_kernel(w.kw, [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned) w.ranges), dim3(spmv::kWinBlock), w.lds_bytes, s, pl->rows, pl->cols, w.R, d_row_ptr,
                           d_column_index, d_value, d_x, d_y, w.d_win, w.stride, w.slots);
        return 0;
    });
    HIP_TRY(hipGetLastError());
    return SPMV_HIP_OK;
}

int spmv_hip_tr_plan_info(const spmv_hip_tr_plan * pl, int64_t * out, int n)
{
    if (!pl || !out || n < 0)
        return fail(SPMV_HIP_ERR_INVALID, "plan/out null");
    plan_numbers(*pl, out, n);
    return SPMV_HIP_OK;
}

void spmv_hip_tr_plan_destroy(spmv_hip_tr_plan * pl)
{
    free_plan(pl);
}

// ---- Level 1 --------------------------------------------------------------------------------------------------------------------

int spmv_hip_upload_csr_transposed(spmv_hip_ctx * c, int32_t rows, int32_t cols, int32_t nnz, const int32_t * row_ptr,
                                   const int32_t * column_index, const double * value)
{
    int rc = upload_csr_prelude(c, "a transposed multiply runs on one device (a row partition would need a reduction of y across devices)",
                                "SPMV_HIP_FLAG_EXACT_ORDER cannot be kept: a transposed multiply adds its products with atomics", rows, cols, nnz,
                                row_ptr, column_index, value);
    if (rc == 0)
        rc = check_csr_row_ptr(rows, cols, row_ptr);
    if (rc != 0)
        return rc;
    if (row_ptr[rows] != nnz)
        return fail(SPMV_HIP_ERR_INVALID, "row_ptr[rows] must equal nnz");
    // the plan's host part first: it refuses a bad column before anything is freed or copied
    HostPlan<spmv_hip_tr_plan> hp;
    try {
        if ((rc = plan_host(hp, rows, cols, row_ptr, column_index, 0, 0)) != 0)
            return rc;
    } catch (std::bad_alloc const &) {
        return fail(SPMV_HIP_ERR_ALLOC, "transposed plan: host memory");
    }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    free_ctx_matrix(c);
    if ((rc = build_tr_plan(&c->tr_plan, hp)) != 0)
        return rc;
    // the context holds the operator that runs, A': its x has `rows` entries and its y `cols`
    if ((rc = upload_ctx_csr(c, (size_t) rows + 1, (size_t) rows, (size_t) cols, (size_t) nnz, row_ptr, column_index, true, value, false)) != 0)
        return rc;
    c->rows = cols;
    c->cols = rows;
    c->nnz = nnz;
    c->bytes += c->tr_plan->win.device_bytes;
    c->format = 6;
    return SPMV_HIP_OK;
}

} // extern "C"
