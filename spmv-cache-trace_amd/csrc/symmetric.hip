// symmetric.hip -- include/spmv_hip_symmetric.h: the multiply of a stored triangle as the symmetric (or skew-symmetric) matrix it
// stands for.  The plan classifies the triangle here; the ranges, each range's LDS windows of y beside its own rows and their
// table are window_plan.hpp (shared with transpose.hip); the kernel is csr_symmetric.hpp.
#include "internal.hpp"
#include "csr_symmetric.hpp"
#include "window_plan.hpp"

using namespace spmvi;

struct spmv_hip_sym_plan {
    int32_t rows = 0, nnz = 0;
    int kind = SPMV_HIP_SYMMETRIC;
    int triangle = SPMV_HIP_TRIANGLE_DIAGONAL;
    long long diagonal = 0;
    WindowPlan win; // max_windows counts the own window; the table holds the max_windows - 1 others
};

namespace {

int check_csr_host(int32_t rows, const int32_t * rp)
{
    if (rows < 0 || !rp)
        return fail(SPMV_HIP_ERR_INVALID, "bad CSR arguments (rows < 0 or row_ptr null)");
    return check_row_ptr_order(rows, rp);
}

// triangle + diagonal count + column range check; row_ptr already checked
int classify(int32_t rows, const int32_t * rp, const int32_t * col, int * triangle, long long * diagonal)
{
    bool below = false, above = false, bad = false;
    long long diag = 0;
    for (int32_t r = 0; r < rows; ++r)
        for (int32_t e = rp[r]; e < rp[r + 1]; ++e) {
            const int32_t j = col[e];
            bad |= j < 0 || j >= rows;
            below |= j < r;
            above |= j > r;
            diag += j == r;
        }
    if (bad)
        return fail(SPMV_HIP_ERR_INVALID, "column index out of range [0, rows)");
    *triangle = below && above ? SPMV_HIP_TRIANGLE_MIXED
        : below                ? SPMV_HIP_TRIANGLE_LOWER
        : above                ? SPMV_HIP_TRIANGLE_UPPER
                               : SPMV_HIP_TRIANGLE_DIAGONAL;
    *diagonal = diag;
    return SPMV_HIP_OK;
}

// row_ptr already checked; kind, the window arguments and the columns are checked here
int plan_host(HostPlan<spmv_hip_sym_plan> & hp, int32_t rows, const int32_t * rp, const int32_t * col, int kind, int max_windows,
              int window_doubles)
{
    spmv_hip_sym_plan & pl = hp.numbers;
    WindowPlan & w = pl.win;
    if (kind != SPMV_HIP_SYMMETRIC && kind != SPMV_HIP_SKEW_SYMMETRIC)
        return fail(SPMV_HIP_ERR_INVALID, "kind must be SPMV_HIP_SYMMETRIC or SPMV_HIP_SKEW_SYMMETRIC");
    int rc;
    if ((rc = check_windows_args(max_windows, window_doubles)) != 0)
        return rc;
    if (rp[rows] > 0 && !col)
        return fail(SPMV_HIP_ERR_INVALID, "column_index is null");
    if ((rc = classify(rows, rp, col, &pl.triangle, &pl.diagonal)) != 0)
        return rc;
    if (pl.triangle == SPMV_HIP_TRIANGLE_MIXED)
        return fail(SPMV_HIP_ERR_INVALID, "the matrix has entries on both sides of the diagonal: not a stored triangle");
    if (kind == SPMV_HIP_SKEW_SYMMETRIC && pl.diagonal > 0)
        return fail(SPMV_HIP_ERR_INVALID, "a skew-symmetric matrix has no diagonal entries");
    pl.rows = rows;
    pl.nnz = rp[rows];
    pl.kind = kind;
    w.max_windows = max_windows > 0 ? max_windows : kWinAutoWindows;
    w.stride = w.max_windows - 1;
    w.kw = w.stride == 0 ? 0 : w.stride == 1 ? 1 : w.stride <= 3 ? 3 : 7;
    w.R = std::max(1, std::min(kWinRows, window_doubles > 0 ? window_doubles : kWinRows));
    w.ranges = rows > 0 ? (int) ((rows + (long long) w.R - 1) / w.R) : 0;
    // LDS: own rows + extra windows (doubles) + R + 1 ints of row_ptr
    const int budget_all = (int) ((kWinLdsBytes - 4 * ((size_t) w.R + 1)) / 8) - w.R;
    const int budget = window_doubles > 0 ? std::min(budget_all, w.stride * window_doubles) : budget_all;
    const int cap = window_doubles > 0 ? window_doubles : budget;
    plan_windows(w, hp.table, CoverRule{/*own_rows=*/true, /*exact_first=*/false}, rows, rows, rp, col, cap, budget);
    w.lds_bytes = 8 * (size_t) w.slots + 4 * ((size_t) w.R + 1);
    return SPMV_HIP_OK;
}

template <class F>
auto with_sym_kernel(int kw, F && f)
{
    return with_kw<0, 1, 3, 7>(kw, [&](auto k) { return f(spmv::csr_symv_kernel<decltype(k)::value>); });
}

int build_sym_plan(spmv_hip_sym_plan ** out, HostPlan<spmv_hip_sym_plan> const & hp)
{
    return build_plan(out, hp, "symmetric", [](int kw) { return with_sym_kernel(kw, [](auto kernel) { return allow_window_lds(kernel); }); });
}

} // namespace

extern "C" {

int spmv_hip_csr_triangle(int32_t rows, const int32_t * host_row_ptr, const int32_t * host_column_index, int * triangle,
                          int64_t * diagonal_entries)
{
    if (!triangle || !diagonal_entries)
        return fail(SPMV_HIP_ERR_INVALID, "triangle / diagonal_entries is null");
    int rc = check_csr_host(rows, host_row_ptr);
    if (rc != 0)
        return rc;
    if (host_row_ptr[rows] > 0 && !host_column_index)
        return fail(SPMV_HIP_ERR_INVALID, "column_index is null");
    long long diag = 0;
    if ((rc = classify(rows, host_row_ptr, host_column_index, triangle, &diag)) != 0)
        return rc;
    *diagonal_entries = diag;
    return SPMV_HIP_OK;
}

int spmv_hip_sym_plan_csr(spmv_hip_sym_plan ** plan, int32_t rows, const int32_t * host_row_ptr, const int32_t * d_column_index,
                          int kind, int max_windows, int window_doubles, void * stream)
{
    if (!plan)
        return fail(SPMV_HIP_ERR_INVALID, "plan is null");
    *plan = nullptr;
    int rc = check_csr_host(rows, host_row_ptr);
    if (rc != 0)
        return rc;
    if (kind != SPMV_HIP_SYMMETRIC && kind != SPMV_HIP_SKEW_SYMMETRIC)
        return fail(SPMV_HIP_ERR_INVALID, "kind must be SPMV_HIP_SYMMETRIC or SPMV_HIP_SKEW_SYMMETRIC");
    const int32_t nnz = host_row_ptr[rows];
    if (nnz > 0 && !d_column_index)
        return fail(SPMV_HIP_ERR_INVALID, "d_column_index is null");
    std::vector<int32_t> col;
    try {
        if ((rc = read_back_columns(col, nnz, d_column_index, stream)) != 0)
            return rc;
    } catch (std::bad_alloc const &) {
        return fail(SPMV_HIP_ERR_ALLOC, "host copy of the columns");
    }
    HostPlan<spmv_hip_sym_plan> hp;
    try {
        if ((rc = plan_host(hp, rows, host_row_ptr, col.data(), kind, max_windows, window_doubles)) != 0)
            return rc;
    } catch (std::bad_alloc const &) {
        return fail(SPMV_HIP_ERR_ALLOC, "symmetric plan: host memory");
    }
    return build_sym_plan(plan, hp);
}

int spmv_hip_csr_symv(const spmv_hip_sym_plan * pl, const int32_t * d_row_ptr, const int32_t * d_column_index,
                      const double * d_value, const double * d_x, double * d_y, void * stream)
{
    if (!pl)
        return fail(SPMV_HIP_ERR_INVALID, "plan is null");
    if (pl->rows == 0 || pl->nnz == 0)
        return SPMV_HIP_OK;
    int rc = check_multiply_arrays(d_row_ptr, d_column_index, d_value, d_x, d_y);
    if (rc != 0)
        return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const double tsign = pl->kind == SPMV_HIP_SKEW_SYMMETRIC ? -1.0 : 1.0;
    WindowPlan const & w = pl->win;
    with_sym_kernel(w.kw, [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned) w.ranges), dim3(spmv::kWinBlock), w.lds_bytes, s, pl->rows, w.R, d_row_ptr,
                           d_column_index, d_value, d_x, d_y, w.d_win, w.stride, w.slots, tsign);
        return 0;
    });
    HIP_TRY(hipGetLastError());
    return SPMV_HIP_OK;
}

int spmv_hip_sym_plan_info(const spmv_hip_sym_plan * pl, int64_t * out, int n)
{
    if (!pl || !out || n < 0)
        return fail(SPMV_HIP_ERR_INVALID, "plan/out null");
    const int64_t v[16] = {pl->win.ranges,
                           pl->win.R,
                           pl->win.max_windows,
                           pl->win.windows_used,
                           (int64_t) pl->win.lds_bytes,
                           pl->win.spilled,
                           8 * (pl->win.window_slots + pl->win.spilled),
                           pl->nnz,
                           pl->diagonal,
                           pl->triangle,
                           (int64_t) pl->win.device_bytes,
                           pl->kind,
                           pl->rows,
                           12LL * pl->nnz + 4LL * (pl->rows + 1) + 8LL * pl->rows,
                           pl->win.window_slots,
                           2LL * pl->nnz - pl->diagonal};
    for (int i = 0; i < n && i < 16; ++i)
        out[i] = v[i];
    return SPMV_HIP_OK;
}

void spmv_hip_sym_plan_destroy(spmv_hip_sym_plan * pl)
{
    free_plan(pl);
}

// ---- Level 1 --------------------------------------------------------------------------------------------------------------------

int spmv_hip_upload_csr_symmetric(spmv_hip_ctx * c, int32_t rows, int32_t nnz, const int32_t * row_ptr, const int32_t * column_index,
                                  const double * value, int kind)
{
    int rc = upload_csr_prelude(c, "a symmetric multiply runs on one device (spmv_hip_create_multi partitions rows)",
                                "SPMV_HIP_FLAG_EXACT_ORDER cannot be kept: a symmetric multiply adds partial sums with atomics", rows, rows, nnz,
                                row_ptr, column_index, value);
    if (rc == 0)
        rc = check_csr_host(rows, row_ptr);
    if (rc != 0)
        return rc;
    if (row_ptr[rows] != nnz)
        return fail(SPMV_HIP_ERR_INVALID, "row_ptr[rows] must equal nnz");
    // the plan's host part first: it refuses what is not a stored triangle (a column out of range, an entry in the other triangle,
    // an unknown kind) before anything is freed or copied, so that a refused upload leaves the previous matrix usable
    HostPlan<spmv_hip_sym_plan> hp;
    try {
        if ((rc = plan_host(hp, rows, row_ptr, column_index, kind, 0, 0)) != 0)
            return rc;
    } catch (std::bad_alloc const &) {
        return fail(SPMV_HIP_ERR_ALLOC, "symmetric plan: host memory");
    }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    free_ctx_matrix(c);
    if ((rc = build_sym_plan(&c->sym_plan, hp)) != 0)
        return rc;
    if ((rc = upload_ctx_csr(c, (size_t) rows + 1, (size_t) rows, (size_t) rows, (size_t) nnz, row_ptr, column_index, true, value, false)) != 0)
        return rc;
    c->rows = rows;
    c->cols = rows;
    c->nnz = nnz;
    c->bytes += c->sym_plan->win.device_bytes;
    c->format = 5;
    return SPMV_HIP_OK;
}

} // extern "C"
