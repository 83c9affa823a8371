// transpose.hip -- include/spmv_hip_transpose.h: y += A' x from the CSR arrays of A as the caller holds them.  The plan cuts the
// rows into ranges and chooses each range's LDS windows of y on the host (the greedy bucket cover of symmetric.hip without an
// implied own-rows window, over columns instead of rows); the kernel is csr_transpose.hpp.
#include "internal.hpp"
#include "csr_transpose.hpp"

#include <algorithm>
#include <new>
#include <thread>

using namespace spmvi;

struct spmv_hip_tr_plan {
    int32_t rows = 0, cols = 0, nnz = 0;
    int R = 0;           // rows per range
    int ranges = 0;
    int max_windows = 0; // windows per range in the table
    int kw = 0;          // kernel instantiation: 1, 2, 4 or 8 windows
    int slots = 0;       // LDS doubles per workgroup (the largest set of windows)
    size_t lds_bytes = 0;
    int2 * d_win = nullptr; // [ranges][max_windows] {first column, length}
    long long windows_used = 0, window_slots = 0, spilled = 0, most_entries = 0;
    size_t device_bytes = 0;
};

namespace {

constexpr int kTrRows = 2048;              // rows per range (automatic)
constexpr int kTrAutoWindows = 4;          // the spilled share of the stand-ins stops falling there
constexpr size_t kTrLdsBytes = 80 * 1024;  // per workgroup: two workgroups of 512 threads per CU (160 KB)
constexpr int kTrBucket = 32;              // window boundaries in steps of 32 doubles (256 B)

int check_windows_args(int max_windows, int window_doubles)
{
    if (max_windows < 0 || max_windows > spmv::kTrMaxWindows || window_doubles < 0)
        return fail(SPMV_HIP_ERR_INVALID, "max_windows must be 0 .. 8 and window_doubles >= 0");
    return SPMV_HIP_OK;
}

struct RangeWindows {
    int2 w[spmv::kTrMaxWindows];
    int n = 0;
    long long spilled = 0;
};

// The windows of the rows [r0, r0 + nr): the columns of their entries counted per bucket of 32 doubles, then greedily the span
// of at most `cap` doubles (and what is left of `budget`) that covers the most entries, its buckets taken out, and again -- up
// to `nwin` windows, which therefore never overlap.  What no window covers is spilled.
void choose_windows(int32_t cols, const int32_t * rp, const int32_t * col, int r0, int nr, int nwin, int cap, int budget,
                    RangeWindows & out, std::vector<std::pair<int, int>> & buckets)
{
    buckets.clear();
    const long long entries = (long long) rp[r0 + nr] - rp[r0];
    for (int32_t e = rp[r0]; e < rp[r0 + nr]; ++e) {
        const int b = col[e] / kTrBucket;
        if (!buckets.empty() && buckets.back().first == b)
            ++buckets.back().second;
        else
            buckets.emplace_back(b, 1);
    }
    out.n = 0;
    if (!buckets.empty()) {
        std::sort(buckets.begin(), buckets.end());
        size_t m = 0; // merge equal buckets
        for (size_t k = 0; k < buckets.size(); ++k) {
            if (m > 0 && buckets[m - 1].first == buckets[k].first)
                buckets[m - 1].second += buckets[k].second;
            else
                buckets[m++] = buckets[k];
        }
        buckets.resize(m);
    }
    // First the exact cover: the hit buckets cut at their nwin - 1 widest gaps.  Where those runs fit the budget they are the
    // windows -- nothing spilled and no slot spent on a gap (the three lines a range of a 5-point stencil hits, each one
    // window), which a greedy first window as wide as the whole budget would not find.
    if (nwin > 0 && !buckets.empty()) {
        std::vector<std::pair<int, size_t>> gaps; // {empty buckets in front of bucket k, k}
        for (size_t k = 1; k < buckets.size(); ++k)
            if (buckets[k].first - buckets[k - 1].first > 1)
                gaps.emplace_back(buckets[k].first - buckets[k - 1].first - 1, k);
        std::sort(gaps.begin(), gaps.end(), [](std::pair<int, size_t> const & a, std::pair<int, size_t> const & b) {
            return a.first != b.first ? a.first > b.first : a.second < b.second;
        });
        if (gaps.size() > (size_t) nwin - 1)
            gaps.resize((size_t) nwin - 1);
        std::vector<size_t> cut{0};
        for (auto const & g : gaps)
            cut.push_back(g.second);
        cut.push_back(buckets.size());
        std::sort(cut.begin(), cut.end());
        long long total = 0;
        bool fits = true;
        for (size_t k = 0; k + 1 < cut.size(); ++k) {
            const int width = (buckets[cut[k + 1] - 1].first + 1 - buckets[cut[k]].first) * kTrBucket;
            fits &= width <= cap;
            total += width;
        }
        if (fits && total <= budget) {
            for (size_t k = 0; k + 1 < cut.size(); ++k) {
                const int first = buckets[cut[k]].first * kTrBucket;
                const int last = (int) std::min((long long) cols, (long long) (buckets[cut[k + 1] - 1].first + 1) * kTrBucket);
                out.w[out.n++] = make_int2(first, last - first);
            }
            out.spilled = 0;
            return;
        }
    }
    long long covered = 0;
    while (out.n < nwin && !buckets.empty()) {
        const int span = std::min(cap, budget) / kTrBucket; // buckets per window
        if (span < 1)
            break;
        size_t best_lo = 0, best_hi = 0, lo = 0;
        long long best = -1, sum = 0;
        for (size_t hi = 0; hi < buckets.size(); ++hi) {
            sum += buckets[hi].second;
            while (buckets[hi].first - buckets[lo].first >= span)
                sum -= buckets[lo++].second;
            if (sum > best) {
                best = sum;
                best_lo = lo;
                best_hi = hi;
            }
        }
        const int first = buckets[best_lo].first * kTrBucket;
        const int last = (int) std::min((long long) cols, (long long) (buckets[best_hi].first + 1) * kTrBucket);
        out.w[out.n++] = make_int2(first, last - first);
        budget -= (buckets[best_hi].first + 1 - buckets[best_lo].first) * kTrBucket;
        covered += best;
        buckets.erase(buckets.begin() + (long) best_lo, buckets.begin() + (long) best_hi + 1);
    }
    out.spilled = entries - covered;
}

// what the preview and the plan share: every number of plan_info and the window table
struct HostPlan {
    spmv_hip_tr_plan numbers;
    std::vector<int2> table;
};

// row_ptr and the window arguments already checked; the columns are checked here
int plan_host(HostPlan & hp, int32_t rows, int32_t cols, const int32_t * rp, const int32_t * col, int max_windows, int window_doubles)
{
    spmv_hip_tr_plan & pl = hp.numbers;
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
    pl.max_windows = max_windows > 0 ? max_windows : kTrAutoWindows;
    pl.kw = pl.max_windows <= 1 ? 1 : pl.max_windows <= 2 ? 2 : pl.max_windows <= 4 ? 4 : 8;
    pl.R = std::max(1, std::min(kTrRows, window_doubles > 0 ? window_doubles : kTrRows));
    pl.ranges = rows > 0 && cols > 0 && nnz > 0 ? (int) ((rows + (long long) pl.R - 1) / pl.R) : 0;
    // LDS: windows (doubles) + R + 1 ints of row_ptr
    const int budget_all = (int) ((kTrLdsBytes - 4 * ((size_t) pl.R + 1)) / 8) / kTrBucket * kTrBucket;
    const int budget = window_doubles > 0 ? (int) std::min((long long) budget_all, (long long) pl.max_windows * window_doubles) : budget_all;
    const int cap = window_doubles > 0 ? window_doubles : budget;

    std::vector<RangeWindows> wins((size_t) pl.ranges);
    const int threads = (int) std::max(1u, std::min({8u, std::thread::hardware_concurrency(), (unsigned) (pl.ranges / 16 + 1)}));
    std::vector<char> done((size_t) threads, 0);
    auto work = [&](int t) {
        std::vector<std::pair<int, int>> buckets;
        for (int b = t; b < pl.ranges; b += threads) {
            const int r0 = b * pl.R;
            choose_windows(cols, rp, col, r0, std::min(pl.R, rows - r0), pl.max_windows, cap, budget, wins[(size_t) b], buckets);
        }
        done[(size_t) t] = 1;
    };
    {
        std::vector<std::thread> pool;
        try {
            for (int t = 1; t < threads; ++t)
                pool.emplace_back(work, t);
        } catch (...) {
            // fewer helpers: the ranges they would have taken are done below
        }
        work(0);
        for (auto & th : pool)
            th.join();
        for (int t = 1; t < threads; ++t) // helpers that could not be started
            if (!done[(size_t) t])
                work(t);
    }
    int most = 0;
    hp.table.assign((size_t) pl.ranges * (size_t) pl.max_windows, make_int2(0, 0));
    for (int b = 0; b < pl.ranges; ++b) {
        RangeWindows const & w = wins[(size_t) b];
        int sum = 0;
        for (int k = 0; k < w.n; ++k) {
            hp.table[(size_t) b * pl.max_windows + k] = w.w[k];
            sum += w.w[k].y;
        }
        most = std::max(most, sum);
        pl.windows_used += w.n;
        pl.window_slots += sum;
        pl.spilled += w.spilled;
        const int r0 = b * pl.R;
        pl.most_entries = std::max(pl.most_entries, (long long) rp[r0 + std::min(pl.R, rows - r0)] - rp[r0]);
    }
    pl.slots = most;
    pl.lds_bytes = pl.ranges > 0 ? 8 * (size_t) pl.slots + 4 * ((size_t) pl.R + 1) : 0;
    pl.device_bytes = hp.table.size() * sizeof(int2);
    return SPMV_HIP_OK;
}

void plan_numbers(const spmv_hip_tr_plan & pl, int64_t * out, int n)
{
    const int64_t v[SPMV_HIP_TR_INFO] = {pl.ranges,
                                         pl.R,
                                         pl.max_windows,
                                         pl.windows_used,
                                         (int64_t) pl.lds_bytes,
                                         pl.spilled,
                                         8 * (pl.window_slots + pl.spilled),
                                         pl.nnz,
                                         pl.rows,
                                         pl.cols,
                                         (int64_t) pl.device_bytes,
                                         12LL * pl.nnz + 4LL * (pl.rows + 1LL) + 8LL * pl.rows,
                                         pl.window_slots,
                                         pl.most_entries};
    for (int i = 0; i < n && i < SPMV_HIP_TR_INFO; ++i)
        out[i] = v[i];
}

template <int KW>
hipError_t allow_lds()
{
    return hipFuncSetAttribute((const void *) spmv::csr_spmv_t_kernel<KW>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) kTrLdsBytes);
}

// the host plan onto the current device: the window table, and the kernel's LDS limit where it is above the default 64 KB
int build_tr_plan(spmv_hip_tr_plan ** out, HostPlan const & hp)
{
    spmv_hip_tr_plan * pl = new (std::nothrow) spmv_hip_tr_plan(hp.numbers);
    if (!pl)
        return fail(SPMV_HIP_ERR_ALLOC, "plan allocation failed");
    if (!hp.table.empty()) {
        hipError_t e = hipMalloc((void **) &pl->d_win, hp.table.size() * sizeof(int2));
        if (e == hipSuccess)
            e = hipMemcpy(pl->d_win, hp.table.data(), hp.table.size() * sizeof(int2), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            spmv_hip_tr_plan_destroy(pl);
            return fail_hip(e, "transposed plan: window table");
        }
    }
    if (pl->lds_bytes > 64 * 1024) {
        const hipError_t e = pl->kw == 1 ? allow_lds<1>() : pl->kw == 2 ? allow_lds<2>() : pl->kw == 4 ? allow_lds<4>() : allow_lds<8>();
        if (e != hipSuccess) {
            spmv_hip_tr_plan_destroy(pl);
            return fail_hip(e, "transposed plan: LDS size");
        }
    }
    *out = pl;
    return SPMV_HIP_OK;
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
    HostPlan hp;
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
    // the columns come back to the host once: they are checked and the windows are chosen there
    std::vector<int32_t> col;
    HostPlan hp;
    try {
        col.resize((size_t) nnz);
        if (nnz > 0) {
            hipStream_t s = static_cast<hipStream_t>(stream);
            HIP_TRY(hipMemcpyAsync(col.data(), d_column_index, (size_t) nnz * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
        }
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
    if (pl->ranges == 0) // rows, cols or nnz of zero
        return SPMV_HIP_OK;
    if (!d_row_ptr || !d_column_index || !d_value || !d_x || !d_y)
        return fail(SPMV_HIP_ERR_INVALID, "null device pointer");
    if (!aligned16(d_column_index) || !aligned16(d_value))
        return fail(SPMV_HIP_ERR_ALIGN, "column / value arrays must be 16-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned) pl->ranges), block(spmv::kTrBlock);
#define SPMV_TR_LAUNCH(KW)                                                                                                          \
    hipLaunchKernelGGL(spmv::csr_spmv_t_kernel<KW>, grid, block, pl->lds_bytes, s, pl->rows, pl->cols, pl->R, d_row_ptr, d_column_index, \
                       d_value, d_x, d_y, pl->d_win, pl->max_windows, pl->slots)
    switch (pl->kw) {
    case 1: SPMV_TR_LAUNCH(1); break;
    case 2: SPMV_TR_LAUNCH(2); break;
    case 4: SPMV_TR_LAUNCH(4); break;
    default: SPMV_TR_LAUNCH(8); break;
    }
#undef SPMV_TR_LAUNCH
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
    if (!pl)
        return;
    if (pl->d_win)
        (void) hipFree(pl->d_win);
    delete pl;
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
    HostPlan hp;
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
    c->bytes += c->tr_plan->device_bytes;
    c->format = 6;
    return SPMV_HIP_OK;
}

} // extern "C"
