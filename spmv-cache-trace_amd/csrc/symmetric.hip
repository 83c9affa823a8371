// symmetric.hip -- include/spmv_hip_symmetric.h: the multiply of a stored triangle as the symmetric (or skew-symmetric) matrix it
// stands for.  The plan cuts the rows into ranges and chooses each range's LDS windows of y on the host; the kernel is
// csr_symmetric.hpp.
#include "internal.hpp"
#include "csr_symmetric.hpp"

#include <algorithm>
#include <chrono>
#include <new>
#include <thread>

using namespace spmvi;

struct spmv_hip_sym_plan {
    int32_t rows = 0, nnz = 0;
    int kind = SPMV_HIP_SYMMETRIC;
    int triangle = SPMV_HIP_TRIANGLE_DIAGONAL;
    long long diagonal = 0;
    int R = 0;                // rows per range
    int ranges = 0;
    int max_windows = 0;      // own window included
    int stride = 0;           // extra windows per range in the table (max_windows - 1)
    int kw = 0;               // kernel instantiation: 0, 1, 3 or 7 extra windows
    int slots = 0;            // LDS doubles per workgroup (own rows + the largest set of extra windows)
    size_t lds_bytes = 0;
    int2 * d_win = nullptr;   // [ranges][stride] {first row, length}
    long long windows_used = 0, window_slots = 0, spilled = 0;
    size_t device_bytes = 0;
};

namespace {

constexpr int kSymRows = 2048;                      // rows per range (automatic)
constexpr int kSymAutoWindows = 4;                  // own rows + previous line + previous plane + one more
constexpr size_t kSymLdsBytes = 80 * 1024;          // per workgroup: two workgroups of 512 threads per CU (160 KB)
constexpr int kSymBucket = 32;                      // window boundaries in steps of 32 doubles (256 B)

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

struct RangeWindows {
    int2 w[spmv::kSymMaxWindows - 1];
    int n = 0;
    long long spilled = 0;
};

// The extra windows of the range [r0, r0 + nr): the targets j of its off-diagonal entries outside its own rows, counted per
// bucket of 32 doubles, then greedily the span of at most `cap` doubles (and what is left of `budget`) that covers the most
// targets, its buckets taken out, and again -- up to `nwin` windows.  What no window covers is spilled.
void choose_windows(int32_t rows, const int32_t * rp, const int32_t * col, int r0, int nr, int nwin, int cap, int budget,
                    RangeWindows & out, std::vector<std::pair<int, int>> & buckets)
{
    buckets.clear();
    long long outside = 0;
    for (int32_t e = rp[r0]; e < rp[r0 + nr]; ++e) {
        const int j = col[e];
        if ((unsigned) (j - r0) < (unsigned) nr)
            continue; // own rows (the diagonal included)
        ++outside;
        const int b = j / kSymBucket;
        if (!buckets.empty() && buckets.back().first == b)
            ++buckets.back().second;
        else
            buckets.emplace_back(b, 1);
    }
    out.n = 0;
    if (nwin > 0 && !buckets.empty()) {
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
    long long covered = 0;
    while (out.n < nwin && !buckets.empty()) {
        const int span = std::min(cap, budget) / kSymBucket; // buckets per window
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
        const int first = buckets[best_lo].first * kSymBucket;
        const int last = std::min((long long) rows, (long long) (buckets[best_hi].first + 1) * kSymBucket);
        out.w[out.n++] = make_int2(first, last - first);
        budget -= last - first;
        covered += best;
        buckets.erase(buckets.begin() + (long) best_lo, buckets.begin() + (long) best_hi + 1);
    }
    out.spilled = outside - covered;
}

int build_sym_plan(spmv_hip_sym_plan ** out, int32_t rows, const int32_t * rp, const int32_t * col, int kind, int max_windows,
                   int window_doubles)
{
    if (!out)
        return fail(SPMV_HIP_ERR_INVALID, "plan is null");
    *out = nullptr;
    int rc;
    if ((rc = check_csr_host(rows, rp)) != 0)
        return rc;
    if (kind != SPMV_HIP_SYMMETRIC && kind != SPMV_HIP_SKEW_SYMMETRIC)
        return fail(SPMV_HIP_ERR_INVALID, "kind must be SPMV_HIP_SYMMETRIC or SPMV_HIP_SKEW_SYMMETRIC");
    if (max_windows < 0 || max_windows > spmv::kSymMaxWindows || window_doubles < 0)
        return fail(SPMV_HIP_ERR_INVALID, "max_windows must be 0 .. 8 and window_doubles >= 0");
    if (rp[rows] > 0 && !col)
        return fail(SPMV_HIP_ERR_INVALID, "column_index is null");
    int triangle = SPMV_HIP_TRIANGLE_DIAGONAL;
    long long diagonal = 0;
    if ((rc = classify(rows, rp, col, &triangle, &diagonal)) != 0)
        return rc;
    if (triangle == SPMV_HIP_TRIANGLE_MIXED)
        return fail(SPMV_HIP_ERR_INVALID, "the matrix has entries on both sides of the diagonal: not a stored triangle");
    if (kind == SPMV_HIP_SKEW_SYMMETRIC && diagonal > 0)
        return fail(SPMV_HIP_ERR_INVALID, "a skew-symmetric matrix has no diagonal entries");

    spmv_hip_sym_plan * pl = new (std::nothrow) spmv_hip_sym_plan;
    if (!pl)
        return fail(SPMV_HIP_ERR_ALLOC, "plan allocation failed");
    pl->rows = rows;
    pl->nnz = rp[rows];
    pl->kind = kind;
    pl->triangle = triangle;
    pl->diagonal = diagonal;
    pl->max_windows = max_windows > 0 ? max_windows : kSymAutoWindows;
    pl->stride = pl->max_windows - 1;
    pl->kw = pl->stride == 0 ? 0 : pl->stride == 1 ? 1 : pl->stride <= 3 ? 3 : 7;
    pl->R = std::max(1, std::min(kSymRows, window_doubles > 0 ? window_doubles : kSymRows));
    pl->ranges = rows > 0 ? (int) ((rows + (long long) pl->R - 1) / pl->R) : 0;
    // LDS: own rows + extra windows (doubles) + R + 1 ints of row_ptr
    const int budget_all = (int) ((kSymLdsBytes - 4 * ((size_t) pl->R + 1)) / 8) - pl->R;
    const int budget = window_doubles > 0 ? std::min(budget_all, pl->stride * window_doubles) : budget_all;
    const int cap = window_doubles > 0 ? window_doubles : budget;

    std::vector<RangeWindows> wins((size_t) pl->ranges);
    if (pl->stride > 0 && pl->nnz > 0) {
        const int threads = (int) std::max(1u, std::min({8u, std::thread::hardware_concurrency(), (unsigned) (pl->ranges / 16 + 1)}));
        auto work = [&](int t) {
            std::vector<std::pair<int, int>> buckets;
            for (int b = t; b < pl->ranges; b += threads) {
                const int r0 = b * pl->R;
                choose_windows(rows, rp, col, r0, std::min(pl->R, rows - r0), pl->stride, cap, budget, wins[(size_t) b], buckets);
            }
        };
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
        for (int t = (int) pool.size() + 1; t < threads; ++t) // helpers that could not be started
            for (int b = t; b < pl->ranges; b += threads) {
                std::vector<std::pair<int, int>> buckets;
                const int r0 = b * pl->R;
                choose_windows(rows, rp, col, r0, std::min(pl->R, rows - r0), pl->stride, cap, budget, wins[(size_t) b], buckets);
            }
    } else {
        // no extra windows: every off-diagonal entry outside its range's rows is spilled
        for (int b = 0; b < pl->ranges; ++b) {
            const int r0 = b * pl->R, nr = std::min(pl->R, rows - r0);
            long long s = 0;
            for (int32_t e = rp[r0]; e < rp[r0 + nr]; ++e)
                s += (unsigned) (col[e] - r0) >= (unsigned) nr;
            wins[(size_t) b].spilled = s;
        }
    }
    int most = 0;
    std::vector<int2> table((size_t) pl->ranges * (size_t) pl->stride, make_int2(0, 0));
    for (int b = 0; b < pl->ranges; ++b) {
        RangeWindows const & w = wins[(size_t) b];
        int extra = 0;
        for (int k = 0; k < w.n; ++k) {
            table[(size_t) b * pl->stride + k] = w.w[k];
            extra += w.w[k].y;
        }
        most = std::max(most, extra);
        pl->windows_used += 1 + w.n;
        pl->window_slots += std::min(pl->R, rows - b * pl->R) + extra;
        pl->spilled += w.spilled;
    }
    pl->slots = pl->R + most;
    pl->lds_bytes = 8 * (size_t) pl->slots + 4 * ((size_t) pl->R + 1);
    if (!table.empty()) {
        hipError_t e = hipMalloc((void **) &pl->d_win, table.size() * sizeof(int2));
        if (e == hipSuccess)
            e = hipMemcpy(pl->d_win, table.data(), table.size() * sizeof(int2), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            spmv_hip_sym_plan_destroy(pl);
            return fail_hip(e, "symmetric plan: window table");
        }
        pl->device_bytes = table.size() * sizeof(int2);
    }
    if (pl->lds_bytes > 64 * 1024) {
        hipError_t e = hipSuccess;
        const int bytes = (int) kSymLdsBytes;
        switch (pl->kw) {
        case 0: e = hipFuncSetAttribute((const void *) spmv::csr_symv_kernel<0>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes); break;
        case 1: e = hipFuncSetAttribute((const void *) spmv::csr_symv_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes); break;
        case 3: e = hipFuncSetAttribute((const void *) spmv::csr_symv_kernel<3>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes); break;
        default: e = hipFuncSetAttribute((const void *) spmv::csr_symv_kernel<7>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes); break;
        }
        if (e != hipSuccess) {
            spmv_hip_sym_plan_destroy(pl);
            return fail_hip(e, "symmetric plan: LDS size");
        }
    }
    *out = pl;
    return SPMV_HIP_OK;
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
    // the columns come back to the host once: the triangle is checked and the windows are chosen there
    std::vector<int32_t> col;
    try {
        col.resize((size_t) nnz);
    } catch (std::bad_alloc const &) {
        return fail(SPMV_HIP_ERR_ALLOC, "host copy of the columns");
    }
    if (nnz > 0) {
        hipStream_t s = static_cast<hipStream_t>(stream);
        HIP_TRY(hipMemcpyAsync(col.data(), d_column_index, (size_t) nnz * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return build_sym_plan(plan, rows, host_row_ptr, col.data(), kind, max_windows, window_doubles);
}

int spmv_hip_csr_symv(const spmv_hip_sym_plan * pl, const int32_t * d_row_ptr, const int32_t * d_column_index,
                      const double * d_value, const double * d_x, double * d_y, void * stream)
{
    if (!pl)
        return fail(SPMV_HIP_ERR_INVALID, "plan is null");
    if (pl->rows == 0 || pl->nnz == 0)
        return SPMV_HIP_OK;
    if (!d_row_ptr || !d_column_index || !d_value || !d_x || !d_y)
        return fail(SPMV_HIP_ERR_INVALID, "null device pointer");
    if ((const void *) d_x == (const void *) d_y)
        return fail(SPMV_HIP_ERR_INVALID, "d_x and d_y must be different arrays");
    if (!aligned16(d_column_index) || !aligned16(d_value))
        return fail(SPMV_HIP_ERR_ALIGN, "column / value arrays must be 16-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const double tsign = pl->kind == SPMV_HIP_SKEW_SYMMETRIC ? -1.0 : 1.0;
    const dim3 grid((unsigned) pl->ranges), block(spmv::kSymBlock);
    switch (pl->kw) {
    case 0:
        hipLaunchKernelGGL(spmv::csr_symv_kernel<0>, grid, block, pl->lds_bytes, s, pl->rows, pl->R, d_row_ptr, d_column_index, d_value,
                           d_x, d_y, pl->d_win, pl->stride, pl->slots, tsign);
        break;
    case 1:
        hipLaunchKernelGGL(spmv::csr_symv_kernel<1>, grid, block, pl->lds_bytes, s, pl->rows, pl->R, d_row_ptr, d_column_index, d_value,
                           d_x, d_y, pl->d_win, pl->stride, pl->slots, tsign);
        break;
    case 3:
        hipLaunchKernelGGL(spmv::csr_symv_kernel<3>, grid, block, pl->lds_bytes, s, pl->rows, pl->R, d_row_ptr, d_column_index, d_value,
                           d_x, d_y, pl->d_win, pl->stride, pl->slots, tsign);
        break;
    default:
        hipLaunchKernelGGL(spmv::csr_symv_kernel<7>, grid, block, pl->lds_bytes, s, pl->rows, pl->R, d_row_ptr, d_column_index, d_value,
                           d_x, d_y, pl->d_win, pl->stride, pl->slots, tsign);
        break;
    }
    HIP_TRY(hipGetLastError());
    return SPMV_HIP_OK;
}

int spmv_hip_sym_plan_info(const spmv_hip_sym_plan * pl, int64_t * out, int n)
{
    if (!pl || !out || n < 0)
        return fail(SPMV_HIP_ERR_INVALID, "plan/out null");
    const int64_t v[16] = {pl->ranges,
                           pl->R,
                           pl->max_windows,
                           pl->windows_used,
                           (int64_t) pl->lds_bytes,
                           pl->spilled,
                           8 * (pl->window_slots + pl->spilled),
                           pl->nnz,
                           pl->diagonal,
                           pl->triangle,
                           (int64_t) pl->device_bytes,
                           pl->kind,
                           pl->rows,
                           12LL * pl->nnz + 4LL * (pl->rows + 1) + 8LL * pl->rows,
                           pl->window_slots,
                           2LL * pl->nnz - pl->diagonal};
    for (int i = 0; i < n && i < 16; ++i)
        out[i] = v[i];
    return SPMV_HIP_OK;
}

void spmv_hip_sym_plan_destroy(spmv_hip_sym_plan * pl)
{
    if (!pl)
        return;
    if (pl->d_win)
        (void) hipFree(pl->d_win);
    delete pl;
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
    HIP_TRY(hipSetDevice(c->device));
    // the plan first: it refuses what is not a stored triangle (a column out of range, an entry in the other triangle, an unknown
    // kind) before anything is freed or copied, so that a refused upload leaves the previous matrix usable
    spmv_hip_sym_plan * plan = nullptr;
    if ((rc = build_sym_plan(&plan, rows, row_ptr, column_index, kind, 0, 0)) != 0)
        return rc;
    const hipError_t idle = hipStreamSynchronize(c->stream);
    if (idle != hipSuccess) {
        spmv_hip_sym_plan_destroy(plan);
        return fail_hip(idle, "hipStreamSynchronize");
    }
    free_ctx_matrix(c);
    c->sym_plan = plan;
    if ((rc = upload_ctx_csr(c, (size_t) rows + 1, (size_t) rows, (size_t) rows, (size_t) nnz, row_ptr, column_index, true, value, false)) != 0)
        return rc;
    c->rows = rows;
    c->cols = rows;
    c->nnz = nnz;
    c->bytes += c->sym_plan->device_bytes;
    c->format = 5;
    return SPMV_HIP_OK;
}

} // extern "C"
