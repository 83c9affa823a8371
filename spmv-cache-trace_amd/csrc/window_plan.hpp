// window_plan.hpp -- the host side that symmetric.hip and transpose.hip share: the rows cut into ranges, each range's LDS windows
// of y chosen from its columns (a greedy cover of the hit buckets of 32 doubles), the [ranges][stride] table of them on the
// device, and the choice of the kernel instantiation.  The kernels' side is window_walk.hpp.
//
// The two families differ in three parameters of the one cover (CoverRule and the budget their plans pass): whether a range's
// own rows are a window of their own, whether the exact cover is tried before the greedy one, and how much LDS is left for the
// windows.
#pragma once

#include "internal.hpp"
#include "window_walk.hpp"

#include <algorithm>
#include <new>
#include <thread>
#include <type_traits>
#include <utility>

namespace spmvi {

constexpr int kWinRows = 2048;             // rows per range (automatic)
constexpr int kWinAutoWindows = 4;         // symmetric: own rows + previous line + previous plane + one more; transposed: DESIGN
                                           // 3.10, the spilled share of the stand-ins stops falling there
constexpr size_t kWinLdsBytes = 80 * 1024; // per workgroup: two workgroups of 512 threads per CU (160 KB)
constexpr int kWinBucket = 32;             // window boundaries in steps of 32 doubles (256 B)

inline int check_windows_args(int max_windows, int window_doubles)
{
    if (max_windows < 0 || max_windows > spmv::kWinMaxWindows || window_doubles < 0)
        return fail(SPMV_HIP_ERR_INVALID, "max_windows must be 0 .. 8 and window_doubles >= 0");
    return SPMV_HIP_OK;
}

// what both plans hold
struct WindowPlan {
    int R = 0;              // rows per range
    int ranges = 0;
    int max_windows = 0;    // as the caller counts them (symmetric: own window included)
    int stride = 0;         // windows per range in the table
    int kw = 0;             // kernel instantiation: at least `stride` windows
    int slots = 0;          // LDS doubles per workgroup (the largest set of windows; symmetric: own rows included)
    size_t lds_bytes = 0;
    int2 * d_win = nullptr; // [ranges][stride] {first target, length}
    long long windows_used = 0, window_slots = 0, spilled = 0;
    size_t device_bytes = 0;
};

struct CoverRule {
    bool own_rows;    // the range's own rows [r0, r0 + nr) are a window already: targets there are neither counted nor covered
    bool exact_first; // try the cut at the nwin - 1 widest gaps before the greedy cover
};

struct RangeCover {
    int2 w[spmv::kWinMaxWindows];
    int n = 0;
    long long spilled = 0;
};

inline int2 bucket_window(int extent, int first_bucket, int last_bucket)
{
    const int first = first_bucket * kWinBucket;
    const int last = (int) std::min((long long) extent, (long long) (last_bucket + 1) * kWinBucket);
    return make_int2(first, last - first);
}

// The windows of the rows [r0, r0 + nr) over targets in [0, extent): the targets of their entries counted per bucket of 32
// doubles, then greedily the span of at most `cap` doubles (and what is left of `budget`) that covers the most entries, its
// buckets taken out, and again -- up to `nwin` windows, which therefore never overlap.  What no window covers is spilled
// (nwin = 0: every counted entry).
inline void cover_range(CoverRule rule, int extent, const int32_t * rp, const int32_t * col, int r0, int nr, int nwin, int cap, int budget,
                        RangeCover & out, std::vector<std::pair<int, int>> & buckets)
{
    buckets.clear();
    long long entries = 0;
    for (int32_t e = rp[r0]; e < rp[r0 + nr]; ++e) {
        const int j = col[e];
        if (rule.own_rows && (unsigned) (j - r0) < (unsigned) nr)
            continue; // own rows (the diagonal included)
        ++entries;
        const int b = j / kWinBucket;
        if (!buckets.empty() && buckets.back().first == b)
            ++buckets.back().second;
        else
            buckets.emplace_back(b, 1);
    }
    out.n = 0;
    out.spilled = entries;
    if (nwin < 1 || buckets.empty())
        return;
    std::sort(buckets.begin(), buckets.end());
    size_t m = 0; // merge equal buckets
    for (size_t k = 0; k < buckets.size(); ++k) {
        if (m > 0 && buckets[m - 1].first == buckets[k].first)
            buckets[m - 1].second += buckets[k].second;
        else
            buckets[m++] = buckets[k];
    }
    buckets.resize(m);
    // The exact cover: the hit buckets cut at their nwin - 1 widest gaps.  Where those runs fit the budget they are the
    // windows -- nothing spilled and no slot spent on a gap (the three lines a range of a 5-point stencil hits, each one
    // window), which a greedy first window as wide as the whole budget would not find.
    if (rule.exact_first) {
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
            const int width = (buckets[cut[k + 1] - 1].first + 1 - buckets[cut[k]].first) * kWinBucket;
            fits &= width <= cap;
            total += width;
        }
        if (fits && total <= budget) {
            for (size_t k = 0; k + 1 < cut.size(); ++k)
                out.w[out.n++] = bucket_window(extent, buckets[cut[k]].first, buckets[cut[k + 1] - 1].first);
            out.spilled = 0;
            return;
        }
    }
    while (out.n < nwin && !buckets.empty()) {
        const int span = std::min(cap, budget) / kWinBucket; // buckets per window
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
        const int2 w = bucket_window(extent, buckets[best_lo].first, buckets[best_hi].first);
        out.w[out.n++] = w;
        budget -= w.y; // the width after clipping at `extent`
        out.spilled -= best;
        buckets.erase(buckets.begin() + (long) best_lo, buckets.begin() + (long) best_hi + 1);
    }
}

// f(t) for every t in [0, threads): t = 0 on this thread, the others on helper threads of their own; the share of a helper that
// could not be started is done here after the others.  (Thread is a parameter so that a test can make the start fail.)
template <class Thread = std::thread, class F>
void on_threads(int threads, F && f)
{
    std::vector<char> done((size_t) threads, 0);
    auto work = [&](int t) {
        f(t);
        done[(size_t) t] = 1;
    };
    std::vector<Thread> pool;
    try {
        for (int t = 1; t < threads; ++t)
            pool.emplace_back(work, t);
    } catch (...) {
        // fewer helpers
    }
    work(0);
    for (auto & th : pool)
        th.join();
    for (int t = 1; t < threads; ++t)
        if (!done[(size_t) t])
            work(t);
}

inline int range_threads(int ranges)
{
    return (int) std::max(1u, std::min({8u, std::thread::hardware_concurrency(), (unsigned) (ranges / 16 + 1)}));
}

// The windows of every range of pl (R, ranges, stride set; the windows at most `cap` wide and `budget` doubles per range in
// all) into the table, with the accounting: windows_used, window_slots, spilled, slots, device_bytes.  rule.own_rows counts
// each range's own rows as one more window in front of the table's.
inline void plan_windows(WindowPlan & pl, std::vector<int2> & table, CoverRule rule, int32_t rows, int extent, const int32_t * rp,
                         const int32_t * col, int cap, int budget)
{
    std::vector<RangeCover> covers((size_t) pl.ranges);
    const int threads = range_threads(pl.ranges);
    on_threads(threads, [&](int t) {
        std::vector<std::pair<int, int>> buckets;
        for (int b = t; b < pl.ranges; b += threads) {
            const int r0 = b * pl.R;
            cover_range(rule, extent, rp, col, r0, std::min(pl.R, rows - r0), pl.stride, cap, budget, covers[(size_t) b], buckets);
        }
    });
    int most = 0;
    table.assign((size_t) pl.ranges * (size_t) pl.stride, make_int2(0, 0));
    for (int b = 0; b < pl.ranges; ++b) {
        RangeCover const & c = covers[(size_t) b];
        int sum = 0;
        for (int k = 0; k < c.n; ++k) {
            table[(size_t) b * pl.stride + k] = c.w[k];
            sum += c.w[k].y;
        }
        most = std::max(most, sum);
        pl.windows_used += c.n + (rule.own_rows ? 1 : 0);
        pl.window_slots += sum + (rule.own_rows ? std::min(pl.R, rows - b * pl.R) : 0);
        pl.spilled += c.spilled;
    }
    pl.slots = most + (rule.own_rows ? pl.R : 0);
    pl.device_bytes = table.size() * sizeof(int2);
}

// f(std::integral_constant<int, K>) for the K among A, B, C, D that is kw (D where it is none of them): the one place a plan's
// kw becomes a kernel instantiation, for the LDS limit and for the launch alike
template <int A, int B, int C, int D, class F>
auto with_kw(int kw, F && f)
{
    return kw == A ? f(std::integral_constant<int, A>{})
        : kw == B  ? f(std::integral_constant<int, B>{})
        : kw == C  ? f(std::integral_constant<int, C>{})
                   : f(std::integral_constant<int, D>{});
}

template <class Kernel>
hipError_t allow_window_lds(Kernel kernel)
{
    return hipFuncSetAttribute((const void *) kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) kWinLdsBytes);
}

// what a preview and a plan share: every number of plan_info and the window table.  Plan has a WindowPlan member `win`.
template <class Plan>
struct HostPlan {
    Plan numbers;
    std::vector<int2> table;
};

template <class Plan>
void free_plan(Plan * pl)
{
    if (!pl)
        return;
    if (pl->win.d_win)
        (void) hipFree(pl->win.d_win);
    delete pl;
}

// the host plan onto the current device: the window table, and the kernel's LDS limit (allow_lds(kw)) where it is above the
// default 64 KB.  `family` starts the error texts.
template <class Plan, class AllowLds>
int build_plan(Plan ** out, HostPlan<Plan> const & hp, const std::string & family, AllowLds allow_lds)
{
    Plan * pl = new (std::nothrow) Plan(hp.numbers);
    if (!pl)
        return fail(SPMV_HIP_ERR_ALLOC, "plan allocation failed");
    std::string what = family + " plan: window table";
    hipError_t e = hipSuccess;
    if (!hp.table.empty()) {
        e = hipMalloc((void **) &pl->win.d_win, hp.table.size() * sizeof(int2));
        if (e == hipSuccess)
            e = hipMemcpy(pl->win.d_win, hp.table.data(), hp.table.size() * sizeof(int2), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess && pl->win.lds_bytes > 64 * 1024) {
        what = family + " plan: LDS size";
        e = allow_lds(pl->win.kw);
    }
    if (e != hipSuccess) {
        free_plan(pl);
        return fail_hip(e, what.c_str());
    }
    *out = pl;
    return SPMV_HIP_OK;
}

// the columns come back to the host once: they are checked and the windows are chosen there.  May throw std::bad_alloc.
inline int read_back_columns(std::vector<int32_t> & col, int32_t nnz, const int32_t * d_column_index, void * stream)
{
    col.resize((size_t) nnz);
    if (nnz > 0) {
        hipStream_t s = static_cast<hipStream_t>(stream);
        HIP_TRY(hipMemcpyAsync(col.data(), d_column_index, (size_t) nnz * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return SPMV_HIP_OK;
}

// the arrays of a multiply, in the order both families refuse them
inline int check_multiply_arrays(const int32_t * d_row_ptr, const int32_t * d_column_index, const double * d_value, const double * d_x,
                                 const double * d_y)
{
    if (!d_row_ptr || !d_column_index || !d_value || !d_x || !d_y)
        return fail(SPMV_HIP_ERR_INVALID, "null device pointer");
    if ((const void *) d_x == (const void *) d_y)
        return fail(SPMV_HIP_ERR_INVALID, "d_x and d_y must be different arrays");
    if (!aligned16(d_column_index) || !aligned16(d_value))
        return fail(SPMV_HIP_ERR_ALIGN, "column / value arrays must be 16-byte aligned");
    return SPMV_HIP_OK;
}

} // namespace spmvi
