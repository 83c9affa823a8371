// compact.hip -- include/spmv_hip_compact.h: y += fl32(A) x, y += A x on the caller's fp64 values through the same plan
// (include/spmv_hip_compact_f64.h) and y <- fl32(y + fl32(A) x) on float x and y (include/spmv_hip_compact_f32xy.h), with the columns of a tile as 16-bit codes (a 3-bit window number and a 13-bit offset from one of
// eight per-tile bases).  The tiles are f32values.hip's own (f32_plan.hpp): its descriptors as they
// are, with the compact bits and the tile's first code quad added; the bases and the codes are made on the host by a few
// threads, tile by tile -- or, for arrays that are on the device already (include/spmv_hip_compact_device.h), by the two kernels
// of c16_plan_kernels.hpp; the kernel is csr_compact.hpp.  The multiplies' refusals and launches are tile_front.hpp's: this file
// describes its three families to it (C16Family).  Level 1 of formats 7 to 10 is here too, once for both plans: the upload
// (upload_float_tile) and the multiply of a context on its own arrays (ctx_tile_multiply).
#include "tile_front.hpp"
#include "csr_compact.hpp"
#include "c16_plan_kernels.hpp"
#include "spmv_hip_compact_device.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <atomic>
#include <new>
#include <system_error>
#include <thread>
#include <type_traits>
#include <utility>

using namespace spmvi;

struct spmv_hip_c16_plan {
    int32_t rows = 0, cols = 0, nnz = 0;
    unsigned flags = 0;
    int ntiles = 0, compact_tiles = 0, wide_tiles = 0, long_tiles = 0;
    long long compact_entries = 0, streamed_bytes = 0;
    long long windows_hist[SPMV_HIP_C16_WINDOWS] = {0};
    size_t device_bytes = 0;
    // one allocation: descriptors (ntiles + 1), bases (8 per tile), codes
    char * d_all = nullptr;
    const int4 * d_desc = nullptr;
    const int * d_bases = nullptr;
    const uint16_t * d_codes = nullptr;
};

namespace {

struct HostPlan {
    spmv_hip_c16_plan numbers;
    std::vector<int4> desc;
    std::vector<int32_t> bases;    // 8 per tile
    std::vector<int32_t> windows;  // per tile, 0 = wide
    std::vector<uint16_t> by_entry; // nnz codes by entry index (0 in wide tiles)
    std::vector<uint16_t> codes;   // the device layout: a compact tile's codes from a quad of its own
};

// window bases and codes of the entries [k0, k1); returns the windows needed (more than 8: nothing is written)
int code_tile(const int32_t * col, int32_t k0, int32_t k1, int32_t * base, uint16_t * code, std::vector<int32_t> & sorted)
{
    if (k1 == k0) {
        std::fill(base, base + SPMV_HIP_C16_WINDOWS, 0);
        return 1;
    }
    sorted.assign(col + k0, col + k1);
    if (!std::is_sorted(sorted.begin(), sorted.end()))
        std::sort(sorted.begin(), sorted.end());
    int32_t b[SPMV_HIP_C16_WINDOWS];
    int nw = 1;
    b[0] = sorted[0];
    for (int32_t c : sorted)
        if ((long long) c >= (long long) b[nw - 1] + SPMV_HIP_C16_WINDOW_SPAN) {
            if (nw == SPMV_HIP_C16_WINDOWS)
                return nw + 1;
            b[nw++] = c;
        }
    for (int w = 0; w < SPMV_HIP_C16_WINDOWS; ++w)
        base[w] = b[w < nw ? w : nw - 1];
    for (int32_t k = k0; k < k1; ++k) {
        int w = nw - 1;
        while (col[k] < b[w])
            --w;
        code[k] = (uint16_t) ((w << spmv::kC16OffsetBits) | (col[k] - b[w]));
    }
    return nw;
}

// What the host planner and the device planner share once every tile's windows (0 = wide) are known: the compact bits and the
// first code quad into the descriptors, the counts, the plan's bytes; quads: the length of the code stream.
int finish_descriptors(spmv_hip_c16_plan & pl, std::vector<int4> & desc, const int32_t * windows, long long f32_streamed_bytes, long long & quads)
{
    const int nt = pl.ntiles;
    quads = 0;
    for (int w = 0; w < nt; ++w) {
        int4 & d = desc[(size_t) w];
        const int32_t k0 = d.y, k1 = desc[(size_t) w + 1].y, kb = k0 & ~3;
        const int nw = windows[(size_t) w];
        if (nw == 0) {
            ++pl.wide_tiles;
            continue;
        }
        if (quads > 0xFFFFFFFFLL)
            return fail(SPMV_HIP_ERR_OVERFLOW, "the code stream is too long for a 32-bit quad index");
        d.z |= spmv::kC16MetaCompact | (nw == 1 ? spmv::kC16MetaOneWindow : 0);
        d.w = (int) (unsigned) quads;
        if (k1 > k0)
            quads += ((k1 - 1 - kb) >> 2) + 1;
        ++pl.compact_tiles;
        pl.compact_entries += k1 - k0;
        ++pl.windows_hist[nw - 1];
    }
    pl.device_bytes = (16 * ((size_t) nt + 1) + 32 * (size_t) nt + 8 * (size_t) quads + 15) & ~(size_t) 15;
    // the fp32-value plan's bytes with 2 instead of 4 bytes of column per compact entry, and the bases
    pl.streamed_bytes = f32_streamed_bytes - 2LL * pl.compact_entries + 32LL * nt;
    return SPMV_HIP_OK;
}

int plan_host(HostPlan & hp, int32_t rows, int32_t cols, const int32_t * p, const int32_t * col, unsigned flags)
{
    spmv_hip_c16_plan & pl = hp.numbers;
    int rc = f32_check_host(rows, cols, p, flags);
    if (rc != 0)
        return rc;
    F32HostPlan fp;
    f32_plan_host(fp, rows, cols, p, flags);
    const int32_t nnz = p[rows];
    pl.rows = rows;
    pl.cols = cols;
    pl.nnz = nnz;
    pl.flags = flags;
    if (nnz > 0 && !col)
        return fail(SPMV_HIP_ERR_INVALID, "host_column_index is null");
    if ((rc = check_columns(nnz, col, cols)) != 0)
        return rc;
    const int nt = fp.numbers.ntiles;
    if (nt == 0)
        return SPMV_HIP_OK; // the multiply does nothing
    pl.ntiles = nt;
    pl.long_tiles = fp.numbers.long_tiles;
    hp.desc = std::move(fp.desc); // nt + 1 records: tile w ends where tile w + 1 starts
    hp.bases.assign(8 * (size_t) nt, 0);
    hp.windows.assign((size_t) nt, 0);
    hp.by_entry.assign((size_t) nnz, 0);
    // the bases and the codes, tile by tile, on a few host threads
    const int threads = (int) std::max(1u, std::min({8u, std::thread::hardware_concurrency(), (unsigned) (nt / 4096 + 1)}));
    std::atomic<bool> out_of_memory{false};
    auto work = [&](int t) { // (nothing may be thrown out of a thread: a worker's bad_alloc is reported below)
        try {
            std::vector<int32_t> sorted;
            for (int w = (int) ((long long) nt * t / threads), w1 = (int) ((long long) nt * (t + 1) / threads); w < w1; ++w) {
                const int nw = code_tile(col, hp.desc[(size_t) w].y, hp.desc[(size_t) w + 1].y, &hp.bases[8 * (size_t) w], hp.by_entry.data(), sorted);
                hp.windows[(size_t) w] = nw <= SPMV_HIP_C16_WINDOWS ? nw : 0;
            }
        } catch (std::bad_alloc const &) {
            out_of_memory = true;
        }
    };
    {
        std::vector<std::thread> pool;
        int t = 1;
        try {
            pool.reserve((size_t) threads);
            for (; t < threads; ++t)
                pool.emplace_back(work, t);
        } catch (std::system_error const &) { // no more threads to be had: this thread does the parts that were not started
        } catch (std::bad_alloc const &) {
            out_of_memory = true;
        }
        work(0);
        for (; t < threads; ++t)
            work(t);
        for (auto & th : pool)
            th.join();
    }
    if (out_of_memory)
        return fail(SPMV_HIP_ERR_ALLOC, "compact plan: host memory");
    // the compact bits and the first code quad into the descriptors, and the device layout of the codes
    long long quads = 0;
    if ((rc = finish_descriptors(pl, hp.desc, hp.windows.data(), fp.numbers.streamed_bytes, quads)) != 0)
        return rc;
    hp.codes.assign(4 * (size_t) quads, 0);
    for (int w = 0; w < nt; ++w)
        if (hp.windows[(size_t) w] > 0) {
            const int32_t k0 = hp.desc[(size_t) w].y, k1 = hp.desc[(size_t) w + 1].y;
            if (k1 > k0)
                std::memcpy(&hp.codes[4 * (size_t) (unsigned) hp.desc[(size_t) w].w + (size_t) (k0 & 3)], &hp.by_entry[(size_t) k0],
                            (size_t) (k1 - k0) * sizeof(uint16_t));
        }
    return SPMV_HIP_OK;
}

int plan_host_guarded(HostPlan & hp, int32_t rows, int32_t cols, const int32_t * p, const int32_t * col, unsigned flags)
{
    try {
        return plan_host(hp, rows, cols, p, col, flags);
    } catch (std::bad_alloc const &) {
        return fail(SPMV_HIP_ERR_ALLOC, "compact plan: host memory");
    }
}

void plan_numbers(const spmv_hip_c16_plan & pl, int64_t * out, int n)
{
    int64_t v[SPMV_HIP_C16_INFO] = {pl.rows, pl.cols, pl.nnz, pl.flags, (pl.ntiles + 3) / 4, pl.ntiles, pl.compact_tiles, pl.wide_tiles,
                                    pl.long_tiles, pl.compact_entries};
    for (int w = 0; w < SPMV_HIP_C16_WINDOWS; ++w)
        v[10 + w] = pl.windows_hist[w];
    v[18] = (int64_t) pl.device_bytes;
    v[19] = pl.streamed_bytes;
    for (int i = 0; i < n && i < SPMV_HIP_C16_INFO; ++i)
        out[i] = v[i];
}

// the host plan onto the current device
int build_plan(spmv_hip_c16_plan ** out, HostPlan const & hp, hipStream_t s)
{
    spmv_hip_c16_plan * pl = new (std::nothrow) spmv_hip_c16_plan(hp.numbers);
    if (!pl)
        return fail(SPMV_HIP_ERR_ALLOC, "plan allocation failed");
    if (pl->ntiles > 0) {
        const size_t desc_bytes = hp.desc.size() * sizeof(int4), base_bytes = hp.bases.size() * sizeof(int32_t),
                     code_bytes = hp.codes.size() * sizeof(uint16_t);
        hipError_t e = hipMalloc((void **) &pl->d_all, pl->device_bytes);
        if (e == hipSuccess)
            e = hipMemcpyAsync(pl->d_all, hp.desc.data(), desc_bytes, hipMemcpyHostToDevice, s);
        if (e == hipSuccess)
            e = hipMemcpyAsync(pl->d_all + desc_bytes, hp.bases.data(), base_bytes, hipMemcpyHostToDevice, s);
        if (e == hipSuccess && code_bytes > 0)
            e = hipMemcpyAsync(pl->d_all + desc_bytes + base_bytes, hp.codes.data(), code_bytes, hipMemcpyHostToDevice, s);
        if (e == hipSuccess)
            e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            spmv_hip_c16_plan_destroy(pl);
            return fail_hip(e, "compact plan: descriptors, bases and codes");
        }
        pl->d_desc = reinterpret_cast<const int4 *>(pl->d_all);
        pl->d_bases = reinterpret_cast<const int *>(pl->d_all + desc_bytes);
        pl->d_codes = reinterpret_cast<const uint16_t *>(pl->d_all + desc_bytes + base_bytes);
    }
    *out = pl;
    return SPMV_HIP_OK;
}

// ---- the plan from device arrays (include/spmv_hip_compact_device.h): row_ptr to the host for f32_plan_host's tiles, the columns
// to c16_plan_kernels.hpp's two kernels where they are ------------------------------------------------------------------------------

// a device allocation of one call, freed where the call returns
struct DeviceTemp {
    char * p = nullptr;
    ~DeviceTemp()
    {
        if (p)
            (void) hipFree(p);
    }
};

// Wall-clock seconds of the stages of the last spmv_hip_c16_plan_csr_device, for tools/agg_ab.py: {row_ptr copy, tile cut, windows
// kernel, codes kernel, the rest}.  Only libspmv_hip_experiments.so keeps them, and it waits for the stream between the stages
// to do so; in the product library this is nothing.
struct StageClock {
#ifdef SPMV_HIP_EXPERIMENTS
    static double seconds[5];
    hipStream_t s;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    explicit StageClock(hipStream_t stream) : s(stream) { std::fill(seconds, seconds + 5, 0.0); }
    void done(int stage)
    {
        (void) hipStreamSynchronize(s);
        const auto t1 = std::chrono::steady_clock::now();
        seconds[stage] += std::chrono::duration<double>(t1 - t0).count();
        t0 = t1;
    }
#else
    explicit StageClock(hipStream_t) {}
    void done(int) {}
#endif
};
#ifdef SPMV_HIP_EXPERIMENTS
double StageClock::seconds[5] = {0.0};
#endif

int out_of_range(long long count)
{
    char text[160];
    std::snprintf(text, sizeof text, "%lld column index(es) out of range [0, cols)", count);
    return fail(SPMV_HIP_ERR_INVALID, text);
}

// spmv_hip_c16_plan_csr_device behind the refusals that need no device; throws std::bad_alloc
int plan_device(spmv_hip_c16_plan ** out, int32_t rows, int32_t cols, const int32_t * d_row_ptr, const int32_t * d_col, unsigned flags,
                hipStream_t s)
{
    StageClock clock(s);
    std::vector<int32_t> p((size_t) rows + 1);
    HIP_TRY(hipMemcpyAsync(p.data(), d_row_ptr, p.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    clock.done(0);
    int rc = f32_check_host(rows, cols, p.data(), flags);
    if (rc != 0)
        return rc;
    const int32_t nnz = p[(size_t) rows];
    if (nnz > 0 && !d_col)
        return fail(SPMV_HIP_ERR_INVALID, "d_column_index is null");
    if (nnz > 0 && cols == 0)
        return out_of_range(nnz); // no column lies in [0, 0)
    F32HostPlan fp;
    f32_plan_host(fp, rows, cols, p.data(), flags);
    clock.done(1);
    spmv_hip_c16_plan numbers;
    numbers.rows = rows;
    numbers.cols = cols;
    numbers.nnz = nnz;
    numbers.flags = flags;
    const int nt = numbers.ntiles = fp.numbers.ntiles;
    numbers.long_tiles = fp.numbers.long_tiles;
    long long quads = 0;
    DeviceTemp temp;
    const size_t desc_bytes = ((size_t) nt + 1) * sizeof(int4), base_bytes = 8 * (size_t) nt * sizeof(int32_t);
    if (nt > 0) {
        // the descriptors as cut, room for the bases, the count of columns out of range, a window count per tile
        std::vector<int32_t> windows((size_t) nt);
        unsigned long long bad = 0;
        HIP_TRY(hipMalloc((void **) &temp.p, desc_bytes + base_bytes + 16 + (size_t) nt * sizeof(int32_t)));
        unsigned long long * d_bad = reinterpret_cast<unsigned long long *>(temp.p + desc_bytes + base_bytes);
        int * d_windows = reinterpret_cast<int *>(temp.p + desc_bytes + base_bytes + 16);
        HIP_TRY(hipMemcpyAsync(temp.p, fp.desc.data(), desc_bytes, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(d_bad, 0, sizeof bad, s));
        clock.done(4);
        hipLaunchKernelGGL(spmv::c16_windows_kernel, dim3((unsigned) ((nt + 3) / 4)), dim3(256), 0, s, nt, reinterpret_cast<const int4 *>(temp.p),
                           d_col, (int) cols, reinterpret_cast<int *>(temp.p + desc_bytes), d_windows, d_bad);
        HIP_TRY(hipGetLastError());
        clock.done(2);
        HIP_TRY(hipMemcpyAsync(windows.data(), d_windows, (size_t) nt * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (bad > 0)
            return out_of_range((long long) bad);
        if ((rc = finish_descriptors(numbers, fp.desc, windows.data(), fp.numbers.streamed_bytes, quads)) != 0)
            return rc;
    }
    spmv_hip_c16_plan * pl = new (std::nothrow) spmv_hip_c16_plan(numbers);
    if (!pl)
        return fail(SPMV_HIP_ERR_ALLOC, "plan allocation failed");
    if (nt > 0) {
        // the plan's block: the finished descriptors from the host, the bases from the temporary, the codes by the second kernel
        hipError_t e = hipMalloc((void **) &pl->d_all, pl->device_bytes);
        if (e == hipSuccess)
            e = hipMemcpyAsync(pl->d_all, fp.desc.data(), desc_bytes, hipMemcpyHostToDevice, s);
        if (e == hipSuccess)
            e = hipMemcpyAsync(pl->d_all + desc_bytes, temp.p + desc_bytes, base_bytes, hipMemcpyDeviceToDevice, s);
        clock.done(4);
        if (e == hipSuccess && quads > 0) {
            hipLaunchKernelGGL(spmv::c16_codes_kernel, dim3((unsigned) ((nt + 3) / 4)), dim3(256), 0, s, nt, reinterpret_cast<const int4 *>(pl->d_all),
                               reinterpret_cast<const int *>(pl->d_all + desc_bytes), d_col,
                               reinterpret_cast<uint16_t *>(pl->d_all + desc_bytes + base_bytes));
            e = hipGetLastError();
        }
        if (e == hipSuccess)
            e = hipStreamSynchronize(s);
        clock.done(3);
        if (e != hipSuccess) {
            spmv_hip_c16_plan_destroy(pl);
            return fail_hip(e, "compact plan from device arrays");
        }
        pl->d_desc = reinterpret_cast<const int4 *>(pl->d_all);
        pl->d_bases = reinterpret_cast<const int *>(pl->d_all + desc_bytes);
        pl->d_codes = reinterpret_cast<const uint16_t *>(pl->d_all + desc_bytes + base_bytes);
    }
    *out = pl;
    return SPMV_HIP_OK;
}

// spmv_hip_csr_spmv_c16 (V = float, T = double), spmv_hip_csr_spmv_c16_f64 (V = double) and spmv_hip_csr_spmv_c16_f32xy (V = T =
// float), three families over one plan, which knows neither the value type nor the vectors' element type.  csr_compact.hpp's
// kernels take the descriptors, the bases and the codes in front of the arrays; the 32-bit columns are read by wide tiles alone.
template <class V, class T>
struct C16Family {
    const spmv_hip_c16_plan * pl;
    static const char * null_columns() { return "d_column_index is null and the plan has wide tiles, which read the 32-bit columns"; }
    bool columns_read() const { return pl->wide_tiles > 0; }
    // this family's among the three kernels of a launch shape
    template <class A, class B, class D>
    static auto mine(A f32xy, B c16, D c16_f64)
    {
        if constexpr (std::is_same<T, float>::value)
            return f32xy;
        else if constexpr (std::is_same<V, float>::value)
            return c16;
        else
            return c16_f64;
    }
    static auto plain(bool x32)
    {
        return with_bools([](auto X) { return mine(spmv::csr_compact_f32xy_kernel<X()>, spmv::csr_compact_kernel<X()>, spmv::csr_compact_f64_kernel<X()>); }, x32);
    }
    static auto scaled(bool x32, bool beta0)
    {
        return with_bools([](auto X, auto B0) { return mine(spmv::csr_compact_f32xy_scaled_kernel<X(), B0()>, spmv::csr_compact_scaled_kernel<X(), B0()>,
                                                            spmv::csr_compact_f64_scaled_kernel<X(), B0()>); }, x32, beta0);
    }
    static auto dots(bool beta0, bool hasw)
    {
        return with_bools([](auto B0, auto W) { return mine(spmv::csr_compact_f32xy_scaled_dots_kernel<B0(), W()>, spmv::csr_compact_scaled_dots_kernel<B0(), W()>,
                                                            spmv::csr_compact_f64_scaled_dots_kernel<B0(), W()>); }, beta0, hasw);
    }
    template <class K, class... A>
    void launch(K kernel, dim3 grid, hipStream_t s, A... a) const
    {
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, pl->ntiles, pl->d_desc, pl->d_bases, pl->d_codes, a...);
    }
};

template <class V, class T>
int c16_multiply(const spmv_hip_c16_plan * pl, const int32_t * d_row_ptr, const int32_t * d_column_index, const V * d_value,
                 const T * d_x, T * d_y, void * stream, const ScaledArgs<T> * scale = nullptr, const DotsArgs * dots = nullptr)
{
    return tile_multiply(C16Family<V, T>{pl}, d_row_ptr, d_column_index, d_value, d_x, d_y, stream, scale, dots);
}

// ctx_tile_multiply once the format has chosen the plan, the value array and the vector pair: in place on y, w = x where A is square
template <class Plan, class V, class T>
int ctx_multiply(const spmv_hip_ctx * c, const Plan * pl, const V * value, const T * x, T * y, const double * ab, bool with_dots)
{
    const ScaledArgs<T> scale{ab ? ab[0] : 0.0, ab ? ab[1] : 0.0, y}, *sp = ab ? &scale : nullptr;
    const DotsArgs dots{c->rows == c->cols ? x : nullptr, c->d_dots, with_dots ? c->d_dots + 2 : nullptr, c->dots_work_bytes},
        *dp = with_dots ? &dots : nullptr;
    if constexpr (std::is_same<Plan, spmv_hip_f32_plan>::value)
        return f32_multiply(pl, c->d_ptr, c->d_col, value, x, y, c->stream, sp, dp);
    else
        return c16_multiply(pl, c->d_ptr, c->d_col, value, x, y, c->stream, sp, dp);
}

} // namespace

namespace spmvi {

int ctx_tile_multiply(spmv_hip_ctx * c, const double * scale, bool with_dots)
{
    switch (c->format) {
    case 7: return ctx_multiply(c, c->f32_plan, c->d_val32, c->d_x, c->d_y, scale, with_dots);
    case 8: return ctx_multiply(c, c->c16_plan, c->d_val32, c->d_x, c->d_y, scale, with_dots);
    case 9: return ctx_multiply(c, c->c16_plan, c->d_val, c->d_x, c->d_y, scale, with_dots);
    case 10: return ctx_multiply(c, c->c16_plan, c->d_val32, c->d_x32, c->d_y32, scale, with_dots);
    }
    return fail(SPMV_HIP_ERR_STATE, "the context holds none of the formats 7 to 10");
}

int upload_float_tile(spmv_hip_ctx * c, int format, const char * multi, int32_t rows, int32_t cols, int32_t nnz, const int32_t * row_ptr,
                      const int32_t * column_index, const double * value, bool narrow_values, int allow_rounding, bool float_vectors)
{
    int rc = upload_csr_prelude(c, multi, nullptr, rows, cols, nnz, row_ptr, column_index, value);
    if (rc != 0)
        return rc;
    const unsigned flags = c->flags & SPMV_HIP_FLAG_EXACT_ORDER;
    // everything that can refuse the matrix happens before anything is freed or copied
    if ((rc = f32_check_host(rows, cols, row_ptr, flags)) != 0)
        return rc;
    if (row_ptr[rows] != nnz)
        return fail(SPMV_HIP_ERR_INVALID, "row_ptr[rows] must equal nnz");
    const bool f32 = format == 7;
    F32HostPlan fp;
    HostPlan hp;
    if ((rc = f32 ? check_columns(nnz, column_index, cols) : plan_host_guarded(hp, rows, cols, row_ptr, column_index, flags)) != 0)
        return rc; // (the columns: the compact plan looks at them itself)
    std::vector<float> narrow;
    if (narrow_values) {
        try {
            narrow.resize((size_t) nnz);
        } catch (std::bad_alloc const &) {
            return fail(SPMV_HIP_ERR_ALLOC, f32 ? "fp32-value upload: host memory" : "compact upload: host memory");
        }
        if ((rc = narrow_refusal(narrow_host(nnz, value, narrow.data()), allow_rounding)) != 0)
            return rc;
    }
    if (f32 && (rc = f32_plan_host_guarded(fp, rows, cols, row_ptr, flags, "fp32-value upload: host memory")) != 0)
        return rc;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    free_ctx_matrix(c);
    if ((rc = f32 ? f32_build_plan(&c->f32_plan, fp, c->stream) : build_plan(&c->c16_plan, hp, c->stream)) != 0)
        return rc;
    // the values narrowed (d_val32) or as they are (d_val); of the compact plans only wide tiles read 32-bit columns
    if ((rc = upload_ctx_csr(c, (size_t) rows + 1, (size_t) cols, (size_t) rows, (size_t) nnz, row_ptr, column_index,
                             f32 || c->c16_plan->wide_tiles > 0, narrow_values ? (const void *) narrow.data() : value, narrow_values,
                             float_vectors)) != 0)
        return rc;
    c->rows = rows;
    c->cols = cols;
    c->nnz = nnz;
    c->bytes += f32 ? c->f32_plan->device_bytes : c->c16_plan->device_bytes;
    c->format = format;
    return SPMV_HIP_OK;
}

} // namespace spmvi

extern "C" {

int spmv_hip_c16_plan_preview(int32_t rows, int32_t cols, const int32_t * host_row_ptr, const int32_t * host_column_index, unsigned flags,
                              int64_t * out, int n, int32_t * tile_table, int64_t tile_table_ints, uint16_t * codes)
{
    if (!out || n < 0 || tile_table_ints < 0)
        return fail(SPMV_HIP_ERR_INVALID, "out is null, or a negative count");
    HostPlan hp;
    int rc = plan_host_guarded(hp, rows, cols, host_row_ptr, host_column_index, flags);
    if (rc != 0)
        return rc;
    const int nt = hp.numbers.ntiles;
    if (tile_table) {
        if ((long long) SPMV_HIP_C16_TILE_INTS * nt > tile_table_ints)
            return fail(SPMV_HIP_ERR_INVALID, "tile_table is too small: it takes 13 int32 values per tile");
        for (int w = 0; w < nt; ++w) {
            int32_t * t = tile_table + (size_t) SPMV_HIP_C16_TILE_INTS * w;
            tile_table_row(t, &hp.desc[(size_t) w]);
            t[4] = hp.windows[(size_t) w];
            for (int b = 0; b < 8; ++b)
                t[5 + b] = t[4] ? hp.bases[8 * (size_t) w + b] : 0;
        }
    }
    if (codes && hp.numbers.nnz > 0) {
        if (hp.by_entry.empty())
            std::memset(codes, 0, (size_t) hp.numbers.nnz * sizeof(uint16_t)); // (rows or cols of zero cannot have entries: not reached)
        else
            std::memcpy(codes, hp.by_entry.data(), hp.by_entry.size() * sizeof(uint16_t));
    }
    plan_numbers(hp.numbers, out, n);
    return SPMV_HIP_OK;
}

int spmv_hip_c16_plan_csr(spmv_hip_c16_plan ** plan, int32_t rows, int32_t cols, const int32_t * host_row_ptr,
                          const int32_t * host_column_index, unsigned flags, void * stream)
{
    if (!plan)
        return fail(SPMV_HIP_ERR_INVALID, "plan is null");
    *plan = nullptr;
    HostPlan hp;
    int rc = plan_host_guarded(hp, rows, cols, host_row_ptr, host_column_index, flags);
    if (rc != 0)
        return rc;
    int devices = 0;
    if (hipGetDeviceCount(&devices) != hipSuccess || devices < 1)
        return fail(SPMV_HIP_ERR_NO_DEVICE, "no HIP device visible");
    return build_plan(plan, hp, static_cast<hipStream_t>(stream));
}

int spmv_hip_c16_plan_csr_device(spmv_hip_c16_plan ** plan, int32_t rows, int32_t cols, const int32_t * d_row_ptr,
                                 const int32_t * d_column_index, unsigned flags, void * stream)
{
    if (!plan)
        return fail(SPMV_HIP_ERR_INVALID, "plan is null");
    if (rows < 0 || cols < 0)
        return fail(SPMV_HIP_ERR_INVALID, "bad CSR arguments (rows < 0 or cols < 0)");
    if (flags & ~SPMV_HIP_FLAG_EXACT_ORDER)
        return fail(SPMV_HIP_ERR_INVALID, "unknown flag bits (0 or SPMV_HIP_FLAG_EXACT_ORDER)");
    if (!d_row_ptr)
        return fail(SPMV_HIP_ERR_INVALID, "d_row_ptr is null");
    if ((reinterpret_cast<uintptr_t>(d_row_ptr) | reinterpret_cast<uintptr_t>(d_column_index)) & 3u)
        return fail(SPMV_HIP_ERR_ALIGN, "d_row_ptr and d_column_index must be 4-byte aligned");
    int devices = 0;
    if (hipGetDeviceCount(&devices) != hipSuccess || devices < 1)
        return fail(SPMV_HIP_ERR_NO_DEVICE, "no HIP device visible");
    try {
        return plan_device(plan, rows, cols, d_row_ptr, d_column_index, flags, static_cast<hipStream_t>(stream));
    } catch (std::bad_alloc const &) {
        return fail(SPMV_HIP_ERR_ALLOC, "compact plan from device arrays: host memory");
    }
}

int spmv_hip_c16_plan_table(const spmv_hip_c16_plan * pl, int32_t * tile_table, int64_t tile_table_ints, uint16_t * codes, int64_t codes_len,
                            void * stream)
{
    if (!pl)
        return fail(SPMV_HIP_ERR_INVALID, "plan is null");
    if (tile_table_ints < 0 || codes_len < 0)
        return fail(SPMV_HIP_ERR_INVALID, "a negative count");
    const int nt = pl->ntiles;
    if (tile_table && (long long) SPMV_HIP_C16_TILE_INTS * nt > tile_table_ints)
        return fail(SPMV_HIP_ERR_INVALID, "tile_table is too small: it takes 13 int32 values per tile");
    if (codes && pl->nnz > codes_len)
        return fail(SPMV_HIP_ERR_INVALID, "codes is too small: it takes one value per stored entry");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (nt == 0 || (!tile_table && !codes)) {
        if (codes && pl->nnz > 0)
            std::memset(codes, 0, (size_t) pl->nnz * sizeof(uint16_t));
        if (pl->d_all)
            HIP_TRY(hipStreamSynchronize(s));
        return SPMV_HIP_OK;
    }
    try {
        // the descriptors and the bases always (they say where a tile's codes are), the code stream where the codes are asked for
        const size_t desc_bytes = ((size_t) nt + 1) * sizeof(int4), base_bytes = 8 * (size_t) nt * sizeof(int32_t),
                     code_bytes = codes ? pl->device_bytes - desc_bytes - base_bytes : 0;
        std::vector<int4> desc((size_t) nt + 1);
        std::vector<int32_t> bases(8 * (size_t) nt);
        std::vector<uint16_t> stream_codes(code_bytes / sizeof(uint16_t));
        HIP_TRY(hipMemcpyAsync(desc.data(), pl->d_desc, desc_bytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(bases.data(), pl->d_bases, base_bytes, hipMemcpyDeviceToHost, s));
        if (code_bytes > 0)
            HIP_TRY(hipMemcpyAsync(stream_codes.data(), pl->d_codes, code_bytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (codes)
            std::memset(codes, 0, (size_t) pl->nnz * sizeof(uint16_t));
        for (int w = 0; w < nt; ++w) {
            const int4 & d = desc[(size_t) w];
            const bool compact = (d.z & spmv::kC16MetaCompact) != 0;
            const int32_t * b = &bases[8 * (size_t) w];
            if (tile_table) {
                int32_t * t = tile_table + (size_t) SPMV_HIP_C16_TILE_INTS * w;
                tile_table_row(t, &d);
                int nw = compact ? 1 : 0; // ascending bases up to the last window, which the others repeat
                for (int i = 1; compact && i < SPMV_HIP_C16_WINDOWS; ++i)
                    nw += b[i] > b[i - 1];
                t[4] = nw;
                for (int i = 0; i < SPMV_HIP_C16_WINDOWS; ++i)
                    t[5 + i] = compact ? b[i] : 0;
            }
            const int32_t k0 = d.y, k1 = desc[(size_t) w + 1].y;
            if (codes && compact && k1 > k0)
                std::memcpy(codes + k0, &stream_codes[4 * (size_t) (unsigned) d.w + (size_t) (k0 & 3)], (size_t) (k1 - k0) * sizeof(uint16_t));
        }
    } catch (std::bad_alloc const &) {
        return fail(SPMV_HIP_ERR_ALLOC, "compact plan table: host memory");
    }
    return SPMV_HIP_OK;
}

#ifdef SPMV_HIP_EXPERIMENTS
// not part of the C ABI: the stage times of the last spmv_hip_c16_plan_csr_device of this library (StageClock)
void spmv_hip_c16_plan_device_times(double * out)
{
    std::copy(StageClock::seconds, StageClock::seconds + 5, out);
}
#endif

int spmv_hip_csr_spmv_c16(const spmv_hip_c16_plan * pl, const int32_t * d_row_ptr, const int32_t * d_column_index, const float * d_value,
                          const double * d_x, double * d_y, void * stream)
{
    return c16_multiply(pl, d_row_ptr, d_column_index, d_value, d_x, d_y, stream);
}

int spmv_hip_csr_spmv_c16_f64(const spmv_hip_c16_plan * pl, const int32_t * d_row_ptr, const int32_t * d_column_index, const double * d_value,
                              const double * d_x, double * d_y, void * stream)
{
    return c16_multiply(pl, d_row_ptr, d_column_index, d_value, d_x, d_y, stream);
}

int spmv_hip_csr_spmv_c16_f32xy(const spmv_hip_c16_plan * pl, const int32_t * d_row_ptr, const int32_t * d_column_index, const float * d_value,
                                const float * d_x, float * d_y, void * stream)
{
    return c16_multiply(pl, d_row_ptr, d_column_index, d_value, d_x, d_y, stream);
}

int spmv_hip_csr_spmv_c16_scaled(const spmv_hip_c16_plan * pl, const int32_t * d_row_ptr, const int32_t * d_column_index, const float * d_value,
                                 const double * d_x, double alpha, double beta, const double * d_y_in, double * d_y_out, void * stream)
{
    const ScaledArgs<double> scale{alpha, beta, d_y_in};
    return c16_multiply(pl, d_row_ptr, d_column_index, d_value, d_x, d_y_out, stream, &scale);
}

int spmv_hip_csr_spmv_c16_f64_scaled(const spmv_hip_c16_plan * pl, const int32_t * d_row_ptr, const int32_t * d_column_index, const double * d_value,
                                     const double * d_x, double alpha, double beta, const double * d_y_in, double * d_y_out, void * stream)
{
    const ScaledArgs<double> scale{alpha, beta, d_y_in};
    return c16_multiply(pl, d_row_ptr, d_column_index, d_value, d_x, d_y_out, stream, &scale);
}

int spmv_hip_csr_spmv_c16_f32xy_scaled(const spmv_hip_c16_plan * pl, const int32_t * d_row_ptr, const int32_t * d_column_index, const float * d_value,
                                       const float * d_x, double alpha, double beta, const float * d_y_in, float * d_y_out, void * stream)
{
    const ScaledArgs<float> scale{alpha, beta, d_y_in};
    return c16_multiply(pl, d_row_ptr, d_column_index, d_value, d_x, d_y_out, stream, &scale);
}

int spmv_hip_c16_dots_workspace(const spmv_hip_c16_plan * pl, size_t * bytes)
{
    if (!pl || !bytes)
        return fail(SPMV_HIP_ERR_INVALID, "plan is null, or bytes");
    *bytes = dots_workspace_bytes(pl->ntiles, pl->rows);
    return SPMV_HIP_OK;
}

int spmv_hip_csr_spmv_c16_scaled_dots(const spmv_hip_c16_plan * pl, const int32_t * d_row_ptr, const int32_t * d_column_index, const float * d_value,
                                      const double * d_x, double alpha, double beta, const double * d_y_in, double * d_y_out, const double * d_w,
                                      double * d_dots, void * d_work, size_t work_bytes, void * stream)
{
    const ScaledArgs<double> scale{alpha, beta, d_y_in};
    const DotsArgs dots{d_w, d_dots, d_work, work_bytes};
    return c16_multiply(pl, d_row_ptr, d_column_index, d_value, d_x, d_y_out, stream, &scale, &dots);
}

int spmv_hip_csr_spmv_c16_f64_scaled_dots(const spmv_hip_c16_plan * pl, const int32_t * d_row_ptr, const int32_t * d_column_index,
                                          const double * d_value, const double * d_x, double alpha, double beta, const double * d_y_in,
                                          double * d_y_out, const double * d_w, double * d_dots, void * d_work, size_t work_bytes, void * stream)
{
    const ScaledArgs<double> scale{alpha, beta, d_y_in};
    const DotsArgs dots{d_w, d_dots, d_work, work_bytes};
    return c16_multiply(pl, d_row_ptr, d_column_index, d_value, d_x, d_y_out, stream, &scale, &dots);
}

int spmv_hip_csr_spmv_c16_f32xy_scaled_dots(const spmv_hip_c16_plan * pl, const int32_t * d_row_ptr, const int32_t * d_column_index,
                                            const float * d_value, const float * d_x, double alpha, double beta, const float * d_y_in,
                                            float * d_y_out, const float * d_w, double * d_dots, void * d_work, size_t work_bytes, void * stream)
{
    const ScaledArgs<float> scale{alpha, beta, d_y_in};
    const DotsArgs dots{d_w, d_dots, d_work, work_bytes};
    return c16_multiply(pl, d_row_ptr, d_column_index, d_value, d_x, d_y_out, stream, &scale, &dots);
}

int spmv_hip_c16_plan_verify(const spmv_hip_c16_plan * pl, const int32_t * d_column_index, int64_t * mismatches, void * stream)
{
    if (!pl || !mismatches)
        return fail(SPMV_HIP_ERR_INVALID, "plan / mismatches null");
    *mismatches = 0;
    if (pl->ntiles == 0)
        return SPMV_HIP_OK;
    if (!d_column_index)
        return fail(SPMV_HIP_ERR_INVALID, "d_column_index is null");
    hipStream_t s = static_cast<hipStream_t>(stream);
    unsigned long long * d_count = nullptr, count = 0;
    HIP_TRY(hipMalloc((void **) &d_count, sizeof count));
    hipError_t e = hipMemsetAsync(d_count, 0, sizeof count, s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(spmv::c16_verify_kernel, dim3((unsigned) ((pl->ntiles + 3) / 4)), dim3(256), 0, s, pl->ntiles, pl->d_desc,
                           pl->d_bases, pl->d_codes, d_column_index, d_count);
        e = hipGetLastError();
    }
    if (e == hipSuccess)
        e = hipMemcpyAsync(&count, d_count, sizeof count, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess)
        e = hipStreamSynchronize(s);
    (void) hipFree(d_count);
    if (e != hipSuccess)
        return fail_hip(e, "c16_plan_verify");
    *mismatches = (int64_t) count;
    return SPMV_HIP_OK;
}

int spmv_hip_c16_plan_info(const spmv_hip_c16_plan * pl, int64_t * out, int n)
{
    if (!pl || !out || n < 0)
        return fail(SPMV_HIP_ERR_INVALID, "plan/out null");
    plan_numbers(*pl, out, n);
    return SPMV_HIP_OK;
}

void spmv_hip_c16_plan_destroy(spmv_hip_c16_plan * pl)
{
    if (!pl)
        return;
    if (pl->d_all)
        (void) hipFree(pl->d_all);
    delete pl;
}

// ---- Level 1 --------------------------------------------------------------------------------------------------------------------

static const char kCompactOneDevice[] = "the compact multiply runs on one device (a context of spmv_hip_create)";

int spmv_hip_upload_csr_compact(spmv_hip_ctx * c, int32_t rows, int32_t cols, int32_t nnz, const int32_t * row_ptr,
                                const int32_t * column_index, const double * value, int allow_rounding)
{
    return upload_float_tile(c, 8, kCompactOneDevice, rows, cols, nnz, row_ptr, column_index, value, true, allow_rounding, false);
}

int spmv_hip_upload_csr_compact_f32xy(spmv_hip_ctx * c, int32_t rows, int32_t cols, int32_t nnz, const int32_t * row_ptr,
                                      const int32_t * column_index, const double * value, int allow_rounding)
{
    return upload_float_tile(c, 10, kCompactOneDevice, rows, cols, nnz, row_ptr, column_index, value, true, allow_rounding, true);
}

int spmv_hip_upload_csr_compact_f64(spmv_hip_ctx * c, int32_t rows, int32_t cols, int32_t nnz, const int32_t * row_ptr,
                                    const int32_t * column_index, const double * value)
{
    return upload_float_tile(c, 9, kCompactOneDevice, rows, cols, nnz, row_ptr, column_index, value, false, 0, false);
}

} // extern "C"
