// compact.hip -- include/spmv_hip_compact.h: y += fl32(A) x, y += A x on the caller's fp64 values through the same plan
// (include/spmv_hip_compact_f64.h) and y <- fl32(y + fl32(A) x) on float x and y (include/spmv_hip_compact_f32xy.h), with the columns of a tile as 16-bit codes (a 3-bit window number and a 13-bit offset from one of
// eight per-tile bases).  The tiles are f32values.hip's own (f32_plan.hpp): its descriptors as they
// are, with the compact bits and the tile's first code quad added; the bases and the codes are made on the host by a few
// threads, tile by tile; the kernel is csr_compact.hpp.
#include "f32_plan.hpp"
#include "csr_compact.hpp"

#include <algorithm>
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
    bool bad = false;
    for (int32_t e = 0; e < nnz; ++e)
        bad |= col[e] < 0 || col[e] >= cols;
    if (bad)
        return fail(SPMV_HIP_ERR_INVALID, "column index out of range [0, cols)");
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
    for (int w = 0; w < nt; ++w) {
        int4 & d = hp.desc[(size_t) w];
        const int32_t k0 = d.y, k1 = hp.desc[(size_t) w + 1].y, kb = k0 & ~3;
        const int nw = hp.windows[(size_t) w];
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
    hp.codes.assign(4 * (size_t) quads, 0);
    for (int w = 0; w < nt; ++w)
        if (hp.windows[(size_t) w] > 0) {
            const int32_t k0 = hp.desc[(size_t) w].y, k1 = hp.desc[(size_t) w + 1].y;
            if (k1 > k0)
                std::memcpy(&hp.codes[4 * (size_t) (unsigned) hp.desc[(size_t) w].w + (size_t) (k0 & 3)], &hp.by_entry[(size_t) k0],
                            (size_t) (k1 - k0) * sizeof(uint16_t));
        }
    pl.device_bytes = (16 * ((size_t) nt + 1) + 32 * (size_t) nt + 8 * (size_t) quads + 15) & ~(size_t) 15;
    // the fp32-value plan's bytes with 2 instead of 4 bytes of column per compact entry, and the bases
    pl.streamed_bytes = fp.numbers.streamed_bytes - 2LL * pl.compact_entries + 32LL * nt;
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

// spmv_hip_csr_spmv_c16 (V = float, T = double), spmv_hip_csr_spmv_c16_f64 (V = double) and spmv_hip_csr_spmv_c16_f32xy (V = T =
// float): the plan knows neither the value type nor the vectors' element type.  With a scale (spmv_hip_scaled.h) d_y is y_out
// and the same refusals apply; without one it is y += A x.
template <class V, class T>
int c16_multiply(const spmv_hip_c16_plan * pl, const int32_t * d_row_ptr, const int32_t * d_column_index, const V * d_value,
                 const T * d_x, T * d_y, void * stream, const ScaledArgs<T> * scale = nullptr, const DotsArgs * dots = nullptr)
{
    if (!pl)
        return fail(SPMV_HIP_ERR_INVALID, "plan is null");
    if (d_x && (const void *) d_x == (const void *) d_y)
        return fail(SPMV_HIP_ERR_INVALID, "d_x and d_y must be different arrays");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (scale) {
        int rc = scaled_vectors_check(pl->rows, sizeof(T), scale->beta, scale->y_in, d_y);
        if (rc == 0 && dots)
            rc = dots_check(*dots, pl->ntiles, pl->rows, pl->cols, pl->nnz, sizeof(T), sizeof(V), d_row_ptr, d_column_index, d_value, d_x,
                            scale->beta, scale->y_in, d_y);
        if (rc != 0)
            return rc;
        if (pl->rows == 0)
            return dots ? dots_reduce(*dots, 0, s) : SPMV_HIP_OK;
        if (scale->alpha == 0.0 || pl->ntiles == 0) { // the beta part alone: neither the matrix nor x is read
            if (dots)
                return scaled_rows_only_dots(pl->rows, std::is_same<T, float>::value, scale->alpha != 0.0, scale->alpha, scale->beta, scale->y_in,
                                             d_y, *dots, s);
            return scaled_rows_only(pl->rows, std::is_same<T, float>::value, scale->alpha != 0.0, scale->alpha, scale->beta, scale->y_in, d_y, s);
        }
    }
    if (pl->ntiles == 0) // rows, cols or nnz of zero
        return SPMV_HIP_OK;
    if (!d_row_ptr || !d_value || !d_x || !d_y)
        return fail(SPMV_HIP_ERR_INVALID, "null device pointer");
    if (!d_column_index && pl->wide_tiles > 0)
        return fail(SPMV_HIP_ERR_INVALID, "d_column_index is null and the plan has wide tiles, which read the 32-bit columns");
    if (!aligned16(d_column_index) || !aligned16(d_value))
        return fail(SPMV_HIP_ERR_ALIGN, "column / value arrays must be 16-byte aligned");
    if constexpr (std::is_same<T, float>::value) // (the kernel reads and writes x and y one element at a time)
        if ((reinterpret_cast<uintptr_t>(d_x) | reinterpret_cast<uintptr_t>(d_y)) & 3u)
            return fail(SPMV_HIP_ERR_ALIGN, "d_x and d_y must be 4-byte aligned");
    const dim3 grid((unsigned) ((pl->ntiles + 3) / 4)), block(256);
    const int exact = (pl->flags & SPMV_HIP_FLAG_EXACT_ORDER) ? 1 : 0;
    const bool x32 = (long long) pl->cols * (long long) sizeof(T) < (1LL << 32);
    if (dots) { // (x32 holds: dots_check)
        const bool beta0 = scale->beta == 0.0, hasw = dots->w != nullptr;
        void (*kernel)(int, const int4 *, const int *, const uint16_t *, const int32_t *, const int32_t *, const V *, const T *, double, double,
                       const T *, T *, const T *, spmv::v2d *, int);
#define SPMV_C16_PICK(NAME) (beta0 ? (hasw ? spmv::NAME<true, true> : spmv::NAME<true, false>) : (hasw ? spmv::NAME<false, true> : spmv::NAME<false, false>))
        if constexpr (std::is_same<T, float>::value)
            kernel = SPMV_C16_PICK(csr_compact_f32xy_scaled_dots_kernel);
        else if constexpr (std::is_same<V, float>::value)
            kernel = SPMV_C16_PICK(csr_compact_scaled_dots_kernel);
        else
            kernel = SPMV_C16_PICK(csr_compact_f64_scaled_dots_kernel);
#undef SPMV_C16_PICK
        hipLaunchKernelGGL(kernel, grid, block, 0, s, pl->ntiles, pl->d_desc, pl->d_bases, pl->d_codes, d_row_ptr, d_column_index, d_value, d_x,
                           scale->alpha, scale->beta, scale->y_in, d_y, static_cast<const T *>(dots->w), static_cast<spmv::v2d *>(dots->work), exact);
        HIP_TRY(hipGetLastError());
        return dots_reduce(*dots, pl->ntiles, s);
    }
    if (scale) {
        const bool beta0 = scale->beta == 0.0;
        void (*kernel)(int, const int4 *, const int *, const uint16_t *, const int32_t *, const int32_t *, const V *, const T *, double, double,
                       const T *, T *, int);
#define SPMV_C16_PICK(NAME) (x32 ? (beta0 ? spmv::NAME<true, true> : spmv::NAME<true, false>) : (beta0 ? spmv::NAME<false, true> : spmv::NAME<false, false>))
        if constexpr (std::is_same<T, float>::value)
            kernel = SPMV_C16_PICK(csr_compact_f32xy_scaled_kernel);
        else if constexpr (std::is_same<V, float>::value)
            kernel = SPMV_C16_PICK(csr_compact_scaled_kernel);
        else
            kernel = SPMV_C16_PICK(csr_compact_f64_scaled_kernel);
#undef SPMV_C16_PICK
        hipLaunchKernelGGL(kernel, grid, block, 0, s, pl->ntiles, pl->d_desc, pl->d_bases, pl->d_codes, d_row_ptr, d_column_index, d_value, d_x,
                           scale->alpha, scale->beta, scale->y_in, d_y, exact);
        HIP_TRY(hipGetLastError());
        return SPMV_HIP_OK;
    }
    void (*kernel)(int, const int4 *, const int *, const uint16_t *, const int32_t *, const int32_t *, const V *, const T *, T *, int);
    if constexpr (std::is_same<T, float>::value)
        kernel = x32 ? spmv::csr_compact_f32xy_kernel<true> : spmv::csr_compact_f32xy_kernel<false>;
    else if constexpr (std::is_same<V, float>::value)
        kernel = x32 ? spmv::csr_compact_kernel<true> : spmv::csr_compact_kernel<false>;
    else
        kernel = x32 ? spmv::csr_compact_f64_kernel<true> : spmv::csr_compact_f64_kernel<false>;
    hipLaunchKernelGGL(kernel, grid, block, 0, s, pl->ntiles, pl->d_desc, pl->d_bases, pl->d_codes, d_row_ptr, d_column_index, d_value, d_x,
                       d_y, exact);
    HIP_TRY(hipGetLastError());
    return SPMV_HIP_OK;
}

// spmv_hip_upload_csr_compact (format 8) and spmv_hip_upload_csr_compact_f32xy (format 10: float_vectors)
int upload_compact_floats(spmv_hip_ctx * c, int32_t rows, int32_t cols, int32_t nnz, const int32_t * row_ptr, const int32_t * column_index,
                          const double * value, int allow_rounding, bool float_vectors)
{
    if (!c)
        return fail(SPMV_HIP_ERR_INVALID, "ctx is null");
    if (c->multi)
        return fail(SPMV_HIP_ERR_STATE, "the compact multiply runs on one device (a context of spmv_hip_create)");
    if (rows < 0 || cols < 0 || nnz < 0 || !row_ptr || (nnz > 0 && (!column_index || !value)))
        return fail(SPMV_HIP_ERR_INVALID, "bad CSR arguments");
    const unsigned flags = c->flags & SPMV_HIP_FLAG_EXACT_ORDER;
    // everything that can refuse the matrix happens before anything is freed or copied
    int rc = f32_check_host(rows, cols, row_ptr, flags);
    if (rc != 0)
        return rc;
    if (row_ptr[rows] != nnz)
        return fail(SPMV_HIP_ERR_INVALID, "row_ptr[rows] must equal nnz");
    HostPlan hp;
    if ((rc = plan_host_guarded(hp, rows, cols, row_ptr, column_index, flags)) != 0) // (... the columns here)
        return rc;
    std::vector<float> narrow;
    try {
        narrow.resize((size_t) nnz);
    } catch (std::bad_alloc const &) {
        return fail(SPMV_HIP_ERR_ALLOC, "compact upload: host memory");
    }
    if ((rc = narrow_refusal(narrow_host(nnz, value, narrow.data()), allow_rounding)) != 0)
        return rc;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    free_ctx_matrix(c);
    if ((rc = build_plan(&c->c16_plan, hp, c->stream)) != 0)
        return rc;
    // only wide tiles read 32-bit columns
    if ((rc = upload_ctx_csr(c, (size_t) rows + 1, (size_t) cols, (size_t) rows, (size_t) nnz, row_ptr,
                             column_index, c->c16_plan->wide_tiles > 0, narrow.data(), true, float_vectors)) != 0)
        return rc;
    c->rows = rows;
    c->cols = cols;
    c->nnz = nnz;
    c->bytes += c->c16_plan->device_bytes;
    c->format = float_vectors ? 10 : 8;
    return SPMV_HIP_OK;
}

} // namespace

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
            t[0] = hp.desc[(size_t) w].x;
            t[1] = hp.desc[(size_t) w].y;
            t[2] = hp.desc[(size_t) w + 1].x - hp.desc[(size_t) w].x;
            t[3] = (hp.desc[(size_t) w].z >> spmv::kTileMetaLanesShift) & 7;
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

int spmv_hip_upload_csr_compact(spmv_hip_ctx * c, int32_t rows, int32_t cols, int32_t nnz, const int32_t * row_ptr,
                                const int32_t * column_index, const double * value, int allow_rounding)
{
    return upload_compact_floats(c, rows, cols, nnz, row_ptr, column_index, value, allow_rounding, false);
}

int spmv_hip_upload_csr_compact_f32xy(spmv_hip_ctx * c, int32_t rows, int32_t cols, int32_t nnz, const int32_t * row_ptr,
                                      const int32_t * column_index, const double * value, int allow_rounding)
{
    return upload_compact_floats(c, rows, cols, nnz, row_ptr, column_index, value, allow_rounding, true);
}

int spmv_hip_upload_csr_compact_f64(spmv_hip_ctx * c, int32_t rows, int32_t cols, int32_t nnz, const int32_t * row_ptr,
                                    const int32_t * column_index, const double * value)
{
    if (!c)
        return fail(SPMV_HIP_ERR_INVALID, "ctx is null");
    if (c->multi)
        return fail(SPMV_HIP_ERR_STATE, "the compact multiply runs on one device (a context of spmv_hip_create)");
    if (rows < 0 || cols < 0 || nnz < 0 || !row_ptr || (nnz > 0 && (!column_index || !value)))
        return fail(SPMV_HIP_ERR_INVALID, "bad CSR arguments");
    const unsigned flags = c->flags & SPMV_HIP_FLAG_EXACT_ORDER;
    // everything that can refuse the matrix happens before anything is freed or copied
    int rc = f32_check_host(rows, cols, row_ptr, flags);
    if (rc != 0)
        return rc;
    if (row_ptr[rows] != nnz)
        return fail(SPMV_HIP_ERR_INVALID, "row_ptr[rows] must equal nnz");
    HostPlan hp;
    if ((rc = plan_host_guarded(hp, rows, cols, row_ptr, column_index, flags)) != 0) // (... the columns here)
        return rc;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    free_ctx_matrix(c);
    if ((rc = build_plan(&c->c16_plan, hp, c->stream)) != 0)
        return rc;
    // the values as they are (d_val); only wide tiles read 32-bit columns
    if ((rc = upload_ctx_csr(c, (size_t) rows + 1, (size_t) cols, (size_t) rows, (size_t) nnz, row_ptr,
                             column_index, c->c16_plan->wide_tiles > 0, value, false)) != 0)
        return rc;
    c->rows = rows;
    c->cols = cols;
    c->nnz = nnz;
    c->bytes += c->c16_plan->device_bytes;
    c->format = 9;
    return SPMV_HIP_OK;
}

} // extern "C"
