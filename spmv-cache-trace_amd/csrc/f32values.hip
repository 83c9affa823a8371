// f32values.hip -- include/spmv_hip_f32values.h: y += fl32(A) x with the values stored and streamed as 4-byte floats.  The plan
// cuts the rows into wave tiles on the host from row_ptr alone (the plain tiles of plan_csr.hip: lanes per row from the tile's
// longest row, at most 16 entries per lane); the kernel is csr_f32values.hpp.  The multiply's refusals and launches are
// tile_front.hpp's: this file describes the family to it (F32Family) and defines what f32_plan.hpp declares for compact.hip,
// whose upload_float_tile is the Level-1 upload of this format too.
#include "tile_front.hpp"
#include "csr_dots.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <new>

using namespace spmvi;

namespace {

int lanes_for(int len)
{
    int l = 0;
    while (l < 6 && (16 << l) < len)
        ++l;
    return l;
}

void plan_numbers(const spmv_hip_f32_plan & pl, int64_t * out, int n)
{
    const int64_t v[SPMV_HIP_F32_INFO] = {pl.rows, pl.cols, pl.nnz, pl.ntiles, pl.long_tiles, pl.longest, pl.flags,
                                          (int64_t) pl.device_bytes, pl.streamed_bytes, pl.uniform_tiles, pl.scalar_tiles,
                                          (pl.ntiles + 3) / 4};
    for (int i = 0; i < n && i < SPMV_HIP_F32_INFO; ++i)
        out[i] = v[i];
}

int narrow_report(NarrowResult const & c, int64_t * inexact, double * max_rel_err)
{
    if (c.overflow > 0) {
        char text[160];
        std::snprintf(text, sizeof text, "%lld finite value(s) are infinite as floats (the first is entry %lld)", c.overflow, c.first_overflow);
        return fail(SPMV_HIP_ERR_OVERFLOW, text);
    }
    if (inexact)
        *inexact = c.inexact;
    if (max_rel_err)
        *max_rel_err = c.max_rel;
    return SPMV_HIP_OK;
}

// csr_f32values.hpp's kernels take the descriptors alone in front of the arrays; a null column array is one more null pointer
struct F32Family {
    const spmv_hip_f32_plan * pl;
    static const char * null_columns() { return nullptr; }
    static bool columns_read() { return true; }
    static auto plain(bool x32) { return with_bools([](auto X) { return spmv::csr_f32values_kernel<X()>; }, x32); }
    static auto scaled(bool x32, bool b0) { return with_bools([](auto X, auto B0) { return spmv::csr_f32values_scaled_kernel<X(), B0()>; }, x32, b0); }
    static auto dots(bool b0, bool w) { return with_bools([](auto B0, auto W) { return spmv::csr_f32values_scaled_dots_kernel<B0(), W()>; }, b0, w); }
    template <class K, class... A>
    void launch(K kernel, dim3 grid, hipStream_t s, A... a) const
    {
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, pl->ntiles, pl->d_desc, a...);
    }
};

// slots of the path without tiles (one per wave of scaled_rows_only_dots_kernel)
long long row_slots(int32_t rows) { return ((long long) rows + 63) / 64; }

// the vector kernel of a scaled call where no tile runs, over T; d: with the dots of what it stores
template <class T>
int rows_only(int32_t rows, bool zterm, double alpha, double beta, const T * y_in, T * y_out, const DotsArgs * d, hipStream_t s)
{
    const dim3 grid((unsigned) (((long long) rows + 255) / 256));
    if (!d) {
        hipLaunchKernelGGL(with_bools([](auto B0, auto Z) { return spmv::scaled_rows_only_kernel<T, B0(), Z()>; }, beta == 0.0, zterm), grid,
                           dim3(256), 0, s, (int) rows, alpha, beta, y_in, y_out);
        HIP_TRY(hipGetLastError());
        return SPMV_HIP_OK;
    }
    hipLaunchKernelGGL(with_bools([](auto B0, auto Z, auto W) { return spmv::scaled_rows_only_dots_kernel<T, B0(), Z(), W()>; }, beta == 0.0, zterm,
                                  d->w != nullptr),
                       grid, dim3(256), 0, s, (int) rows, alpha, beta, y_in, y_out, static_cast<const T *>(d->w), static_cast<spmv::v2d *>(d->work));
    HIP_TRY(hipGetLastError());
    return dots_reduce(*d, (int) row_slots(rows), s);
}

} // namespace

// ---- what compact.hip and krylov.hip share (f32_plan.hpp) ------------------------------------------------------------------------------------

namespace spmvi {

long long reduce_blocks(long long n) { return (n + spmv::kDotsChunk - 1) / spmv::kDotsChunk; }

bool overlap(const void * a, unsigned long long abytes, const void * b, unsigned long long bbytes)
{
    if (!a || !b || abytes == 0 || bbytes == 0)
        return false;
    const uintptr_t p = reinterpret_cast<uintptr_t>(a), q = reinterpret_cast<uintptr_t>(b);
    return p < q + bbytes && q < p + abytes;
}

int f32_multiply(const spmv_hip_f32_plan * pl, const int32_t * d_row_ptr, const int32_t * d_column_index, const float * d_value,
                 const double * d_x, double * d_y, void * stream, const ScaledArgs<double> * scale, const DotsArgs * dots)
{
    return tile_multiply(F32Family{pl}, d_row_ptr, d_column_index, d_value, d_x, d_y, stream, scale, dots);
}

int f32_build_plan(spmv_hip_f32_plan ** out, F32HostPlan const & hp, hipStream_t s)
{
    spmv_hip_f32_plan * pl = new (std::nothrow) spmv_hip_f32_plan(hp.numbers);
    if (!pl)
        return fail(SPMV_HIP_ERR_ALLOC, "plan allocation failed");
    if (!hp.desc.empty()) {
        hipError_t e = hipMalloc((void **) &pl->d_desc, hp.desc.size() * sizeof(int4));
        if (e == hipSuccess)
            e = hipMemcpyAsync(pl->d_desc, hp.desc.data(), hp.desc.size() * sizeof(int4), hipMemcpyHostToDevice, s);
        if (e == hipSuccess)
            e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            spmv_hip_f32_plan_destroy(pl);
            return fail_hip(e, "fp32-value plan: tile descriptors");
        }
    }
    *out = pl;
    return SPMV_HIP_OK;
}

int f32_plan_host_guarded(F32HostPlan & hp, int32_t rows, int32_t cols, const int32_t * rp, unsigned flags, const char * out_of_memory)
{
    const int rc = f32_check_host(rows, cols, rp, flags);
    if (rc != 0)
        return rc;
    try {
        f32_plan_host(hp, rows, cols, rp, flags);
    } catch (std::bad_alloc const &) {
        return fail(SPMV_HIP_ERR_ALLOC, out_of_memory);
    }
    return SPMV_HIP_OK;
}

int check_columns(int32_t nnz, const int32_t * col, int32_t cols)
{
    bool bad = false;
    for (int32_t e = 0; e < nnz; ++e)
        bad |= col[e] < 0 || col[e] >= cols;
    return bad ? fail(SPMV_HIP_ERR_INVALID, "column index out of range [0, cols)") : SPMV_HIP_OK;
}

void tile_table_row(int32_t * t, const int4 * d)
{
    t[0] = d[0].x;
    t[1] = d[0].y;
    t[2] = d[1].x - d[0].x;
    t[3] = (d[0].z >> spmv::kTileMetaLanesShift) & 7;
}

int f32_check_host(int32_t rows, int32_t cols, const int32_t * rp, unsigned flags)
{
    if (rows < 0 || cols < 0 || !rp)
        return fail(SPMV_HIP_ERR_INVALID, "bad CSR arguments (rows < 0, cols < 0 or row_ptr null)");
    if (flags & ~SPMV_HIP_FLAG_EXACT_ORDER)
        return fail(SPMV_HIP_ERR_INVALID, "unknown flag bits (0 or SPMV_HIP_FLAG_EXACT_ORDER)");
    return check_row_ptr_order(rows, rp);
}

void f32_plan_host(F32HostPlan & hp, int32_t rows, int32_t cols, const int32_t * p, unsigned flags)
{
    spmv_hip_f32_plan & pl = hp.numbers;
    const int32_t nnz = p[rows];
    const bool exact = (flags & SPMV_HIP_FLAG_EXACT_ORDER) != 0;
    pl.rows = rows;
    pl.cols = cols;
    pl.nnz = nnz;
    pl.flags = flags;
    for (int32_t r = 0; r < rows; ++r)
        pl.longest = std::max(pl.longest, p[r + 1] - p[r]);
    if (rows == 0 || cols == 0 || nnz == 0)
        return; // the multiply does nothing
    long long row_ptr_bytes = 0;
    for (int32_t r = 0; r < rows;) {
        const int32_t k0 = p[r], kb = k0 & ~3;
        if ((long long) p[r + 1] - kb > spmv::kF32Tile) {
            // a row longer than a tile: a tile of its own, the whole wave (one lane in exact order)
            const int len = p[r + 1] - k0;
            hp.desc.push_back(make_int4(r, k0, std::min(len, 0xFFFF) | ((exact ? 0 : 6) << spmv::kTileMetaLanesShift), 0));
            ++pl.long_tiles;
            ++r;
            continue;
        }
        int32_t r1 = r;
        int maxlen = 0, minlen = INT32_MAX;
        while (r1 < rows && r1 - r < spmv::kF32TileRows && (long long) p[r1 + 1] - kb <= spmv::kF32Tile) {
            const int len = p[r1 + 1] - p[r1];
            if (!exact && r1 > r) { // only as many rows as the wave has lanes for at <= 16 entries per lane
                const int l = lanes_for(std::max(maxlen, len));
                if (l > 0 && ((r1 - r + 1) << l) > 64)
                    break;
            }
            maxlen = std::max(maxlen, len);
            minlen = std::min(minlen, len);
            ++r1;
        }
        const int lanes_log2 = exact ? 0 : lanes_for(maxlen);
        const int32_t k1 = p[r1];
        const bool fast = k1 > k0 && (long long) ((k1 - 1) & ~3) + 4 <= nnz;
        const bool uniform = fast && minlen == maxlen;
        hp.desc.push_back(make_int4(r, k0, maxlen | (lanes_log2 << spmv::kTileMetaLanesShift) | (fast ? spmv::kTileMetaFast : 0) |
                                               (uniform ? spmv::kTileMetaUniform : 0), 0));
        if (uniform)
            ++pl.uniform_tiles;
        else
            row_ptr_bytes += 4LL * (r1 - r + 1);
        if (!fast)
            ++pl.scalar_tiles;
        r = r1;
    }
    pl.ntiles = (int) hp.desc.size();
    hp.desc.push_back(make_int4(rows, nnz, 0, 0));
    pl.device_bytes = hp.desc.size() * sizeof(int4);
    pl.streamed_bytes = 8LL * nnz + row_ptr_bytes + 16LL * rows + 8LL * cols + 16LL * (pl.ntiles + 1);
}

NarrowResult narrow_host(int64_t n, const double * value, float * out)
{
    NarrowResult c;
    for (int64_t k = 0; k < n; ++k) {
        const double v = value[k];
        const float f = static_cast<float>(v);
        out[k] = f;
        const double back = static_cast<double>(f);
        if (back != v && v == v) {
            if (std::isinf(back)) {
                ++c.overflow;
                if (c.first_overflow < 0)
                    c.first_overflow = k;
            } else {
                ++c.inexact;
                if (c.first_inexact < 0)
                    c.first_inexact = k;
                c.max_rel = std::max(c.max_rel, std::fabs(back - v) / std::fabs(v));
            }
        }
    }
    return c;
}

int narrow_refusal(NarrowResult const & c, int allow_rounding)
{
    const int rc = narrow_report(c, nullptr, nullptr);
    if (rc != 0 || c.inexact == 0 || allow_rounding)
        return rc;
    char text[200];
    std::snprintf(text, sizeof text, "%lld value(s) are not floats (the first is entry %lld, relative change at most %.3g) and allow_rounding is 0",
                  c.inexact, c.first_inexact, c.max_rel);
    return fail(SPMV_HIP_ERR_INVALID, text);
}

int scaled_vectors_check(int32_t rows, size_t elem, double beta, const void * y_in, const void * y_out)
{
    if (rows == 0)
        return SPMV_HIP_OK;
    if (!y_out)
        return fail(SPMV_HIP_ERR_INVALID, "d_y_out is null");
    const uintptr_t in = reinterpret_cast<uintptr_t>(y_in), out = reinterpret_cast<uintptr_t>(y_out), bytes = (uintptr_t) rows * elem;
    if (elem == 4 && ((out | (beta != 0.0 ? in : 0)) & 3u))
        return fail(SPMV_HIP_ERR_ALIGN, "d_y_in and d_y_out must be 4-byte aligned");
    if (beta == 0.0) // y_in is never read
        return SPMV_HIP_OK;
    if (!y_in)
        return fail(SPMV_HIP_ERR_INVALID, "d_y_in is null and beta is not 0");
    if (in != out && in < out + bytes && out < in + bytes)
        return fail(SPMV_HIP_ERR_INVALID, "d_y_in and d_y_out overlap without being the same array");
    return SPMV_HIP_OK;
}

int scaled_rows_only(int32_t rows, bool float_vectors, bool zterm, double alpha, double beta, const void * y_in, void * y_out, hipStream_t s)
{
    if (float_vectors)
        return rows_only(rows, zterm, alpha, beta, static_cast<const float *>(y_in), static_cast<float *>(y_out), nullptr, s);
    return rows_only(rows, zterm, alpha, beta, static_cast<const double *>(y_in), static_cast<double *>(y_out), nullptr, s);
}

int scaled_rows_only_dots(int32_t rows, bool float_vectors, bool zterm, double alpha, double beta, const void * y_in, void * y_out,
                          const DotsArgs & d, hipStream_t s)
{
    if (float_vectors)
        return rows_only(rows, zterm, alpha, beta, static_cast<const float *>(y_in), static_cast<float *>(y_out), &d, s);
    return rows_only(rows, zterm, alpha, beta, static_cast<const double *>(y_in), static_cast<double *>(y_out), &d, s);
}

size_t dots_workspace_bytes(int ntiles, int32_t rows)
{
    const long long slots = std::max<long long>(ntiles, row_slots(rows));
    return (size_t) std::max<long long>(16, 16 * (slots + reduce_blocks(slots)));
}

int dots_check(const DotsArgs & d, int ntiles, int32_t rows, int32_t cols, int32_t nnz, size_t elem, size_t value_elem, const void * row_ptr,
               const void * column_index, const void * value, const void * x, double beta, const void * y_in, const void * y_out)
{
    if (!d.dots || !d.work)
        return fail(SPMV_HIP_ERR_INVALID, "d_dots or d_work is null");
    const size_t need = dots_workspace_bytes(ntiles, rows);
    if (d.work_bytes < need) {
        char text[160];
        std::snprintf(text, sizeof text, "work_bytes is %zu and the plan needs %zu (spmv_hip_*_dots_workspace)", d.work_bytes, need);
        return fail(SPMV_HIP_ERR_INVALID, text);
    }
    if (!aligned16(d.dots) || !aligned16(d.work))
        return fail(SPMV_HIP_ERR_ALIGN, "d_dots and d_work must be 16-byte aligned");
    if (elem == 4 && (reinterpret_cast<uintptr_t>(d.w) & 3u))
        return fail(SPMV_HIP_ERR_ALIGN, "d_w must be 4-byte aligned");
    if ((unsigned long long) cols * elem >= (1ULL << 32))
        return fail(SPMV_HIP_ERR_INVALID, "x spans 4 GiB or more: the multiplies with dots have no kernel for such vectors");
    const unsigned long long vec = (unsigned long long) rows * elem;
    if (overlap(d.w, vec, y_out, vec))
        return fail(SPMV_HIP_ERR_INVALID, "d_w overlaps d_y_out");
    if (overlap(d.dots, 16, d.work, need))
        return fail(SPMV_HIP_ERR_INVALID, "d_dots and d_work overlap");
    const struct {
        const void * p;
        unsigned long long bytes;
    } arrays[] = {{row_ptr, 4ULL * ((unsigned long long) rows + 1)}, {column_index, 4ULL * (unsigned long long) nnz},
                  {value, (unsigned long long) value_elem * (unsigned long long) nnz}, {x, (unsigned long long) cols * elem},
                  {beta != 0.0 ? y_in : nullptr, vec}, {y_out, vec}, {d.w, vec}};
    for (auto const & a : arrays)
        if (overlap(d.dots, 16, a.p, a.bytes) || overlap(d.work, need, a.p, a.bytes))
            return fail(SPMV_HIP_ERR_INVALID, "d_dots or d_work overlaps an array of the call");
    return SPMV_HIP_OK;
}

int dots_reduce(const DotsArgs & d, int n, hipStream_t s)
{
    spmv::v2d * slots = static_cast<spmv::v2d *>(d.work);
    spmv::v2d * out = reinterpret_cast<spmv::v2d *>(d.dots);
    const long long blocks = reduce_blocks(n);
    if (blocks > 1) { // two stages: a partial sum per chunk of slots behind the slots, then their sum
        hipLaunchKernelGGL(spmv::dots_reduce_kernel<256>, dim3((unsigned) blocks), dim3(256), 0, s, n, spmv::kDotsChunk, slots, slots + n);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(spmv::dots_reduce_kernel<256>, dim3(1), dim3(256), 0, s, (int) blocks, (int) blocks, slots + n, out);
    } else
        hipLaunchKernelGGL(spmv::dots_reduce_kernel<256>, dim3(1), dim3(256), 0, s, n, spmv::kDotsChunk, slots, out);
    HIP_TRY(hipGetLastError());
    return SPMV_HIP_OK;
}

} // namespace spmvi

extern "C" {

int spmv_hip_f32_dots_workspace(const spmv_hip_f32_plan * pl, size_t * bytes)
{
    if (!pl || !bytes)
        return fail(SPMV_HIP_ERR_INVALID, "plan is null, or bytes");
    *bytes = dots_workspace_bytes(pl->ntiles, pl->rows);
    return SPMV_HIP_OK;
}

int spmv_hip_csr_spmv_f32_scaled_dots(const spmv_hip_f32_plan * pl, const int32_t * d_row_ptr, const int32_t * d_column_index,
                                      const float * d_value, const double * d_x, double alpha, double beta, const double * d_y_in,
                                      double * d_y_out, const double * d_w, double * d_dots, void * d_work, size_t work_bytes, void * stream)
{
    const ScaledArgs<double> scale{alpha, beta, d_y_in};
    const DotsArgs dots{d_w, d_dots, d_work, work_bytes};
    return f32_multiply(pl, d_row_ptr, d_column_index, d_value, d_x, d_y_out, stream, &scale, &dots);
}

int spmv_hip_narrow_values_host(int64_t n, const double * value, float * out, int64_t * inexact, double * max_rel_err)
{
    if (n < 0 || (n > 0 && (!value || !out)))
        return fail(SPMV_HIP_ERR_INVALID, "n < 0, or value / out null");
    return narrow_report(narrow_host(n, value, out), inexact, max_rel_err);
}

int spmv_hip_narrow_values(int64_t n, const double * d_value, float * d_out, int64_t * inexact, double * max_rel_err, void * stream)
{
    if (n < 0 || (n > 0 && (!d_value || !d_out)))
        return fail(SPMV_HIP_ERR_INVALID, "n < 0, or d_value / d_out null");
    NarrowResult c;
    if (n > 0) {
        hipStream_t s = static_cast<hipStream_t>(stream);
        const int blocks = (int) std::min<int64_t>(1024, (n + 255) / 256);
        spmv::NarrowCounts * d_counts = nullptr;
        HIP_TRY(hipMalloc((void **) &d_counts, (size_t) blocks * sizeof(spmv::NarrowCounts)));
        std::vector<spmv::NarrowCounts> counts((size_t) blocks);
        hipLaunchKernelGGL(spmv::narrow_values_kernel, dim3((unsigned) blocks), dim3(256), 0, s, (long long) n, d_value, d_out, d_counts);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess)
            e = hipMemcpyAsync(counts.data(), d_counts, counts.size() * sizeof(spmv::NarrowCounts), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess)
            e = hipStreamSynchronize(s);
        (void) hipFree(d_counts);
        if (e != hipSuccess)
            return fail_hip(e, "narrow_values");
        auto first = [](long long a, long long b) { return a < 0 ? b : (b < 0 ? a : std::min(a, b)); };
        for (auto const & b : counts) {
            c.inexact += b.inexact;
            c.overflow += b.overflow;
            c.first_inexact = first(c.first_inexact, b.first_inexact);
            c.first_overflow = first(c.first_overflow, b.first_overflow);
            c.max_rel = std::max(c.max_rel, b.max_rel);
        }
    }
    return narrow_report(c, inexact, max_rel_err);
}

int spmv_hip_f32_plan_preview(int32_t rows, int32_t cols, const int32_t * host_row_ptr, unsigned flags, int64_t * out, int n,
                              int32_t * tile_table, int64_t tile_table_ints)
{
    if (!out || n < 0 || tile_table_ints < 0)
        return fail(SPMV_HIP_ERR_INVALID, "out is null, or a negative count");
    F32HostPlan hp;
    const int rc = f32_plan_host_guarded(hp, rows, cols, host_row_ptr, flags);
    if (rc != 0)
        return rc;
    const int nt = hp.numbers.ntiles;
    if (tile_table) {
        if (4LL * nt > tile_table_ints)
            return fail(SPMV_HIP_ERR_INVALID, "tile_table is too small: it takes 4 int32 values per tile");
        for (int w = 0; w < nt; ++w)
            tile_table_row(tile_table + 4 * (size_t) w, &hp.desc[(size_t) w]);
    }
    plan_numbers(hp.numbers, out, n);
    return SPMV_HIP_OK;
}

int spmv_hip_f32_plan_csr(spmv_hip_f32_plan ** plan, int32_t rows, int32_t cols, const int32_t * host_row_ptr, unsigned flags,
                          void * stream)
{
    if (!plan)
        return fail(SPMV_HIP_ERR_INVALID, "plan is null");
    *plan = nullptr;
    F32HostPlan hp;
    const int rc = f32_plan_host_guarded(hp, rows, cols, host_row_ptr, flags);
    if (rc != 0)
        return rc;
    int devices = 0;
    if (hipGetDeviceCount(&devices) != hipSuccess || devices < 1)
        return fail(SPMV_HIP_ERR_NO_DEVICE, "no HIP device visible");
    return f32_build_plan(plan, hp, static_cast<hipStream_t>(stream));
}

int spmv_hip_csr_spmv_f32(const spmv_hip_f32_plan * pl, const int32_t * d_row_ptr, const int32_t * d_column_index,
                          const float * d_value, const double * d_x, double * d_y, void * stream)
{
    return f32_multiply(pl, d_row_ptr, d_column_index, d_value, d_x, d_y, stream, nullptr, nullptr);
}

int spmv_hip_csr_spmv_f32_scaled(const spmv_hip_f32_plan * pl, const int32_t * d_row_ptr, const int32_t * d_column_index,
                                 const float * d_value, const double * d_x, double alpha, double beta, const double * d_y_in,
                                 double * d_y_out, void * stream)
{
    const ScaledArgs<double> scale{alpha, beta, d_y_in};
    return f32_multiply(pl, d_row_ptr, d_column_index, d_value, d_x, d_y_out, stream, &scale, nullptr);
}

int spmv_hip_f32_plan_info(const spmv_hip_f32_plan * pl, int64_t * out, int n)
{
    if (!pl || !out || n < 0)
        return fail(SPMV_HIP_ERR_INVALID, "plan/out null");
    plan_numbers(*pl, out, n);
    return SPMV_HIP_OK;
}

void spmv_hip_f32_plan_destroy(spmv_hip_f32_plan * pl)
{
    if (!pl)
        return;
    if (pl->d_desc)
        (void) hipFree(pl->d_desc);
    delete pl;
}

// ---- Level 1 --------------------------------------------------------------------------------------------------------------------

int spmv_hip_upload_csr_f32values(spmv_hip_ctx * c, int32_t rows, int32_t cols, int32_t nnz, const int32_t * row_ptr,
                                  const int32_t * column_index, const double * value, int allow_rounding)
{
    return upload_float_tile(c, 7, "the fp32-value multiply runs on one device (a context of spmv_hip_create)", rows, cols, nnz, row_ptr, column_index,
                             value, true, allow_rounding, false);
}

} // extern "C"
