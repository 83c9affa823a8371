// multivec.hip -- include/spmv_hip_multivec.h: Y += A X for up to 16 vectors of one CSR matrix.  The plan cuts wave tiles from
// row lengths on the host and splits k into passes of compiled widths; the kernels are csr_multivec.hpp.
#include "internal.hpp"
#include "csr_multivec.hpp"

#include <algorithm>
#include <new>

using namespace spmvi;

struct spmv_hip_mv_plan {
    int32_t rows = 0, cols = 0, nnz = 0;
    int k = 0;
    unsigned flags = 0;
    std::vector<int> pass_width; // vectors per pass (compiled widths), summing to k
    int ntiles = 0, nlong = 0;
    int2 * d_tiles = nullptr;     // [ntiles] {first row, rows | log2 lanes << 8}
    int32_t * d_long = nullptr;   // [nlong] rows of a workgroup each
    size_t device_bytes = 0;
};

namespace {

constexpr int kMvWidths[] = {8, 6, 4, 3, 2, 1}; // compiled K, widest first

bool k_ok(int k) { return k >= 1 && k <= SPMV_HIP_MV_MAX_VECTORS; }

int check_row_ptr(int32_t rows, int32_t cols, const int32_t * rp)
{
    if (rows < 0 || cols < 0 || !rp)
        return fail(SPMV_HIP_ERR_INVALID, "bad CSR arguments (rows or cols < 0, or row_ptr null)");
    if (int rc = check_row_ptr_order(rows, rp))
        return rc;
    if (rp[rows] > 0 && cols == 0)
        return fail(SPMV_HIP_ERR_INVALID, "entries in a matrix without columns");
    return SPMV_HIP_OK;
}

// log2 of the lanes a row of `len` entries asks for: the fewest that leave at most kMvEntriesPerLane entries per lane
int mv_lanes_for(long long len)
{
    int lg = 0;
    while (lg < 6 && ((long long) spmv::kMvEntriesPerLane << lg) < len)
        ++lg;
    return lg;
}

// Tiles of consecutive rows, from row lengths alone.  A row joins the open tile while (rows + 1) * lanes fits a wave, lanes
// being the most any of its rows asks for; a long row (non-exact plans) closes it and goes to the long list.  EXACT_ORDER: one
// lane per row, up to 64 rows and (beyond the first row) kMvExactTileEntries entries per tile.
void cut_tiles(int32_t rows, const int32_t * rp, bool exact, std::vector<int2> & tiles, std::vector<int32_t> & longs)
{
    int r0 = 0, n = 0, lg = 0;
    long long entries = 0;
    auto close = [&]() {
        if (n > 0)
            tiles.push_back(make_int2(r0, spmv::mv_tile_code(n, lg)));
        n = 0;
        lg = 0;
        entries = 0;
    };
    for (int32_t r = 0; r < rows; ++r) {
        const long long len = (long long) rp[r + 1] - rp[r];
        if (exact) {
            if (n > 0 && (n == spmv::kWave || entries + len > spmv::kMvExactTileEntries))
                close();
        } else {
            if (len > spmv::kMvLongRow) {
                close();
                longs.push_back(r);
                continue;
            }
            const int want = std::max(lg, mv_lanes_for(len));
            if (n > 0 && (long long) (n + 1) << want > spmv::kWave)
                close();
            lg = std::max(lg, mv_lanes_for(len));
        }
        if (n == 0)
            r0 = r;
        ++n;
        entries += len;
    }
    close();
}

int build_mv_plan(spmv_hip_mv_plan ** out, int32_t rows, int32_t cols, const int32_t * rp, int k, unsigned flags, hipStream_t s)
{
    spmv_hip_mv_plan * pl = new (std::nothrow) spmv_hip_mv_plan;
    if (!pl)
        return fail(SPMV_HIP_ERR_ALLOC, "plan allocation failed");
    pl->rows = rows;
    pl->cols = cols;
    pl->nnz = rp[rows];
    pl->k = k;
    pl->flags = flags;
    for (int left = k; left > 0;) {
        for (int w : kMvWidths)
            if (w <= left) {
                pl->pass_width.push_back(w);
                left -= w;
                break;
            }
    }
    std::vector<int2> tiles;
    std::vector<int32_t> longs;
    try {
        cut_tiles(rows, rp, (flags & SPMV_HIP_FLAG_EXACT_ORDER) != 0, tiles, longs);
    } catch (std::bad_alloc const &) {
        delete pl;
        return fail(SPMV_HIP_ERR_ALLOC, "tile list");
    }
    pl->ntiles = (int) tiles.size();
    pl->nlong = (int) longs.size();
    hipError_t e = hipSuccess;
    if (!tiles.empty()) {
        e = hipMalloc((void **) &pl->d_tiles, tiles.size() * sizeof(int2));
        if (e == hipSuccess)
            e = hipMemcpyAsync(pl->d_tiles, tiles.data(), tiles.size() * sizeof(int2), hipMemcpyHostToDevice, s);
        pl->device_bytes += tiles.size() * sizeof(int2);
    }
    if (e == hipSuccess && !longs.empty()) {
        e = hipMalloc((void **) &pl->d_long, longs.size() * sizeof(int32_t));
        if (e == hipSuccess)
            e = hipMemcpyAsync(pl->d_long, longs.data(), longs.size() * sizeof(int32_t), hipMemcpyHostToDevice, s);
        pl->device_bytes += longs.size() * sizeof(int32_t);
    }
    if (e == hipSuccess && (pl->ntiles > 0 || pl->nlong > 0)) // (an empty matrix needs no device: its plan is argument checks only)
        e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        spmv_hip_mv_plan_destroy(pl);
        return fail_hip(e, "multivector plan: tile list");
    }
    *out = pl;
    return SPMV_HIP_OK;
}

template <int K, bool VEC>
void launch_pass(const spmv_hip_mv_plan * pl, const int32_t * p, const int32_t * j, const double * a, const double * X, long long ldx,
                 double * Y, long long ldy, hipStream_t s)
{
    if (pl->ntiles > 0)
        hipLaunchKernelGGL((spmv::csr_mv_tile_kernel<K, VEC>), dim3((unsigned) grid_for(pl->ntiles, spmv::kMvWaves, 8 * cu_count())),
                           dim3(spmv::kMvBlock), 0, s, pl->ntiles, pl->d_tiles, p, j, a, X, ldx, Y, ldy);
    if (pl->nlong > 0)
        hipLaunchKernelGGL((spmv::csr_mv_long_kernel<K, VEC>), dim3((unsigned) pl->nlong), dim3(spmv::kMvLongBlock), 0, s, pl->d_long, p, j,
                           a, X, ldx, Y, ldy);
}

template <int K>
void launch_width(const spmv_hip_mv_plan * pl, bool vec, const int32_t * p, const int32_t * j, const double * a, const double * X,
                  long long ldx, double * Y, long long ldy, hipStream_t s)
{
    if (vec)
        launch_pass<K, true>(pl, p, j, a, X, ldx, Y, ldy, s);
    else
        launch_pass<K, false>(pl, p, j, a, X, ldx, Y, ldy, s);
}

} // namespace

extern "C" {

int spmv_hip_mv_plan_csr(spmv_hip_mv_plan ** plan, int32_t rows, int32_t cols, const int32_t * host_row_ptr, int k, unsigned flags,
                         void * stream)
{
    if (!plan)
        return fail(SPMV_HIP_ERR_INVALID, "plan is null");
    *plan = nullptr;
    if (!k_ok(k))
        return fail(SPMV_HIP_ERR_INVALID, "k must be 1 .. 16");
    if (flags & ~SPMV_HIP_FLAG_EXACT_ORDER)
        return fail(SPMV_HIP_ERR_INVALID, "flags: only SPMV_HIP_FLAG_EXACT_ORDER is known to the multivector plan");
    int rc = check_row_ptr(rows, cols, host_row_ptr);
    if (rc != 0)
        return rc;
    return build_mv_plan(plan, rows, cols, host_row_ptr, k, flags, static_cast<hipStream_t>(stream));
}

int spmv_hip_csr_spmm(const spmv_hip_mv_plan * pl, const int32_t * d_row_ptr, const int32_t * d_column_index, const double * d_value,
                      const double * d_X, int64_t ldx, double * d_Y, int64_t ldy, void * stream)
{
    if (!pl)
        return fail(SPMV_HIP_ERR_INVALID, "plan is null");
    if (!d_row_ptr || !d_column_index || !d_value || !d_X || !d_Y)
        return fail(SPMV_HIP_ERR_INVALID, "null device pointer");
    if (ldx < pl->k || ldy < pl->k)
        return fail(SPMV_HIP_ERR_INVALID, "ldx and ldy must be at least k");
    if ((const void *) d_X == (const void *) d_Y)
        return fail(SPMV_HIP_ERR_INVALID, "d_X and d_Y must be different arrays");
    if (!aligned16(d_column_index) || !aligned16(d_value))
        return fail(SPMV_HIP_ERR_ALIGN, "column / value arrays must be 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(d_X) | reinterpret_cast<uintptr_t>(d_Y)) & 7u)
        return fail(SPMV_HIP_ERR_ALIGN, "X and Y must be 8-byte aligned");
    if (pl->rows == 0 || pl->nnz == 0)
        return SPMV_HIP_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int c0 = 0;
    for (int w : pl->pass_width) {
        const double * X = d_X + c0;
        double * Y = d_Y + c0;
        // 16-byte loads of X and Y rows when every row start is 16-byte aligned
        const bool vec = ldx % 2 == 0 && ldy % 2 == 0 && aligned16(X) && aligned16(Y);
        switch (w) {
        case 8: launch_width<8>(pl, vec, d_row_ptr, d_column_index, d_value, X, ldx, Y, ldy, s); break;
        case 6: launch_width<6>(pl, vec, d_row_ptr, d_column_index, d_value, X, ldx, Y, ldy, s); break;
        case 4: launch_width<4>(pl, vec, d_row_ptr, d_column_index, d_value, X, ldx, Y, ldy, s); break;
        case 3: launch_width<3>(pl, vec, d_row_ptr, d_column_index, d_value, X, ldx, Y, ldy, s); break;
        case 2: launch_width<2>(pl, vec, d_row_ptr, d_column_index, d_value, X, ldx, Y, ldy, s); break;
        default: launch_width<1>(pl, vec, d_row_ptr, d_column_index, d_value, X, ldx, Y, ldy, s); break;
        }
        HIP_TRY(hipGetLastError());
        c0 += w;
    }
    return SPMV_HIP_OK;
}

int spmv_hip_mv_plan_info(const spmv_hip_mv_plan * pl, int64_t * out, int n)
{
    if (!pl || !out || n < 0)
        return fail(SPMV_HIP_ERR_INVALID, "plan/out null");
    const long long passes = (long long) pl->pass_width.size();
    const int64_t v[11] = {pl->rows,
                           pl->cols,
                           pl->k,
                           passes,
                           pl->ntiles,
                           pl->nlong,
                           passes * (12LL * pl->nnz + 4LL * (pl->rows + 1LL)) + 8LL * pl->k * pl->cols + 16LL * pl->k * pl->rows,
                           (int64_t) pl->device_bytes,
                           pl->nnz,
                           (int64_t) pl->flags,
                           pl->pass_width.empty() ? 0 : pl->pass_width.front()};
    for (int i = 0; i < n && i < 11; ++i)
        out[i] = v[i];
    return SPMV_HIP_OK;
}

void spmv_hip_mv_plan_destroy(spmv_hip_mv_plan * pl)
{
    if (!pl)
        return;
    if (pl->d_tiles)
        (void) hipFree(pl->d_tiles);
    if (pl->d_long)
        (void) hipFree(pl->d_long);
    delete pl;
}

// ---- Level 1 --------------------------------------------------------------------------------------------------------------------

namespace {

int block_state(spmv_hip_ctx * c, int k)
{
    if (!c)
        return fail(SPMV_HIP_ERR_INVALID, "ctx is null");
    if (!k_ok(k))
        return fail(SPMV_HIP_ERR_INVALID, "k must be 1 .. 16");
    if (c->multi)
        return fail(SPMV_HIP_ERR_STATE, "block runs need a context of spmv_hip_create (one device)");
    if (c->format != 1)
        return fail(SPMV_HIP_ERR_STATE, "block runs need a matrix uploaded with spmv_hip_upload_csr");
    return SPMV_HIP_OK;
}

// X and Y of width k (a new k: new arrays, Y zero, X unset)
int block_arrays(spmv_hip_ctx * c, int k)
{
    if (c->block_k == k && c->d_bx && c->d_by)
        return SPMV_HIP_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->d_bx) (void) hipFree(c->d_bx);
    if (c->d_by) (void) hipFree(c->d_by);
    c->d_bx = c->d_by = nullptr;
    c->block_k = 0;
    c->block_x_set = false;
    c->block_bytes = 0;
    if (c->mv_plan) {
        spmv_hip_mv_plan_destroy(c->mv_plan);
        c->mv_plan = nullptr;
    }
    const size_t xb = (size_t) c->cols * k * sizeof(double) + 64, yb = (size_t) c->rows * k * sizeof(double) + 64;
    hipError_t e = hipMalloc((void **) &c->d_bx, xb);
    if (e == hipSuccess)
        e = hipMalloc((void **) &c->d_by, yb);
    if (e == hipSuccess)
        e = hipMemsetAsync(c->d_by, 0, yb, c->stream);
    if (e == hipSuccess)
        e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        if (c->d_bx) (void) hipFree(c->d_bx);
        if (c->d_by) (void) hipFree(c->d_by);
        c->d_bx = c->d_by = nullptr;
        return fail_hip(e, "block vectors");
    }
    c->block_k = k;
    c->block_bytes = xb + yb;
    return SPMV_HIP_OK;
}

} // namespace

int spmv_hip_set_block_x(spmv_hip_ctx * c, int k, const double * X)
{
    int rc = block_state(c, k);
    if (rc != 0)
        return rc;
    if (!X)
        return fail(SPMV_HIP_ERR_INVALID, "X is null");
    if ((rc = block_arrays(c, k)) != 0)
        return rc;
    if (c->cols > 0)
        HIP_TRY(hipMemcpyAsync(c->d_bx, X, (size_t) c->cols * k * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->block_x_set = true;
    return SPMV_HIP_OK;
}

int spmv_hip_set_block_y(spmv_hip_ctx * c, int k, const double * Y)
{
    int rc = block_state(c, k);
    if (rc != 0)
        return rc;
    if (!Y)
        return fail(SPMV_HIP_ERR_INVALID, "Y is null");
    if ((rc = block_arrays(c, k)) != 0)
        return rc;
    if (c->rows > 0)
        HIP_TRY(hipMemcpyAsync(c->d_by, Y, (size_t) c->rows * k * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SPMV_HIP_OK;
}

int spmv_hip_get_block_y(spmv_hip_ctx * c, int k, double * Y)
{
    int rc = block_state(c, k);
    if (rc != 0)
        return rc;
    if (!Y)
        return fail(SPMV_HIP_ERR_INVALID, "Y is null");
    if (c->block_k != k || !c->d_by)
        return fail(SPMV_HIP_ERR_STATE, "no block Y of this k (set_block_x / set_block_y first)");
    HIP_TRY(hipSetDevice(c->device));
    if (c->rows > 0)
        HIP_TRY(hipMemcpyAsync(Y, c->d_by, (size_t) c->rows * k * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SPMV_HIP_OK;
}

int spmv_hip_run_block(spmv_hip_ctx * c)
{
    if (!c)
        return fail(SPMV_HIP_ERR_INVALID, "ctx is null");
    if (c->multi)
        return fail(SPMV_HIP_ERR_STATE, "block runs need a context of spmv_hip_create (one device)");
    if (c->format != 1)
        return fail(SPMV_HIP_ERR_STATE, "block runs need a matrix uploaded with spmv_hip_upload_csr");
    if (!c->block_x_set)
        return fail(SPMV_HIP_ERR_STATE, "no block X (spmv_hip_set_block_x first)");
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if (!c->mv_plan) {
        // row_ptr comes back once: the context keeps no host copy
        std::vector<int32_t> rp;
        try {
            rp.resize((size_t) c->rows + 1);
        } catch (std::bad_alloc const &) {
            return fail(SPMV_HIP_ERR_ALLOC, "host copy of row_ptr");
        }
        HIP_TRY(hipMemcpyAsync(rp.data(), c->d_ptr, rp.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if ((rc = spmv_hip_mv_plan_csr(&c->mv_plan, c->rows, c->cols, rp.data(), c->block_k, c->flags & SPMV_HIP_FLAG_EXACT_ORDER,
                                       c->stream)) != 0)
            return rc;
    }
    const bool timed = !(c->flags & SPMV_HIP_FLAG_NO_RUN_EVENTS);
    if (timed)
        HIP_TRY(hipEventRecord(c->ev0, c->stream));
    if ((rc = spmv_hip_csr_spmm(c->mv_plan, c->d_ptr, c->d_col, c->d_val, c->d_bx, c->block_k, c->d_by, c->block_k, c->stream)) != 0)
        return rc;
    if (timed) {
        HIP_TRY(hipEventRecord(c->ev1, c->stream));
        c->timed = true;
    }
    return SPMV_HIP_OK;
}

} // extern "C"
