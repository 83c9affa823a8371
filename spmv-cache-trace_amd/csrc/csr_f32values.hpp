// csr_f32values.hpp -- y += fl32(A) x (include/spmv_hip_f32values.h): the plain path of csr_wavetile_kernel with the value
// stream at 4 bytes per entry.  A wave per tile of up to 512 entries counted from a 4-aligned entry, four waves per workgroup,
// each with an LDS slice of its own; per lane and quad ONE load of four columns and ONE 16-byte load of four floats, both
// quads of a lane issued before anything waits; then the four x gathers, four widenings (v_cvt_f64_f32: exact, denormals
// included) and four fp64 multiplies, the rounded products parked in the slice and added up row by row by L lanes exactly as
// the plain tile does (tile_common.hpp: tile_row_sum, group_sum).  No atomics anywhere: a row is written by one lane.
// A row longer than a tile is a tile of its own: the whole wave in registers, 512 entries per step, one butterfly at the end.
//
// The tile is written once, f32_tile, over a COLUMN SOURCE: the only thing in which csr_f32values_kernel (32-bit columns,
// WideColumns below) and csr_compact_kernel (16-bit window codes, csr_compact.hpp) differ.  A source says where the columns
// of a quad come from -- load(o): the stored quad at offset o, columns(quad): its four column indices, at(k): the column at
// offset k (WideColumns here, CodeColumns<ONE> there).  A kernel's SOURCE (WideSource here, CompactSource there) counts from
// entry 0 and runs the two loops that read quads, quad_products and long_row_sum_f32, on the columns it chooses.
//
// The tile also has a VALUE TYPE V: float for the two multiplies of fl32(A), double for csr_compact_f64_kernel
// (y += A x on the caller's fp64 values beside the 16-bit codes, 10 bytes per entry).  Only ValueQuad<V> differs: how the four
// values of a quad are loaded and that a float is widened before it is multiplied.
//
// ... and a VECTOR ELEMENT TYPE T for x and y: double everywhere but in csr_compact_f32xy_kernel (csr_compact.hpp), whose x and
// y are floats.  Every x[...] and the row's old y are widened where they are read (exact), the products, the LDS slice and the
// sums stay fp64, and the one store of a row is (T)(y + sum): one rounding per row and call.  No load or store of x or y is
// wider than one element, so a float vector needs 4-byte alignment only.
#pragma once

#include "tile_common.hpp"

namespace spmv {

// descriptor {first row, first entry, meta, 0}; tile w ends where tile w + 1 starts (the table has tiles + 1 records)
// meta = longest row (stream tiles: <= 512) | log2(lanes per row) << 16 | fast << 25 | uniform << 26
constexpr int kF32Tile = 512;
constexpr int kF32TileRows = 64;

typedef float v4f __attribute__((ext_vector_type(4)));

// The four values of a quad as they are stored, V = float or double, and each of them as the fp64 factor of its product.
// Floats: one 16-byte load, widened where they are multiplied (v_cvt_f64_f32: exact).  Doubles: 32 bytes as TWO 16-byte loads,
// so the array need only be 16-byte aligned (a 4-aligned entry of it is then 16-, not 32-byte aligned); nothing is widened.
template <class V>
struct ValueQuad;
template <>
struct ValueQuad<float> {
    v4f q;
    static __device__ __forceinline__ ValueQuad load(const float * __restrict__ a) { return ValueQuad{*reinterpret_cast<const v4f *>(a)}; }
    __device__ __forceinline__ double x() const { return (double) q.x; }
    __device__ __forceinline__ double y() const { return (double) q.y; }
    __device__ __forceinline__ double z() const { return (double) q.z; }
    __device__ __forceinline__ double w() const { return (double) q.w; }
};
template <>
struct ValueQuad<double> {
    v2d lo, hi;
    static __device__ __forceinline__ ValueQuad load(const double * __restrict__ a)
    {
        const v2d * q = reinterpret_cast<const v2d *>(a);
        return ValueQuad{q[0], q[1]};
    }
    __device__ __forceinline__ double x() const { return lo.x; }
    __device__ __forceinline__ double y() const { return lo.y; }
    __device__ __forceinline__ double z() const { return hi.x; }
    __device__ __forceinline__ double w() const { return hi.y; }
};

// tile_products_wide's rules: lanes past the tile's end re-read its last quad; entries in front of the tile that share its
// first quad are multiplied and never read back.  cols and at count from the tile's first quad.  Every lane works out its
// columns (the lanes past the tile's end hold its last quad's); only the gathers are predicated.
template <int QUADS, bool X32, class Columns, class V, class T>
__device__ __forceinline__ void quad_products(double * prod, const Columns cols, const V * __restrict__ at,
                                              const T * __restrict__ x, int last, int lane)
{
    typename Columns::quad c[QUADS];
    ValueQuad<V> v[QUADS];
#pragma unroll
    for (int q = 0; q < QUADS; ++q) {
        int o = 256 * q + 4 * lane;
        o = o < last ? o : last;
        c[q] = cols.load(o);
        v[q] = ValueQuad<V>::load(at + o);
    }
#pragma unroll
    for (int q = 0; q < QUADS; ++q) {
        const int o = 256 * q + 4 * lane;
        const v4i j = cols.columns(c[q]);
        if (o <= last) {
            const double q0 = v[q].x() * gather_x<X32>(x, j.x);
            const double q1 = v[q].y() * gather_x<X32>(x, j.y);
            const double q2 = v[q].z() * gather_x<X32>(x, j.z);
            const double q3 = v[q].w() * gather_x<X32>(x, j.w);
            v2d * dst = reinterpret_cast<v2d *>(prod + o);
            dst[0] = v2d{q0, q1};
            dst[1] = v2d{q2, q3};
        }
    }
}

// long_row_sum (tile_common.hpp) over float values: the 4-aligned interior [ka, kz) in quads, two per lane and step in
// flight, four accumulators per lane; the up to three entries in front of ka and behind kz by single lanes.  Nothing is read
// outside [k0, k1).  cols and a count from entry 0.
template <bool X32, class Columns, class V, class T>
__device__ __forceinline__ double long_row_sum_f32(const Columns cols, const V * __restrict__ a, const T * __restrict__ x,
                                                   int k0, int k1, int lane)
{
    double z0 = 0.0, z1 = 0.0, z2 = 0.0, z3 = 0.0;
    const int ka = (k0 + 3) & ~3, kz = k1 & ~3;
    if (ka >= kz) {
        for (int k = k0 + lane; k < k1; k += kWave)
            z0 += (double) a[k] * (double) x[cols.at(k)];
        return group_sum<kWave>(z0);
    }
    if (lane < ka - k0)
        z0 += (double) a[k0 + lane] * (double) x[cols.at(k0 + lane)];
    if (lane >= 4 && lane - 4 < k1 - kz)
        z1 += (double) a[kz + lane - 4] * (double) x[cols.at(kz + lane - 4)];
    for (int o = ka + 4 * lane; o < kz; o += 2 * 4 * kWave) {
        const bool two = o + 4 * kWave < kz;
        const int o2 = two ? o + 4 * kWave : o;
        const typename Columns::quad ca = cols.load(o), cb = cols.load(o2);
        const ValueQuad<V> va = ValueQuad<V>::load(a + o), vb = ValueQuad<V>::load(a + o2);
        const v4i ja = cols.columns(ca), jb = cols.columns(cb);
        const double xa0 = gather_x<X32>(x, ja.x), xa1 = gather_x<X32>(x, ja.y), xa2 = gather_x<X32>(x, ja.z), xa3 = gather_x<X32>(x, ja.w);
        const double xb0 = gather_x<X32>(x, jb.x), xb1 = gather_x<X32>(x, jb.y), xb2 = gather_x<X32>(x, jb.z), xb3 = gather_x<X32>(x, jb.w);
        z0 += va.x() * xa0;
        z1 += va.y() * xa1;
        z2 += va.z() * xa2;
        z3 += va.w() * xa3;
        if (two) {
            z0 += vb.x() * xb0;
            z1 += vb.y() * xb1;
            z2 += vb.z() * xb2;
            z3 += vb.w() * xb3;
        }
    }
    return group_sum<kWave>((z0 + z1) + (z2 + z3));
}

// the caller's 32-bit columns: the stored quad is a 16-byte load and the column is the word
struct WideColumns {
    typedef v4i quad;
    const int32_t * __restrict__ j;
    __device__ __forceinline__ quad load(int o) const { return *reinterpret_cast<const v4i *>(j + o); }
    __device__ __forceinline__ v4i columns(quad c) const { return c; }
    __device__ __forceinline__ int at(int k) const { return j[k]; }
};

// csr_f32values_kernel's source: j[k] is the column of entry k
struct WideSource {
    const int32_t * __restrict__ j;
    __device__ __forceinline__ int at(int k) const { return j[k]; }
    // the products of the tile whose first quad starts at entry kb (at = a + kb)
    template <int QUADS, bool X32, class V, class T>
    __device__ __forceinline__ void products(double * prod, const V * __restrict__ at, const T * __restrict__ x, int kb,
                                             int last, int lane) const
    {
        quad_products<QUADS, X32>(prod, WideColumns{j + kb}, at, x, last, lane);
    }
    template <bool X32, class V, class T>
    __device__ __forceinline__ double long_row(const V * __restrict__ a, const T * __restrict__ x, int k0, int k1, int lane) const
    {
        return long_row_sum_f32<X32>(WideColumns{j}, a, x, k0, k1, lane);
    }
};

// same-wave LDS operations execute in order; the fences only pin the compiler
__device__ __forceinline__ void wave_lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// a tile's descriptor and where it ends, wave-uniform
struct F32Tile {
    int r0, k0, meta, w, r1, k1;
};
__device__ __forceinline__ F32Tile load_f32_tile(const int4 * __restrict__ desc, int w)
{
    const TilePair dp = load_tile_pair(desc, w);
    return F32Tile{__builtin_amdgcn_readfirstlane(dp.d0.x), __builtin_amdgcn_readfirstlane(dp.d0.y), __builtin_amdgcn_readfirstlane(dp.d0.z),
                   __builtin_amdgcn_readfirstlane(dp.d0.w), __builtin_amdgcn_readfirstlane(dp.d1.x), __builtin_amdgcn_readfirstlane(dp.d1.y)};
}

// What a tile does with a row's sum z: its EPILOGUE (include/spmv_hip_scaled.h).  Every row's sum is formed once, by one lane,
// so the epilogue is that lane's: old(i) is what it reads of row i beforehand (the stream tile asks early, beside its loads),
// store(i, old, z) the row's one store.
//     AccumulateRows            y[i] <- (T)(y[i] + z): every multiply that is y += A x
//     ScaledRows<T, false>      y_out[i] <- (T)(fl(alpha z) + fl(beta y_in[i])): two multiplies and an add, each rounded
//     ScaledRows<T, true>       y_out[i] <- (T) fl(alpha z): beta == 0, and y_in is not a load that is skipped but no load at all
// alpha and beta are kernel arguments: wave-uniform, in scalar registers.  y_in may be y_out (a row is read and written by the
// same lane) and is not __restrict__.
template <class T>
struct AccumulateRows {
    T * y;
    __device__ __forceinline__ double old(int i) const { return (double) y[i]; }
    __device__ __forceinline__ void store(int i, double yv, double z) const { y[i] = (T) (yv + z); }
};
template <class T, bool BETA0>
struct ScaledRows {
    double alpha, beta;
    const T * y_in;
    T * y_out;
    __device__ __forceinline__ double old(int i) const
    {
        if (BETA0)
            return 0.0;
        return (double) y_in[i];
    }
    __device__ __forceinline__ void store(int i, double yv, double z) const
    {
        if (BETA0)
            y_out[i] = (T) (alpha * z);
        else
            y_out[i] = (T) (alpha * z + beta * yv);
    }
};

// One tile by one wave; prod is the wave's LDS slice (kF32Tile + 4 doubles), src the kernel's column source, out the epilogue.
template <bool X32, class Source, class V, class T, class Rows>
__device__ __forceinline__ void f32_tile(double * prod, const F32Tile t, const Source src, const int32_t * __restrict__ p,
                                         const V * __restrict__ a, const T * __restrict__ x, const Rows out, int exact_order)
{
    constexpr int TILE = kF32Tile, QUADS = TILE / 256;
    const int lane = (int) __lane_id();
    const int r0 = t.r0, k0 = t.k0, meta = t.meta, k1 = t.k1;
    const int nrows = t.r1 - r0;
    const int kb = k0 & ~3;
    const int maxlen = meta & 0xFFFF;
    const int lanes_log2 = (meta >> kTileMetaLanesShift) & 0x7;

    if (meta & kTileMetaFast) {
        // ---- stream tile: rows << lanes_log2 <= 64, not empty, its last quad inside the arrays ----
        const int sub = lane >> lanes_log2;
        const int part = lane & ((1 << lanes_log2) - 1);
        const int rowi = sub < nrows ? sub : nrows - 1;
        int ps, pe;
        if (meta & kTileMetaUniform) { // all rows equally long: row_ptr is not read
            ps = k0 + rowi * maxlen;
            pe = ps + maxlen;
        } else {
            const int32_t * pt = p + r0;
            ps = pt[rowi];
            pe = pt[rowi + 1];
        }
        const double yv = out.old(r0 + rowi);
        const int last = (k1 - 1 - kb) & ~3;
        src.template products<QUADS, X32>(prod, a + kb, x, kb, last, lane);
        wave_lds_fence();
        const int s = ps - kb, e_row = pe - kb;
        double z;
        if (lanes_log2 == 0) { // one lane per row, left to right: the reference's order
            z = tile_row_sum<1>(prod, s, e_row, 0, maxlen);
        } else {
            const int trips = (maxlen + (1 << lanes_log2) - 1) >> lanes_log2;
            switch (lanes_log2) {
            case 1: z = tile_row_sum<2>(prod, s, e_row, part, trips); break;
            case 2: z = tile_row_sum<4>(prod, s, e_row, part, trips); break;
            case 3: z = tile_row_sum<8>(prod, s, e_row, part, trips); break;
            case 4: z = tile_row_sum<16>(prod, s, e_row, part, trips); break;
            case 5: z = tile_row_sum<32>(prod, s, e_row, part, trips); break;
            default: z = tile_row_sum<64>(prod, s, e_row, part, trips); break;
            }
        }
        if (sub < nrows && part == 0)
            out.store(r0 + sub, yv, z);
    } else if (k1 - kb <= TILE) {
        // ---- a tile of empty rows, or the tile whose last quad is not whole (the ragged end of the arrays): entry by entry,
        // one lane per row, left to right
        for (int k = k0 + lane; k < k1; k += kWave)
            prod[k - kb] = (double) a[k] * (double) x[src.at(k)];
        wave_lds_fence();
        for (int r = lane; r < nrows; r += kWave) {
            const int s = p[r0 + r] - kb, e_row = p[r0 + r + 1] - kb;
            double z = 0.0;
            for (int k = s; k < e_row; ++k)
                z += prod[k];
            out.store(r0 + r, out.old(r0 + r), z);
        }
    } else if (!exact_order) {
        // ---- one row longer than a tile: the whole wave, in registers ----
        const double z = src.template long_row<X32>(a, x, k0, k1, lane);
        if (lane == 0)
            out.store(r0, out.old(r0), z);
    } else {
        // ---- ... in the reference's order: lane 0 adds tiles of products left to right ----
        double z = 0.0;
        for (int t0 = k0; t0 < k1; t0 += TILE) {
            const int t1 = (t0 + TILE < k1) ? t0 + TILE : k1;
            for (int k = t0 + lane; k < t1; k += kWave)
                prod[k - t0] = (double) a[k] * (double) x[src.at(k)];
            wave_lds_fence();
            if (lane == 0)
                for (int k = 0; k < t1 - t0; ++k)
                    z += prod[k];
            wave_lds_fence();
        }
        if (lane == 0)
            out.store(r0, out.old(r0), z);
    }
}

template <bool X32>
__global__ __launch_bounds__(256, 8) void csr_f32values_kernel(int ntiles, const int4 * __restrict__ desc, const int32_t * __restrict__ p,
                                                               const int32_t * __restrict__ j, const float * __restrict__ a,
                                                               const double * __restrict__ x, double * y, int exact_order)
{
    __shared__ __attribute__((aligned(16))) double prod_all[4][kF32Tile + 4];
    const int wave = __builtin_amdgcn_readfirstlane((int) threadIdx.x >> 6);
    const int w = (int) blockIdx.x * 4 + wave;
    if (w >= ntiles)
        return; // whole wave leaves; no workgroup barrier in this kernel
    f32_tile<X32>(prod_all[wave], load_f32_tile(desc, w), WideSource{j}, p, a, x, AccumulateRows<double>{y}, exact_order);
}

// y_out <- alpha fl32(A) x + beta y_in (include/spmv_hip_scaled.h): the same tile with the scaled epilogue; BETA0: beta == 0
template <bool X32, bool BETA0>
__global__ __launch_bounds__(256, 8) void csr_f32values_scaled_kernel(int ntiles, const int4 * __restrict__ desc, const int32_t * __restrict__ p,
                                                                      const int32_t * __restrict__ j, const float * __restrict__ a,
                                                                      const double * __restrict__ x, double alpha, double beta,
                                                                      const double * y_in, double * y_out, int exact_order)
{
    __shared__ __attribute__((aligned(16))) double prod_all[4][kF32Tile + 4];
    const int wave = __builtin_amdgcn_readfirstlane((int) threadIdx.x >> 6);
    const int w = (int) blockIdx.x * 4 + wave;
    if (w >= ntiles)
        return; // whole wave leaves; no workgroup barrier in this kernel
    f32_tile<X32>(prod_all[wave], load_f32_tile(desc, w), WideSource{j}, p, a, x, ScaledRows<double, BETA0>{alpha, beta, y_in, y_out}, exact_order);
}

// The scaled multiplies where no tile runs -- alpha == 0, or a plan without tiles (rows, cols or nnz of zero): a lane per row,
//     y_out[i] <- (T)(fl(alpha * +0.0) + fl(beta y_in[i]))     ZTERM: alpha != 0, every row sum is +0.0
//     y_out[i] <- (T) fl(beta y_in[i])                         alpha == 0
// and without the beta term (and without a load of y_in) where BETA0; alpha == 0 and beta == 0 store +0.0.
template <class T, bool BETA0, bool ZTERM>
__global__ __launch_bounds__(256) void scaled_rows_only_kernel(int rows, double alpha, double beta, const T * y_in, T * y_out)
{
    const int i = (int) blockIdx.x * 256 + (int) threadIdx.x;
    if (i >= rows)
        return;
    double r = 0.0;
    if (ZTERM)
        r = alpha * 0.0;
    if (!BETA0)
        r = ZTERM ? r + beta * (double) y_in[i] : beta * (double) y_in[i];
    y_out[i] = (T) r;
}

// spmv_hip_narrow_values: out[k] = (float) value[k]; per workgroup {values that changed, finite values that became infinite,
// index of the first of either kind} and the largest relative change, reduced by the host (no atomics: the same numbers on
// every run)
struct NarrowCounts {
    long long inexact, overflow, first_inexact, first_overflow;
    double max_rel;
};

static __global__ __launch_bounds__(256) void narrow_values_kernel(long long n, const double * __restrict__ value, float * __restrict__ out,
                                                                   NarrowCounts * __restrict__ counts)
{
    __shared__ NarrowCounts part[256];
    NarrowCounts c{0, 0, -1, -1, 0.0};
    for (long long k = (long long) blockIdx.x * 256 + threadIdx.x; k < n; k += (long long) gridDim.x * 256) {
        const double v = value[k];
        const float f = (float) v;
        out[k] = f;
        const double back = (double) f;
        if (back != v && v == v) {
            if (__builtin_isinf(back)) {
                ++c.overflow;
                if (c.first_overflow < 0)
                    c.first_overflow = k;
            } else {
                ++c.inexact;
                if (c.first_inexact < 0)
                    c.first_inexact = k;
                const double rel = __builtin_fabs(back - v) / __builtin_fabs(v);
                c.max_rel = rel > c.max_rel ? rel : c.max_rel;
            }
        }
    }
    part[threadIdx.x] = c;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int) threadIdx.x < s) {
            NarrowCounts & m = part[threadIdx.x];
            const NarrowCounts o = part[threadIdx.x + s];
            m.inexact += o.inexact;
            m.overflow += o.overflow;
            m.first_inexact = m.first_inexact < 0 ? o.first_inexact : (o.first_inexact < 0 ? m.first_inexact : (m.first_inexact < o.first_inexact ? m.first_inexact : o.first_inexact));
            m.first_overflow = m.first_overflow < 0 ? o.first_overflow : (o.first_overflow < 0 ? m.first_overflow : (m.first_overflow < o.first_overflow ? m.first_overflow : o.first_overflow));
            m.max_rel = o.max_rel > m.max_rel ? o.max_rel : m.max_rel;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0)
        counts[blockIdx.x] = part[0];
}

} // namespace spmv
