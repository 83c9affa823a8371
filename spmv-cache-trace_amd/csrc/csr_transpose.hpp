// csr_transpose.hpp -- y += A' x from the CSR arrays of A as they are (include/spmv_hip_transpose.h): the scatter half of
// csr_symmetric.hpp alone, for a general and possibly rectangular matrix.  x has `rows` entries, y has `cols`.
//
// One workgroup per range of R consecutive rows.  The workgroup keeps, in LDS, up to KW windows of y that cover the columns
// its entries hit (chosen by the plan from the columns; none is implied: the range's own diagonal block is a window only where
// the columns say so).  For a stored entry (i, j, a) of its rows, a * x[i] is added to the slot of j with ds_add_f64 -- or, when
// no window covers j (a "spilled" entry), straight into y[j] with global_atomic_add_f64.  After a barrier every window slot that
// is not zero is added to y with global_atomic_add_f64, consecutive lanes on consecutive addresses.  Every write of y is
// atomic and the order in which the partial sums meet is not fixed: y is not reproducible bit for bit.
//
// Entries are walked in quads: a lane loads four consecutive column indices (16 B) and values (2 x 16 B) at a quad-aligned entry,
// exactly as they lie in the caller's arrays.  The row of an entry is needed only to fetch x[i]: the row of a quad's first entry
// comes from a binary search in the range's row_ptr, kept in LDS, and x[i] is read through the cache (once per quad, and again
// where a quad crosses into a later row).  Columns outside [0, cols) are skipped (the plan refused them; a caller who changes
// the columns afterwards gets the changed matrix's product, never an access outside x, y or LDS).
#pragma once

#include "tile_common.hpp"

namespace spmv {

constexpr int kTrBlock = 512;      // threads per workgroup
constexpr int kTrMaxWindows = 8;   // windows of y per range, at most
constexpr int kTrQuadsPerLane = 2; // quads whose loads are in flight together per lane

template <int KW>
__device__ __forceinline__ int tr_slot(int j, const int (&wb)[KW], const int (&wl)[KW], const int (&wo)[KW])
{
    int slot = -1;
#pragma unroll
    for (int w = 0; w < KW; ++w)
        if ((unsigned) (j - wb[w]) < (unsigned) wl[w])
            slot = wo[w] + (j - wb[w]);
    return slot;
}

// win: [ranges][stride] {first column, length} of the windows (length 0: unused; windows of a range do not overlap), stride <= KW
template <int KW>
__global__ __launch_bounds__(kTrBlock, 2) void csr_spmv_t_kernel(
    int rows, int cols, int R, const int32_t * __restrict__ p, const int32_t * __restrict__ col, const double * __restrict__ val,
    const double * __restrict__ x, double * __restrict__ y, const int2 * __restrict__ win, int stride, int slots)
{
    extern __shared__ double tr_lds[]; // [slots] window slots, then R + 1 ints of row_ptr
    int * rp = reinterpret_cast<int *>(tr_lds + slots);
    const int r0 = blockIdx.x * R;
    const int nr = min(R, rows - r0);
    int wb[KW], wl[KW], wo[KW];
    int off = 0;
#pragma unroll
    for (int w = 0; w < KW; ++w) {
        const int2 d = w < stride ? win[(size_t) blockIdx.x * stride + w] : make_int2(0, 0);
        wb[w] = d.x;
        wl[w] = d.y;
        wo[w] = off;
        off += d.y;
    }
    const int used = off; // slots of this range (<= slots)
    for (int t = threadIdx.x; t < used; t += kTrBlock)
        tr_lds[t] = 0.0;
    for (int t = threadIdx.x; t <= nr; t += kTrBlock)
        rp[t] = p[r0 + t];
    __syncthreads();
    const long long eb = rp[0], ee = rp[nr];

    for (long long q0 = (eb >> 2) + threadIdx.x; 4 * q0 < ee; q0 += (long long) kTrQuadsPerLane * kTrBlock) {
        v4i c[kTrQuadsPerLane];
        v2d a01[kTrQuadsPerLane], a23[kTrQuadsPerLane];
#pragma unroll
        for (int u = 0; u < kTrQuadsPerLane; ++u) {
            const long long e0 = 4 * (q0 + (long long) u * kTrBlock);
            if (e0 >= eb && e0 + 3 < ee) {
                c[u] = __builtin_nontemporal_load(reinterpret_cast<const v4i *>(col + e0));
                a01[u] = __builtin_nontemporal_load(reinterpret_cast<const v2d *>(val + e0));
                a23[u] = __builtin_nontemporal_load(reinterpret_cast<const v2d *>(val + e0 + 2));
            } else {
                // the range's first and last quads: only the entries inside [eb, ee) are read; the others get column -1 (skipped)
                double a[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const bool in = e0 + k >= eb && e0 + k < ee;
                    c[u][k] = in ? col[e0 + k] : -1;
                    a[k] = in ? val[e0 + k] : 0.0;
                }
                a01[u] = v2d{a[0], a[1]};
                a23[u] = v2d{a[2], a[3]};
            }
        }
        // the row of every quad's first entry inside the range (the last r with rp[r] <= max(e0, eb)) and its x, before any add
        int rq[kTrQuadsPerLane];
        double xq[kTrQuadsPerLane];
#pragma unroll
        for (int u = 0; u < kTrQuadsPerLane; ++u) {
            const long long e0 = 4 * (q0 + (long long) u * kTrBlock);
            rq[u] = 0;
            xq[u] = 0.0;
            if (e0 >= ee)
                continue;
            const long long ef = e0 > eb ? e0 : eb;
            int lo = 0, hi = nr;
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (rp[mid] <= ef)
                    lo = mid;
                else
                    hi = mid;
            }
            rq[u] = lo;
            xq[u] = x[r0 + lo];
        }
#pragma unroll
        for (int u = 0; u < kTrQuadsPerLane; ++u) {
            const long long e0 = 4 * (q0 + (long long) u * kTrBlock);
            if (e0 >= ee)
                continue;
            int r = rq[u];
            double xi = xq[u];
            const double av[4] = {a01[u][0], a01[u][1], a23[u][0], a23[u][1]};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int j = c[u][k];
                if ((unsigned) j >= (unsigned) cols)
                    continue; // outside the range (or a bad column)
                const long long e = e0 + k;
                if (rp[r + 1] <= e) { // the quad crosses into a later row (e < ee, so r stays below nr)
                    do
                        ++r;
                    while (rp[r + 1] <= e);
                    xi = x[r0 + r];
                }
                const double t = av[k] * xi;
                const int slot = tr_slot<KW>(j, wb, wl, wo);
                if (slot >= 0)
                    atomicAdd(tr_lds + slot, t);
                else
                    atomicAdd(y + j, t); // spilled: global_atomic_add_f64
            }
        }
    }
    __syncthreads();
    // flush: every window, lanes on consecutive addresses, zero slots skipped
#pragma unroll
    for (int w = 0; w < KW; ++w)
        for (int t = threadIdx.x; t < wl[w]; t += kTrBlock) {
            const double v = tr_lds[wo[w] + t];
            if (v != 0.0)
                atomicAdd(y + wb[w] + t, v);
        }
}

} // namespace spmv
