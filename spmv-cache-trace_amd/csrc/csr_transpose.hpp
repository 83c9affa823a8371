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
// The windows, the range's row_ptr in LDS, the walk over the entries in quads and the flush are window_walk.hpp, shared with
// csr_symmetric.hpp; the loop over a quad's entries below is this kernel's own.  The row of an entry is needed only to fetch
// x[i]: it is read through the cache, once per quad before any add, and again where a quad crosses into a later row.  Columns outside [0, cols) are skipped (the plan refused them; a caller who changes
// the columns afterwards gets the changed matrix's product, never an access outside x, y or LDS).
#pragma once

#include "window_walk.hpp"

namespace spmv {

// win: [ranges][stride] {first column, length} of the windows (length 0: unused; windows of a range do not overlap), stride <= KW
template <int KW>
__global__ __launch_bounds__(kWinBlock, 2) void csr_spmv_t_kernel(
    int rows, int cols, int R, const int32_t * __restrict__ p, const int32_t * __restrict__ col, const double * __restrict__ val,
    const double * __restrict__ x, double * __restrict__ y, const int2 * __restrict__ win, int stride, int slots)
{
    extern __shared__ double tr_lds[]; // [slots] window slots, then R + 1 ints of row_ptr
    int * rp = reinterpret_cast<int *>(tr_lds + slots);
    const int r0 = blockIdx.x * R;
    const int nr = min(R, rows - r0);
    RangeWindows<KW> ws;
    ws.load(win, stride, 0);
    range_prologue(tr_lds, ws.used, rp, p, r0, nr);
    const long long eb = rp[0], ee = rp[nr];

    for (long long q0 = (eb >> 2) + threadIdx.x; 4 * q0 < ee; q0 += (long long) kWinQuadsPerLane * kWinBlock) {
        v4i c[kWinQuadsPerLane];
        v2d a01[kWinQuadsPerLane], a23[kWinQuadsPerLane];
#pragma unroll
        for (int u = 0; u < kWinQuadsPerLane; ++u)
            load_quad(4 * (q0 + (long long) u * kWinBlock), eb, ee, col, val, c[u], a01[u], a23[u]);
        // the row of every quad's first entry and its x, before any add
        int rq[kWinQuadsPerLane];
        double xq[kWinQuadsPerLane];
#pragma unroll
        for (int u = 0; u < kWinQuadsPerLane; ++u) {
            const long long e0 = 4 * (q0 + (long long) u * kWinBlock);
            rq[u] = 0;
            xq[u] = 0.0;
            if (e0 >= ee)
                continue;
            rq[u] = quad_first_row(rp, nr, e0, eb);
            xq[u] = x[r0 + rq[u]];
        }
#pragma unroll
        for (int u = 0; u < kWinQuadsPerLane; ++u) {
            const long long e0 = 4 * (q0 + (long long) u * kWinBlock);
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
                const int slot = ws.slot_of(j);
                if (slot >= 0)
                    atomicAdd(tr_lds + slot, t);
                else
                    atomicAdd(y + j, t); // spilled: global_atomic_add_f64
            }
        }
    }
    __syncthreads();
    ws.flush(tr_lds, y);
}

} // namespace spmv
