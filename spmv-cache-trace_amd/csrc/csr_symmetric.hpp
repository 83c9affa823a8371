// csr_symmetric.hpp -- y += (T + T' - diag(T)) x  (symmetric) or  y += (T - T') x  (skew-symmetric) from the STORED
// TRIANGLE T of a matrix in CSR: every stored value is read once and used twice (include/spmv_hip_symmetric.h).
//
// One workgroup per range of R consecutive rows (the plan's "ranges").  The workgroup keeps, in LDS, a window of y for its own
// rows and up to KW more windows that cover the y positions its TRANSPOSED products hit (chosen by the plan from the columns:
// the previous line and the previous plane of a mesh in natural order, the band of an RCM ordering).  For a stored entry
// (i, j, a) of its rows:
//   1. a * x[j] goes to row i's sum, which is added to the own window's slot of i;
//   2. if j != i, sign * a * x[i] is added to the slot of j with ds_add_f64 -- or, when no window covers j (a "spilled" entry),
//      straight into y[j] with global_atomic_add_f64.
// After a barrier every window slot that is not zero is added to y with global_atomic_add_f64, consecutive lanes on consecutive
// addresses.  Every write of y is atomic: a later range's windows cover an earlier range's rows.  The order in which the partial
// sums meet is not fixed, so y is not reproducible bit for bit (like the column panels of the general kernel).
//
// The windows, the range's row_ptr in LDS, the walk over the entries in quads and the flush are window_walk.hpp, shared with
// csr_transpose.hpp; the loop over a quad's entries below is this kernel's own.  Columns outside [0, rows) are skipped (the plan
// refused them; a caller who changes the columns afterwards gets a wrong y, never an access outside x, y or LDS).
#pragma once

#include "window_walk.hpp"

namespace spmv {

// win: [ranges][stride] {first row, length} of the extra windows (length 0: unused), stride <= KW
template <int KW>
__global__ __launch_bounds__(kWinBlock, 2) void csr_symv_kernel(
    int rows, int R, const int32_t * __restrict__ p, const int32_t * __restrict__ col, const double * __restrict__ val,
    const double * __restrict__ x, double * __restrict__ y, const int2 * __restrict__ win, int stride, int slots, double tsign)
{
    extern __shared__ double sym_lds[]; // [slots] window slots (own rows first), then R + 1 ints of row_ptr
    int * rp = reinterpret_cast<int *>(sym_lds + slots);
    const int r0 = blockIdx.x * R;
    const int nr = min(R, rows - r0);
    RangeWindows<KW> ws;
    ws.load(win, stride, nr);
    range_prologue(sym_lds, ws.used, rp, p, r0, nr);
    const long long eb = rp[0], ee = rp[nr];

    for (long long q0 = (eb >> 2) + threadIdx.x; 4 * q0 < ee; q0 += (long long) kWinQuadsPerLane * kWinBlock) {
        v4i c[kWinQuadsPerLane];
        v2d a01[kWinQuadsPerLane], a23[kWinQuadsPerLane];
#pragma unroll
        for (int u = 0; u < kWinQuadsPerLane; ++u)
            load_quad(4 * (q0 + (long long) u * kWinBlock), eb, ee, col, val, c[u], a01[u], a23[u]);
#pragma unroll
        for (int u = 0; u < kWinQuadsPerLane; ++u) {
            const long long e0 = 4 * (q0 + (long long) u * kWinBlock);
            if (e0 >= ee)
                continue;
            int r = quad_first_row(rp, nr, e0, eb);
            double sum = 0.0;
            const double av[4] = {a01[u][0], a01[u][1], a23[u][0], a23[u][1]};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int j = c[u][k];
                if ((unsigned) j >= (unsigned) rows)
                    continue; // outside the range (or a bad column)
                const long long e = e0 + k;
                if (rp[r + 1] <= e) { // the quad crosses into a later row: hand over the finished sum
                    if (sum != 0.0)
                        atomicAdd(sym_lds + r, sum);
                    sum = 0.0;
                    do
                        ++r;
                    while (rp[r + 1] <= e);
                }
                const double a = av[k];
                sum += a * x[j];
                const int i = r0 + r;
                if (j != i) {
                    const double t = (tsign * a) * x[i];
                    const int slot = ws.slot_of(j, (unsigned) (j - r0) < (unsigned) nr ? j - r0 : -1);
                    if (slot >= 0)
                        atomicAdd(sym_lds + slot, t);
                    else
                        atomicAdd(y + j, t); // spilled: global_atomic_add_f64
                }
            }
            if (sum != 0.0)
                atomicAdd(sym_lds + r, sum);
        }
    }
    __syncthreads();
    // flush: own rows, then every extra window
    for (int t = threadIdx.x; t < nr; t += kWinBlock) {
        const double v = sym_lds[t];
        if (v != 0.0)
            atomicAdd(y + r0 + t, v);
    }
    ws.flush(sym_lds, y);
}

} // namespace spmv
