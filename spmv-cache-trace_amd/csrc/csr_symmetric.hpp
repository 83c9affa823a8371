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
// Entries are walked in quads: a lane loads four consecutive column indices (16 B) and values (2 x 16 B) at a quad-aligned entry,
// exactly as they lie in the caller's arrays; the row of its first entry comes from a binary search in the range's row_ptr, kept
// in LDS.  Columns outside [0, rows) are skipped (the plan refused them; a caller who changes the columns afterwards gets a
// wrong y, never an access outside x, y or LDS).
#pragma once

#include "tile_common.hpp"

namespace spmv {

constexpr int kSymBlock = 512;      // threads per workgroup
constexpr int kSymMaxWindows = 8;   // the own window + at most 7 more
constexpr int kSymQuadsPerLane = 2; // quads whose loads are in flight together per lane

template <int KW>
__device__ __forceinline__ int sym_slot(int j, int r0, int nr, const int (&wb)[KW > 0 ? KW : 1], const int (&wl)[KW > 0 ? KW : 1],
                                        const int (&wo)[KW > 0 ? KW : 1])
{
    int slot = ((unsigned) (j - r0) < (unsigned) nr) ? j - r0 : -1;
#pragma unroll
    for (int w = 0; w < KW; ++w)
        if (slot < 0 && (unsigned) (j - wb[w]) < (unsigned) wl[w])
            slot = wo[w] + (j - wb[w]);
    return slot;
}

// win: [ranges][stride] {first row, length} of the extra windows (length 0: unused), stride <= KW
template <int KW>
__global__ __launch_bounds__(kSymBlock, 2) void csr_symv_kernel(
    int rows, int R, const int32_t * __restrict__ p, const int32_t * __restrict__ col, const double * __restrict__ val,
    const double * __restrict__ x, double * __restrict__ y, const int2 * __restrict__ win, int stride, int slots, double tsign)
{
    extern __shared__ double sym_lds[]; // [slots] window slots (own rows first), then R + 1 ints of row_ptr
    int * rp = reinterpret_cast<int *>(sym_lds + slots);
    const int r0 = blockIdx.x * R;
    const int nr = min(R, rows - r0);
    constexpr int KA = KW > 0 ? KW : 1;
    int wb[KA], wl[KA], wo[KA];
    int off = nr;
#pragma unroll
    for (int w = 0; w < KW; ++w) {
        const int2 d = w < stride ? win[(size_t) blockIdx.x * stride + w] : make_int2(0, 0);
        wb[w] = d.x;
        wl[w] = d.y;
        wo[w] = off;
        off += d.y;
    }
    if (KW == 0)
        wb[0] = wl[0] = wo[0] = 0;
    const int used = off; // slots of this range (<= slots)
    for (int t = threadIdx.x; t < used; t += kSymBlock)
        sym_lds[t] = 0.0;
    for (int t = threadIdx.x; t <= nr; t += kSymBlock)
        rp[t] = p[r0 + t];
    __syncthreads();
    const long long eb = rp[0], ee = rp[nr];

    for (long long q0 = (eb >> 2) + threadIdx.x; 4 * q0 < ee; q0 += (long long) kSymQuadsPerLane * kSymBlock) {
        v4i c[kSymQuadsPerLane];
        v2d a01[kSymQuadsPerLane], a23[kSymQuadsPerLane];
#pragma unroll
        for (int u = 0; u < kSymQuadsPerLane; ++u) {
            const long long e0 = 4 * (q0 + (long long) u * kSymBlock);
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
#pragma unroll
        for (int u = 0; u < kSymQuadsPerLane; ++u) {
            const long long e0 = 4 * (q0 + (long long) u * kSymBlock);
            if (e0 >= ee)
                continue;
            // the row of the quad's first entry inside the range: the last r with rp[r] <= max(e0, eb)
            const long long ef = e0 > eb ? e0 : eb;
            int lo = 0, hi = nr;
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (rp[mid] <= ef)
                    lo = mid;
                else
                    hi = mid;
            }
            int r = lo;
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
                    const int slot = sym_slot<KW>(j, r0, nr, wb, wl, wo);
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
    // flush: own rows, then every extra window; lanes on consecutive addresses, zero slots skipped
    for (int t = threadIdx.x; t < nr; t += kSymBlock) {
        const double v = sym_lds[t];
        if (v != 0.0)
            atomicAdd(y + r0 + t, v);
    }
#pragma unroll
    for (int w = 0; w < KW; ++w)
        for (int t = threadIdx.x; t < wl[w]; t += kSymBlock) {
            const double v = sym_lds[wo[w] + t];
            if (v != 0.0)
                atomicAdd(y + wb[w] + t, v);
        }
}

} // namespace spmv
