// window_walk.hpp -- what csr_symmetric.hpp and csr_transpose.hpp share on the device: one workgroup per range of R consecutive
// rows, the range's windows of y in LDS (chosen by window_plan.hpp), its row_ptr behind them, and the entries walked in quads.
//
// A lane loads four consecutive column indices (16 B) and values (2 x 16 B) at a quad-aligned entry, exactly as they lie in the
// caller's arrays; the row of a quad's first entry comes from a binary search in the range's row_ptr.  A product goes to the
// LDS slot of its target with ds_add_f64, or -- when no window covers the target (a "spilled" entry) -- straight into y with
// global_atomic_add_f64.  After a barrier every window slot that is not zero is added to y with global_atomic_add_f64,
// consecutive lanes on consecutive addresses.  Every write of y is atomic and the order in which the partial sums meet is not
// fixed: y is not reproducible bit for bit.  What a kernel does with an entry is its own inner loop.
#pragma once

#include "tile_common.hpp"

namespace spmv {

constexpr int kWinBlock = 512;      // threads per workgroup
constexpr int kWinMaxWindows = 8;   // windows of y per range, at most (the symmetric kernel's own rows included)
constexpr int kWinQuadsPerLane = 2; // quads whose loads are in flight together per lane

// The windows of one range: {first target, length, first LDS slot}, uniform over the workgroup.  KW = 0: none.
template <int KW>
struct RangeWindows {
    static constexpr int KA = KW > 0 ? KW : 1;
    int wb[KA], wl[KA], wo[KA];
    int used; // slots of this range, first_slot included (<= the plan's slots)

    // win: [ranges][stride] {first target, length} (length 0: unused), stride <= KW; the windows take the slots from first_slot on
    __device__ __forceinline__ void load(const int2 * __restrict__ win, int stride, int first_slot)
    {
        wb[0] = wl[0] = wo[0] = 0;
        int off = first_slot;
#pragma unroll
        for (int w = 0; w < KW; ++w) {
            const int2 d = w < stride ? win[(size_t) blockIdx.x * stride + w] : make_int2(0, 0);
            wb[w] = d.x;
            wl[w] = d.y;
            wo[w] = off;
            off += d.y;
        }
        used = off;
    }

    // the slot of target j after the caller's own window: `slot` where that is one (>= 0), else the first window that covers j,
    // else -1
    __device__ __forceinline__ int slot_of(int j, int slot) const
    {
#pragma unroll
        for (int w = 0; w < KW; ++w)
            if (slot < 0 && (unsigned) (j - wb[w]) < (unsigned) wl[w])
                slot = wo[w] + (j - wb[w]);
        return slot;
    }

    // the slot of target j where the windows do not overlap and there is no other: no test of what was found so far.  (The form
    // above in its place costs the transposed kernel 1 to 3 % of its time: profiles/window_walk_ab.log.)
    __device__ __forceinline__ int slot_of(int j) const
    {
        int slot = -1;
#pragma unroll
        for (int w = 0; w < KW; ++w)
            if ((unsigned) (j - wb[w]) < (unsigned) wl[w])
                slot = wo[w] + (j - wb[w]);
        return slot;
    }

    // every window to y, lanes on consecutive addresses, zero slots skipped
    __device__ __forceinline__ void flush(const double * lds, double * __restrict__ y) const
    {
#pragma unroll
        for (int w = 0; w < KW; ++w)
            for (int t = threadIdx.x; t < wl[w]; t += kWinBlock) {
                const double v = lds[wo[w] + t];
                if (v != 0.0)
                    atomicAdd(y + wb[w] + t, v);
            }
    }
};

// zero the range's `used` slots and copy its nr + 1 entries of row_ptr into LDS; returns after the barrier
__device__ __forceinline__ void range_prologue(double * lds, int used, int * rp, const int32_t * __restrict__ p, int r0, int nr)
{
    for (int t = threadIdx.x; t < used; t += kWinBlock)
        lds[t] = 0.0;
    for (int t = threadIdx.x; t <= nr; t += kWinBlock)
        rp[t] = p[r0 + t];
    __syncthreads();
}

// the quad at entry e0 of a range whose entries are [eb, ee)
__device__ __forceinline__ void load_quad(long long e0, long long eb, long long ee, const int32_t * __restrict__ col,
                                          const double * __restrict__ val, v4i & c, v2d & a01, v2d & a23)
{
    if (e0 >= eb && e0 + 3 < ee) {
        c = __builtin_nontemporal_load(reinterpret_cast<const v4i *>(col + e0));
        a01 = __builtin_nontemporal_load(reinterpret_cast<const v2d *>(val + e0));
        a23 = __builtin_nontemporal_load(reinterpret_cast<const v2d *>(val + e0 + 2));
    } else {
        // the range's first and last quads: only the entries inside [eb, ee) are read; the others get column -1 (skipped)
        double a[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool in = e0 + k >= eb && e0 + k < ee;
            c[k] = in ? col[e0 + k] : -1;
            a[k] = in ? val[e0 + k] : 0.0;
        }
        a01 = v2d{a[0], a[1]};
        a23 = v2d{a[2], a[3]};
    }
}

// the row of the quad's first entry inside the range: the last r in [0, nr) with rp[r] <= max(e0, eb)
__device__ __forceinline__ int quad_first_row(const int * rp, int nr, long long e0, long long eb)
{
    const long long ef = e0 > eb ? e0 : eb;
    int lo = 0, hi = nr;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (rp[mid] <= ef)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

} // namespace spmv
