/*
 * spmv_hip_mcgs.h -- a multicolour Gauss-Seidel / SSOR preconditioner: the first preconditioner here that uses the off-diagonal
 * entries of A.  The rows are coloured on the device so that no two rows of a colour couple; a sweep is then one launch per
 * colour, without a sequential triangular solve and without a wave that waits for another.
 *
 *     colour:   colour[i] in 0 ... 63 for every row, by Jones-Plassmann with first fit, bit for bit reproducible
 *     permute:  a plan: the rows listed colour by colour, and a copy of the CSR arrays with its rows in that order
 *     sweep:    for the colours first ... last in turn, every row i of the colour:
 *                   x_i <- (1 - w) x_i + w m_i (b_i - sum_{j != i} a_ij x_j)           SOR, m_i = 1 / a_ii
 *     apply:    z <- 0, a sweep over the colours 0 ... C - 1, a sweep over C - 1 ... 0, with b = r: the SSOR operator, and
 *               with z AS STORED  dots[0] = sum_i fl(z_i r_i), dots[1] = sum_i fl(z_i z_i)
 *
 * Same conventions as spmv_hip.h and spmv_hip_krylov.h.  T is double (_f64) or float (_f32) for the vectors; the matrix values are
 * the fp64 CSR values the multiplies read.  All arithmetic is fp64; every product, quotient, sum and difference is rounded on its
 * own (no FMA); a float gets ONE rounding to float, at its store.  No floating-point atomics anywhere.
 *
 * COLOUR.  Jones-Plassmann in rounds that all read the state of the round's start.  The key of row i is the pair
 * (fmix32((uint32) i ^ seed), i), compared lexicographically; fmix32 is the murmur3 finaliser in 32 bits:
 *     h ^= h >> 16; h *= 0x85ebca6b; h ^= h >> 13; h *= 0xc2b2ae35; h ^= h >> 16.
 * A neighbour of i is a stored column j != i of row i (duplicates and any column order are fine; the pattern is taken as stored,
 * NOT as the pattern of A + A').  In a round an uncoloured row WINS if its key is larger than the key of every uncoloured
 * neighbour; a winner takes the smallest colour that none of its neighbours coloured in EARLIER rounds holds (64 colours, a
 * 64-bit mask).  A winner without a free colour is counted and left at colour 63.  The winners are marked in one kernel and
 * coloured in a second that reads only rows that are not marked, so the colours depend on the arrays and the seed alone, never
 * on scheduling, also where the structure is not symmetric.  Behind the last round a check counts the stored entries (i, j),
 * j != i, with colour[i] == colour[j]: 0 for a structurally symmetric pattern without overflow.
 *     d_status[0] = colours (the largest colour + 1; 0 without rows)     d_status[1] = rounds
 *     d_status[2] = conflicts                                            d_status[3] = overflowed rows
 * The host reads the number of winners behind every round: spmv_hip_mcgs_colour SYNCHRONISES `stream` (once per round and at its
 * end) and cannot be captured into a graph.  Every round colours at least the row with the largest remaining key, so it ends
 * after at most `rows` rounds (4 ... 6 on a path, 9 ... 19 on grids, 40 ... 60 on 3-D meshes of 16 ... 25 entries a row); a
 * round without a winner -- arrays that are not a CSR matrix, or that change under the call -- ends it with SPMV_HIP_ERR_STATE.
 * The workspace is the caller's, spmv_hip_mcgs_workspace(rows) bytes, 16-byte aligned; nothing is allocated.
 *
 * PERMUTE.  Fills the plan (a plain struct, every field public):
 *     rows, colours, conflicts     as given and as d_status holds them (it is read back: this call synchronises `stream` too)
 *     colour_ptr[c]                the first position of colour c in d_order; colour_ptr[c] = rows for c >= colours
 *     d_order                      the rows colour by colour, ascending row index inside a colour (a stable 6-bit counting sort)
 *     d_row_ptr, d_column_index, d_value
 *                                  the matrix with its rows in that order: row k of the copy is row d_order[k], its entries in
 *                                  stored order, its columns NOT renumbered -- x, b and minv keep the caller's numbering -- so a
 *                                  colour is a contiguous range of rows and of entries
 *     group                        lanes per row in the sweep: the smallest power of two >= nnz / rows, clamped to 4 ... 64;
 *                                  a caller may set any power of two 1 ... 64
 * The four arrays are the caller's: rows, rows + 1, nnz and nnz elements.  The copy costs 12 bytes per stored entry of device
 * memory; it is what keeps a colour's launch from touching every cache line of the matrix (in the original arrays a red-black
 * colour owns every other 60-byte row).  The workspace is spmv_hip_mcgs_workspace(rows) again.
 *
 * SWEEP.  One launch per colour from `first` to `last`, descending where last < first; the launches form a line on `stream`.
 * It only enqueues: it neither synchronises nor allocates and may be captured.  For row i = d_order[k] of the colour, with
 * G = plan->group lanes:
 *     lane l of the row's group adds fl(a_ij x_j) over the entries l, l + G, ... of the row in stored order, starting from +0.0;
 *         an entry with j == i adds nothing (its x_i is not read into the sum);
 *     a butterfly over the group follows: p += p[lane ^ step] for step = G / 2 ... 1, which leaves s;
 *     x_i <- fl_T(fl(fl(1 - w) x_i) + fl(w fl(m_i fl(b_i - s)))), m_i = d_minv[i]: the b == 1 array of
 *         spmv_hip_bjacobi_setup_* (1 where row i stores no diagonal entry or a zero one).
 * x is read and written in place; rows of one colour do not read each other, which is why a plan with conflicts != 0 is refused:
 * its rows would race.  A NaN or Inf in x_j reaches the rows that store column j and no other.  w is a host double, 0 < w < 2.
 *
 * APPLY.  z is zeroed on the stream, then swept forwards over the colours 0 ... C - 1 and backwards over C - 1 ... 0 with b = r
 * (2 C launches).  For a symmetric positive definite A and 0 < w < 2 that is the symmetric positive definite SSOR operator
 * applied to r, so CG stays valid.  With d_dots and d_work, {r'z, z'z} of z as stored are formed BEHIND the last colour by one
 * element-wise pass in the cut, the workspace (spmv_hip_krylov_workspace(rows)) and the reduction of spmv_hip_cg_step_*
 * (spmv_hip_krylov.h).  The dots cannot ride on the last colour's launch: it writes only its own rows, and the sums run over all
 * of z.  With both null no sums are formed and no reduction is launched.  rows == 0: with dots, +0.0, +0.0 are stored;
 * otherwise nothing is launched.  It only enqueues and may be captured.
 *
 * Composition (no existing call changes): exactly as spmv_hip_bjacobi_apply_* in spmv_hip_bjacobi.h, with
 *     z = M^-1 r, {r'z, z'z}        spmv_hip_mcgs_apply_*(dots = rz_new)
 * in PCG, and without dots for shat, phat of BiCGStab and vhat of right-preconditioned GMRES.  A sweep alone is an SOR smoother,
 * and repeated it is a stationary solver.
 *
 * Refusals (checked before the first HIP call: nothing is launched, nothing is written): SPMV_HIP_ERR_INVALID for rows < 0, nnz < 0,
 * a null required pointer (every one but stream, and the pair d_dots, d_work; also where rows == 0), exactly one of d_dots and
 * d_work null, w not finite or outside (0, 2), a colour index outside the plan (first, last outside 0 ... colours - 1; 0 is
 * accepted where the plan has no colour), plan->colours outside 0 ... 64, a colour_ptr that is not 0 = colour_ptr[0] <= ... <=
 * colour_ptr[colours] = rows, plan->group not a power of two in 1 ... 64, plan->conflicts != 0, rows sizeof(T) >= 2^32, a
 * workspace below its rule, and a written array (colour, status, the plan's four arrays, x, z, dots, the workspace) overlapping
 * any other array of the call (of arrays whose length a call does not know -- the columns and values of colour, sweep and apply
 * -- the first element); SPMV_HIP_ERR_ALIGN for a vector, dots or a workspace off 16-byte alignment, values off 8-byte and
 * an index array (row_ptr, columns, colour, status, order) off 4-byte alignment.
 *
 * Callers detect the feature by the presence of the symbols (SPMV_HIP_VERSION is unchanged).
 */
#ifndef SPMV_HIP_MCGS_H
#define SPMV_HIP_MCGS_H

#include <stddef.h>

#include "spmv_hip_krylov.h"

#ifdef __cplusplus
extern "C" {
#endif

/* colours are 0 ... 63 */
#define SPMV_HIP_MCGS_MAX_COLOURS 64

typedef struct spmv_hip_mcgs_plan {
    int32_t rows, colours, conflicts, group;
    int32_t colour_ptr[SPMV_HIP_MCGS_MAX_COLOURS + 1]; /* host */
    int32_t *d_order;                                  /* rows */
    int32_t *d_row_ptr;                                /* rows + 1 */
    int32_t *d_column_index;                           /* nnz */
    double *d_value;                                   /* nnz */
} spmv_hip_mcgs_plan;

/* the workspace of spmv_hip_mcgs_colour and of spmv_hip_mcgs_permute: a function of rows alone, at least 16 */
int spmv_hip_mcgs_workspace(int32_t rows, size_t *bytes);

/* d_colour (rows int32) <- the colours, d_status (four int32) <- { colours, rounds, conflicts, overflowed rows }; synchronises */
int spmv_hip_mcgs_colour(int32_t rows, const int32_t *d_row_ptr, const int32_t *d_column_index, uint32_t seed, int32_t *d_colour,
                         int32_t *d_status, void *d_work, size_t work_bytes, void *stream);

/* *plan and the four arrays it points to <- the colour-major order and copy of the matrix; synchronises */
int spmv_hip_mcgs_permute(int32_t rows, int32_t nnz, const int32_t *d_row_ptr, const int32_t *d_column_index, const double *d_value,
                          const int32_t *d_colour, const int32_t *d_status, int32_t *d_order, int32_t *d_perm_row_ptr,
                          int32_t *d_perm_column_index, double *d_perm_value, spmv_hip_mcgs_plan *plan, void *d_work, size_t work_bytes,
                          void *stream);

/* the SOR update of the colours first ... last (descending where last < first), x in place */
int spmv_hip_mcgs_sweep_f64(const spmv_hip_mcgs_plan *plan, int32_t first, int32_t last, double omega, const double *d_b,
                            const double *d_minv, double *d_x, void *stream);
int spmv_hip_mcgs_sweep_f32(const spmv_hip_mcgs_plan *plan, int32_t first, int32_t last, double omega, const float *d_b,
                            const float *d_minv, float *d_x, void *stream);

/* z <- the SSOR operator applied to r, and (d_dots, d_work not null) d_dots <- { r'z, z'z } of z as stored */
int spmv_hip_mcgs_apply_f64(const spmv_hip_mcgs_plan *plan, double omega, const double *d_r, const double *d_minv, double *d_z,
                            double *d_dots, void *d_work, size_t work_bytes, void *stream);
int spmv_hip_mcgs_apply_f32(const spmv_hip_mcgs_plan *plan, double omega, const float *d_r, const float *d_minv, float *d_z,
                            double *d_dots, void *d_work, size_t work_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* SPMV_HIP_MCGS_H */
