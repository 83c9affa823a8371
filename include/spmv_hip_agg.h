/*
 * spmv_hip_agg.h -- one level of a plain (unsmoothed) aggregation multigrid: which rows form a coarse unknown, the restriction
 * r_c = P'r, the prolongation x += w P e_c and the coarse matrix A_c = P'AP.  P has one entry 1 per row, so it is the int32 array
 * agg and not a matrix: restriction and prolongation stream at the vector rate, and the Galerkin product is a sort and a
 * segmented sum instead of a sparse matrix-matrix product.
 *
 *     aggregate:  agg[i] in 0 ... aggregates - 1 for every row, by a maximal independent set of roots, bit for bit reproducible
 *     plan:       the rows listed aggregate by aggregate (member_ptr, member), ascending row index inside an aggregate
 *     symbolic:   the pattern of A_c as CSR with distinct ascending columns, and for every coarse entry the run of fine entries
 *     numeric:    a_c[e] = the sum of the fine values of entry e's run, added left to right from +0.0
 *     restrict:   r_c[I] = fl_T(((+0.0 + r[m_0]) + r[m_1]) + ...) over the members m_0 < m_1 < ... of aggregate I
 *     prolong:    x_i <- fl_T(x_i + fl(w e_c[agg[i]])), in place
 *
 * Same conventions as spmv_hip_mcgs.h.  T is double (_f64) or float (_f32) for the vectors; the matrix values are the fp64 CSR
 * values the multiplies read.  All arithmetic is fp64; every product and sum is rounded on its own (no FMA); a float gets ONE
 * rounding to float, at its store.  No floating-point atomics anywhere.
 *
 * AGGREGATE.  A neighbour of row i is a stored column j != i of row i, taken as stored (duplicates, any column order and
 * patterns that are not symmetric are fine: the pattern is NOT that of A + A').  With d_value not null and theta > 0 the entry
 * also needs |a_ij| >= fl(theta m_i), m_i the largest |a_ik| over the stored entries k != i of row i (formed once, before the
 * first round; an entry that is NaN is neither a maximum nor strong); with theta == 0 or d_value null every stored off-diagonal
 * entry counts.  The key of row i is the pair (fmix32((uint32) i ^ seed), i), compared lexicographically: the key and the fmix32
 * of spmv_hip_mcgs.h.  Rounds of two kernels that read the state of the round's start:
 *     mark:    an undecided row WINS if its key is larger than the key of every undecided neighbour (vacuously without one);
 *     assign:  a winner becomes a ROOT; an undecided row that did not win and has a neighbour that is a root or a winner
 *              becomes COVERED.
 * Behind the last round a covered row joins the root among its neighbours with the largest key and a root joins itself; the
 * roots are numbered by their rank in ascending row index (a prefix sum), and d_agg[i] is the number of the root row i joined.
 * Rows without a neighbour -- empty rows and rows that store their diagonal alone among them -- are roots of their own.  The
 * result depends on the arrays, theta and the seed alone, never on scheduling.
 *     d_status[0] = aggregates          d_status[1] = rounds
 *     d_status[2] = the largest aggregate's rows          d_status[3] = the aggregates of a single row
 * The host reads the number of rows still undecided behind every round: spmv_hip_agg_aggregate SYNCHRONISES `stream` and cannot
 * be captured.  Every round decides at least the row with the largest remaining key; a round that decides nobody -- arrays that
 * are not a CSR matrix, or that change under the call -- ends it with SPMV_HIP_ERR_STATE.  rows == 0: nothing is launched but
 * the store of the status, four zeros.
 *
 * PLAN.  Fills the plan (a plain struct, every field public): rows; aggregates and largest as d_status holds them (it is read
 * back: this call synchronises too); d_agg as given; d_member_ptr (aggregates + 1 int32) and d_member (rows int32), the caller's:
 * the members of aggregate I are d_member[d_member_ptr[I] ... d_member_ptr[I + 1]), ascending.  A d_agg that holds a number
 * outside 0 ... aggregates - 1 ends the call with SPMV_HIP_ERR_STATE.
 *
 * SYMBOLIC.  The fine entries are taken in member order -- aggregate by aggregate, a member's entries in stored order -- and
 * sorted stably by (agg[row], agg[column]); as the members of an aggregate ascend that is the stable sort of the entries as
 * stored.  d_entry_order (nnz int32) lists the positions of the fine entries in that order; a coarse entry e is a run of equal
 * pairs, d_entry_order[d_entry_ptr[e] ... d_entry_ptr[e + 1]); d_coarse_row_ptr (aggregates + 1) and d_coarse_column_index are
 * the CSR pattern of A_c, its columns distinct and ascending in every row.  The caller passes d_coarse_column_index with nnz and
 * d_entry_ptr with nnz + 1 elements, the upper bounds; nnz_c and nnz_c + 1 of them are written, and d_status[0] (one int32) is
 * set to nnz_c.  Synchronises.
 *
 * NUMERIC.  d_coarse_value[e] = (((+0.0 + a[o_0]) + a[o_1]) + ...) over the run o_0, o_1, ... of entry e, a lane per coarse
 * entry, so any run length works.  It only enqueues, may be captured, and is repeated alone when the values change and the
 * pattern does not.
 *
 * RESTRICT and PROLONG_ADD are the hot path: they only enqueue, allocate nothing and may be captured.  A member of another
 * aggregate is never read into a sum (selection, not a product with zero): a NaN in r_i reaches r_c[agg[i]] and no other
 * element.  w is a finite host double; w = 1 is the plain correction, w > 1 the over-correction plain aggregation wants.
 *
 * The workspace is the caller's, 16-byte aligned, spmv_hip_agg_workspace(rows, nnz) bytes, a function of (rows, nnz) alone:
 * spmv_hip_agg_aggregate and spmv_hip_agg_plan, which are not told nnz, need spmv_hip_agg_workspace(rows, 0), the symbolic
 * product spmv_hip_agg_workspace(plan->rows, nnz).  The three calls that synchronise may
 * in addition allocate and free temporary device memory inside the call (the radix sort's and the prefix sum's own, as
 * spmv_hip_coo_sort_by_row does).
 *
 * Refusals (checked before the first HIP call: nothing is launched, nothing is written): SPMV_HIP_ERR_INVALID for rows < 0,
 * nnz < 0, nnz_c < 0 or nnz_c > nnz, a null required pointer (every one but stream and, in aggregate, d_value; also where rows ==
 * 0), theta not finite or outside [0, 1], w not finite, a plan with aggregates outside 0 ... rows or with aggregates == 0 and
 * rows > 0, rows sizeof(T) >= 2^32, a workspace below its rule, and a written array overlapping any other array of the call (of
 * arrays whose length a call does not know -- the columns and values of aggregate -- the first element); SPMV_HIP_ERR_ALIGN
 * for a vector or a workspace off 16-byte alignment, values off 8-byte and an index array off 4-byte alignment.
 *
 * Callers detect the feature by the presence of the symbols (SPMV_HIP_VERSION is unchanged).  The aggregates of a distance-2
 * independent set and a restriction by a group of lanes per aggregate, on the same d_agg, d_status and plan, are two further calls
 * in a header of their own: spmv_hip_agg_mis2.h.
 */
#ifndef SPMV_HIP_AGG_H
#define SPMV_HIP_AGG_H

#include <stddef.h>

#include "spmv_hip_krylov.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the call that fills it has the struct's name: write `struct spmv_hip_agg_plan` */
struct spmv_hip_agg_plan {
    int32_t rows, aggregates, largest;
    const int32_t *d_agg;  /* rows */
    int32_t *d_member_ptr; /* aggregates + 1 */
    int32_t *d_member;     /* rows */
};

/* the workspace of the three setup calls: a function of (rows, nnz) alone, at least 16 */
int spmv_hip_agg_workspace(int32_t rows, int32_t nnz, size_t *bytes);

/* d_agg (rows int32) <- the aggregate of every row, d_status (four int32) <- { aggregates, rounds, largest, singletons }; synchronises */
int spmv_hip_agg_aggregate(int32_t rows, const int32_t *d_row_ptr, const int32_t *d_column_index, const double *d_value, double theta,
                           uint32_t seed, int32_t *d_agg, int32_t *d_status, void *d_work, size_t work_bytes, void *stream);

/* *plan, d_member_ptr and d_member <- the rows aggregate by aggregate; synchronises */
int spmv_hip_agg_plan(int32_t rows, const int32_t *d_agg, const int32_t *d_status, int32_t *d_member_ptr, int32_t *d_member,
                      struct spmv_hip_agg_plan *plan, void *d_work, size_t work_bytes, void *stream);

/* the pattern of A_c = P'AP and every coarse entry's run of fine entries; d_status[0] <- nnz_c; synchronises */
int spmv_hip_agg_galerkin_symbolic(const struct spmv_hip_agg_plan *plan, int32_t nnz, const int32_t *d_row_ptr, const int32_t *d_column_index,
                                   int32_t *d_coarse_row_ptr, int32_t *d_coarse_column_index, int32_t *d_entry_order,
                                   int32_t *d_entry_ptr, int32_t *d_status, void *d_work, size_t work_bytes, void *stream);

/* d_coarse_value[e] <- the sum of the fine values of entry e's run, e < nnz_c */
int spmv_hip_agg_galerkin_numeric(int32_t nnz, int32_t nnz_c, const int32_t *d_entry_order, const int32_t *d_entry_ptr,
                                  const double *d_value, double *d_coarse_value, void *stream);

/* r_c[I] <- the sum of r over the members of aggregate I in plan order */
int spmv_hip_agg_restrict_f64(const struct spmv_hip_agg_plan *plan, const double *d_r, double *d_rc, void *stream);
int spmv_hip_agg_restrict_f32(const struct spmv_hip_agg_plan *plan, const float *d_r, float *d_rc, void *stream);

/* x_i <- x_i + omega e_c[agg[i]], in place */
int spmv_hip_agg_prolong_add_f64(const struct spmv_hip_agg_plan *plan, double omega, const double *d_ec, double *d_x, void *stream);
int spmv_hip_agg_prolong_add_f32(const struct spmv_hip_agg_plan *plan, double omega, const float *d_ec, float *d_x, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* SPMV_HIP_AGG_H */
