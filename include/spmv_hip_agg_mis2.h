/*
 * spmv_hip_agg_mis2.h -- two calls beside those of spmv_hip_agg.h: aggregates from a DISTANCE-2 independent set of roots, which
 * are three to four times larger than the distance-1 ones and do not leave hubs whose leaves end up alone, and a restriction
 * that gives every aggregate a GROUP OF LANES instead of one lane.  d_agg, d_status and the plan keep their meaning:
 * spmv_hip_agg_plan, the Galerkin product, spmv_hip_agg_restrict_* and spmv_hip_agg_prolong_add_* take the new aggregates as they
 * are.  Conventions, neighbours, theta, keys, error codes and refusals are those of spmv_hip_agg.h.
 *
 * AGGREGATE_MIS2.  A neighbour of row i is what it is in spmv_hip_agg_aggregate: a stored column j != i of row i, taken as
 * stored, that with d_value not null and theta > 0 also has |a_ij| >= fl(theta m_i) (the row threshold formed once; a NaN entry
 * is neither a maximum nor strong).  The key of row i is (fmix32((uint32) i ^ seed), i).  Write N(i) for the neighbours of i.
 * Every round reads the state of the round's start, in four kernels, and EVERY row relays, whatever its own state is -- that is
 * what keeps two roots from standing two steps apart through a covered row:
 *     t1[i] = the largest key among the UNDECIDED rows of {i} + N(i), or none;
 *     t2[i] = the largest t1[j] over j in {i} + N(i); an undecided row i WINS if t2[i] is its own key, that is, if its key is
 *             the largest among the undecided rows within two stored steps;
 *     n1[i] = i or a row of N(i) won;
 *     a winner becomes a ROOT; an undecided row that did not win becomes COVERED if n1[j] for some j in {i} + N(i).
 * A row without a neighbour wins vacuously.  The undecided row with the largest key of all always wins, so every round decides
 * somebody.  Behind the last round the rows join roots in two passes:
 *     pass 1:  a row that is no root and has a root among its neighbours joins the root neighbour with the largest key;
 *     pass 2:  every other row looks at those of its neighbours that joined in pass 1 and joins the root one of them joined:
 *              among those roots, the one with the largest key.  A covered row has such a neighbour by construction; a row
 *              that finds none -- arrays that changed under the call -- ends the call with SPMV_HIP_ERR_STATE.
 * The roots are numbered by their rank in ascending row index; d_agg[i] is the number of the root row i joined and d_status[0 ...
 * 3] = {aggregates, rounds, the largest aggregate's rows, the aggregates of a single row}.  On a symmetric pattern at theta 0 no
 * two roots lie within two steps of each other, every row lies within two steps of its root and every aggregate is connected.
 * The result depends on the arrays, theta and the seed alone.  Like spmv_hip_agg_aggregate the call SYNCHRONISES `stream` once a
 * round, cannot be captured, and returns SPMV_HIP_ERR_STATE for a round that decides nobody; rows == 0 stores four zeros.  Its
 * workspace is spmv_hip_agg_mis2_workspace(rows) bytes, a function of rows alone (spmv_hip_agg_workspace is another rule).
 *
 * RESTRICT_GROUP.  group = G is a power of two in 1 ... 64; anything else is SPMV_HIP_ERR_INVALID, and the other refusals are
 * those of spmv_hip_agg_restrict_*.  The summation order is fixed, and is not that of spmv_hip_agg_restrict_* where G > 1:
 *     lane l of an aggregate's G lanes adds the members l, l + G, l + 2 G, ... of the aggregate in plan order, left to right
 *     from +0.0, in fp64 and without FMA; a lane without a member holds +0.0;
 *     then p += p[lane ^ step] for step = 1, 2, 4, ... G / 2, every lane of the group at once;
 *     r_c[I] = fl_T(p) of the group's first lane: a float gets ONE rounding to float, at its store.
 * G == 1 is spmv_hip_agg_restrict_* bit for bit.  A member of another aggregate is never loaded into a sum: a NaN in r_i reaches
 * r_c[agg[i]] and no other element.  The call only enqueues, allocates nothing and may be captured.  spmv_hip_agg_group is the
 * recommended G, host arithmetic on the plan's two counts: the smallest power of two >= rows / aggregates inside 1 ... 64, and 1
 * for a plan without rows, without aggregates or null.
 *
 * Callers detect the feature by the presence of the symbols (SPMV_HIP_VERSION is unchanged).
 */
#ifndef SPMV_HIP_AGG_MIS2_H
#define SPMV_HIP_AGG_MIS2_H

#include "spmv_hip_agg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the workspace of spmv_hip_agg_aggregate_mis2: a function of rows alone, at least 16 */
int spmv_hip_agg_mis2_workspace(int32_t rows, size_t *bytes);

/* d_agg (rows int32) <- the aggregate of every row, d_status (four int32) <- { aggregates, rounds, largest, singletons }; synchronises */
int spmv_hip_agg_aggregate_mis2(int32_t rows, const int32_t *d_row_ptr, const int32_t *d_column_index, const double *d_value, double theta,
                                uint32_t seed, int32_t *d_agg, int32_t *d_status, void *d_work, size_t work_bytes, void *stream);

/* r_c[I] <- the sum of r over the members of aggregate I: `group` lanes stride the member list, then a butterfly */
int spmv_hip_agg_restrict_group_f64(const struct spmv_hip_agg_plan *plan, int32_t group, const double *d_r, double *d_rc, void *stream);
int spmv_hip_agg_restrict_group_f32(const struct spmv_hip_agg_plan *plan, int32_t group, const float *d_r, float *d_rc, void *stream);

/* the recommended group: the smallest power of two >= rows / aggregates, inside 1 ... 64 */
int32_t spmv_hip_agg_group(const struct spmv_hip_agg_plan *plan);

#ifdef __cplusplus
}
#endif

#endif /* SPMV_HIP_AGG_MIS2_H */
