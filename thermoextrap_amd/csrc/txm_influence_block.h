// txm_influence_block.h -- pass 1 of the blocked delta-method covariance (txm_influence_block.hip), shared by
// txm_influence_block_cov (f-11) and txm_influence_block_cross_cov (f-13): ONE kernel, ONE plan, the same bits in both.
#pragma once
#include "txm_influence_common.h"

namespace txm {

// Enqueues influence_block_sums_kernel under ib_plan: the unnormalised block sums zt [nb][C][n_f] and the block weights
// wb [nb], nb = ceil(N / block).  The arguments are the entry points' (already validated: n_q in [1, TXM_MAXK]).
int ib_block_sums(const double *x, int64_t ldx_s, const double *u, const double *w, int64_t N, int64_t C, int n_f, int n_q,
                  double center_u, const double *center_x, const double *a, const double *b, int64_t block, double *zt,
                  double *wb, hipStream_t st);

}  // namespace txm
