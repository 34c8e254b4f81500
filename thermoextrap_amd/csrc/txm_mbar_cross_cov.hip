// txm_mbar_cross_cov.hip -- the Gram matrix over the pooled samples behind MBAR's asymptotic covariance ACROSS observable
// columns and across targets (MBARModel.predict_with_covariance).  Theta is bilinear in the columns that were
// not sampled, so with y_n,(a,c) = W_na (x_nc - mean_ac)
//   cov(A_ac, A_a'c') = sum_n y_n,(a,c) y_n,(a',c')  +  (sqrt(N) b_ac)^T (I_K - sqrt(N) G_s sqrt(N))^+ (sqrt(N) b_a'c').
// txm_mbar_cov gives b (and the diagonal of the first term, yy); this file gives the first term in full:
//   cross_alpha = 0   out [n_alpha][C][C]          = sum_n W_na^2     d_nac d_nac'
//   cross_alpha = 1   out [n_alpha C][n_alpha C]   = sum_n W_na W_na' d_nac d_na'c'      (index a C + c)
// The call follows the txm_mbar_cov call of the same targets and takes its device output lnw = ln sum_n e^{-a ut_n - logD_n}:
// the normalised weight is ONE exponential, W_na = e^{-a ut_n - logD_n - lnw_a} -- no max pass, no denominator, no softmax
// over the states.  K enters only through the state table and the pooled offset of logD.
//
// The C columns are cut into T = ceil(C / 16) tiles; only tile pairs (ti <= tj) are computed.
//   mbar_cross_cov_kernel   grid (sample workgroups, tile pairs[, row target a_row]).  A workgroup (four waves) walks the
//       states one after the other, and of each state the 64-sample tiles blockIdx.x, blockIdx.x + gridDim.x, ...
//       phase 1  four lanes per sample, lane q of them the targets q and q + 4: one exponential per (sample, target) into
//                LDS, none computed twice in the workgroup; samples past the state's end get zero.
//       phase 2  a wave takes four of the tile's sixteen 4-sample steps.  Lane (m = lane & 15, k = lane >> 4) has loaded x
//                of sample k of the step once for column 16 ti + m and once for column 16 tj + m (before phase 1, so the
//                loads fly behind the exponentials), and issues one v_mfma_f64_16x16x4_f64 per accumulator target a with
//                B[k][m] = W_a (x - mean[a]) on tile tj and A[m][k] = W_a (x - mean[a]) on tile ti (same-alpha mode) or
//                A[m][k] = W_a_row (x - mean[a_row]) on tile ti, formed once per step (cross mode).
//       A cross-mode workgroup of row target a_row thus covers the blocks (a_row, ti; a', tj) of all a'; with ti <= tj that
//       reaches every block of the result or its transpose.  At the end the four waves' tiles are added in wave order
//       through LDS: ONE record of n_alpha tiles per (sample workgroup, pair[, row target]).
//   mbar_cross_cov_final_kernel   a thread per output pair (P <= Q): adds the records in index order, reads only entries
//       at (row <= column) of a diagonal tile -- the MFMA rounds (m, n) and (n, m) differently -- and of the two records that
//       hold a diagonal tile of two targets the one with a <= a'; stores the entry and its mirror.
// No floating-point atomics: two calls give the same bits and out is exactly symmetric.  Both modes form the same operands
// and cut the samples by the same rule, so with the same number of sample workgroups the diagonal blocks of the cross form
// ARE the same-alpha result.
//
// Workspace: the call runs in the workspace of the txm_mbar_cov call it follows (txm_mbar_cov_ws_bytes(K, C, n_alpha)) and
// plans its launch from the ws_bytes it is given (xc_plan; txm_mbar_cross_cov_plan shows it).  The states are walked
// inside the workgroup, not spread over the grid: a record per state would need 64 x 1088 x 16 KiB = 1.1 GB at K = 64,
// C = 255, 8 targets in cross mode, where txm_mbar_cov's workspace has 89 MB; without the state the smallest plan is
// pairs x rows records (17.8 MB there) and fits the query for every (K, C, n_alpha).
#include <cmath>
#include <cstring>

#include "txm_influence_common.h"  // inf_pair, inf_pair_index, inf_v4d: the tile pairs of the Gram passes
#include "txm_mbar.h"

namespace txm {

constexpr int XC_TILE = 64;    // samples per tile
constexpr int XC_SHARE = 256;  // samples of the longest state per sample workgroup before the rest is strided
constexpr int XC_MAXC = 255;   // at most 16 column tiles a side

// grid (sample workgroups, tile pairs, CROSS ? n_alpha : 1); partial [gridDim.x][pairs][gridDim.z] records of n_alpha tiles
template <int NA, bool CROSS>
__global__ __launch_bounds__(MB_BLOCK) void mbar_cross_cov_kernel(const txm_mbar_state *__restrict__ tab, int K, int C,
                                                                  int T, const double *__restrict__ logD, double upiv,
                                                                  const MbarTargets ta, const double *__restrict__ lnw,
                                                                  const double *__restrict__ mean, int n_alpha,
                                                                  double *__restrict__ partial) {
  constexpr int NI = CROSS ? 1 : NA;
  __shared__ double V[XC_TILE * MB_MAXA];
  __shared__ double red[4 * 256];
  const int tid = threadIdx.x;
  const int a_row = CROSS ? (int)blockIdx.z : 0;
  int ti, tj;
  inf_pair((int)blockIdx.y, T, ti, tj);
  const bool diag = ti == tj;
  // phase 1 roles
  const int j = tid >> 2, q = tid & 3;
  double al1[2], lw1[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int a = q + 4 * t < n_alpha ? q + 4 * t : n_alpha - 1;
    al1[t] = ta.a[a];
    lw1[t] = lnw[a];
  }
  // phase 2 roles
  const int wave = tid >> 6, lane = tid & 63, m = lane & 15, k4 = lane >> 4;
  const int ci = 16 * ti + m, cj = 16 * tj + m;  // columns of this lane's A row and B column: >= C nothing
  const bool i_x = ci < C, j_x = cj < C;
  double mui[NI], muj[NA];
#pragma unroll
  for (int a = 0; a < NA; ++a) {
    const size_t r = (size_t)(a < n_alpha ? a : n_alpha - 1) * C;
    muj[a] = j_x ? mean[r + cj] : 0.0;
    if (!CROSS) mui[a] = i_x ? mean[r + ci] : 0.0;
  }
  if (CROSS) mui[0] = i_x ? mean[(size_t)a_row * C + ci] : 0.0;
  inf_v4d acc[NA];
#pragma unroll
  for (int a = 0; a < NA; ++a) acc[a] = inf_v4d{0.0, 0.0, 0.0, 0.0};

  int64_t off = 0;
  for (int s = 0; s < K; ++s) {
    const double *__restrict__ x = tab[s].x;
    const double *__restrict__ u = tab[s].u;
    const int64_t n = tab[s].n, ldx = tab[s].ldx_s;
    for (int64_t base = (int64_t)blockIdx.x * XC_TILE; base < n; base += (int64_t)gridDim.x * XC_TILE) {
      double xi[4], xj[4];
#pragma unroll
      for (int st = 0; st < 4; ++st) {
        const int64_t i = base + 4 * (4 * wave + st) + k4;
        const bool ok = i < n;
        xi[st] = (ok && i_x) ? x[i * ldx + ci] : 0.0;
        xj[st] = diag ? xi[st] : ((ok && j_x) ? x[i * ldx + cj] : 0.0);
      }
      {
        const int64_t i = base + j;
        const bool ok = i < n;
        const double ut = ok ? u[i] - upiv : 0.0;
        const double nld = ok ? -logD[off + i] : 0.0;
#pragma unroll
        for (int t = 0; t < 2; ++t)
          if (q + 4 * t < NA) V[j * MB_MAXA + q + 4 * t] = ok ? exp(fma(-al1[t], ut, nld) - lw1[t]) : 0.0;
      }
      __syncthreads();
#pragma unroll
      for (int st = 0; st < 4; ++st) {
        const int nn = 4 * (4 * wave + st) + k4;
        // (a sample past the end has weight zero and x = 0; a column past C has x = 0 and mean = 0: the operand is zero)
        double ar = 0.0;
        if (CROSS) ar = V[nn * MB_MAXA + a_row] * (xi[st] - mui[0]);
#pragma unroll
        for (int a = 0; a < NA; ++a) {
          const double wa = V[nn * MB_MAXA + a];
          const double av = CROSS ? ar : wa * (xi[st] - mui[CROSS ? 0 : a]);
          acc[a] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, wa * (xj[st] - muj[a]), acc[a], 0, 0, 0);
        }
      }
      __syncthreads();
    }
    off += n;
  }
  // the four waves' tiles in wave order.  D layout: column = lane & 15, row = (lane >> 4) + 4 * reg
  double *dst = partial + (((size_t)blockIdx.x * gridDim.y + blockIdx.y) * gridDim.z + blockIdx.z) * ((size_t)n_alpha * 256);
#pragma unroll
  for (int a = 0; a < NA; ++a) {
    if (a < n_alpha) {
#pragma unroll
      for (int r = 0; r < 4; ++r) red[wave * 256 + (k4 + 4 * r) * 16 + m] = acc[a][r];
      __syncthreads();
      dst[a * 256 + tid] = ((red[tid] + red[256 + tid]) + red[512 + tid]) + red[768 + tid];
      __syncthreads();
    }
  }
}

// A thread per pair of outputs (P <= Q).  Same-alpha mode: P = (a, c), Q = (a, c'), out [n_alpha][C][C]; cross mode:
// P = a C + c, Q = a' C + c', out [n_alpha C][n_alpha C].  The nblk records of its tile in index order.
template <bool CROSS>
__global__ __launch_bounds__(MB_BLOCK) void mbar_cross_cov_final_kernel(const double *__restrict__ partial, int nblk,
                                                                        int pairs, int T, int C, int n_alpha,
                                                                        double *__restrict__ out) {
  const size_t e = (size_t)blockIdx.x * MB_BLOCK + threadIdx.x;
  const size_t CC = (size_t)C * C, M = (size_t)n_alpha * C;
  int a, b, c, d;  // P = (a, c), Q = (b, d)
  size_t at_pq, at_qp;
  if (CROSS) {
    if (e >= M * M) return;
    const size_t P = e / M, Q = e % M;
    if (P > Q) return;
    a = (int)(P / C), c = (int)(P % C), b = (int)(Q / C), d = (int)(Q % C);  // a <= b
    at_pq = P * M + Q;
    at_qp = Q * M + P;
  } else {
    if (e >= (size_t)n_alpha * CC) return;
    a = b = (int)(e / CC);
    c = (int)((e % CC) / C), d = (int)(e % C);
    if (c > d) return;
    at_pq = (size_t)a * CC + (size_t)c * C + d;
    at_qp = (size_t)a * CC + (size_t)d * C + c;
  }
  // the record (row target, tile pair, accumulator target) and the entry of its tile.  A block below the diagonal of the
  // tile grid is the transpose of the one its mirror workgroup computed; on a diagonal tile a <= b and (a == b: c <= d).
  const int tc = c >> 4, td = d >> 4;
  int row, accq, pr, er, ec;
  if (tc <= td) {
    row = a, accq = b, pr = inf_pair_index(tc, td, T), er = c & 15, ec = d & 15;
  } else {
    row = b, accq = a, pr = inf_pair_index(td, tc, T), er = d & 15, ec = c & 15;
  }
  const int rows = CROSS ? n_alpha : 1;
  const size_t rec = (size_t)n_alpha * 256, per_blk = (size_t)pairs * rows * rec;
  const double *src = partial + ((size_t)pr * rows + (CROSS ? row : 0)) * rec + (size_t)accq * 256 + er * 16 + ec;
  double v = 0.0;
  for (int blk = 0; blk < nblk; ++blk) v += src[(size_t)blk * per_blk];
  out[at_pq] = v;
  out[at_qp] = v;
}

struct XcPlan {
  int64_t T, pairs, gx;
  size_t bytes;
};

// The launch plan from the bytes the caller has: as many sample workgroups as records fit, at most one per
// XC_SHARE samples of the longest state and about eight workgroups per CU in all.  TXM_OK or TXM_ERR_WORKSPACE.
static int xc_plan(int64_t C, int32_t n_alpha, int32_t cross_alpha, int64_t n_max, size_t ws_bytes, XcPlan *p) {
  p->T = (C + 15) / 16;
  p->pairs = p->T * (p->T + 1) / 2;
  const int64_t per_gx = p->pairs * (cross_alpha ? n_alpha : 1);  // records per sample workgroup
  const size_t rec_bytes = (size_t)n_alpha * 256 * sizeof(double);
  p->gx = 0;
  p->bytes = MB_HEAD_BYTES + (size_t)per_gx * rec_bytes;  // the smallest plan: one sample workgroup
  if (ws_bytes < p->bytes) return TXM_ERR_WORKSPACE;
  int64_t gx = (int64_t)((ws_bytes - MB_HEAD_BYTES) / rec_bytes / (size_t)per_gx);
  const int64_t share = n_max / XC_SHARE + (n_max % XC_SHARE != 0);
  int64_t cap = (int64_t)num_cus() * 8 / per_gx;
  cap = cap < 1 ? 1 : cap;
  gx = gx > share ? share : gx;
  gx = gx > cap ? cap : gx;
  p->gx = gx < 1 ? 1 : gx;
  p->bytes = MB_HEAD_BYTES + (size_t)(p->gx * per_gx) * rec_bytes;
  return TXM_OK;
}

static int xc_check_shape(const char *who, int32_t K, int64_t C, int32_t n_alpha, int32_t cross_alpha) {
  TXM_REQUIRE(C >= 1 && C <= XC_MAXC, "%s: C = %lld outside [1, %d] (the result has C^2 entries per target pair)", who,
              (long long)C, XC_MAXC);
  TXM_REQUIRE(K >= 1 && K <= MB_MAXK, "%s: K = %d states outside [1, %d]", who, (int)K, MB_MAXK);
  TXM_REQUIRE(n_alpha >= 1 && n_alpha <= MB_MAXA, "%s: n_alpha = %d outside [1, %d]", who, (int)n_alpha, MB_MAXA);
  TXM_REQUIRE(cross_alpha == 0 || cross_alpha == 1, "%s: cross_alpha = %d is neither 0 nor 1", who, (int)cross_alpha);
  return TXM_OK;
}

template <bool CROSS>
static int xc_launch(const XcPlan &p, const txm_mbar_state *tab, int K, int C, const double *logD, double upiv,
                     const MbarTargets &ta, const double *lnw, const double *mean, int n_alpha, double *partial, double *out,
                     hipStream_t st) {
  const dim3 grid((unsigned)p.gx, (unsigned)p.pairs, CROSS ? (unsigned)n_alpha : 1u), block(MB_BLOCK);
#define TXM_XC(NA_)                                                                                                    \
  hipLaunchKernelGGL((mbar_cross_cov_kernel<NA_, CROSS>), grid, block, 0, st, tab, K, C, (int)p.T, logD, upiv, ta, lnw, \
                     mean, n_alpha, partial)
  TXM_MB_NA_DISPATCH(n_alpha, TXM_XC)
#undef TXM_XC
  TXM_LAUNCH_CHECK();
  const int64_t M = CROSS ? (int64_t)n_alpha * C : (int64_t)C;
  const int64_t total = CROSS ? M * M : (int64_t)n_alpha * M * M;
  hipLaunchKernelGGL((mbar_cross_cov_final_kernel<CROSS>), dim3((unsigned)cdiv(total, MB_BLOCK)), block, 0, st, partial,
                     (int)p.gx, (int)p.pairs, (int)p.T, C, n_alpha, out);
  TXM_LAUNCH_CHECK();
  return TXM_OK;
}

}  // namespace txm

using namespace txm;

extern "C" int txm_mbar_cross_cov_plan(int32_t K, int64_t C, int32_t n_alpha, int32_t cross_alpha, int64_t n_max,
                                       size_t ws_bytes, int64_t *plan_host) {
  if (const int rc = xc_check_shape("mbar_cross_cov_plan", K, C, n_alpha, cross_alpha)) return rc;
  TXM_REQUIRE(n_max >= 1, "mbar_cross_cov_plan: n_max = %lld samples (need >= 1)", (long long)n_max);
  TXM_REQUIRE(plan_host, "mbar_cross_cov_plan: null pointer");
  XcPlan p;
  const int rc = xc_plan(C, n_alpha, cross_alpha, n_max, ws_bytes, &p);
  plan_host[0] = p.T;
  plan_host[1] = p.pairs;
  plan_host[2] = p.gx;
  plan_host[3] = (int64_t)p.bytes;  // refused: the smallest workspace the call takes
  if (rc != TXM_OK) set_error("mbar_cross_cov_plan: workspace too small (%zu bytes, the smallest plan needs %zu)", ws_bytes, p.bytes);
  return rc;
}

extern "C" int txm_mbar_cross_cov(const txm_mbar_state *states_host, int32_t K, int64_t C, double upiv, const double *logD,
                                  const double *alpha_host, int32_t n_alpha, const double *mean, const double *lnw,
                                  int32_t cross_alpha, double *out, void *ws, size_t ws_bytes, txm_stream stream) {
  if (const int rc = xc_check_shape("mbar_cross_cov", K, C, n_alpha, cross_alpha)) return rc;
  int64_t nmax = 0;
  if (const int rc = mb_check_states(states_host, K, true, true, C, "mbar_cross_cov", nullptr, &nmax)) return rc;
  TXM_REQUIRE(logD && alpha_host && mean && lnw && out && ws, "mbar_cross_cov: null pointer");
  if (const int rc = mb_check_finite("mbar_cross_cov", K, nullptr, nullptr, n_alpha, alpha_host, upiv)) return rc;
  XcPlan p;
  if (xc_plan(C, n_alpha, cross_alpha, nmax, ws_bytes, &p) != TXM_OK) {
    set_error("mbar_cross_cov: workspace too small (%zu bytes, the smallest plan needs %zu)", ws_bytes, p.bytes);
    return TXM_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  // the state table at the head of the workspace, where txm_mbar_cov keeps it
  MbarHead h;
  if (const int rc = mb_stage_head(ws, states_host, K, nullptr, nullptr, MB_MAXK * sizeof(txm_mbar_state), nullptr, 0, st, &h))
    return rc;
  const txm_mbar_state *tab = h.tab;
  double *partial = (double *)((char *)ws + MB_HEAD_BYTES);
  const MbarTargets ta = mb_targets(alpha_host, n_alpha);
  if (cross_alpha)
    return xc_launch<true>(p, tab, (int)K, (int)C, logD, upiv, ta, lnw, mean, (int)n_alpha, partial, out, st);
  return xc_launch<false>(p, tab, (int)K, (int)C, logD, upiv, ta, lnw, mean, (int)n_alpha, partial, out, st);
}
