// txm_influence_cross.hip -- the delta-method covariance of txm_influence.hip ACROSS observable columns
// (ExtrapModel.derivs_cross_cov / predict_cov).
//
// With the influence polynomials of txm_influence.hip,
//      psi_k(n, c) = sum_q (a[c][k][q] + b[c][k][q] dx_nc) du_n^q,   dx_nc = x[n][c] - center_x[c],  du_n = u[n] - center_u,
// the caller wants every block of
//      cov[c][i][c'][j] = sum_n w_n^2 psi_i(n, c) psi_j(n, c') / (sum_n w_n)^2           ((C n_f)^2, symmetric).
//
// psi psi' depends on (q, q') through r = q + q' alone (a Hankel structure), so the sample pass needs no coefficient:
// it accumulates the R = 2 n_q - 1 weighted Gram matrices
//      G_r = sum_n w_n^2 du_n^r z_n z_n^T,     z_n = (dx_n0, ..., dx_n,C-1, 1)           (C + 1 logical columns)
// and a finalize contracts them:  sum_{q,q'} a a' G_r[1][1] + a b' G_r[1][c'] + b a' G_r[c][1] + b b' G_r[c][c'],  where
// index 1 stands for the column of ones -- logical column C, BEHIND the observables, so that every entry the finalize
// needs lies at (row <= column).  G_r[1][1] is txm_influence_cov's T_0, the border G_r[c][1] its T_1, the diagonal of the
// C x C block its T_2; the off-diagonal of that block is what is new.
//
// The Grams are FP64 matrix-pipe work (v_mfma_f64_16x16x4_f64; operand layout as txm_mbar_cov.hip phase 2).  The
// C + 1 logical columns are cut into T = ceil((C + 1) / 16) tiles of 16; only tile pairs (ti <= tj) are computed.
//   influence_cross_kernel   grid (tile pairs, sample workgroups) -- the pair is the fast index, so the workgroups that
//                            read the same rows are dispatched together.  A wave owns samples 4 at a time: lane
//                            (m = lane & 15, k = lane >> 4) holds A[m][k] = w^2 du^r z_{16 ti + m} and
//                            B[k][m] = z_{16 tj + m} of sample k of the step.  One MFMA per r into the accumulator tile
//                            of G_r; from r to r + 1 the A operand is multiplied by du once.  R accumulator tiles of
//                            8 VGPRs live in the wave (R = 7 at order 3 ... 17 at order 8).  At the end the four waves'
//                            tiles are added in wave order through LDS: one record per (workgroup, tile pair).
//                            The total weight sum_n w_n rides on the VALU (lanes m == 0) behind the tiles of the record.
//   influence_cross_sum_kernel     adds the workgroups' records in index order into one record per tile pair.
//   influence_cross_final_kernel   a thread per pair of outputs {(c,i), (c',j)} with (c,i) <= (c',j): reads G at
//                            (row <= column) only -- inside a diagonal tile the MFMA rounds (m,n) and (n,m) differently
//                            -- contracts in one fixed order, divides by (sum w)^2 and stores the entry and its mirror.
// No floating-point atomics: two calls give the same bits.  A row of weight zero is selected out (its operands are set
// to zero, not multiplied by zero) and may hold anything; total weight zero gives zeros.
// Rounding: every product of the expansion is bounded by the matching product of B_k(n, c) = sum_q (|a| + |b| |dx|) |du|^q,
// so the first-order bound is eps * sum_n p_n^2 B_i(n, c) B_j(n, c'),  p_n = w_n / sum w.
//
// txm_influence_cross_cov_batched runs the same three bodies for S states in ONE launch each, the state on
// a grid axis, under a plan of its own: the states share the eight workgroups per CU (cx_batch_q), and every state has
// its own slice of the workspace.  Inside a state nothing changes, so a state whose sample workgroups are as many as
// cx_plan would give it alone has the single call's bits.
#include <vector>

#include "txm_influence_common.h"

namespace txm {

constexpr int CX_BLOCK = 256;  // four waves
constexpr int CX_SHARE = 256;  // samples a workgroup takes before the grid grows by one workgroup
constexpr int CX_MAXC = 255;   // C + 1 logical columns <= 256: at most 16 tiles a side
constexpr int CX_UNR = 4;      // 4-sample steps a wave has in flight

// doubles of one (workgroup, tile pair) record: R tiles of 16 x 16, then the total weight (padded to 8)
__host__ __device__ constexpr int cx_rec(int n_q) { return (2 * n_q - 1) * 256 + 8; }

// One state of a batched call as the kernels read it (built on the host from txm_inf_state and the batch's plan):
// grid_x sample workgroups, its slice of the workspace at `off` doubles: grid_x * pairs records, then pairs summed ones.
struct cx_dev_state {
  const double *x, *u, *w;
  int64_t n;
  int64_t grid_x;
  size_t off;
};

// Sample workgroup `by` of `ny` of one state.  partial [ny sample workgroups][gridDim.x tile pairs][cx_rec]
template <int NQ, bool WEIGHTED>
__device__ __forceinline__ void influence_cross_body(const double *__restrict__ x, int64_t ldx_s,
                                                     const double *__restrict__ u, const double *__restrict__ w,
                                                     int64_t N, int C, int T, double cu, const double *__restrict__ cx,
                                                     int by, int ny, double *__restrict__ partial) {
  constexpr int R = 2 * NQ - 1, REC = cx_rec(NQ);
  __shared__ double red[4 * 256];
  __shared__ double sws[16];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, m = lane & 15, k4 = lane >> 4;
  int ti, tj;
  inf_pair((int)blockIdx.x, T, ti, tj);  // tile pair (ti <= tj)
  const bool diag = ti == tj;
  // logical columns of this lane's A row and B column: < C an observable, C the ones, above it nothing
  const int ca = 16 * ti + m, cb = 16 * tj + m;
  const bool a_x = ca < C, b_x = cb < C;
  const double a_one = ca == C ? 1.0 : 0.0, b_one = cb == C ? 1.0 : 0.0;
  const double pa = a_x ? cx[ca] : 0.0, pb = b_x ? cx[cb] : 0.0;

  inf_v4d acc[R];
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = inf_v4d{0.0, 0.0, 0.0, 0.0};
  double sw = 0.0;

  // wave wg of NW takes the 4-sample steps wg, wg + NW, ...; the loop bounds are wave-uniform
  const int64_t NW = (int64_t)ny * 4, stride = NW * 4;
  for (int64_t ib = ((int64_t)by * 4 + wave) * 4; ib < N; ib += CX_UNR * stride) {
    double ui[CX_UNR], wi[CX_UNR], xa[CX_UNR], xb[CX_UNR];
    bool ok[CX_UNR];
#pragma unroll
    for (int s = 0; s < CX_UNR; ++s) {
      const int64_t i = ib + s * stride + k4;
      ok[s] = i < N;
      const int64_t ic = ok[s] ? i : 0;  // (a row that exists: the value is selected out below)
      ui[s] = u[ic];
      wi[s] = WEIGHTED ? w[ic] : 1.0;
      xa[s] = a_x ? x[ic * ldx_s + ca] : 0.0;
      xb[s] = diag ? xa[s] : (b_x ? x[ic * ldx_s + cb] : 0.0);
    }
#pragma unroll
    for (int s = 0; s < CX_UNR; ++s) {
      const bool live = ok[s] && (!WEIGHTED || wi[s] != 0.0);
      const double du = live ? ui[s] - cu : 0.0;
      const double za = live ? (a_x ? xa[s] - pa : a_one) : 0.0;
      const double zb = live ? (b_x ? xb[s] - pb : b_one) : 0.0;
      const double wl = live ? wi[s] : 0.0;
      sw += wl;
      double av = wl * wl * za;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        acc[r] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, zb, acc[r], 0, 0, 0);
        av *= du;
      }
    }
  }

  // the four waves' tiles in wave order.  D layout: column = lane & 15, row = (lane >> 4) + 4 * reg
  double *dst = partial + ((size_t)by * gridDim.x + blockIdx.x) * REC;
#pragma unroll
  for (int r = 0; r < R; ++r) {
#pragma unroll
    for (int g = 0; g < 4; ++g) red[wave * 256 + (k4 + 4 * g) * 16 + m] = acc[r][g];
    __syncthreads();
    dst[r * 256 + tid] = ((red[tid] + red[256 + tid]) + red[512 + tid]) + red[768 + tid];
    __syncthreads();
  }
  // total weight: the lanes m == 0 of a wave hold its four sample slots
  if (m == 0) sws[wave * 4 + k4] = sw;
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < 16; ++q) s += sws[q];
    dst[R * 256] = s;
  }
}

template <int NQ, bool WEIGHTED>
__global__ __launch_bounds__(CX_BLOCK) void influence_cross_kernel(const double *__restrict__ x, int64_t ldx_s,
                                                                   const double *__restrict__ u,
                                                                   const double *__restrict__ w, int64_t N, int C, int T,
                                                                   double cu, const double *__restrict__ cx,
                                                                   double *__restrict__ partial) {
  influence_cross_body<NQ, WEIGHTED>(x, ldx_s, u, w, N, C, T, cu, cx, (int)blockIdx.y, (int)gridDim.y, partial);
}

// blockIdx.z = state; a workgroup beyond the state's own grid leaves at once
template <int NQ, bool WEIGHTED>
__global__ __launch_bounds__(CX_BLOCK) void influence_cross_batch_kernel(const cx_dev_state *__restrict__ tab,
                                                                         int64_t ldx_s, int C, int T,
                                                                         const double *__restrict__ cu,
                                                                         const double *__restrict__ cx,
                                                                         double *__restrict__ ws) {
  const cx_dev_state s = tab[blockIdx.z];
  if ((int64_t)blockIdx.y >= s.grid_x) return;
  influence_cross_body<NQ, WEIGHTED>(s.x, ldx_s, s.u, s.w, s.n, C, T, cu[blockIdx.z], cx + (size_t)blockIdx.z * C,
                                     (int)blockIdx.y, (int)s.grid_x, ws + s.off);
}

// the workgroups' records in index order (inf_sum_records): per_blk = pairs * REC
__global__ __launch_bounds__(CX_BLOCK) void influence_cross_sum_kernel(const double *__restrict__ partial, int nblk,
                                                                       size_t per_blk, double *__restrict__ G) {
  inf_sum_records(partial, nblk, per_blk, G);
}

// blockIdx.y = state: its grid_x records of per_blk doubles, the summed record behind them
__global__ __launch_bounds__(CX_BLOCK) void influence_cross_sum_batch_kernel(const cx_dev_state *__restrict__ tab,
                                                                             size_t per_blk, double *__restrict__ ws) {
  const cx_dev_state s = tab[blockIdx.y];
  double *partial = ws + s.off;
  inf_sum_records(partial, (int)s.grid_x, per_blk, partial + (size_t)s.grid_x * per_blk);
}

// cov [C n_f][C n_f]; a thread per (P, Q) = ((c, i), (c', j)), the threads with P <= Q compute and store both
template <int NQ>
__device__ __forceinline__ void influence_cross_final_body(const double *__restrict__ G, int C, int T, int n_f,
                                                           const double *__restrict__ a, const double *__restrict__ b,
                                                           double *__restrict__ cov) {
  constexpr int R = 2 * NQ - 1, REC = cx_rec(NQ);
  const size_t M = (size_t)C * n_f;
  const size_t e = (size_t)blockIdx.x * CX_BLOCK + threadIdx.x;
  if (e >= M * M) return;
  const size_t P = e / M, Q = e % M;
  if (P > Q) return;
  const int c = (int)(P / n_f), i = (int)(P % n_f), d = (int)(Q / n_f), j = (int)(Q % n_f);  // c <= d
  // G_r at (row, col), row <= col, as logical columns: the ones are column C
  auto at = [&](int row, int col) {
    return G + (size_t)inf_pair_index(row >> 4, col >> 4, T) * REC + (row & 15) * 16 + (col & 15);
  };
  const double *g11 = at(C, C), *g1d = at(d, C), *gc1 = at(c, C), *gcd = at(c, d);
  double t11[R], t1d[R], tc1[R], tcd[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    t11[r] = g11[r * 256];
    t1d[r] = g1d[r * 256];
    tc1[r] = gc1[r * 256];
    tcd[r] = gcd[r * 256];
  }
  const double *ai = a + (P * NQ), *bi = b + (P * NQ), *aj = a + (Q * NQ), *bj = b + (Q * NQ);
  double s = 0.0;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const double aiq = ai[q], biq = bi[q];
#pragma unroll
    for (int p = 0; p < NQ; ++p) {
      const double ajp = aj[p], bjp = bj[p];
      s += ((aiq * ajp * t11[q + p] + aiq * bjp * t1d[q + p]) + biq * ajp * tc1[q + p]) + biq * bjp * tcd[q + p];
    }
  }
  const double W = G[R * 256];  // the record of tile pair 0
  const double v = W == 0.0 ? 0.0 : s / (W * W);
  cov[P * M + Q] = v;
  cov[Q * M + P] = v;
}

template <int NQ>
__global__ __launch_bounds__(CX_BLOCK) void influence_cross_final_kernel(const double *__restrict__ G, int C, int T,
                                                                         int n_f, const double *__restrict__ a,
                                                                         const double *__restrict__ b,
                                                                         double *__restrict__ cov) {
  influence_cross_final_body<NQ>(G, C, T, n_f, a, b, cov);
}

// blockIdx.y = state: its summed records, its slices of a, b [S][C][n_f][NQ] and of cov [S][C n_f][C n_f]
template <int NQ>
__global__ __launch_bounds__(CX_BLOCK) void influence_cross_final_batch_kernel(const cx_dev_state *__restrict__ tab,
                                                                               const double *__restrict__ ws,
                                                                               size_t per_blk, int C, int T, int n_f,
                                                                               const double *__restrict__ a,
                                                                               const double *__restrict__ b,
                                                                               double *__restrict__ cov) {
  const cx_dev_state s = tab[blockIdx.y];
  const size_t M = (size_t)C * n_f, sb = (size_t)blockIdx.y;
  influence_cross_final_body<NQ>(ws + s.off + (size_t)s.grid_x * per_blk, C, T, n_f, a + sb * M * NQ, b + sb * M * NQ,
                                 cov + sb * M * M);
}

struct CxPlan {
  int T, pairs, grid_x;
};

// One workgroup per CX_SHARE samples and tile pair, up to about eight workgroups per CU in all; the rest is strided.
static CxPlan cx_plan(int64_t N, int64_t C) {
  CxPlan p{};
  p.T = (int)((C + 1 + 15) / 16);
  p.pairs = p.T * (p.T + 1) / 2;
  int64_t cap = (int64_t)num_cus() * 8 / p.pairs;
  if (cap < 1) cap = 1;
  const int64_t gx = cdiv(N, CX_SHARE);
  p.grid_x = (int)(gx > cap ? cap : gx);
  return p;
}

// records of partials the plan can ask for, nondecreasing in C: grid_x * pairs <= min(shares * pairs, max(cap, pairs))
static size_t cx_ws_records(int64_t N, int64_t C) {
  const CxPlan p = cx_plan(N, C);
  const int64_t cap = (int64_t)num_cus() * 8, shares = cdiv(N, CX_SHARE);
  const int64_t hi = cap > p.pairs ? cap : p.pairs;
  const int64_t part = shares <= hi / p.pairs ? shares * p.pairs : hi;  // (no overflow for N near 2^63)
  return (size_t)part + (size_t)p.pairs;                                 // the partials, then the summed records
}

template <int NQ>
static int cx_launch(const CxPlan &p, const double *x, int64_t ldx_s, const double *u, const double *w, int64_t N, int C,
                     int n_f, double cu, const double *cx, const double *a, const double *b, double *cov, double *ws,
                     hipStream_t st) {
  const size_t per_blk = (size_t)p.pairs * cx_rec(NQ);
  double *partial = ws, *G = ws + (size_t)p.grid_x * per_blk;
  const dim3 grid(p.pairs, p.grid_x), block(CX_BLOCK);
  if (w)
    hipLaunchKernelGGL((influence_cross_kernel<NQ, true>), grid, block, 0, st, x, ldx_s, u, w, N, C, p.T, cu, cx, partial);
  else
    hipLaunchKernelGGL((influence_cross_kernel<NQ, false>), grid, block, 0, st, x, ldx_s, u, w, N, C, p.T, cu, cx, partial);
  TXM_LAUNCH_CHECK();
  hipLaunchKernelGGL(influence_cross_sum_kernel, dim3((unsigned)cdiv((int64_t)per_blk, CX_BLOCK)), block, 0, st, partial,
                     p.grid_x, per_blk, G);
  TXM_LAUNCH_CHECK();
  const int64_t M = (int64_t)C * n_f;
  hipLaunchKernelGGL((influence_cross_final_kernel<NQ>), dim3((unsigned)cdiv(M * M, CX_BLOCK)), block, 0, st, G, C, p.T, n_f,
                     a, b, cov);
  TXM_LAUNCH_CHECK();
  return TXM_OK;
}

// The batch's own plan: q sample workgroups a state may have, so that all S states together stay at about
// eight workgroups per CU; q never exceeds cx_plan's cap, so a state with ceil(n / CX_SHARE) <= q runs the single plan.
static int64_t cx_batch_q(int64_t S, int pairs) {
  const int64_t q = (int64_t)num_cus() * 8 / ((int64_t)pairs * S);
  return q < 1 ? 1 : q;
}

static int64_t cx_batch_grid(int64_t S, int64_t n, int64_t C) {
  const int T = (int)((C + 1 + 15) / 16);
  const int64_t q = cx_batch_q(S, T * (T + 1) / 2), gx = n / CX_SHARE + (n % CX_SHARE != 0);  // (no overflow near 2^63)
  return gx > q ? q : gx;
}

template <int NQ>
static int cx_launch_batched(const cx_dev_state *tab, int64_t S, bool weighted, int T, int pairs, int64_t grid_max,
                             int64_t ldx_s, int C, int n_f, const double *cu, const double *cx, const double *a,
                             const double *b, double *cov, double *ws, hipStream_t st) {
  const size_t per_blk = (size_t)pairs * cx_rec(NQ);
  const dim3 grid(pairs, (unsigned)grid_max, (unsigned)S), block(CX_BLOCK);
  if (weighted)
    hipLaunchKernelGGL((influence_cross_batch_kernel<NQ, true>), grid, block, 0, st, tab, ldx_s, C, T, cu, cx, ws);
  else
    hipLaunchKernelGGL((influence_cross_batch_kernel<NQ, false>), grid, block, 0, st, tab, ldx_s, C, T, cu, cx, ws);
  TXM_LAUNCH_CHECK();
  hipLaunchKernelGGL(influence_cross_sum_batch_kernel, dim3((unsigned)cdiv((int64_t)per_blk, CX_BLOCK), (unsigned)S), block,
                     0, st, tab, per_blk, ws);
  TXM_LAUNCH_CHECK();
  const int64_t M = (int64_t)C * n_f;
  hipLaunchKernelGGL((influence_cross_final_batch_kernel<NQ>), dim3((unsigned)cdiv(M * M, CX_BLOCK), (unsigned)S), block, 0,
                     st, tab, ws, per_blk, C, T, n_f, a, b, cov);
  TXM_LAUNCH_CHECK();
  return TXM_OK;
}

}  // namespace txm

using namespace txm;

extern "C" size_t txm_influence_cross_cov_ws_bytes(int64_t N, int64_t C, int n_f, int n_q) {
  if (N < 1 || C < 1 || C > CX_MAXC || n_f < 1 || n_f > TXM_MAXK || n_q < 1 || n_q > TXM_MAXK) return 0;
  return cx_ws_records(N, C) * (size_t)cx_rec(n_q) * sizeof(double) + 256;
}

extern "C" int txm_influence_cross_cov(const double *x, int64_t ldx_s, const double *u, const double *w, int64_t N,
                                       int64_t C, int n_f, int n_q, double center_u, const double *center_x,
                                       const double *a, const double *b, double *cov, void *ws, size_t ws_bytes,
                                       txm_stream stream) {
  if (const int rc = inf_check_args("influence_cross_cov", x && u && center_x && a && b && cov && ws, N, C, CX_MAXC,
                                    " (the result has (C n_f)^2 entries)", n_f, n_q, ldx_s >= C, "row pitch ldx_s < C", center_u))
    return rc;
  if (ws_bytes < txm_influence_cross_cov_ws_bytes(N, C, n_f, n_q)) {
    set_error("influence_cross_cov: workspace too small");
    return TXM_ERR_WORKSPACE;
  }
  const CxPlan p = cx_plan(N, C);
  hipStream_t st = (hipStream_t)stream;
  return inf_dispatch(n_q, "influence_cross_cov: n_q", [&](auto Q) {
    return cx_launch<decltype(Q)::value>(p, x, ldx_s, u, w, N, (int)C, n_f, center_u, center_x, a, b, cov, (double *)ws, st);
  });
}

static bool cx_batched_shape_ok(int64_t S, int64_t C, int n_f, int n_q) {
  return S >= 1 && S <= 65535 && C >= 1 && C <= CX_MAXC && n_f >= 1 && n_f <= TXM_MAXK && n_q >= 1 && n_q <= TXM_MAXK;
}

extern "C" int txm_influence_cross_cov_batched_grid(int64_t S, int64_t n, int64_t C) {
  if (S < 1 || S > 65535 || n < 1 || C < 1 || C > CX_MAXC) return 0;
  return (int)cx_batch_grid(S, n, C);
}

extern "C" size_t txm_influence_cross_cov_batched_ws_bytes(int64_t S, int64_t n_max, int64_t C, int n_f, int n_q) {
  if (!cx_batched_shape_ok(S, C, n_f, n_q) || n_max < 1) return 0;
  const int T = (int)((C + 1 + 15) / 16), pairs = T * (T + 1) / 2;
  const size_t records = (size_t)S * (size_t)(cx_batch_grid(S, n_max, C) + 1) * (size_t)pairs;
  return align_up((size_t)S * sizeof(cx_dev_state), 256) + records * (size_t)cx_rec(n_q) * sizeof(double) + 256;
}

extern "C" int txm_influence_cross_cov_batched(const txm_inf_state *states_host, int64_t S, int64_t ldx_s, int64_t C,
                                               int n_f, int n_q, const double *center_u, const double *center_x,
                                               const double *a, const double *b, double *cov, void *ws, size_t ws_bytes,
                                               txm_stream stream) {
  bool weighted;
  int64_t n_max;
  if (const int rc = inf_check_batch("influence_cross_cov_batched", states_host && center_u && center_x && a && b && cov && ws,
                                     states_host, S, ldx_s, C, CX_MAXC, " (the result has (C n_f)^2 entries)", n_f, n_q,
                                     weighted, n_max))
    return rc;
  const int T = (int)((C + 1 + 15) / 16), pairs = T * (T + 1) / 2;
  const size_t rec = (size_t)cx_rec(n_q);
  static thread_local std::vector<cx_dev_state> tab_host;
  tab_host.resize((size_t)S);
  size_t off = 0;
  int64_t grid_max = 1;
  for (int64_t s = 0; s < S; ++s) {
    const txm_inf_state &h = states_host[s];
    const int64_t gx = cx_batch_grid(S, h.n, C);
    tab_host[(size_t)s] = cx_dev_state{h.x, h.u, h.w, h.n, gx, off};
    off += (size_t)(gx + 1) * (size_t)pairs * rec;
    if (gx > grid_max) grid_max = gx;
  }
  const size_t tab_bytes = align_up((size_t)S * sizeof(cx_dev_state), 256);
  if (ws_bytes < txm_influence_cross_cov_batched_ws_bytes(S, n_max, C, n_f, n_q) || ws_bytes < tab_bytes + off * sizeof(double)) {
    set_error("influence_cross_cov_batched: workspace too small");
    return TXM_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  cx_dev_state *tab = (cx_dev_state *)ws;
  TXM_HIP(hipMemcpyAsync(tab, tab_host.data(), (size_t)S * sizeof(cx_dev_state), hipMemcpyHostToDevice, st));
  double *recs = (double *)((char *)ws + tab_bytes);
  return inf_dispatch(n_q, "influence_cross_cov_batched: n_q", [&](auto Q) {
    return cx_launch_batched<decltype(Q)::value>(tab, S, weighted, T, pairs, grid_max, ldx_s, (int)C, n_f, center_u, center_x, a,
                                                 b, cov, recs, st);
  });
}
