// txm_mbar_cov.hip -- the sums over the pooled samples behind MBAR's asymptotic covariance (Shirts & Chodera 2008,
// eq. 8 and appendix D; MBARModel.predict_with_error / free_energy / effective_samples).  With the columns
//   W_nk = p_kn / N_k              (sampled state k; p_kn the softmax of txm_mbar_eval at the solution's g)
//   W_na = v_an / sum_n v_an       (target a; v_an = e^{-a ut_n - logDt_n - M_a}, the weight of txm_mbar_predict)
// and d_nc = x_nc - mean_ac (mean: txm_mbar_predict's output, known before the pass) the covariance needs, per target,
//   Q_a = sum_n W_na^2   B_ak = sum_n W_nk W_na   yy_ac = sum_n W_na^2 d_nc^2   b_kac = sum_n W_nk W_na d_nc.
//
// One pass over u, logD and x behind predict's exact max pass (mbar_max_kernel: M_a, so no exponent is positive).  Per
// target the contraction over the sample axis is the product of the rows {p_k v_a (k < K), v_a} with the columns
// {d_c (c < C), 1}: FP64 matrix-pipe work.  The row of v_a against the column of ones is the denominator sum_n v_an, which
// so rides in the same pass; the rows p_k v_a against it are B_ak.
//
// A workgroup (four waves) takes (sample block, group of 16 columns, state, tile of 16 rows) and walks its samples in
// tiles of 64:
//   phase 1  four lanes per sample: the softmax p_kn of all K states (two reads of g, alpha0 from LDS, K exps per sample;
//            only the 16 rows of this workgroup are kept, P[sample][row]) and the NA target weights V[sample][a];
//            samples past the state's end get zeros.
//   phase 2  a wave takes four of the tile's sixteen 4-sample steps.  Lane (m = lane & 15, q = lane >> 4) holds
//            A[m][q] = P[sample q][row m] V[sample q][a] and B[q][m] = d of (sample q, column m) -- one
//            v_mfma_f64_16x16x4_f64 per (step, target) into the target's accumulator tile D[row][column] -- and adds
//            (v_a d)^2 for its own (sample, column) on the VALU: yy_ac, and Q_a in the column of ones.
// At the end the four waves' tiles are added in wave order through LDS and ONE partial per (workgroup, target, row,
// column) is written; mbar_cov_final_kernel adds the workgroups in index order and normalises.  No atomics: two runs give
// the same bits.
#include <cmath>
#include <cstring>

#include "txm_mbar.h"

namespace txm {

typedef double cv_v4d __attribute__((ext_vector_type(4)));

constexpr int CV_TILE = 64;               // samples per tile
constexpr int CV_LDP = 17;                // row pitch of P (16 rows + one pad double)
constexpr int CV_ROWS = 17;               // partial rows per target: 16 matrix rows, then yy
constexpr int CV_PART = MB_MAXA * CV_ROWS * 16;  // doubles per workgroup

// grid (sample blocks, column groups, K * RT); partial [state][gridDim.x][NCG][RT][MB_MAXA][CV_ROWS][16]
template <int NA>
__global__ __launch_bounds__(MB_BLOCK) void mbar_cov_kernel(const txm_mbar_state *__restrict__ tab, int K, int RT,
                                                            int64_t C, const double *__restrict__ gk,
                                                            const double *__restrict__ a0k,
                                                            const double *__restrict__ logD, double upiv,
                                                            const MbarTargets ta, const double *__restrict__ M,
                                                            const double *__restrict__ mean, int n_alpha,
                                                            double *__restrict__ partial) {
  __shared__ double P[CV_TILE * CV_LDP];
  __shared__ double V[CV_TILE * MB_MAXA];
  __shared__ double sg[MB_MAXK], sa[MB_MAXK];
  __shared__ double red[4 * 16 * 16], redy[4 * 64];
  const int tid = threadIdx.x;
  const int s = blockIdx.z / RT, rt = blockIdx.z % RT, cg = blockIdx.y;
  const double *__restrict__ x = tab[s].x;
  const double *__restrict__ u = tab[s].u;
  const int64_t n = tab[s].n, ldx = tab[s].ldx_s;
  const int64_t off = mb_state_offset(tab, s);
  const int row0 = 16 * rt;  // logical rows row0 .. row0 + 15: k < K the states, K the row of ones, above it zeros
  if (tid < K) {
    sg[tid] = gk[tid];
    sa[tid] = a0k[tid];
  }
  for (int e = tid; e < CV_TILE * CV_LDP; e += MB_BLOCK) P[e] = 0.0;
  // phase 1 roles
  const int j = tid >> 2, q = tid & 3;
  double al1[2], M1[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int a = q + 4 * t < NA ? q + 4 * t : NA - 1;
    al1[t] = ta.a[a];
    M1[t] = M[a];
  }
  // phase 2 roles
  const int wave = tid >> 6, lane = tid & 63, m = lane & 15, k4 = lane >> 4;
  const int64_t col = (int64_t)cg * 16 + m;  // logical column: < C an observable, C the ones, above it nothing
  const bool is_x = col < C, is_one = col == C;
  double mu[NA];
#pragma unroll
  for (int a = 0; a < NA; ++a) mu[a] = is_x ? mean[(int64_t)(a < n_alpha ? a : n_alpha - 1) * C + col] : 0.0;
  cv_v4d acc[NA];
  double yy[NA];
#pragma unroll
  for (int a = 0; a < NA; ++a) {
    acc[a] = cv_v4d{0.0, 0.0, 0.0, 0.0};
    yy[a] = 0.0;
  }
  __syncthreads();
  for (int64_t base = (int64_t)blockIdx.x * CV_TILE; base < n; base += (int64_t)gridDim.x * CV_TILE) {
    {
      const int64_t i = base + j;
      const bool ok = i < n;
      const double ut = ok ? u[i] - upiv : 0.0;
      const double nld = ok ? -logD[off + i] : 0.0;
      double mx = -INFINITY;
      for (int k = q; k < K; k += 4) mx = fmax(mx, fma(-sa[k], ut, sg[k]));
      mx = fmax(mx, __shfl_xor(mx, 1));
      mx = fmax(mx, __shfl_xor(mx, 2));
      double sum = 0.0;
      for (int k = q; k < K; k += 4) {
        const double e = exp(fma(-sa[k], ut, sg[k]) - mx);  // K < 4 leaves lanes with mx = -inf and no k: no exp taken
        sum += e;
        if (k >= row0 && k < row0 + 16) P[j * CV_LDP + k - row0] = e;
      }
      sum += __shfl_xor(sum, 1);
      sum += __shfl_xor(sum, 2);
      const double inv = ok ? 1.0 / sum : 0.0;
      for (int k = q; k < K; k += 4)
        if (k >= row0 && k < row0 + 16) P[j * CV_LDP + k - row0] *= inv;
      if (q == 0 && K >= row0 && K < row0 + 16) P[j * CV_LDP + K - row0] = ok ? 1.0 : 0.0;
#pragma unroll
      for (int t = 0; t < 2; ++t)
        if (q + 4 * t < NA) V[j * MB_MAXA + q + 4 * t] = ok ? exp(fma(-al1[t], ut, nld) - M1[t]) : 0.0;
    }
    __syncthreads();
#pragma unroll 1  // unrolled, eight targets take 198 + 64 registers: one wave per SIMD instead of two
    for (int st = 0; st < 4; ++st) {
      const int nn = 4 * (4 * wave + st) + k4;
      const int64_t i = base + nn;
      const bool ok = i < n;
      const double pm = P[nn * CV_LDP + m];
      double xv = 0.0;
      if (ok && is_x) xv = x[i * ldx + col];
#pragma unroll
      for (int a = 0; a < NA; ++a) {
        const double va = V[nn * MB_MAXA + a];
        const double d = (ok && is_x) ? xv - mu[a] : ((ok && is_one) ? 1.0 : 0.0);
        acc[a] = __builtin_amdgcn_mfma_f64_16x16x4f64(pm * va, d, acc[a], 0, 0, 0);
        const double t = va * d;
        yy[a] = fma(t, t, yy[a]);
      }
    }
    __syncthreads();
  }
  // the four waves' tiles in wave order.  D layout: column = lane & 15, row = (lane >> 4) + 4 * reg
  double *dst = partial + ((((size_t)s * gridDim.x + blockIdx.x) * gridDim.y + cg) * RT + rt) * CV_PART;
#pragma unroll
  for (int a = 0; a < NA; ++a) {
#pragma unroll
    for (int r = 0; r < 4; ++r) red[(wave * 16 + k4 + 4 * r) * 16 + m] = acc[a][r];
    redy[(wave * 4 + k4) * 16 + m] = yy[a];
    __syncthreads();
    {
      double v = red[tid];
#pragma unroll
      for (int w = 1; w < 4; ++w) v += red[w * 256 + tid];
      dst[(size_t)a * CV_ROWS * 16 + tid] = v;
    }
    if (tid < 16) {
      double v = redy[tid];
#pragma unroll
      for (int w = 1; w < 16; ++w) v += redy[w * 16 + tid];
      dst[((size_t)a * CV_ROWS + 16) * 16 + tid] = v;
    }
    __syncthreads();
  }
}

// one block per (output entry, target): the workgroups' partials in index order (strided, then a tree), the denominator
// the same way, then the normalisation.  out [n_alpha][1 + K + C (1 + K)]: Q_a, B_ak, then (yy_ac, b_kac) per column
__global__ __launch_bounds__(MB_BLOCK) void mbar_cov_final_kernel(const txm_mbar_state *__restrict__ tab,
                                                                  const double *__restrict__ partial, int nblk, int NCG,
                                                                  int RT, int K, int64_t C, const double *__restrict__ M,
                                                                  double *__restrict__ out, double *__restrict__ lnw) {
  const int64_t e = blockIdx.x;
  const int a = blockIdx.y;
  // entry -> (logical row, logical column); row -1 is yy
  int row;
  int64_t col;
  if (e <= K) {
    col = C;
    row = e == 0 ? -1 : (int)(e - 1);
  } else {
    const int64_t r = e - 1 - K;
    col = r / (1 + K);
    row = (int)(r % (1 + K)) - 1;
  }
  const size_t pitch = (size_t)NCG * RT * CV_PART;
  const size_t at_num = ((size_t)(col / 16) * RT + (row < 0 ? 0 : row / 16)) * CV_PART +
                        ((size_t)a * CV_ROWS + (row < 0 ? 16 : row % 16)) * 16 + (size_t)(col % 16);
  const size_t at_den = ((size_t)(C / 16) * RT + K / 16) * CV_PART + ((size_t)a * CV_ROWS + K % 16) * 16 + (size_t)(C % 16);
  double num = 0.0, den = 0.0;
  for (int b = threadIdx.x; b < nblk; b += MB_BLOCK) {
    num += partial[(size_t)b * pitch + at_num];
    den += partial[(size_t)b * pitch + at_den];
  }
  __shared__ double sn[MB_BLOCK], sd[MB_BLOCK];
  sn[threadIdx.x] = num;
  sd[threadIdx.x] = den;
  __syncthreads();
  for (int o = MB_BLOCK / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      sn[threadIdx.x] += sn[threadIdx.x + o];
      sd[threadIdx.x] += sd[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double scale = row < 0 ? sd[0] * sd[0] : (double)tab[row].n * sd[0];
    out[(size_t)a * (size_t)(1 + K + C * (1 + K)) + (size_t)e] = sn[0] / scale;
    if (e == 0 && lnw) lnw[a] = M[a] + log(sd[0]);
  }
}

static void cv_plan(int32_t K, int64_t C, int64_t *ncg, int64_t *rt, int64_t *cap) {
  *ncg = C / 16 + 1;             // the columns and the column of ones
  *rt = K / 16 + 1;              // the states and the row of ones
  int64_t c = (int64_t)num_cus() * 8 / ((int64_t)K * *ncg * *rt);  // about num_cus * 8 workgroups in all
  *cap = c < 1 ? 1 : c;
}

}  // namespace txm

using namespace txm;

extern "C" size_t txm_mbar_cov_ws_bytes(int32_t K, int64_t C, int32_t n_alpha) {
  if (K < 1 || K > MB_MAXK || C < 1 || C > 65535 || n_alpha < 1 || n_alpha > MB_MAXA) return 0;
  int64_t ncg, rt, cap;
  cv_plan(K, C, &ncg, &rt, &cap);
  const size_t pcov = (size_t)K * cap * ncg * rt * CV_PART;
  const size_t pmax = (size_t)K * (size_t)mb_blocks_per_state(K) * MB_MAXA;
  return MB_HEAD_BYTES + (pcov > pmax ? pcov : pmax) * sizeof(double) + 256;
}

extern "C" int txm_mbar_cov(const txm_mbar_state *states_host, int32_t K, int64_t C, double upiv,
                            const double *alpha0_host, const double *g_host, const double *logD,
                            const double *alpha_host, int32_t n_alpha, const double *mean, double *out, double *lnw,
                            void *ws, size_t ws_bytes, txm_stream stream) {
  TXM_REQUIRE(C >= 1 && C <= 65535, "mbar_cov: C = %lld outside [1, 65535]", (long long)C);
  TXM_REQUIRE(states_host && K >= 1 && K <= MB_MAXK, "mbar_cov: K = %d states outside [1, %d] or a null state table",
              (int)K, MB_MAXK);
  int64_t nmax = 0;
  if (const int rc = mb_check_states(states_host, K, true, true, C, "mbar_cov", nullptr, &nmax)) return rc;
  TXM_REQUIRE(alpha0_host && g_host && logD && alpha_host && mean && out && ws, "mbar_cov: null pointer");
  TXM_REQUIRE(n_alpha >= 1 && n_alpha <= MB_MAXA, "mbar_cov: n_alpha = %d outside [1, %d]", (int)n_alpha, MB_MAXA);
  if (const int rc = mb_check_finite("mbar_cov", K, alpha0_host, g_host, n_alpha, alpha_host, upiv)) return rc;
  if (ws_bytes < txm_mbar_cov_ws_bytes(K, C, n_alpha)) {
    set_error("mbar_cov: workspace too small");
    return TXM_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  // one staging copy: state table, g, alpha0 (the head of txm_mbar_eval)
  MbarHead h;
  if (const int rc = mb_stage_head(ws, states_host, K, g_host, alpha0_host, MB_TAB_BYTES, nullptr, 0, st, &h)) return rc;
  const txm_mbar_state *tab = h.tab;
  const double *gk = h.gk, *a0k = h.a0k;
  double *M = h.M;
  double *partial = (double *)((char *)ws + MB_HEAD_BYTES);
  const MbarTargets ta = mb_targets(alpha_host, n_alpha);
  // exact per-target maximum of the exponent (predict's pass)
  if (const int rc = mb_max_pass(tab, K, nmax, mb_blocks_per_state(K), logD, upiv, ta, partial, M, st)) return rc;
  int64_t ncg, rt, cap;
  cv_plan(K, C, &ncg, &rt, &cap);
  int64_t gx = cdiv(nmax, (int64_t)CV_TILE * 4);
  gx = gx > cap ? cap : (gx < 1 ? 1 : gx);
  const dim3 grid((unsigned)gx, (unsigned)ncg, (unsigned)(K * rt)), block(MB_BLOCK);
#define TXM_CV(NA_)                                                                                                 \
  hipLaunchKernelGGL((mbar_cov_kernel<NA_>), grid, block, 0, st, tab, (int)K, (int)rt, C, gk, a0k, logD, upiv, ta, M, \
                     mean, (int)n_alpha, partial)
  TXM_MB_NA_DISPATCH(n_alpha, TXM_CV)
#undef TXM_CV
  TXM_LAUNCH_CHECK();
  hipLaunchKernelGGL(mbar_cov_final_kernel, dim3((unsigned)(1 + K + C * (1 + K)), (unsigned)n_alpha), dim3(MB_BLOCK), 0,
                     st, tab, partial, (int)(gx * K), (int)ncg, (int)rt, (int)K, C, M, out, lnw);
  TXM_LAUNCH_CHECK();
  return TXM_OK;
}
