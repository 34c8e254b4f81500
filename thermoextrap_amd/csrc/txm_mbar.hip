// txm_mbar.hip -- MBAR over the pooled samples of K states (MBARModel, reference models.py:1049-1111, which
// hands u_kn = alpha0_k u_n to pymbar):
//
//   logD_n = ln sum_k N_k e^{f_k - alpha0_k u_n}          (every pooled sample n)
//   f_j    = -ln sum_n e^{-alpha0_j u_n - logD_n}          (the self-consistent free energies, gauge f_0 = 0)
//   <x>(a) = sum_n x_n e^{-a u_n - logD_n} / sum_n e^{-a u_n - logD_n}
//
// The kernels see u only as ut_n = u_n - upiv (one host-chosen pivot) and the free energies only as the shifted
// log-weights g_k = ln N_k + f_k - alpha0_k upiv (+ any constant the host picks), so that
//   p_kn = softmax_k(g_k - alpha0_k ut_n)   (taken with the max subtracted: no exponent is ever positive)
//   logDt_n = max_k(.) + ln sum_k e^{. - max}  (= logD_n + that constant; predictions do not see the constant).
//
// Evaluation pass (the solve's hot loop, one read of u): S_k = sum_n p_kn (the gradient of the MBAR objective is
// S_k - N_k), the Hessian term H_jk = sum_n p_jn p_kn (upper triangle), the objective sum_n logDt_n, and -- when
// asked -- logDt_n of every pooled sample, which predict then reads instead of recomputing the K exps.
// K <= 8: one sample per lane, every sum in registers (K exps, one log, K(K+1)/2 FMAs per sample).
// 8 < K <= 64: tiles of 64 samples, four lanes per sample for the exps, the p_kn of a tile in LDS, and each lane owns
// fixed entries of the upper triangle.
//
// Predict (targets in tiles of <= 8, as txm_perturb): a max pass over ut and logDt gives the exact per-target maximum
// M_a = max_n (-a ut_n - logDt_n); the contraction pass forms w_an = e^{-a ut_n - logDt_n - M_a} and sums w and w x_c
// in txm_perturb's layout (a lane owns VEC fixed columns, the lanes of a row share the exps of the targets); a finalize
// kernel divides.
//
// The states are never pooled into one copy: every grid has an axis over states and reads a table of per-state
// pointers that the call copies into the workspace (as txm_reduce_vals_batched).  All partials are combined in a
// fixed order (no atomics): results are bitwise reproducible from run to run on one device.
#include <cmath>
#include <cstring>

#include "txm_mbar.h"

namespace txm {

__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ inline double wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}

// partial layout: [state][gridDim.x][NV], NV = K + K(K+1)/2 + 1: S_k, H (upper triangle, row-major), objective
template <int K>
__global__ __launch_bounds__(MB_BLOCK) void mbar_eval_kernel(const txm_mbar_state *__restrict__ tab,
                                                             const double *__restrict__ gk,
                                                             const double *__restrict__ a0k, double upiv,
                                                             double *__restrict__ logD, double *__restrict__ partial) {
  constexpr int NH = K * (K + 1) / 2;
  constexpr int NV = K + NH + 1;
  const int s = blockIdx.y;
  const double *__restrict__ u = tab[s].u;
  const int64_t n = tab[s].n;
  const int64_t off = mb_state_offset(tab, s);
  double g[K], a0[K], S[K], H[NH], obj = 0.0;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    g[k] = gk[k];
    a0[k] = a0k[k];
    S[k] = 0.0;
  }
#pragma unroll
  for (int h = 0; h < NH; ++h) H[h] = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * MB_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * MB_BLOCK) {
    const double ut = u[i] - upiv;
    double e[K], m = -INFINITY;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      e[k] = fma(-a0[k], ut, g[k]);
      m = fmax(m, e[k]);
    }
    double sum = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      e[k] = exp(e[k] - m);
      sum += e[k];
    }
    const double ld = m + log(sum);
    if (logD) logD[off + i] = ld;
    obj += ld;
    const double inv = 1.0 / sum;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      e[k] *= inv;
      S[k] += e[k];
    }
    int h = 0;
#pragma unroll
    for (int j = 0; j < K; ++j)
#pragma unroll
      for (int k = j; k < K; ++k, ++h) H[h] = fma(e[j], e[k], H[h]);
  }
  // wave sums (butterfly: every lane ends with the same bits), then the four waves in order
  __shared__ double sw[MB_BLOCK / TXM_WAVE][NV];
  const int wave = threadIdx.x / TXM_WAVE, lane = threadIdx.x % TXM_WAVE;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double v = wave_sum(S[k]);
    if (lane == 0) sw[wave][k] = v;
  }
#pragma unroll
  for (int h = 0; h < NH; ++h) {
    const double v = wave_sum(H[h]);
    if (lane == 0) sw[wave][K + h] = v;
  }
  {
    const double v = wave_sum(obj);
    if (lane == 0) sw[wave][K + NH] = v;
  }
  __syncthreads();
  double *dst = partial + ((size_t)s * gridDim.x + blockIdx.x) * NV;
  for (int q = threadIdx.x; q < NV; q += MB_BLOCK) {
    double acc = 0.0;
    for (int w = 0; w < MB_BLOCK / TXM_WAVE; ++w) acc += sw[w][q];
    dst[q] = acc;
  }
}

// 8 < K <= KB: a tile of MB_TILE samples per step, four lanes per sample (lane q of a sample takes k = q, q+4, ...)
template <int KB>
__global__ __launch_bounds__(MB_BLOCK) void mbar_eval_lds_kernel(const txm_mbar_state *__restrict__ tab, int K,
                                                                 const double *__restrict__ gk,
                                                                 const double *__restrict__ a0k, double upiv,
                                                                 double *__restrict__ logD,
                                                                 double *__restrict__ partial) {
  constexpr int R = (KB * (KB + 1) / 2 + MB_BLOCK - 1) / MB_BLOCK;  // upper-triangle entries per lane
  __shared__ double P[MB_TILE][KB + 1];
  __shared__ double sg[KB], sa[KB], so[MB_TILE];
  const int tid = threadIdx.x, j = tid >> 2, q = tid & 3;
  const int NH = K * (K + 1) / 2, NV = K + NH + 1;
  const int s = blockIdx.y;
  const double *__restrict__ u = tab[s].u;
  const int64_t n = tab[s].n;
  const int64_t off = mb_state_offset(tab, s);
  if (tid < K) {
    sg[tid] = gk[tid];
    sa[tid] = a0k[tid];
  }
  // the (row, column) of the upper-triangle entries this lane owns: e = tid + r * MB_BLOCK
  int hr[R], hc[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    int e = tid + r * MB_BLOCK, row = 0;
    if (e < NH) {
      while (e >= K - row) {
        e -= K - row;
        ++row;
      }
      hr[r] = row;
      hc[r] = row + e;
    } else {
      hr[r] = hc[r] = -1;
    }
  }
  double h[R], Sk = 0.0, obj = 0.0;
#pragma unroll
  for (int r = 0; r < R; ++r) h[r] = 0.0;
  __syncthreads();
  for (int64_t base = (int64_t)blockIdx.x * MB_TILE; base < n; base += (int64_t)gridDim.x * MB_TILE) {
    const int64_t i = base + j;
    const bool ok = i < n;
    const double ut = ok ? u[i] - upiv : 0.0;
    double m = -INFINITY;
    for (int k = q; k < K; k += 4) {
      const double t = fma(-sa[k], ut, sg[k]);
      P[j][k] = t;
      m = fmax(m, t);
    }
    m = fmax(m, __shfl_xor(m, 1));
    m = fmax(m, __shfl_xor(m, 2));
    double sum = 0.0;
    for (int k = q; k < K; k += 4) {
      const double e = exp(P[j][k] - m);
      P[j][k] = e;
      sum += e;
    }
    sum += __shfl_xor(sum, 1);
    sum += __shfl_xor(sum, 2);
    const double inv = ok ? 1.0 / sum : 0.0;
    for (int k = q; k < K; k += 4) P[j][k] *= inv;
    if (q == 0 && ok) {
      const double ld = m + log(sum);
      obj += ld;
      if (logD) logD[off + i] = ld;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (hr[r] >= 0)
        for (int t = 0; t < MB_TILE; ++t) h[r] = fma(P[t][hr[r]], P[t][hc[r]], h[r]);
    if (tid < K)
      for (int t = 0; t < MB_TILE; ++t) Sk += P[t][tid];
    __syncthreads();
  }
  if (q == 0) so[j] = obj;
  __syncthreads();
  double *dst = partial + ((size_t)s * gridDim.x + blockIdx.x) * NV;
  if (tid < K) dst[tid] = Sk;
#pragma unroll
  for (int r = 0; r < R; ++r)
    if (hr[r] >= 0) dst[K + tid + r * MB_BLOCK] = h[r];
  if (tid == 0) {
    double acc = 0.0;
    for (int t = 0; t < MB_TILE; ++t) acc += so[t];
    dst[K + NH] = acc;
  }
}

// one block per output entry: sum over all (state, block) partials, strided then a tree (fixed order)
__global__ __launch_bounds__(MB_BLOCK) void mbar_sum_kernel(const double *__restrict__ partial, int nblk, int NV,
                                                            double *__restrict__ out) {
  const int q = blockIdx.x;
  double acc = 0.0;
  for (int b = threadIdx.x; b < nblk; b += MB_BLOCK) acc += partial[(size_t)b * NV + q];
  __shared__ double sh[MB_BLOCK];
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int o = MB_BLOCK / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[q] = sh[0];
}

// ---- predict --------------------------------------------------------------------------------------------------
// partial layout: [state][gridDim.x][MB_MAXA]; unused targets repeat the last one
__global__ __launch_bounds__(MB_BLOCK) void mbar_max_kernel(const txm_mbar_state *__restrict__ tab,
                                                            const double *__restrict__ logD, double upiv,
                                                            const MbarTargets ta, double *__restrict__ partial) {
  const int s = blockIdx.y;
  const double *__restrict__ u = tab[s].u;
  const int64_t n = tab[s].n;
  const int64_t off = mb_state_offset(tab, s);
  double m[MB_MAXA];
#pragma unroll
  for (int a = 0; a < MB_MAXA; ++a) m[a] = -INFINITY;
  for (int64_t i = (int64_t)blockIdx.x * MB_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * MB_BLOCK) {
    const double ut = u[i] - upiv, ld = logD[off + i];
#pragma unroll
    for (int a = 0; a < MB_MAXA; ++a) m[a] = fmax(m[a], fma(-ta.a[a], ut, -ld));
  }
  __shared__ double sw[MB_BLOCK / TXM_WAVE][MB_MAXA];
  const int wave = threadIdx.x / TXM_WAVE, lane = threadIdx.x % TXM_WAVE;
#pragma unroll
  for (int a = 0; a < MB_MAXA; ++a) {
    const double v = wave_max(m[a]);
    if (lane == 0) sw[wave][a] = v;
  }
  __syncthreads();
  if (threadIdx.x < MB_MAXA) {
    double v = sw[0][threadIdx.x];
    for (int w = 1; w < MB_BLOCK / TXM_WAVE; ++w) v = fmax(v, sw[w][threadIdx.x]);
    partial[((size_t)s * gridDim.x + blockIdx.x) * MB_MAXA + threadIdx.x] = v;
  }
}

// one block: strided over the partials, then a tree (a max is exact in any order; one serial lane took 0.3 ms)
__global__ __launch_bounds__(MB_BLOCK) void mbar_max_final_kernel(const double *__restrict__ partial, int nblk,
                                                                  double *__restrict__ M) {
  double m[MB_MAXA];
#pragma unroll
  for (int a = 0; a < MB_MAXA; ++a) m[a] = -INFINITY;
  for (int b = threadIdx.x; b < nblk; b += MB_BLOCK)
#pragma unroll
    for (int a = 0; a < MB_MAXA; ++a) m[a] = fmax(m[a], partial[(size_t)b * MB_MAXA + a]);
  __shared__ double sw[MB_BLOCK / TXM_WAVE][MB_MAXA];
  const int wave = threadIdx.x / TXM_WAVE, lane = threadIdx.x % TXM_WAVE;
#pragma unroll
  for (int a = 0; a < MB_MAXA; ++a) {
    const double v = wave_max(m[a]);
    if (lane == 0) sw[wave][a] = v;
  }
  __syncthreads();
  if (threadIdx.x < MB_MAXA) {
    double v = sw[0][threadIdx.x];
    for (int w = 1; w < MB_BLOCK / TXM_WAVE; ++w) v = fmax(v, sw[w][threadIdx.x]);
    M[threadIdx.x] = v;
  }
}

// partial layout: [state][gridDim.x][cols_pad][NA][2]  (num, den) -- txm_perturb's, with the state on grid z
template <int NA, int VEC, int LPR_LOG2>
__global__ __launch_bounds__(MB_BLOCK) void mbar_predict_kernel(const txm_mbar_state *__restrict__ tab, int64_t C,
                                                                const double *__restrict__ logD, double upiv,
                                                                const MbarTargets ta, const double *__restrict__ M,
                                                                double *__restrict__ partial) {
  constexpr int LPR = 1 << LPR_LOG2;
  constexpr int ROWS = MB_BLOCK / LPR;
  const int tid = threadIdx.x;
  const int lir = tid & (LPR - 1), rib = tid >> LPR_LOG2;
  const int s = blockIdx.z;
  const double *__restrict__ x = tab[s].x;
  const double *__restrict__ u = tab[s].u;
  const int64_t N = tab[s].n, ldx_s = tab[s].ldx_s;
  const int64_t off = mb_state_offset(tab, s);
  const int64_t col0 = (int64_t)blockIdx.y * (LPR * VEC) + (int64_t)lir * VEC;
  const bool col_ok = col0 < C;
  double Ma[NA];
#pragma unroll
  for (int a = 0; a < NA; ++a) Ma[a] = M[a];
  double num[NA][VEC], den[NA];
#pragma unroll
  for (int a = 0; a < NA; ++a) {
    den[a] = 0.0;
#pragma unroll
    for (int v = 0; v < VEC; ++v) num[a][v] = 0.0;
  }
  const int64_t stride = (int64_t)gridDim.x * ROWS;
  const int64_t cols_left = C - (int64_t)blockIdx.y * (LPR * VEC);
  const int64_t nvalid = (cols_left + VEC - 1) / VEC;
  const bool share = (LPR >= NA) && (LPR <= 64) && (NA > 1) && (nvalid >= NA);
  if (col_ok) {
    for (int64_t i = (int64_t)blockIdx.x * ROWS + rib; i < N; i += stride) {
      double xv[VEC];
      if constexpr (VEC == 2) {
        const double2 t2 = *reinterpret_cast<const double2 *>(x + i * ldx_s + col0);
        xv[0] = t2.x;
        xv[1] = t2.y;
      } else {
        xv[0] = x[i * ldx_s + col0];
      }
      const double ut = u[i] - upiv, nld = -logD[off + i];
      if (share) {
        // lane `lir` of a row evaluates target number lir; the row's lanes fetch the NA weights (as txm_perturb)
        const int a_mine = lir < NA ? lir : 0;
        double al_mine = ta.a[0], M_mine = Ma[0];
#pragma unroll
        for (int a = 1; a < NA; ++a)
          if (a_mine == a) {
            al_mine = ta.a[a];
            M_mine = Ma[a];
          }
        const double w_mine = exp(fma(-al_mine, ut, nld) - M_mine);
        const int lane = tid & 63;
        const int row_lane0 = lane & ~(LPR - 1);
#pragma unroll
        for (int a = 0; a < NA; ++a) {
          const double w = __shfl(w_mine, row_lane0 + a);
          den[a] += w;
#pragma unroll
          for (int v = 0; v < VEC; ++v) num[a][v] = fma(w, xv[v], num[a][v]);
        }
      } else {
#pragma unroll
        for (int a = 0; a < NA; ++a) {
          const double w = exp(fma(-ta.a[a], ut, nld) - Ma[a]);
          den[a] += w;
#pragma unroll
          for (int v = 0; v < VEC; ++v) num[a][v] = fma(w, xv[v], num[a][v]);
        }
      }
    }
  }
  // block reduction over the ROWS row slots of a column (fixed order)
  constexpr int NV = NA * (1 + VEC);
  __shared__ double sh[MB_BLOCK * NV];
  double *mine = sh + (size_t)tid * NV;
#pragma unroll
  for (int a = 0; a < NA; ++a) {
    mine[a * (1 + VEC)] = den[a];
#pragma unroll
    for (int v = 0; v < VEC; ++v) mine[a * (1 + VEC) + 1 + v] = num[a][v];
  }
  __syncthreads();
  const size_t cols_pad = (size_t)gridDim.y * LPR * VEC;
  for (int e = tid; e < LPR * NV; e += MB_BLOCK) {
    const int l = e / NV, q = e % NV;
    double acc = 0.0;
    for (int r = 0; r < ROWS; ++r) acc += sh[((size_t)r * LPR + l) * NV + q];
    const int a = q / (1 + VEC), k = q % (1 + VEC);
    double *dst = partial + (((size_t)s * gridDim.x + blockIdx.x) * cols_pad + (size_t)blockIdx.y * LPR * VEC +
                             (size_t)l * VEC) * NA * 2;
    if (k == 0) {
#pragma unroll
      for (int v = 0; v < VEC; ++v) dst[((size_t)v * NA + a) * 2 + 1] = acc;
    } else {
      dst[((size_t)(k - 1) * NA + a) * 2] = acc;
    }
  }
}

__global__ __launch_bounds__(MB_BLOCK) void mbar_predict_final_kernel(const double *__restrict__ partial, int nblk,
                                                                      int64_t cols_pad, int64_t C, int NA,
                                                                      double *__restrict__ out) {
  const int64_t c = blockIdx.x;
  const int a = blockIdx.z;
  double num = 0.0, den = 0.0;
  for (int b = threadIdx.x; b < nblk; b += MB_BLOCK) {
    const double *src = partial + (((size_t)b * cols_pad + c) * NA + a) * 2;
    num += src[0];
    den += src[1];
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
  if (threadIdx.x == 0) out[(size_t)a * C + c] = sn[0] / sd[0];
}

// ---- host side ------------------------------------------------------------------------------------------------
static int64_t mb_cols_pad_bound(int64_t C) {  // as txm_perturb_ws_bytes
  int64_t cols_pad = 1;
  while (cols_pad < C) cols_pad <<= 1;
  if (cols_pad > 512) cols_pad = cdiv(C, 512) * 512;
  return cols_pad;
}

}  // namespace txm

using namespace txm;

extern "C" size_t txm_mbar_ws_bytes(int32_t K, int64_t C, int32_t n_alpha) {
  if (K < 1 || K > MB_MAXK || C < 1 || C > 65535 || n_alpha < 1 || n_alpha > MB_MAXA) return 0;
  const size_t nblk = (size_t)K * mb_blocks_per_state(K);
  const size_t nv = (size_t)K + (size_t)K * (K + 1) / 2 + 1;
  size_t part = nblk * nv;
  const size_t pmax = nblk * MB_MAXA;
  const size_t pcon = nblk * (size_t)mb_cols_pad_bound(C) * n_alpha * 2;
  part = part > pmax ? part : pmax;
  part = part > pcon ? part : pcon;
  return MB_HEAD_BYTES + part * sizeof(double) + 256;
}

extern "C" int txm_mbar_eval(const txm_mbar_state *states_host, int32_t K, const double *alpha0_host,
                             const double *g_host, double upiv, double *out, double *logD, void *ws, size_t ws_bytes,
                             txm_stream stream) {
  int64_t ntot = 0, nmax = 0;
  if (const int rc = mb_check_states(states_host, K, false, false, 0, "mbar_eval", &ntot, &nmax)) return rc;
  TXM_REQUIRE(alpha0_host && g_host && out && ws, "mbar_eval: null pointer");
  if (const int rc = mb_check_finite("mbar_eval", K, alpha0_host, g_host, 0, nullptr, upiv)) return rc;
  if (ws_bytes < txm_mbar_ws_bytes(K, 1, 1)) {
    set_error("mbar_eval: workspace too small");
    return TXM_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  // one staging copy: state table, g, alpha0
  MbarHead h;
  if (const int rc = mb_stage_head(ws, states_host, K, g_host, alpha0_host, MB_TAB_BYTES, nullptr, 0, st, &h)) return rc;
  const txm_mbar_state *tab = h.tab;
  const double *gk = h.gk, *a0k = h.a0k;
  double *partial = (double *)((char *)ws + MB_HEAD_BYTES);
  const int NV = K + K * (K + 1) / 2 + 1;
  int64_t gx;
  if (K <= MB_REGK) {
    gx = cdiv(nmax, (int64_t)MB_BLOCK * 4);
  } else {
    gx = cdiv(nmax, (int64_t)MB_TILE * 4);
  }
  const int64_t cap = mb_blocks_per_state(K);
  gx = gx > cap ? cap : gx;
  gx = gx < 1 ? 1 : gx;
  const dim3 grid((unsigned)gx, (unsigned)K), block(MB_BLOCK);
  switch (K) {
#define TXM_MB_EVAL(KK) \
  case KK: hipLaunchKernelGGL((mbar_eval_kernel<KK>), grid, block, 0, st, tab, gk, a0k, upiv, logD, partial); break;
    TXM_MB_EVAL(1) TXM_MB_EVAL(2) TXM_MB_EVAL(3) TXM_MB_EVAL(4) TXM_MB_EVAL(5) TXM_MB_EVAL(6) TXM_MB_EVAL(7)
    TXM_MB_EVAL(8)
#undef TXM_MB_EVAL
    default:
      if (K <= 16)
        hipLaunchKernelGGL((mbar_eval_lds_kernel<16>), grid, block, 0, st, tab, (int)K, gk, a0k, upiv, logD, partial);
      else if (K <= 32)
        hipLaunchKernelGGL((mbar_eval_lds_kernel<32>), grid, block, 0, st, tab, (int)K, gk, a0k, upiv, logD, partial);
      else
        hipLaunchKernelGGL((mbar_eval_lds_kernel<64>), grid, block, 0, st, tab, (int)K, gk, a0k, upiv, logD, partial);
  }
  TXM_LAUNCH_CHECK();
  hipLaunchKernelGGL(mbar_sum_kernel, dim3((unsigned)NV), dim3(MB_BLOCK), 0, st, partial, (int)(gx * K), NV, out);
  TXM_LAUNCH_CHECK();
  return TXM_OK;
}

extern "C" int txm_mbar_predict(const txm_mbar_state *states_host, int32_t K, int64_t C, double upiv,
                                const double *logD, const double *alpha_host, int32_t n_alpha, double *out, void *ws,
                                size_t ws_bytes, txm_stream stream) {
  TXM_REQUIRE(C >= 1 && C <= 65535, "mbar_predict: C = %lld outside [1, 65535]", (long long)C);
  int64_t ntot = 0, nmax = 0;
  if (const int rc = mb_check_states(states_host, K, true, false, C, "mbar_predict", &ntot, &nmax)) return rc;
  TXM_REQUIRE(logD && alpha_host && out && ws, "mbar_predict: null pointer");
  TXM_REQUIRE(n_alpha >= 1 && n_alpha <= MB_MAXA, "mbar_predict: n_alpha = %d outside [1, %d]", (int)n_alpha, MB_MAXA);
  if (const int rc = mb_check_finite("mbar_predict", K, nullptr, nullptr, 0, nullptr, upiv)) return rc;  // (targets: not looked at)
  if (ws_bytes < txm_mbar_ws_bytes(K, C, n_alpha)) {
    set_error("mbar_predict: workspace too small");
    return TXM_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  // only the K entries of the state table, straight from the caller
  TXM_HIP(hipMemcpyAsync(ws, states_host, (size_t)K * sizeof(txm_mbar_state), hipMemcpyHostToDevice, st));
  const MbarHead h = mb_head(ws);
  const txm_mbar_state *tab = h.tab;
  double *M = h.M;
  double *partial = (double *)((char *)ws + MB_HEAD_BYTES);
  const MbarTargets ta = mb_targets(alpha_host, n_alpha);
  // exact per-target maximum of the exponent
  const int64_t cap = mb_blocks_per_state(K);
  if (const int rc = mb_max_pass(tab, K, nmax, cap, logD, upiv, ta, partial, M, st)) return rc;
  // the contraction: txm_perturb's plan (a lane owns VEC columns, 2^l2 lanes span a row); VEC = 2 when every state allows it
  bool v2 = (C % 2 == 0);
  for (int32_t s = 0; s < K && v2; ++s)
    v2 = (states_host[s].ldx_s % 2 == 0) && ((reinterpret_cast<uintptr_t>(states_host[s].x) & 15) == 0);
  const int vec = v2 ? 2 : 1;
  const int64_t lanes = cdiv(C, vec);
  int l2 = 0;
  while ((1 << l2) < lanes && l2 < 8) ++l2;
  const int cpc = (1 << l2) * vec;
  const int64_t chunks = cdiv(C, cpc);
  const int64_t cols_pad = chunks * cpc;
  int64_t gx = cdiv(nmax, (int64_t)(MB_BLOCK >> l2) * 4);
  gx = gx > cap ? cap : (gx < 1 ? 1 : gx);
  const dim3 grid((unsigned)gx, (unsigned)chunks, (unsigned)K), block(MB_BLOCK);
  bool launched = false;
#define TXM_MB(NA_, VEC_, L2_)                                                                                     \
  if (!launched && n_alpha == NA_ && vec == VEC_ && l2 == L2_) {                                                  \
    hipLaunchKernelGGL((mbar_predict_kernel<NA_, VEC_, L2_>), grid, block, 0, st, tab, C, logD, upiv, ta, M, partial); \
    launched = true;                                                                                               \
  }
#define TXM_MB_L(NA_, VEC_) \
  TXM_MB(NA_, VEC_, 0) TXM_MB(NA_, VEC_, 1) TXM_MB(NA_, VEC_, 2) TXM_MB(NA_, VEC_, 3) TXM_MB(NA_, VEC_, 4) \
  TXM_MB(NA_, VEC_, 5) TXM_MB(NA_, VEC_, 6) TXM_MB(NA_, VEC_, 7) TXM_MB(NA_, VEC_, 8)
#define TXM_MB_A(NA_) TXM_MB_L(NA_, 1) TXM_MB_L(NA_, 2)
  TXM_MB_A(1) TXM_MB_A(2) TXM_MB_A(3) TXM_MB_A(4) TXM_MB_A(5) TXM_MB_A(6) TXM_MB_A(7) TXM_MB_A(8)
#undef TXM_MB_A
#undef TXM_MB_L
#undef TXM_MB
  if (!launched) {
    set_error("mbar_predict: no kernel variant");
    return TXM_ERR_UNSUPPORTED;
  }
  TXM_LAUNCH_CHECK();
  hipLaunchKernelGGL(mbar_predict_final_kernel, dim3((unsigned)C, 1, (unsigned)n_alpha), dim3(MB_BLOCK), 0, st,
                     partial, (int)(gx * K), cols_pad, C, (int)n_alpha, out);
  TXM_LAUNCH_CHECK();
  return TXM_OK;
}
