// txm_mbar_boot.hip -- bootstrap of MBAR (MBARModel.bootstrap; extends reference models.py:1049-1111, whose
// MBARModel.resample raises at 1109-1111): nrep weighted MBAR problems over the same pooled samples of K states,
// replicate r giving pooled sample n the integer count c_n^r of the counter-based multinomial sampler (txm_sampler.h).
//
//   logD_n^r = ln sum_k e^{g_k^r - alpha0_k ut_n}                      (g, ut as in txm_mbar.hip)
//   S_k^r = sum_n c_n^r p_kn^r,  H_jk^r = sum_n c_n^r p_jn^r p_kn^r,  obj^r = sum_n c_n^r logD_n^r
//   <x>^r(a) = sum_n c_n^r w_an^r x_n / sum_n c_n^r w_an^r,  w_an^r = e^{-a ut_n - logD_n^r}
//
// Work unit: ONE WAVE per (replicate, state, chunk of whole 1024-sample sampler tiles).  For each tile the wave draws
// the replicate's per-sample counts into a wave-private LDS tile (sampler_fine_tile, LDS integer atomics), compacts
// the samples with a non-zero count into a list in sample order (ballot + prefix count: e^-1 = 37 % of the samples of
// a bootstrap replicate are not drawn and cost nothing after this), and spends one lane per listed sample.  Nothing of
// size nrep x N_total exists: the counts live in LDS, logD is recomputed from g^r by predict.
//
// The chunking of a state's tiles depends on (n_s, K) only, every partial is written by exactly one wave and the
// partials are added in index order by one thread per output: results are bitwise reproducible, and a replicate's
// result does not depend on which other replicates are in the call.
//
// Evaluation: K <= 8 keeps S, the triangle and the objective of a lane in registers (as mbar_eval_kernel); 8 < K <= 64
// puts the p_kn of 64 listed samples in LDS and gives each lane fixed triangle entries (as mbar_eval_lds_kernel).
// Predict: the exponent of (replicate r, target a) is shifted by M_a^r = Mref_a - min_k (g_k^r - gref_k), with Mref_a the
// exact maximum of -a ut_n - logD_n at the reference log-weights gref (the point solution: a max pass of its own).
// Because D_n^r >= e^{min_k (g^r - gref)_k} D_n^ref, no shifted exponent is positive (no overflow), and the largest is
// no lower than -(max_k - min_k)(g^r - gref) minus the gap to the largest DRAWN sample -- a few units for a bootstrap
// replicate, at most ~50 along the flat valley of states without overlap, against an underflow threshold of 708.
#include <cmath>
#include <cstring>

#include "txm_mbar.h"  // mb_check_state, mb_na_class
#include "txm_sampler.h"

namespace txm {

constexpr int BT_MAXK = 64;
constexpr int BT_REGK = 8;
constexpr int BT_MAXA = 8;
constexpr int BT_WAVES = 4;  // tasks (waves) per workgroup of the register and predict kernels
constexpr int BT_REFMAX_BLOCKS = 2048;

struct BootDev {
  const double *x, *u;
  const uint32_t *counts;  // [nrep][ntiles]
  int64_t n, ldx_s;
  uint32_t k0, k1, rep0;
  int32_t ntiles, last_tile, tpc, nchunks, choff;  // tiles per chunk, chunks, index of this state's first chunk
};

struct BootTargets {
  double a[BT_MAXA];
};

// workspace: [state table | alpha0 | gref | Mref] [partials of the reference max pass] [partials]
constexpr size_t BT_OFF_A0 = BT_MAXK * sizeof(BootDev);
constexpr size_t BT_OFF_GREF = BT_OFF_A0 + BT_MAXK * sizeof(double);
constexpr size_t BT_OFF_MREF = BT_OFF_GREF + BT_MAXK * sizeof(double);
constexpr size_t BT_HEAD_BYTES = (BT_OFF_MREF + BT_MAXA * sizeof(double) + 255) / 256 * 256;
constexpr size_t BT_REFMAX_BYTES = (size_t)BT_REFMAX_BLOCKS * BT_MAXA * sizeof(double);

static inline int64_t bt_chunk_cap(int64_t K) { return 256 / K < 1 ? 1 : 256 / K; }

__device__ __forceinline__ void wave_lds_sync() {
  // wave-private LDS: the DS operations of one wave execute in order, only the compiler needs fencing
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ double bt_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ double bt_wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}

// Counts of (row r of the state's sampler, tile t) into cnt[1024], then the drawn samples into list[] in sample
// order as (offset in tile) | (count << 10).  Returns how many are listed.  One wave; cnt and list are its own.
__device__ __forceinline__ uint32_t boot_draw_tile(const BootDev &st, uint32_t r, uint32_t t, uint32_t *cnt,
                                                   uint32_t *list, int lane) {
  uint4 *z = reinterpret_cast<uint4 *>(cnt);
#pragma unroll
  for (int e = 0; e < SM_T / 4 / 64; ++e) z[e * 64 + lane] = make_uint4(0, 0, 0, 0);
  wave_lds_sync();
  const uint32_t tsize = (t == (uint32_t)st.ntiles - 1u) ? (uint32_t)st.last_tile : (uint32_t)SM_T;
  const uint32_t n = st.counts[(size_t)r * st.ntiles + t];
  sampler_fine_tile(st.k0, st.k1, st.rep0 + r, t, n, tsize, lane, [&](uint32_t off) { atomicAdd(&cnt[off], 1u); });
  wave_lds_sync();
  uint32_t nnz = 0;
#pragma unroll 4
  for (int j = 0; j < SM_T / 64; ++j) {
    const uint32_t idx = (uint32_t)(j * 64 + lane);
    const uint32_t c = cnt[idx];
    const unsigned long long mask = __ballot(c != 0u);
    if (c) list[nnz + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = idx | (c << SM_LT);
    nnz += (uint32_t)__popcll(mask);
  }
  wave_lds_sync();
  return nnz;
}

// ---- evaluation, K <= 8 ------------------------------------------------------------------------------------------
// grid: flat over (group of 4 active replicates, chunk, state); partial [slot][total chunks][NV]
template <int K>
__global__ __launch_bounds__(BT_WAVES * 64) void mbar_boot_eval_kernel(const BootDev *__restrict__ tab,
                                                                       const double *__restrict__ a0k,
                                                                       const double *__restrict__ gall,
                                                                       const int32_t *__restrict__ active,
                                                                       int64_t n_active, int64_t ngroups, int maxch,
                                                                       int64_t TC, double upiv,
                                                                       double *__restrict__ partial) {
  constexpr int NH = K * (K + 1) / 2;
  constexpr int NV = K + NH + 1;
  __shared__ uint32_t s_cnt[BT_WAVES][SM_T], s_list[BT_WAVES][SM_T];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t b = blockIdx.x;
  const int64_t slot = (b % ngroups) * BT_WAVES + wave;
  const int64_t rest = b / ngroups;
  const int chunk = (int)(rest % maxch), s = (int)(rest / maxch);
  if (slot >= n_active) return;  // (no workgroup barrier below: waves leave on their own)
  const BootDev st = tab[s];
  if (chunk >= st.nchunks) return;
  const uint32_t r = active ? (uint32_t)active[slot] : (uint32_t)slot;
  uint32_t *cnt = s_cnt[wave], *list = s_list[wave];
  double g[K], a0[K], S[K], H[NH], obj = 0.0;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    g[k] = gall[(size_t)r * K + k];
    a0[k] = a0k[k];
    S[k] = 0.0;
  }
#pragma unroll
  for (int h = 0; h < NH; ++h) H[h] = 0.0;
  const int t_end = min((chunk + 1) * st.tpc, st.ntiles);
  for (int t = chunk * st.tpc; t < t_end; ++t) {
    const uint32_t nnz = boot_draw_tile(st, r, (uint32_t)t, cnt, list, lane);
    const double *__restrict__ ub = st.u + (int64_t)t * SM_T;
    for (uint32_t q0 = 0; q0 < nnz; q0 += 64u) {
      const uint32_t q = q0 + (uint32_t)lane;
      if (q < nnz) {
        const uint32_t ent = list[q];
        const double cw = (double)(ent >> SM_LT);
        const double ut = ub[ent & (uint32_t)(SM_T - 1)] - upiv;
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
        obj = fma(cw, m + log(sum), obj);
        const double inv = 1.0 / sum;
        double cp[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
          e[k] *= inv;
          cp[k] = cw * e[k];
          S[k] += cp[k];
        }
        int h = 0;
#pragma unroll
        for (int j = 0; j < K; ++j)
#pragma unroll
          for (int k = j; k < K; ++k, ++h) H[h] = fma(cp[j], e[k], H[h]);
      }
    }
    wave_lds_sync();
  }
  double *dst = partial + ((size_t)slot * TC + st.choff + chunk) * NV;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double v = bt_wave_sum(S[k]);
    if (lane == 0) dst[k] = v;
  }
#pragma unroll
  for (int h = 0; h < NH; ++h) {
    const double v = bt_wave_sum(H[h]);
    if (lane == 0) dst[K + h] = v;
  }
  {
    const double v = bt_wave_sum(obj);
    if (lane == 0) dst[K + NH] = v;
  }
}

// ---- evaluation, 8 < K <= KB: one wave per workgroup, the p of 64 listed samples in LDS --------------------------
template <int KB>
__global__ __launch_bounds__(64) void mbar_boot_eval_lds_kernel(const BootDev *__restrict__ tab, int K,
                                                                const double *__restrict__ a0k,
                                                                const double *__restrict__ gall,
                                                                const int32_t *__restrict__ active, int64_t n_active,
                                                                int maxch, int64_t TC, double upiv,
                                                                double *__restrict__ partial) {
  constexpr int R = (KB * (KB + 1) / 2 + 63) / 64;  // upper-triangle entries per lane
  __shared__ uint32_t cnt[SM_T], list[SM_T];
  __shared__ double P[64][KB + 1];
  __shared__ double sg[KB], sa[KB], cwv[64];
  const int lane = threadIdx.x;
  const int NH = K * (K + 1) / 2, NV = K + NH + 1;
  const int64_t b = blockIdx.x;
  const int64_t slot = b % n_active;
  const int64_t rest = b / n_active;
  const int chunk = (int)(rest % maxch), s = (int)(rest / maxch);
  const BootDev st = tab[s];
  if (chunk >= st.nchunks) return;
  const uint32_t r = active ? (uint32_t)active[slot] : (uint32_t)slot;
  for (int k = lane; k < K; k += 64) {
    sg[k] = gall[(size_t)r * K + k];
    sa[k] = a0k[k];
  }
  int hr[R], hc[R];
#pragma unroll
  for (int i = 0; i < R; ++i) {
    int e = lane + i * 64, row = 0;
    if (e < NH) {
      while (e >= K - row) {
        e -= K - row;
        ++row;
      }
      hr[i] = row;
      hc[i] = row + e;
    } else {
      hr[i] = hc[i] = -1;
    }
  }
  double h[R], Sk = 0.0, obj = 0.0;
#pragma unroll
  for (int i = 0; i < R; ++i) h[i] = 0.0;
  wave_lds_sync();
  const int t_end = min((chunk + 1) * st.tpc, st.ntiles);
  for (int t = chunk * st.tpc; t < t_end; ++t) {
    const uint32_t nnz = boot_draw_tile(st, r, (uint32_t)t, cnt, list, lane);
    const double *__restrict__ ub = st.u + (int64_t)t * SM_T;
    for (uint32_t q0 = 0; q0 < nnz; q0 += 64u) {
      const uint32_t q = q0 + (uint32_t)lane;
      const bool ok = q < nnz;
      const uint32_t ent = ok ? list[q] : 0u;
      const double cw = ok ? (double)(ent >> SM_LT) : 0.0;
      const double ut = ok ? ub[ent & (uint32_t)(SM_T - 1)] - upiv : 0.0;
      double m = -INFINITY;
      for (int k = 0; k < K; ++k) m = fmax(m, fma(-sa[k], ut, sg[k]));
      double sum = 0.0;
      for (int k = 0; k < K; ++k) {
        const double e = exp(fma(-sa[k], ut, sg[k]) - m);
        P[lane][k] = e;
        sum += e;
      }
      const double inv = ok ? 1.0 / sum : 0.0;
      for (int k = 0; k < K; ++k) P[lane][k] *= inv;
      cwv[lane] = cw;
      obj = fma(cw, m + log(sum), obj);
      wave_lds_sync();
#pragma unroll
      for (int i = 0; i < R; ++i)
        if (hr[i] >= 0)
          for (int j = 0; j < 64; ++j) h[i] = fma(cwv[j] * P[j][hr[i]], P[j][hc[i]], h[i]);
      if (lane < K)
        for (int j = 0; j < 64; ++j) Sk = fma(cwv[j], P[j][lane], Sk);
      wave_lds_sync();
    }
  }
  double *dst = partial + ((size_t)slot * TC + st.choff + chunk) * NV;
  if (lane < K) dst[lane] = Sk;
#pragma unroll
  for (int i = 0; i < R; ++i)
    if (hr[i] >= 0) dst[K + lane + i * 64] = h[i];
  const double v = bt_wave_sum(obj);
  if (lane == 0) dst[K + NH] = v;
}

// one thread per (slot, entry): the chunk partials in index order
__global__ __launch_bounds__(256) void mbar_boot_sum_kernel(const double *__restrict__ partial,
                                                            const int32_t *__restrict__ active, int64_t n_active,
                                                            int64_t TC, int NV, double *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_active * NV) return;
  const int64_t slot = i / NV;
  const int q = (int)(i % NV);
  const double *src = partial + (size_t)slot * TC * NV + q;
  double acc = 0.0;
  for (int64_t j = 0; j < TC; ++j) acc += src[(size_t)j * NV];
  const int64_t r = active ? (int64_t)active[slot] : slot;
  out[(size_t)r * NV + q] = acc;
}

// ---- predict -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ double boot_logd(const double *sg, const double *sa, int K, double ut) {
  double m = -INFINITY;
  for (int k = 0; k < K; ++k) m = fmax(m, fma(-sa[k], ut, sg[k]));
  double sum = 0.0;
  for (int k = 0; k < K; ++k) sum += exp(fma(-sa[k], ut, sg[k]) - m);
  return m + log(sum);
}

// Mref: exact max over ALL pooled samples of -a ut - logD at the reference log-weights; partial [state][gridDim.x][8]
__global__ __launch_bounds__(256) void mbar_boot_refmax_kernel(const BootDev *__restrict__ tab, int K,
                                                               const double *__restrict__ a0k,
                                                               const double *__restrict__ gref, double upiv,
                                                               const BootTargets ta, double *__restrict__ partial) {
  __shared__ double sg[BT_MAXK], sa[BT_MAXK];
  __shared__ double sw[4][BT_MAXA];
  if ((int)threadIdx.x < K) {
    sg[threadIdx.x] = gref[threadIdx.x];
    sa[threadIdx.x] = a0k[threadIdx.x];
  }
  __syncthreads();
  const int s = blockIdx.y;
  const double *__restrict__ u = tab[s].u;
  const int64_t n = tab[s].n;
  double m[BT_MAXA];
#pragma unroll
  for (int a = 0; a < BT_MAXA; ++a) m[a] = -INFINITY;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const double ut = u[i] - upiv;
    const double nld = -boot_logd(sg, sa, K, ut);
#pragma unroll
    for (int a = 0; a < BT_MAXA; ++a) m[a] = fmax(m[a], fma(-ta.a[a], ut, nld));
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int a = 0; a < BT_MAXA; ++a) {
    const double v = bt_wave_max(m[a]);
    if (lane == 0) sw[wave][a] = v;
  }
  __syncthreads();
  if (threadIdx.x < BT_MAXA) {
    double v = sw[0][threadIdx.x];
    for (int w = 1; w < 4; ++w) v = fmax(v, sw[w][threadIdx.x]);
    partial[((size_t)s * gridDim.x + blockIdx.x) * BT_MAXA + threadIdx.x] = v;
  }
}

__global__ __launch_bounds__(256) void mbar_boot_refmax_final_kernel(const double *__restrict__ partial, int nblk,
                                                                     double *__restrict__ M) {
  __shared__ double sw[4][BT_MAXA];
  double m[BT_MAXA];
#pragma unroll
  for (int a = 0; a < BT_MAXA; ++a) m[a] = -INFINITY;
  for (int b = threadIdx.x; b < nblk; b += 256)
#pragma unroll
    for (int a = 0; a < BT_MAXA; ++a) m[a] = fmax(m[a], partial[(size_t)b * BT_MAXA + a]);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int a = 0; a < BT_MAXA; ++a) {
    const double v = bt_wave_max(m[a]);
    if (lane == 0) sw[wave][a] = v;
  }
  __syncthreads();
  if (threadIdx.x < BT_MAXA) {
    double v = sw[0][threadIdx.x];
    for (int w = 1; w < 4; ++w) v = fmax(v, sw[w][threadIdx.x]);
    M[threadIdx.x] = v;
  }
}

// grid: flat over (group of 4 replicates, chunk, state, column chunk of LPR = 2^lpr_log2 columns).
// Phase 1 (a lane per listed sample): logD from g^r, the NA weights c w_a into LDS, the denominators.
// Phase 2 (a lane per (row group, column)): num_a[col] += w_a[sample] x[sample][col] over the 64 listed samples.
// partial [replicate][total chunks][NA][cpad + 1]: the numerators of the cpad padded columns, then the denominator.
// PIPE: phase 2 keeps eight x loads in flight per lane (the rows are a gather through the list; one at a time the loop
// runs at the latency of a miss per listed sample).  Chosen by the host when a lane has >= 8 samples per step (>= 8 columns
// per row group); with fewer the extra registers cost a wave per SIMD and the plain loop is faster.
template <int NA, bool PIPE>
__global__ __launch_bounds__(BT_WAVES * 64) void mbar_boot_predict_kernel(
    const BootDev *__restrict__ tab, int K, int64_t C, int lpr_log2, int64_t cpad, const double *__restrict__ a0k,
    const double *__restrict__ gall, const double *__restrict__ gref, const double *__restrict__ Mref,
    const BootTargets ta, double upiv, int64_t nrep, int64_t ngroups, int maxch, int64_t TC,
    double *__restrict__ partial) {
  __shared__ uint32_t s_cnt[BT_WAVES][SM_T], s_list[BT_WAVES][SM_T];
  __shared__ double s_g[BT_WAVES][BT_MAXK], s_a[BT_WAVES][BT_MAXK];
  static_assert(64 * BT_MAXA * sizeof(double) <= SM_T * sizeof(uint32_t), "the weights reuse the count tile");
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int64_t rest = blockIdx.x;
  const int64_t r64 = (rest % ngroups) * BT_WAVES + wave;
  rest /= ngroups;
  const int chunk = (int)(rest % maxch);
  rest /= maxch;
  const int s = (int)(rest % K);
  const int64_t cc = rest / K;
  if (r64 >= nrep) return;
  const BootDev st = tab[s];
  if (chunk >= st.nchunks) return;
  const uint32_t r = (uint32_t)r64;
  uint32_t *cnt = s_cnt[wave], *list = s_list[wave];
  double *W = reinterpret_cast<double *>(cnt);  // [64][NA], live between a tile's listing and the next tile's draw
  double *sg = s_g[wave], *sa = s_a[wave];
  for (int k = lane; k < K; k += 64) {
    sg[k] = gall[(size_t)r * K + k];
    sa[k] = a0k[k];
  }
  double dmin = INFINITY;
  for (int k = 0; k < K; ++k) dmin = fmin(dmin, gall[(size_t)r * K + k] - gref[k]);
  double M[NA], den[NA], num[NA];
#pragma unroll
  for (int a = 0; a < NA; ++a) {
    M[a] = Mref[a] - dmin;
    den[a] = 0.0;
    num[a] = 0.0;
  }
  const int LPR = 1 << lpr_log2, ROWS = 64 >> lpr_log2;
  const int rg = lane >> lpr_log2;
  const int64_t col = cc * LPR + (lane & (LPR - 1));
  const bool col_ok = col < C;
  wave_lds_sync();
  const int t_end = min((chunk + 1) * st.tpc, st.ntiles);
  for (int t = chunk * st.tpc; t < t_end; ++t) {
    const uint32_t nnz = boot_draw_tile(st, r, (uint32_t)t, cnt, list, lane);
    const double *__restrict__ ub = st.u + (int64_t)t * SM_T;
    const double *__restrict__ xb = st.x + (int64_t)t * SM_T * st.ldx_s;
    for (uint32_t q0 = 0; q0 < nnz; q0 += 64u) {
      const uint32_t q = q0 + (uint32_t)lane;
      const bool ok = q < nnz;
      const uint32_t ent = ok ? list[q] : 0u;
      const double cw = ok ? (double)(ent >> SM_LT) : 0.0;
      const double ut = ok ? ub[ent & (uint32_t)(SM_T - 1)] - upiv : 0.0;
      const double nld = -boot_logd(sg, sa, K, ut);
#pragma unroll
      for (int a = 0; a < NA; ++a) {
        const double w = ok ? cw * exp(fma(-ta.a[a], ut, nld) - M[a]) : 0.0;
        den[a] += w;
        W[lane * NA + a] = w;
      }
      wave_lds_sync();
      const int here = (int)min(64u, nnz - q0);
      if (col_ok && !PIPE) {
        for (int j = rg; j < here; j += ROWS) {
          const uint32_t off = list[q0 + (uint32_t)j] & (uint32_t)(SM_T - 1);
          const double xv = xb[(int64_t)off * st.ldx_s + col];
#pragma unroll
          for (int a = 0; a < NA; ++a) num[a] = fma(W[j * NA + a], xv, num[a]);
        }
      }
      if (col_ok && PIPE) {
        constexpr int XU = 8;
        for (int j0 = rg; j0 < here; j0 += ROWS * XU) {
          double xv[XU];
#pragma unroll
          for (int e = 0; e < XU; ++e) {
            const int j = j0 + e * ROWS;
            xv[e] = 0.0;
            if (j < here) {
              const uint32_t off = list[q0 + (uint32_t)j] & (uint32_t)(SM_T - 1);
              xv[e] = xb[(int64_t)off * st.ldx_s + col];
            }
          }
#pragma unroll
          for (int e = 0; e < XU; ++e) {
            const int j = j0 + e * ROWS;
            if (j < here) {
#pragma unroll
              for (int a = 0; a < NA; ++a) num[a] = fma(W[j * NA + a], xv[e], num[a]);
            }
          }
        }
      }
      wave_lds_sync();
    }
  }
  double *dst = partial + ((size_t)r * TC + st.choff + chunk) * NA * (size_t)(cpad + 1);
#pragma unroll
  for (int a = 0; a < NA; ++a) {
    double v = num[a];
    for (int o = 32; o >= LPR; o >>= 1) v += __shfl_xor(v, o);  // the row groups of a column, butterfly
    if (rg == 0) dst[(size_t)a * (cpad + 1) + cc * LPR + lane] = v;
    const double d = bt_wave_sum(den[a]);
    if (lane == 0 && cc == 0) dst[(size_t)a * (cpad + 1) + cpad] = d;
  }
}

// one thread per (replicate, target, column): the chunk partials in index order, then the quotient
__global__ __launch_bounds__(256) void mbar_boot_predict_final_kernel(const double *__restrict__ partial, int64_t nrep,
                                                                      int64_t TC, int NA, int n_alpha, int64_t C,
                                                                      int64_t cpad, double *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nrep * n_alpha * C) return;
  const int64_t c = i % C;
  const int a = (int)((i / C) % n_alpha);
  const int64_t r = i / (C * n_alpha);
  const double *src = partial + ((size_t)r * TC * NA + a) * (size_t)(cpad + 1);
  const size_t stride = (size_t)NA * (cpad + 1);
  double num = 0.0, den = 0.0;
  for (int64_t j = 0; j < TC; ++j) {
    num += src[j * stride + c];
    den += src[j * stride + cpad];
  }
  out[i] = num / den;
}

// ---- host side ---------------------------------------------------------------------------------------------------
static int64_t bt_chunks_bound(int32_t K, int64_t n_total) {
  const int64_t a = cdiv(n_total, SM_T) + K, b = (int64_t)K * bt_chunk_cap(K);
  return a < b ? a : b;
}

static int bt_lpr_log2(int64_t C) {
  int l2 = 0;
  while ((1 << l2) < C && l2 < 6) ++l2;
  return l2;
}

// checks the two host tables and fills the device table; TC = chunks over all states, maxch = most of one state
static int bt_check(const txm_mbar_state *states, const txm_mbar_boot_state *samp, int32_t K, bool need_x, int64_t C,
                    const char *what, BootDev *dev, int64_t *ntot, int64_t *nrep, int64_t *TC, int *maxch) {
  TXM_REQUIRE(states, "%s: null state table", what);
  TXM_REQUIRE(samp, "%s: null sampler table", what);
  TXM_REQUIRE(K >= 1 && K <= BT_MAXK, "%s: K = %d states outside [1, %d]", what, (int)K, BT_MAXK);
  *ntot = 0;
  *TC = 0;
  *maxch = 0;
  *nrep = samp[0].spec.nrep;
  TXM_REQUIRE(*nrep >= 1 && *nrep <= ((int64_t)1 << 24), "%s: nrep = %lld outside [1, 2^24]", what, (long long)*nrep);
  for (int32_t s = 0; s < K; ++s) {
    const txm_mbar_state &st = states[s];
    const txm_sampler_spec &sp = samp[s].spec;
    if (const int rc = mb_check_state(st, s, need_x, false, C, what)) return rc;
    TXM_REQUIRE(st.n <= ((int64_t)1 << 30), "%s: state %d has n = %lld samples (sampler limit 2^30)", what, (int)s,
                (long long)st.n);
    TXM_REQUIRE(samp[s].counts, "%s: state %d has null sampler counts", what, (int)s);
    TXM_REQUIRE(sp.ndat == st.n, "%s: state %d: sampler ndat = %lld but n = %lld", what, (int)s, (long long)sp.ndat,
                (long long)st.n);
    TXM_REQUIRE(sp.nsamp == 0 || sp.nsamp == sp.ndat, "%s: state %d: sampler nsamp = %lld (MBAR resamples n out of n)",
                what, (int)s, (long long)sp.nsamp);
    TXM_REQUIRE(sp.nrep == *nrep, "%s: state %d: sampler nrep = %lld differs from state 0's %lld", what, (int)s,
                (long long)sp.nrep, (long long)*nrep);
    TXM_REQUIRE(sp.rep0 >= 0 && sp.rep0 + sp.nrep <= ((int64_t)1 << 32),
                "%s: state %d: stream replicates [%lld, %lld) outside [0, 2^32)", what, (int)s, (long long)sp.rep0,
                (long long)(sp.rep0 + sp.nrep));
    BootDev &d = dev[s];
    d.x = st.x;
    d.u = st.u;
    d.counts = samp[s].counts;
    d.n = st.n;
    d.ldx_s = st.ldx_s;
    d.k0 = (uint32_t)sp.seed;
    d.k1 = (uint32_t)(sp.seed >> 32);
    d.rep0 = (uint32_t)sp.rep0;
    const int64_t ntiles = cdiv(st.n, SM_T), cap = bt_chunk_cap(K);
    const int64_t nch0 = ntiles < cap ? ntiles : cap;
    d.ntiles = (int32_t)ntiles;
    d.last_tile = (int32_t)(st.n - (ntiles - 1) * SM_T);
    d.tpc = (int32_t)cdiv(ntiles, nch0);
    d.nchunks = (int32_t)cdiv(ntiles, d.tpc);
    d.choff = (int32_t)*TC;
    *TC += d.nchunks;
    *maxch = d.nchunks > *maxch ? d.nchunks : *maxch;
    *ntot += st.n;
  }
  return TXM_OK;
}

}  // namespace txm

using namespace txm;

extern "C" size_t txm_mbar_boot_ws_bytes(int32_t K, int64_t C, int32_t n_alpha, int64_t n_total, int64_t nrep) {
  if (K < 1 || K > BT_MAXK || C < 1 || C > 65535 || n_alpha < 1 || n_alpha > BT_MAXA || n_total < K ||
      n_total > (int64_t)K << 30 || nrep < 1 || nrep > ((int64_t)1 << 24))
    return 0;
  const size_t TC = (size_t)bt_chunks_bound(K, n_total);
  const size_t nv = (size_t)K + (size_t)K * (K + 1) / 2 + 1;
  const int l2 = bt_lpr_log2(C);
  const size_t cpad = (size_t)cdiv(C, (int64_t)1 << l2) << l2;
  const size_t pe = (size_t)nrep * TC * nv;
  const size_t pp = (size_t)nrep * TC * (size_t)mb_na_class(n_alpha) * (cpad + 1);
  return BT_HEAD_BYTES + BT_REFMAX_BYTES + (pe > pp ? pe : pp) * sizeof(double) + 256;
}

extern "C" int txm_mbar_boot_eval(const txm_mbar_state *states_host, const txm_mbar_boot_state *samplers_host,
                                  int32_t K, const double *alpha0_host, const double *g, const int32_t *active,
                                  int64_t n_active, double upiv, double *out, void *ws, size_t ws_bytes,
                                  txm_stream stream) {
  alignas(16) unsigned char head[BT_HEAD_BYTES] = {};
  int64_t ntot = 0, nrep = 0, TC = 0;
  int maxch = 0;
  const int rc = bt_check(states_host, samplers_host, K, false, 0, "mbar_boot_eval", reinterpret_cast<BootDev *>(head),
                          &ntot, &nrep, &TC, &maxch);
  if (rc != TXM_OK) return rc;
  TXM_REQUIRE(alpha0_host && g && out && ws, "mbar_boot_eval: null pointer");
  for (int32_t k = 0; k < K; ++k)
    TXM_REQUIRE(std::isfinite(alpha0_host[k]), "mbar_boot_eval: alpha0 of state %d not finite", (int)k);
  TXM_REQUIRE(std::isfinite(upiv), "mbar_boot_eval: pivot not finite");
  TXM_REQUIRE(n_active >= 1 && n_active <= nrep, "mbar_boot_eval: n_active = %lld outside [1, nrep = %lld]",
              (long long)n_active, (long long)nrep);
  if (ws_bytes < txm_mbar_boot_ws_bytes(K, 1, 1, ntot, nrep)) {
    set_error("mbar_boot_eval: workspace too small");
    return TXM_ERR_WORKSPACE;
  }
  const int64_t ngroups = K <= BT_REGK ? cdiv(n_active, BT_WAVES) : n_active;
  const int64_t blocks = ngroups * maxch * K;
  TXM_REQUIRE(blocks < ((int64_t)1 << 31), "mbar_boot_eval: %lld workgroups exceed the grid limit", (long long)blocks);
  hipStream_t st = (hipStream_t)stream;
  memcpy(head + BT_OFF_A0, alpha0_host, (size_t)K * sizeof(double));
  TXM_HIP(hipMemcpyAsync(ws, head, BT_OFF_GREF, hipMemcpyHostToDevice, st));
  const BootDev *tab = (const BootDev *)ws;
  const double *a0k = (const double *)((char *)ws + BT_OFF_A0);
  double *partial = (double *)((char *)ws + BT_HEAD_BYTES + BT_REFMAX_BYTES);
  const int NV = K + K * (K + 1) / 2 + 1;
  const dim3 grid((unsigned)blocks);
  switch (K) {
#define TXM_BT_EVAL(KK)                                                                                              \
  case KK:                                                                                                           \
    hipLaunchKernelGGL((mbar_boot_eval_kernel<KK>), grid, dim3(BT_WAVES * 64), 0, st, tab, a0k, g, active, n_active, \
                       ngroups, maxch, TC, upiv, partial);                                                           \
    break;
    TXM_BT_EVAL(1) TXM_BT_EVAL(2) TXM_BT_EVAL(3) TXM_BT_EVAL(4) TXM_BT_EVAL(5) TXM_BT_EVAL(6) TXM_BT_EVAL(7)
    TXM_BT_EVAL(8)
#undef TXM_BT_EVAL
    default:
      if (K <= 16)
        hipLaunchKernelGGL((mbar_boot_eval_lds_kernel<16>), grid, dim3(64), 0, st, tab, (int)K, a0k, g, active,
                           n_active, maxch, TC, upiv, partial);
      else if (K <= 32)
        hipLaunchKernelGGL((mbar_boot_eval_lds_kernel<32>), grid, dim3(64), 0, st, tab, (int)K, a0k, g, active,
                           n_active, maxch, TC, upiv, partial);
      else
        hipLaunchKernelGGL((mbar_boot_eval_lds_kernel<64>), grid, dim3(64), 0, st, tab, (int)K, a0k, g, active,
                           n_active, maxch, TC, upiv, partial);
  }
  TXM_LAUNCH_CHECK();
  hipLaunchKernelGGL(mbar_boot_sum_kernel, dim3((unsigned)cdiv(n_active * NV, 256)), dim3(256), 0, st, partial, active,
                     n_active, TC, NV, out);
  TXM_LAUNCH_CHECK();
  return TXM_OK;
}

extern "C" int txm_mbar_boot_predict(const txm_mbar_state *states_host, const txm_mbar_boot_state *samplers_host,
                                     int32_t K, int64_t C, double upiv, const double *alpha0_host, const double *g,
                                     const double *gref_host, const double *alpha_host, int32_t n_alpha, double *out,
                                     void *ws, size_t ws_bytes, txm_stream stream) {
  TXM_REQUIRE(C >= 1 && C <= 65535, "mbar_boot_predict: C = %lld outside [1, 65535]", (long long)C);
  alignas(16) unsigned char head[BT_HEAD_BYTES] = {};
  int64_t ntot = 0, nrep = 0, TC = 0;
  int maxch = 0;
  const int rc = bt_check(states_host, samplers_host, K, true, C, "mbar_boot_predict",
                          reinterpret_cast<BootDev *>(head), &ntot, &nrep, &TC, &maxch);
  if (rc != TXM_OK) return rc;
  TXM_REQUIRE(alpha0_host && g && gref_host && alpha_host && out && ws, "mbar_boot_predict: null pointer");
  TXM_REQUIRE(n_alpha >= 1 && n_alpha <= BT_MAXA, "mbar_boot_predict: n_alpha = %d outside [1, %d]", (int)n_alpha,
              BT_MAXA);
  for (int32_t k = 0; k < K; ++k)
    TXM_REQUIRE(std::isfinite(alpha0_host[k]) && std::isfinite(gref_host[k]),
                "mbar_boot_predict: alpha0 / gref of state %d not finite", (int)k);
  for (int32_t a = 0; a < n_alpha; ++a)
    TXM_REQUIRE(std::isfinite(alpha_host[a]), "mbar_boot_predict: target %d not finite", (int)a);
  TXM_REQUIRE(std::isfinite(upiv), "mbar_boot_predict: pivot not finite");
  if (ws_bytes < txm_mbar_boot_ws_bytes(K, C, n_alpha, ntot, nrep)) {
    set_error("mbar_boot_predict: workspace too small");
    return TXM_ERR_WORKSPACE;
  }
  const int l2 = bt_lpr_log2(C);
  const int64_t colchunks = cdiv(C, (int64_t)1 << l2), cpad = colchunks << l2;
  const int64_t ngroups = cdiv(nrep, BT_WAVES);
  const int64_t blocks = ngroups * maxch * K * colchunks;
  TXM_REQUIRE(blocks < ((int64_t)1 << 31), "mbar_boot_predict: %lld workgroups exceed the grid limit",
              (long long)blocks);
  hipStream_t st = (hipStream_t)stream;
  memcpy(head + BT_OFF_A0, alpha0_host, (size_t)K * sizeof(double));
  memcpy(head + BT_OFF_GREF, gref_host, (size_t)K * sizeof(double));
  TXM_HIP(hipMemcpyAsync(ws, head, BT_OFF_MREF, hipMemcpyHostToDevice, st));
  const BootDev *tab = (const BootDev *)ws;
  const double *a0k = (const double *)((char *)ws + BT_OFF_A0);
  const double *gref = (const double *)((char *)ws + BT_OFF_GREF);
  double *Mref = (double *)((char *)ws + BT_OFF_MREF);
  double *pmax = (double *)((char *)ws + BT_HEAD_BYTES);
  double *partial = (double *)((char *)ws + BT_HEAD_BYTES + BT_REFMAX_BYTES);
  BootTargets ta;
  for (int a = 0; a < BT_MAXA; ++a) ta.a[a] = alpha_host[a < n_alpha ? a : n_alpha - 1];
  int64_t nmax = 0;
  for (int32_t s = 0; s < K; ++s) nmax = states_host[s].n > nmax ? states_host[s].n : nmax;
  int64_t gm = cdiv(nmax, (int64_t)256 * 8);
  const int64_t capm = BT_REFMAX_BLOCKS / K;
  gm = gm > capm ? capm : (gm < 1 ? 1 : gm);
  hipLaunchKernelGGL(mbar_boot_refmax_kernel, dim3((unsigned)gm, (unsigned)K), dim3(256), 0, st, tab, (int)K, a0k,
                     gref, upiv, ta, pmax);
  TXM_LAUNCH_CHECK();
  hipLaunchKernelGGL(mbar_boot_refmax_final_kernel, dim3(1), dim3(256), 0, st, pmax, (int)(gm * K), Mref);
  TXM_LAUNCH_CHECK();
  const int NA = mb_na_class(n_alpha);
  const dim3 grid((unsigned)blocks), block(BT_WAVES * 64);
#define TXM_BT_PRED(NA_)                                                                                              \
  do {                                                                                                                \
    if (l2 >= 3)                                                                                                      \
      hipLaunchKernelGGL((mbar_boot_predict_kernel<NA_, true>), grid, block, 0, st, tab, (int)K, C, l2, cpad, a0k, g, \
                         gref, Mref, ta, upiv, nrep, ngroups, maxch, TC, partial);                                    \
    else                                                                                                              \
      hipLaunchKernelGGL((mbar_boot_predict_kernel<NA_, false>), grid, block, 0, st, tab, (int)K, C, l2, cpad, a0k,   \
                         g, gref, Mref, ta, upiv, nrep, ngroups, maxch, TC, partial);                                 \
  } while (0)
  TXM_MB_NA_DISPATCH(n_alpha, TXM_BT_PRED)
#undef TXM_BT_PRED
  TXM_LAUNCH_CHECK();
  hipLaunchKernelGGL(mbar_boot_predict_final_kernel, dim3((unsigned)cdiv(nrep * n_alpha * C, 256)), dim3(256), 0, st,
                     partial, nrep, TC, NA, (int)n_alpha, C, cpad, out);
  TXM_LAUNCH_CHECK();
  return TXM_OK;
}
