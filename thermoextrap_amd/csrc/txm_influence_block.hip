// txm_influence_block.hip -- blocked (batch-means) delta-method covariance of derivative estimates for CORRELATED samples,
// with the whole blocking curve from one pass (ExtrapModel.derivs_cov(block=...) / blocking_curve).
//
// With psi_k(n) = sum_q (a[c][k][q] + b[c][k][q] dx) du^q as in txm_influence.hip and p_n = w_n / sum w, level-l block j
// covers the rows [j B 2^l, min(N, (j + 1) B 2^l)) and
//      z_j[c][k]      = sum_{n in block j} p_n psi_k(n)
//      cov[l][c][i][j'] = sum_j z_j[c][i] z_j[c][j']          (no nb / (nb - 1) factor: block = 1, level 0 is the iid V)
//      mean[c][k]     = sum_n p_n psi_k(n).
//
// psi is linear in the per-block shifted power sums, so the sample pass needs no coefficient per element:
//   pass 1 (influence_block_sums_kernel): per level-0 block and column  S0[q] = sum w du^q,  S1[q] = sum w dx du^q  (q < n_q:
//     one power chain and (1 + VEC) n_q fused multiply-adds per row at 8 bytes per value read), contracted ONCE PER BLOCK to the
//     unnormalised  zt[blk][c][k] = sum_q a_kq S0[q] + b_kq S1[q]  and  wb[blk] = S0[0].  The thread layout is
//     txm_influence.hip's row-major one (a lane owns VEC fixed columns; x read non-temporally); a block belongs to ONE
//     workgroup: its rows go round-robin over min(B, ROWS) row slots whose sums are added in slot order, so a block's bits
//     depend on (B, C, n_q, alignment) only, never on the launch width.  Blocks shorter than the ROWS row slots of a
//     workgroup are packed ROWS / B to a workgroup step.
//   pass 2 (influence_block_levels_kernel): a workgroup per column adds W = sum wb in a fixed order and then, level by
//     level, merges the pairs of the level below IN PLACE (zt[j 2^l] += zt[j 2^l + 2^(l-1)]; a last unpaired block stays)
//     while it accumulates the upper triangle of zt zt' -- fixed-order block sums, cov = that / W^2 mirrored, so every
//     cov[l][c] is bitwise symmetric.  No floating-point atomics anywhere: two calls give the same bits.
// A row of weight zero is selected out (it may hold anything); a block of total weight zero gives zt = 0; W = 0 gives zeros.
// First-order rounding bound: |cov - exact|[i][j'] <= few eps * sum_b beta_bi beta_bj',  beta_bk = sum_{n in b} p_n B_k(n),
// B_k = sum_q (|a_kq| + |b_kq| |dx|) |du|^q.
#include "txm_influence_block.h"

namespace txm {

constexpr int IB_BLOCK = 256;
constexpr int IB_CH = 8;  // values per pass of the workgroup reductions (8 * 256 doubles of LDS)

typedef double ib_v2d __attribute__((ext_vector_type(2)));

// one sample row into a lane's sums: s0[q] += w du^q, s1[v][q] += w dx_v du^q
template <int NQ, int VEC, bool WEIGHTED>
__device__ __forceinline__ void ib_body(double ui, double wi, const double (&xv)[VEC], double cu, const double (&px)[VEC],
                                        double (&s0)[NQ], double (&s1)[VEC][NQ]) {
  const bool live = !WEIGHTED || wi != 0.0;
  const double du = live ? ui - cu : 0.0;
  double dx[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) dx[v] = live ? xv[v] - px[v] : 0.0;
  double p = live ? wi : 0.0;  // w du^q
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    s0[q] += p;
#pragma unroll
    for (int v = 0; v < VEC; ++v) s1[v][q] = fma(dx[v], p, s1[v][q]);
    p *= du;
  }
}

// Thread layout: lane_in_row = tid & (LPR - 1) owns columns col0 + {0 .. VEC-1}, row slot = tid >> lpr_log2 (ROWS of them);
// blockIdx.y selects a chunk of LPR * VEC columns.  A workgroup step serves G = max(1, ROWS / B) consecutive level-0 blocks:
// block g of the step owns the Bs = min(B, ROWS) row slots g Bs .. g Bs + Bs - 1, slot j of a block reads its rows
// r0 + j, r0 + j + Bs, ...  Steps are grid-strided.  Dynamic LDS: stage [IB_CH][256] | s0red [G][NQ] | s1red [G][LPR VEC][NQ].
// zt: [nb][C][n_f], wb: [nb]
template <int NQ, int VEC, bool WEIGHTED>
__global__ __launch_bounds__(IB_BLOCK) void influence_block_sums_kernel(
    const double *__restrict__ x, int64_t ldx_s, const double *__restrict__ u, const double *__restrict__ w, int64_t N,
    int64_t C, double cu, const double *__restrict__ cx, const double *__restrict__ a, const double *__restrict__ b, int n_f,
    int64_t B, int64_t nb, int lpr_log2, int Bs, int G, double *__restrict__ zt, double *__restrict__ wb) {
  extern __shared__ __attribute__((aligned(16))) double ib_smem[];
  constexpr int NV = NQ + VEC * NQ, UNR = 4;
  const int LPR = 1 << lpr_log2, cols = LPR * VEC;
  double(*stage)[IB_BLOCK] = reinterpret_cast<double(*)[IB_BLOCK]>(ib_smem);
  double *s0red = ib_smem + IB_CH * IB_BLOCK;
  double *s1red = s0red + G * NQ;

  const int tid = threadIdx.x;
  const int lir = tid & (LPR - 1), rib = tid >> lpr_log2;
  const int g = rib / Bs, j = rib - g * Bs;
  const int64_t col0 = (int64_t)blockIdx.y * cols + (int64_t)lir * VEC;
  const bool col_ok = col0 < C;  // VEC == 2 requires C even, so col0 + 1 < C too
  double px[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) px[v] = col_ok ? cx[col0 + v] : 0.0;

  auto load = [&](int64_t r, double(&xv)[VEC]) {
    if constexpr (VEC == 2) {  // (read once: non-temporal, as the reduction does)
      const ib_v2d t = __builtin_nontemporal_load(reinterpret_cast<const ib_v2d *>(x + r * ldx_s + col0));
      xv[0] = t.x;
      xv[1] = t.y;
    } else {
      xv[0] = __builtin_nontemporal_load(x + r * ldx_s + col0);
    }
  };

  const int64_t n_steps = (nb + G - 1) / G;
  for (int64_t it = blockIdx.x; it < n_steps; it += gridDim.x) {
    double s0[NQ], s1[VEC][NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      s0[q] = 0.0;
#pragma unroll
      for (int v = 0; v < VEC; ++v) s1[v][q] = 0.0;
    }
    const int64_t blk = it * G + g;
    if (col_ok && g < G && blk < nb) {
      const int64_t r0 = blk * B, rend = (r0 + B < N) ? r0 + B : N;
      int64_t i = r0 + j;
      for (; i + (int64_t)(UNR - 1) * Bs < rend; i += (int64_t)UNR * Bs) {
        double xv[UNR][VEC], ui[UNR], wi[UNR];
#pragma unroll
        for (int q = 0; q < UNR; ++q) {
          const int64_t r = i + (int64_t)q * Bs;
          load(r, xv[q]);
          ui[q] = u[r];
          wi[q] = WEIGHTED ? w[r] : 1.0;
        }
#pragma unroll
        for (int q = 0; q < UNR; ++q) ib_body<NQ, VEC, WEIGHTED>(ui[q], wi[q], xv[q], cu, px, s0, s1);
      }
      for (; i < rend; i += Bs) {
        double xv[VEC];
        load(i, xv);
        ib_body<NQ, VEC, WEIGHTED>(u[i], WEIGHTED ? w[i] : 1.0, xv, cu, px, s0, s1);
      }
    }

    // every block's Bs row slots added in slot order, IB_CH of the lane's NV values per pass
#pragma unroll
    for (int c0 = 0; c0 < NV; c0 += IB_CH) {
#pragma unroll
      for (int k = 0; k < IB_CH; ++k) {
        const int q = c0 + k;  // compile-time: the sums stay in registers
        if (q < NQ)
          stage[k][tid] = s0[q];
        else if (q < NV)
          stage[k][tid] = s1[(q - NQ) / NQ][(q - NQ) % NQ];
      }
      __syncthreads();
      const int per = G << lpr_log2;  // (block of the step, lane in row): <= 256
      for (int e = tid; e < IB_CH * per; e += IB_BLOCK) {
        const int k = e / per, rem = e - k * per, gg = rem >> lpr_log2, l = rem & (LPR - 1), q = c0 + k;
        if (q < NV) {
          double acc = 0.0;
          for (int r = 0; r < Bs; ++r) acc += stage[k][((gg * Bs + r) << lpr_log2) + l];
          if (q < NQ) {  // S0: the same in every lane of a row slot
            if (l == 0) s0red[gg * NQ + q] = acc;
          } else {
            const int v = (q - NQ) / NQ, qq = (q - NQ) % NQ;
            s1red[((size_t)gg * cols + l * VEC + v) * NQ + qq] = acc;
          }
        }
      }
      __syncthreads();
    }

    // the contraction with the coefficients, once per block, column and estimate
    const int per_blk = cols * n_f;
    for (int e = tid; e < G * per_blk; e += IB_BLOCK) {
      const int gg = e / per_blk, rem = e - gg * per_blk, cl = rem / n_f, k = rem - cl * n_f;
      const int64_t bk = it * G + gg, col = (int64_t)blockIdx.y * cols + cl;
      if (bk < nb && col < C) {
        const double *ak = a + ((size_t)col * n_f + k) * NQ, *bkq = b + ((size_t)col * n_f + k) * NQ;
        const double *r0 = s0red + gg * NQ, *r1 = s1red + ((size_t)gg * cols + cl) * NQ;
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < NQ; ++q) s = fma(bkq[q], r1[q], fma(ak[q], r0[q], s));
        zt[((size_t)bk * C + col) * n_f + k] = s;
      }
    }
    if (blockIdx.y == 0)
      for (int e = tid; e < G; e += IB_BLOCK)
        if (it * G + e < nb) wb[it * G + e] = s0red[e * NQ];
    __syncthreads();  // s0red / s1red are rewritten by the next step
  }
}

// sum of lds[k][0 .. 255] for k < IB_CH in a fixed order: thread (k = tid >> 5, j = tid & 31) adds its eight strided
// entries, then the 32 lanes fold downwards; valid in the threads with (tid & 31) == 0
__device__ __forceinline__ double ib_block_sum(const double (*lds)[IB_BLOCK], int tid) {
  const int k = tid >> 5, j = tid & 31;
  double acc = 0.0;
#pragma unroll
  for (int m = 0; m < IB_BLOCK / 32; ++m) acc += lds[k][j + 32 * m];
#pragma unroll
  for (int off = 16; off > 0; off >>= 1) acc += __shfl_down(acc, off, 32);
  return acc;
}

// workgroup per column c.  zt [nb][C][NF] is merged in place level by level (only column c's entries are touched);
// cov: [n_levels][C][NF][NF], mean: [C][NF]
template <int NF>
__global__ __launch_bounds__(IB_BLOCK) void influence_block_levels_kernel(double *zt, const double *__restrict__ wb, int64_t nb,
                                                                        int64_t C, int n_levels, double *__restrict__ cov,
                                                                        double *__restrict__ mean) {
  constexpr int NP = NF * (NF + 1) / 2, NS = NP + NF;  // upper triangle | column sums (level 0 only)
  const int64_t c = blockIdx.x;
  const int tid = threadIdx.x;
  __shared__ double lds[IB_CH][IB_BLOCK];
  __shared__ double sums[NS];
  __shared__ double wtot;

  {
    double acc = 0.0;
    for (int64_t i = tid; i < nb; i += IB_BLOCK) acc += wb[i];
#pragma unroll
    for (int k = 0; k < IB_CH; ++k) lds[k][tid] = k == 0 ? acc : 0.0;
    __syncthreads();
    const double tot = ib_block_sum(lds, tid);
    if (tid == 0) wtot = tot;
    __syncthreads();
  }
  const double W = wtot;

  for (int l = 0; l < n_levels; ++l) {
    const int64_t step = (int64_t)1 << l, half = step >> 1, nbl = (nb + step - 1) >> l;
    double acc[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) acc[q] = 0.0;
#pragma unroll 2
    for (int64_t jb = tid; jb < nbl; jb += IB_BLOCK) {
      double *p = zt + ((size_t)(jb * step) * C + c) * NF;
      double z[NF];
#pragma unroll
      for (int k = 0; k < NF; ++k) z[k] = p[k];
      if (l > 0 && jb * step + half < nb) {
        const double *q = zt + ((size_t)(jb * step + half) * C + c) * NF;
#pragma unroll
        for (int k = 0; k < NF; ++k) {
          z[k] += q[k];
          p[k] = z[k];
        }
      }
      int t = 0;
#pragma unroll
      for (int i = 0; i < NF; ++i)
#pragma unroll
        for (int jj = i; jj < NF; ++jj, ++t) acc[t] = fma(z[i], z[jj], acc[t]);
#pragma unroll
      for (int k = 0; k < NF; ++k) acc[NP + k] += z[k];
    }
    const int nred = l == 0 ? NS : NP;
#pragma unroll
    for (int c0 = 0; c0 < NS; c0 += IB_CH) {
      if (c0 < nred) {  // (uniform)
#pragma unroll
        for (int k = 0; k < IB_CH; ++k) lds[k][tid] = c0 + k < NS ? acc[c0 + k] : 0.0;
        __syncthreads();
        const double tot = ib_block_sum(lds, tid);
        if ((tid & 31) == 0 && c0 + (tid >> 5) < NS) sums[c0 + (tid >> 5)] = tot;
        __syncthreads();
      }
    }
    double *cv = cov + ((size_t)l * C + c) * NF * NF;
    for (int e = tid; e < NF * NF; e += IB_BLOCK) {
      // (i <= j: cov[i][j] and cov[j][i] are the same sum)
      const int i = min(e / NF, e % NF), jj = max(e / NF, e % NF);
      const int t = i * NF - i * (i - 1) / 2 + (jj - i);
      cv[e] = W == 0.0 ? 0.0 : sums[t] / (W * W);
    }
    if (l == 0)
      for (int k = tid; k < NF; k += IB_BLOCK) mean[(size_t)c * NF + k] = W == 0.0 ? 0.0 : sums[NP + k] / W;
    __syncthreads();  // the merged zt of this level is read by other threads at the next; sums is rewritten
  }
}

// ---------------------------------------------------------------------------
// host side

static bool ib_args_ok(int64_t N, int64_t C, int n_f, int n_q, int64_t block) {
  return N >= 1 && C >= 1 && C <= 65535 && n_f >= 1 && n_f <= TXM_MAXK && n_q >= 1 && n_q <= TXM_MAXK && block >= 1;
}

struct IbPlan : InfLanes {
  int rows, Bs, G, grid_x;
  int64_t nb;
  size_t lds_bytes;
};

static IbPlan ib_plan(const double *x, int64_t ldx_s, int64_t N, int64_t C, int n_q, int64_t block) {
  IbPlan p{};
  static_cast<InfLanes &>(p) = inf_lanes(inf_vec2_ok(x, ldx_s, C, n_q), C);
  p.rows = IB_BLOCK >> p.lpr_log2;
  p.Bs = block < p.rows ? (int)block : p.rows;
  p.G = p.rows / p.Bs;
  p.nb = cdiv(N, block);
  const int64_t steps = cdiv(p.nb, p.G), cap = (int64_t)num_cus() * 8;
  p.grid_x = (int)(steps > cap ? cap : steps);
  p.lds_bytes = ((size_t)IB_CH * IB_BLOCK + (size_t)p.G * n_q + (size_t)p.G * p.cols_per_chunk * n_q) * sizeof(double);
  return p;
}

template <int NQ>
static int ib_launch_sums(const IbPlan &p, const double *x, int64_t ldx_s, const double *u, const double *w, int64_t N, int64_t C,
                          int n_f, double cu, const double *cx, const double *a, const double *b, int64_t block, double *zt,
                          double *wb, hipStream_t st) {
  const dim3 grid(p.grid_x, p.chunks), blk(IB_BLOCK);
#define TXM_IB_RM(VEC, WT)                                                                                                \
  hipLaunchKernelGGL((influence_block_sums_kernel<NQ, VEC, WT>), grid, blk, p.lds_bytes, st, x, ldx_s, u, w, N, C, cu, cx, a, b, \
                     n_f, block, p.nb, p.lpr_log2, p.Bs, p.G, zt, wb)
  if (p.vec == 2) {
    if constexpr (NQ <= INF_VEC2_MAXQ) {
      if (w) TXM_IB_RM(2, true); else TXM_IB_RM(2, false);
    } else {
      set_error("influence_block_cov: no two-column kernel for n_q=%d", NQ);
      return TXM_ERR_UNSUPPORTED;
    }
  } else {
    if (w) TXM_IB_RM(1, true); else TXM_IB_RM(1, false);
  }
#undef TXM_IB_RM
  TXM_LAUNCH_CHECK();
  return TXM_OK;
}

int ib_block_sums(const double *x, int64_t ldx_s, const double *u, const double *w, int64_t N, int64_t C, int n_f, int n_q,
                  double center_u, const double *center_x, const double *a, const double *b, int64_t block, double *zt,
                  double *wb, hipStream_t st) {
  const IbPlan p = ib_plan(x, ldx_s, N, C, n_q, block);
  return inf_dispatch(n_q, "influence_block_cov: n_q", [&](auto Q) {
    return ib_launch_sums<decltype(Q)::value>(p, x, ldx_s, u, w, N, C, n_f, center_u, center_x, a, b, block, zt, wb, st);
  });
}

template <int NF>
static int ib_launch_levels(double *zt, const double *wb, int64_t nb, int64_t C, int n_levels, double *cov, double *mean,
                            hipStream_t st) {
  hipLaunchKernelGGL((influence_block_levels_kernel<NF>), dim3((unsigned)C), dim3(IB_BLOCK), 0, st, zt, wb, nb, C, n_levels, cov,
                     mean);
  TXM_LAUNCH_CHECK();
  return TXM_OK;
}

}  // namespace txm

using namespace txm;

extern "C" size_t txm_influence_block_cov_ws_bytes(int64_t N, int64_t C, int n_f, int n_q, int64_t block) {
  if (!ib_args_ok(N, C, n_f, n_q, block)) return 0;
  return (size_t)cdiv(N, block) * ((size_t)C * n_f + 1) * sizeof(double) + 256;
}

extern "C" int txm_influence_block_cov(const double *x, int64_t ldx_s, const double *u, const double *w, int64_t N, int64_t C,
                                       int n_f, int n_q, double center_u, const double *center_x, const double *a,
                                       const double *b, int64_t block, int n_levels, double *cov, double *mean, void *ws,
                                       size_t ws_bytes, txm_stream stream) {
  if (const int rc = inf_check_args("influence_block_cov", x && u && center_x && a && b && cov && mean && ws, N, C, 65535, "",
                                    n_f, n_q, ldx_s >= C, "row pitch ldx_s < C", center_u))
    return rc;
  if (const int rc = inf_check_block("influence_block_cov", block, n_levels)) return rc;
  if (ws_bytes < txm_influence_block_cov_ws_bytes(N, C, n_f, n_q, block)) {
    set_error("influence_block_cov: workspace too small");
    return TXM_ERR_WORKSPACE;
  }
  const int64_t nb = cdiv(N, block);
  hipStream_t st = (hipStream_t)stream;
  double *zt = (double *)ws, *wb = zt + (size_t)nb * C * n_f;
  const int rc = ib_block_sums(x, ldx_s, u, w, N, C, n_f, n_q, center_u, center_x, a, b, block, zt, wb, st);
  if (rc != TXM_OK) return rc;
  return inf_dispatch(n_f, "influence_block_cov: n_f", [&](auto F) {
    return ib_launch_levels<decltype(F)::value>(zt, wb, nb, C, n_levels, cov, mean, st);
  });
}
