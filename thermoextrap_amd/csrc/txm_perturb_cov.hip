// txm_perturb_cov.hip -- delta-method (infinitesimal-jackknife) variance of the exponentially reweighted averages of
// txm_perturb.hip, the Kish effective sample number and the free-energy difference ln<e^{-da u}> with its variance, for up
// to eight alphas in one pass over the samples (PerturbModel.predict_with_error / effective_samples / free_energy /
// blocking_curve).
//
// With w_na = e^{-da_a (u_n - uref_a)} (uref_a from the extremes pre-pass of txm_perturb.h: the same numbers as
// txm_perturb's weights), W_a = sum_n w_na, p_na = w_na / W_a and the caller's mean[a][c] (txm_perturb's output), level-l
// block j covers the rows [j B 2^l, min(N, (j + 1) B 2^l)) and
//      var[l][a][c]   = sum_j z_j^2,   z_j = sum_{n in block j} p_na (x_nc - mean[a][c])     (no nb / (nb - 1) factor)
//      neff[a]        = W_a^2 / sum_n w_na^2
//      lnq[a]         = ln(W_a / N) - da_a uref_a
//      var_lnq[l][a]  = sum_j (sum_{n in j} p_na - n_j / N)^2                                 (block 1: 1 / neff - 1 / N)
// The sums are centred on the GIVEN mean, so nothing cancels (a one-pass shifted-sum form loses digits once n_eff is a
// few samples).  Two sample kernels:
//   iid (block == 1, n_levels == 1): perturb_kernel's layout -- a lane owns VEC columns, 2^L lanes span a row, the NA
//     exponentials of a row are evaluated once and shared across its lanes -- with sum w, sum w^2 per alpha and
//     sum (w (x - m))^2 per (alpha, column) in registers; per-workgroup partials, added in a fixed order by a finalize.
//   blocked: every level-0 block is summed by ONE workgroup, its rows round-robin over min(B, ROWS) row slots added in
//     slot order (txm_influence_block.hip's scheme), so a block's bits depend on (B, C, alignment) only, never on the
//     launch width.  The unnormalised sums go to the workspace as zt [nb][n_alpha][C + 1] (slot C: sum_{n in b} w) and
//     wb [nb][n_alpha][2] (sum w, sum w^2); a second kernel (a workgroup per (slot, alpha)) adds W in a fixed order and
//     merges the pairs of the level below in place, level by level, summing the squares.
// No floating-point atomics: two calls give the same bits.  A row whose weight underflows contributes zero.
// First-order rounding bound, kappa_n = 1 + |da (u_n - uref)| (the exponent's rounding is the weight's relative error):
//   var: few eps * sum_j (sum_{n in j} p_n kappa_n |x_n - m|)^2,  var_lnq: few eps * sum_j (sum_{n in j} p_n kappa_n + n_j / N)^2.
#include "txm_perturb.h"

namespace txm {

// sum of v over the workgroup's threads in a fixed order (a binary tree over the thread index); every thread gets it
__device__ __forceinline__ double pc_block_sum(double v, double *lds) {
  const int tid = threadIdx.x;
  __syncthreads();  // (lds may still be read from the call before)
  lds[tid] = v;
  __syncthreads();
  for (int off = PB_BLOCK / 2; off > 0; off >>= 1) {
    if (tid < off) lds[tid] += lds[tid + off];
    __syncthreads();
  }
  return lds[0];
}

// the NA weights of one row for the lanes of that row.  `share`: lane `lir` of the row evaluates alpha number lir (one
// exp sequence covers all alphas; its da and uref are `mine`, picked once per thread by pc_mine) and the row's lanes
// fetch the weights with cross-lane reads -- needs the lanes 0 .. NA-1 of the row active and the row inside one wave
// (perturb_kernel's rule).
// VEC columns of one row (read once: non-temporal, as the reductions do)
typedef double pc_v2d __attribute__((ext_vector_type(2)));
template <int VEC>
__device__ __forceinline__ void pc_load(const double *__restrict__ p, double (&xv)[VEC]) {
  if constexpr (VEC == 2) {
    const pc_v2d t = __builtin_nontemporal_load(reinterpret_cast<const pc_v2d *>(p));
    xv[0] = t.x;
    xv[1] = t.y;
  } else {
    xv[0] = __builtin_nontemporal_load(p);
  }
}

// rows in flight per lane: the loads of PC_UNR rows are issued before the first is used (the rows are still added in
// index order, so the sums do not depend on it).  The blocked kernel holds more per lane and takes two: both kernels
// keep two waves per SIMD at NA = 8, VEC = 2 (__launch_bounds__'s second argument).
constexpr int PC_UNR = 4, PC_UNR_BLOCK = 2;

template <int NA>
__device__ __forceinline__ void pc_mine(int lir, const PerturbArgs &pa, const double (&uref)[NA], double &da_mine,
                                        double &ur_mine) {
  da_mine = pa.da[0];
  ur_mine = uref[0];
#pragma unroll
  for (int a = 1; a < NA; ++a)
    if (lir == a) {
      da_mine = pa.da[a];
      ur_mine = uref[a];
    }
}

template <int NA>
__device__ __forceinline__ void pc_weights(bool share, int lpr, double ui, double da_mine, double ur_mine,
                                           const PerturbArgs &pa, const double (&uref)[NA], double (&w)[NA]) {
  if (share) {
    const double w_mine = exp(-da_mine * (ui - ur_mine));
    const int row_lane0 = ((int)threadIdx.x & 63) & ~(lpr - 1);
#pragma unroll
    for (int a = 0; a < NA; ++a) w[a] = __shfl(w_mine, row_lane0 + a);
  } else {
#pragma unroll
    for (int a = 0; a < NA; ++a) w[a] = exp(-pa.da[a] * (ui - uref[a]));
  }
}

// ---------------------------------------------------------------------------
// iid: partial_q [gridDim.x][cols_pad][NA] (sum (w (x - m))^2), partial_w [gridDim.x][NA][2] (sum w, sum w^2)
// ---------------------------------------------------------------------------
template <int NA, int VEC, int LPR_LOG2>
__global__ __launch_bounds__(PB_BLOCK, 2) void perturb_cov_kernel(const double *__restrict__ x, int64_t ldx_s,
                                                               const double *__restrict__ u, int64_t N, int64_t C,
                                                               const PerturbArgs pa, const double *__restrict__ mm,
                                                               const double *__restrict__ mean,
                                                               double *__restrict__ partial_q,
                                                               double *__restrict__ partial_w) {
  constexpr int LPR = 1 << LPR_LOG2;
  constexpr int ROWS = PB_BLOCK / LPR;
  const int tid = threadIdx.x;
  const int lir = tid & (LPR - 1), rib = tid >> LPR_LOG2;
  const int64_t col0 = (int64_t)blockIdx.y * (LPR * VEC) + (int64_t)lir * VEC;
  const bool col_ok = col0 < C;  // VEC == 2 requires C even, so col0 + 1 < C too
  double uref[NA];
#pragma unroll
  for (int a = 0; a < NA; ++a) uref[a] = pa.da[a] >= 0.0 ? mm[0] : mm[1];
  double q[NA][VEC], m[NA][VEC], sw[NA], sw2[NA];
#pragma unroll
  for (int a = 0; a < NA; ++a) {
    sw[a] = sw2[a] = 0.0;
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      q[a][v] = 0.0;
      m[a][v] = col_ok ? mean[(size_t)a * C + col0 + v] : 0.0;
    }
  }
  const int64_t stride = (int64_t)gridDim.x * ROWS;
  const int64_t cols_left = C - (int64_t)blockIdx.y * (LPR * VEC);
  const int64_t nvalid = (cols_left + VEC - 1) / VEC;
  const bool share = (LPR >= NA) && (LPR <= 64) && (NA > 1) && (nvalid >= NA);  // block-uniform
  double da_mine, ur_mine;
  pc_mine<NA>(lir, pa, uref, da_mine, ur_mine);
  auto body = [&](double ui, const double(&xv)[VEC]) {
    double w[NA];
    pc_weights<NA>(share, LPR, ui, da_mine, ur_mine, pa, uref, w);
#pragma unroll
    for (int a = 0; a < NA; ++a) {
      sw[a] += w[a];
      sw2[a] = fma(w[a], w[a], sw2[a]);
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        const double t = w[a] * (xv[v] - m[a][v]);
        q[a][v] = fma(t, t, q[a][v]);
      }
    }
  };
  if (col_ok) {
    int64_t i = (int64_t)blockIdx.x * ROWS + rib;
    for (; i + (PC_UNR - 1) * stride < N; i += PC_UNR * stride) {
      double xv[PC_UNR][VEC], ui[PC_UNR];
#pragma unroll
      for (int k = 0; k < PC_UNR; ++k) {
        pc_load<VEC>(x + (i + k * stride) * ldx_s + col0, xv[k]);
        ui[k] = u[i + k * stride];
      }
#pragma unroll
      for (int k = 0; k < PC_UNR; ++k) body(ui[k], xv[k]);
    }
    for (; i < N; i += stride) {
      double xv[VEC];
      pc_load<VEC>(x + i * ldx_s + col0, xv);
      body(u[i], xv);
    }
  }
  // block reduction over the ROWS row slots (fixed order): the column sums, then (chunk 0 only) the weight sums
  constexpr int NQ = NA * VEC;
  __shared__ double sh[PB_BLOCK * NA * 2];
#pragma unroll
  for (int a = 0; a < NA; ++a)
#pragma unroll
    for (int v = 0; v < VEC; ++v) sh[(size_t)tid * NQ + a * VEC + v] = q[a][v];
  __syncthreads();
  const size_t cols_pad = (size_t)gridDim.y * LPR * VEC;
  for (int e = tid; e < LPR * NQ; e += PB_BLOCK) {
    const int l = e / NQ, k = e % NQ;
    double acc = 0.0;
    for (int r = 0; r < ROWS; ++r) acc += sh[((size_t)r * LPR + l) * NQ + k];
    const int a = k / VEC, v = k % VEC;
    partial_q[((size_t)blockIdx.x * cols_pad + (size_t)blockIdx.y * LPR * VEC + (size_t)l * VEC + v) * NA + a] = acc;
  }
  if (blockIdx.y == 0) {
    __syncthreads();
    if (lir == 0) {
#pragma unroll
      for (int a = 0; a < NA; ++a) {
        sh[(size_t)rib * NA * 2 + a * 2] = sw[a];
        sh[(size_t)rib * NA * 2 + a * 2 + 1] = sw2[a];
      }
    }
    __syncthreads();
    for (int e = tid; e < NA * 2; e += PB_BLOCK) {
      double acc = 0.0;
      for (int r = 0; r < ROWS; ++r) acc += sh[(size_t)r * NA * 2 + e];
      partial_w[(size_t)blockIdx.x * NA * 2 + e] = acc;
    }
  }
}

// grid (C + 1, NA): blockIdx.x < C writes var[a][c], blockIdx.x == C writes neff, lnq, var_lnq of alpha a.
// Every workgroup adds W_a itself, in the same order.
__global__ __launch_bounds__(PB_BLOCK) void perturb_cov_final_kernel(const double *__restrict__ partial_q,
                                                                     const double *__restrict__ partial_w, int nblk,
                                                                     int64_t cols_pad, int64_t C, int NA, int64_t N,
                                                                     const PerturbArgs pa, const double *__restrict__ mm,
                                                                     double *__restrict__ var, double *__restrict__ neff,
                                                                     double *__restrict__ lnq,
                                                                     double *__restrict__ var_lnq) {
  __shared__ double lds[PB_BLOCK];
  const int64_t c = blockIdx.x;
  const int a = blockIdx.y, tid = threadIdx.x;
  double s1 = 0.0, s2 = 0.0, sq = 0.0;
  for (int b = tid; b < nblk; b += PB_BLOCK) {
    s1 += partial_w[((size_t)b * NA + a) * 2];
    s2 += partial_w[((size_t)b * NA + a) * 2 + 1];
    if (c < C) sq += partial_q[((size_t)b * cols_pad + c) * NA + a];
  }
  const double W = pc_block_sum(s1, lds);
  if (c < C) {
    const double Q = pc_block_sum(sq, lds);
    if (tid == 0) var[(size_t)a * C + c] = Q / (W * W);
  } else {
    const double W2 = pc_block_sum(s2, lds);
    if (tid == 0) {
      const double uref = pa.da[a] >= 0.0 ? mm[0] : mm[1];
      neff[a] = W * W / W2;
      lnq[a] = log(W / (double)N) - pa.da[a] * uref;
      const double v = W2 / (W * W) - 1.0 / (double)N;  // sum (p - 1/N)^2 >= 0: a rounding-negative value is zero
      var_lnq[a] = v > 0.0 ? v : 0.0;
    }
  }
}

// ---------------------------------------------------------------------------
// blocked.  Thread layout: lane_in_row = tid & (LPR - 1) owns columns col0 + {0 .. VEC-1}, row slot = tid >> lpr_log2
// (ROWS of them); blockIdx.y selects a chunk of LPR * VEC columns.  A workgroup step serves G = max(1, ROWS / B)
// consecutive level-0 blocks: block g of the step owns the Bs = min(B, ROWS) row slots g Bs .. g Bs + Bs - 1, slot j of a
// block reads its rows r0 + j, r0 + j + Bs, ...  Steps are grid-strided.
// zt: [nb][NA][C + 1] (slot C: sum w), wb: [nb][NA][2] (sum w, sum w^2)
// ---------------------------------------------------------------------------
template <int NA, int VEC>
__global__ __launch_bounds__(PB_BLOCK, 2) void perturb_block_sums_kernel(const double *__restrict__ x, int64_t ldx_s,
                                                                      const double *__restrict__ u, int64_t N, int64_t C,
                                                                      const PerturbArgs pa, const double *__restrict__ mm,
                                                                      const double *__restrict__ mean, int64_t B,
                                                                      int64_t nb, int lpr_log2, int Bs, int G,
                                                                      double *__restrict__ zt, double *__restrict__ wb) {
  constexpr int NS = VEC + 2;  // per alpha: sum w dx_v | sum w | sum w^2
  __shared__ double stage[NS][PB_BLOCK];
  const int LPR = 1 << lpr_log2, cols = LPR * VEC;
  const int tid = threadIdx.x;
  const int lir = tid & (LPR - 1), rib = tid >> lpr_log2;
  const int g = rib / Bs, j = rib - g * Bs;
  const int64_t col0 = (int64_t)blockIdx.y * cols + (int64_t)lir * VEC;
  const bool col_ok = col0 < C;
  double uref[NA], m[NA][VEC];
#pragma unroll
  for (int a = 0; a < NA; ++a) {
    uref[a] = pa.da[a] >= 0.0 ? mm[0] : mm[1];
#pragma unroll
    for (int v = 0; v < VEC; ++v) m[a][v] = col_ok ? mean[(size_t)a * C + col0 + v] : 0.0;
  }
  const int64_t cols_left = C - (int64_t)blockIdx.y * cols;
  const int64_t nvalid = (cols_left + VEC - 1) / VEC;
  const bool share = (LPR >= NA) && (LPR <= 64) && (NA > 1) && (nvalid >= NA);  // block-uniform
  double da_mine, ur_mine;
  pc_mine<NA>(lir, pa, uref, da_mine, ur_mine);

  const int64_t n_steps = (nb + G - 1) / G;
  for (int64_t it = blockIdx.x; it < n_steps; it += gridDim.x) {
    double s[NA][VEC], sw[NA], sw2[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) {
      sw[a] = sw2[a] = 0.0;
#pragma unroll
      for (int v = 0; v < VEC; ++v) s[a][v] = 0.0;
    }
    const int64_t blk = it * G + g;
    if (col_ok && g < G && blk < nb) {
      const int64_t r0 = blk * B, rend = (B < N - r0) ? r0 + B : N;
      auto body = [&](double ui, const double(&xv)[VEC]) {
        double w[NA];
        pc_weights<NA>(share, LPR, ui, da_mine, ur_mine, pa, uref, w);
#pragma unroll
        for (int a = 0; a < NA; ++a) {
          sw[a] += w[a];
          sw2[a] = fma(w[a], w[a], sw2[a]);
#pragma unroll
          for (int v = 0; v < VEC; ++v) s[a][v] = fma(w[a], xv[v] - m[a][v], s[a][v]);
        }
      };
      int64_t i = r0 + j;
      for (; i + (int64_t)(PC_UNR_BLOCK - 1) * Bs < rend; i += (int64_t)PC_UNR_BLOCK * Bs) {
        double xv[PC_UNR_BLOCK][VEC], ui[PC_UNR_BLOCK];
#pragma unroll
        for (int k = 0; k < PC_UNR_BLOCK; ++k) {
          pc_load<VEC>(x + (i + (int64_t)k * Bs) * ldx_s + col0, xv[k]);
          ui[k] = u[i + (int64_t)k * Bs];
        }
#pragma unroll
        for (int k = 0; k < PC_UNR_BLOCK; ++k) body(ui[k], xv[k]);
      }
      for (; i < rend; i += Bs) {
        double xv[VEC];
        pc_load<VEC>(x + i * ldx_s + col0, xv);
        body(u[i], xv);
      }
    }
    // every block's Bs row slots added in slot order, one alpha per pass
    const int per = G << lpr_log2;  // (block of the step, lane in row): <= 256
#pragma unroll
    for (int a = 0; a < NA; ++a) {
#pragma unroll
      for (int v = 0; v < VEC; ++v) stage[v][tid] = s[a][v];
      stage[VEC][tid] = sw[a];
      stage[VEC + 1][tid] = sw2[a];
      __syncthreads();
      for (int e = tid; e < NS * per; e += PB_BLOCK) {
        const int k = e / per, rem = e - k * per, gg = rem >> lpr_log2, l = rem & (LPR - 1);
        const int64_t bk = it * G + gg;
        if (bk >= nb) continue;
        double acc = 0.0;
        for (int r = 0; r < Bs; ++r) acc += stage[k][((gg * Bs + r) << lpr_log2) + l];
        if (k < VEC) {
          const int64_t col = (int64_t)blockIdx.y * cols + (int64_t)l * VEC + k;
          if (col < C) zt[((size_t)bk * NA + a) * (C + 1) + col] = acc;
        } else if (l == 0 && blockIdx.y == 0) {  // the weight sums: the same in every lane of a row slot
          wb[((size_t)bk * NA + a) * 2 + (k - VEC)] = acc;
          if (k == VEC) zt[((size_t)bk * NA + a) * (C + 1) + C] = acc;
        }
      }
      __syncthreads();
    }
  }
}

// grid (C + 1, NA), a workgroup per (slot, alpha).  zt is merged in place level by level (only this workgroup's slot is
// touched; W comes from wb, which nobody writes).  Slot c < C: var[l][a][c]; slot C: var_lnq[l][a], neff[a], lnq[a].
__global__ __launch_bounds__(PB_BLOCK) void perturb_block_levels_kernel(double *zt, const double *__restrict__ wb,
                                                                        int64_t nb, int64_t N, int64_t B, int64_t C,
                                                                        int NA, int n_levels, const PerturbArgs pa,
                                                                        const double *__restrict__ mm,
                                                                        double *__restrict__ var,
                                                                        double *__restrict__ neff, double *__restrict__ lnq,
                                                                        double *__restrict__ var_lnq) {
  __shared__ double lds[PB_BLOCK];
  const int64_t c = blockIdx.x;
  const int a = blockIdx.y, tid = threadIdx.x;
  const size_t ld = (size_t)NA * (C + 1);  // doubles from one level-0 block to the next
  double *z0 = zt + (size_t)a * (C + 1) + c;
  double s1 = 0.0, s2 = 0.0;
  for (int64_t i = tid; i < nb; i += PB_BLOCK) {
    s1 += wb[((size_t)i * NA + a) * 2];
    if (c == C) s2 += wb[((size_t)i * NA + a) * 2 + 1];
  }
  const double W = pc_block_sum(s1, lds);
  if (c == C) {
    const double W2 = pc_block_sum(s2, lds);
    if (tid == 0) {
      const double uref = pa.da[a] >= 0.0 ? mm[0] : mm[1];
      neff[a] = W * W / W2;
      lnq[a] = log(W / (double)N) - pa.da[a] * uref;
    }
  }
  for (int l = 0; l < n_levels; ++l) {
    const int64_t step = (int64_t)1 << l, half = step >> 1, nbl = (nb + step - 1) >> l;
    double acc = 0.0;
    for (int64_t jb = tid; jb < nbl; jb += PB_BLOCK) {
      const int64_t b0 = jb * step;  // < nb
      double *p = z0 + (size_t)b0 * ld;
      double z = *p;
      if (l > 0 && b0 + half < nb) {
        z += z0[(size_t)(b0 + half) * ld];
        *p = z;
      }
      if (c < C) {
        acc = fma(z, z, acc);
      } else {
        const int64_t b1 = (nb - b0 > step) ? b0 + step : nb;  // level-0 blocks [b0, b1)
        const int64_t rows = (b1 == nb ? N : b1 * B) - b0 * B;
        const double d = z / W - (double)rows / (double)N;
        acc = fma(d, d, acc);
      }
    }
    const double tot = pc_block_sum(acc, lds);  // (its barriers also order this level's merges before the next level's reads)
    if (tid == 0) {
      if (c < C)
        var[((size_t)l * NA + a) * C + c] = tot / (W * W);
      else
        var_lnq[(size_t)l * NA + a] = tot;
    }
  }
}

struct PcBlockPlan {
  int64_t nb;
  int Bs, G, gx;
};

static PcBlockPlan pc_block_plan(const PbPlan &p, int64_t N, int64_t block) {
  PcBlockPlan q;
  q.nb = (N - 1) / block + 1;
  const int rows = PB_BLOCK >> p.l2;
  q.Bs = block < rows ? (int)block : rows;
  q.G = block < rows ? (int)(rows / block) : 1;
  int64_t gx = cdiv(q.nb, q.G);
  const int64_t cap = (int64_t)num_cus() * 8;
  q.gx = (int)(gx > cap ? cap : gx);
  return q;
}

static bool pc_args_ok(int64_t N, int64_t C, int32_t n_alpha, int64_t block, int32_t n_levels) {
  return N >= 1 && C >= 1 && C <= 65535 && n_alpha >= 1 && n_alpha <= PB_MAXA && block >= 1 && n_levels >= 1 &&
         n_levels <= 32;
}

}  // namespace txm

using namespace txm;

// head (the extremes pre-pass), then
//   iid:     partial_q [gx_cap][cols_pad][n_alpha] and partial_w [gx_cap][n_alpha][2], gx_cap = 8 workgroups per CU;
//   blocked: zt, 8 nb n_alpha (C + 1) bytes with nb = ceil(N / block), and wb, 16 nb n_alpha bytes.
extern "C" size_t txm_perturb_cov_ws_bytes(int64_t N, int64_t C, int32_t n_alpha, int64_t block, int32_t n_levels) {
  if (!pc_args_ok(N, C, n_alpha, block, n_levels)) return 0;
  const size_t head = pb_mm_bytes(N, 1);
  if (block == 1 && n_levels == 1) {
    const size_t gx_cap = (size_t)num_cus() * 8;
    return head + align_up(gx_cap * (size_t)pb_cols_pad_max(C) * n_alpha * sizeof(double), 256) +
           gx_cap * n_alpha * 2 * sizeof(double) + 256;
  }
  const size_t nb = (size_t)((N - 1) / block + 1);
  return head + align_up(8 * nb * (size_t)n_alpha * (size_t)(C + 1), 256) + 16 * nb * (size_t)n_alpha + 256;
}

extern "C" int txm_perturb_cov(const double *x, int64_t ldx_s, const double *u, int64_t N, int64_t C,
                               const double *dalpha_host, int32_t n_alpha, const double *mean, int64_t block,
                               int32_t n_levels, double *var, double *neff, double *lnq, double *var_lnq, void *ws,
                               size_t ws_bytes, txm_stream stream) {
  TXM_REQUIRE(x && u && dalpha_host && mean && var && neff && lnq && var_lnq && ws, "perturb_cov: null pointer");
  TXM_REQUIRE(N >= 1 && C >= 1 && C <= 65535 && ldx_s >= C, "perturb_cov: bad N/C/ldx");
  TXM_REQUIRE(n_alpha >= 1 && n_alpha <= PB_MAXA, "perturb_cov: n_alpha outside [1, %d]", PB_MAXA);
  TXM_REQUIRE(block >= 1 && n_levels >= 1 && n_levels <= 32, "perturb_cov: block < 1 or n_levels outside [1, 32]");
  if (ws_bytes < txm_perturb_cov_ws_bytes(N, C, n_alpha, block, n_levels)) {
    set_error("perturb_cov: workspace too small");
    return TXM_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  const int rc = pb_launch_minmax(u, N, nullptr, 1, ws, st);
  if (rc != TXM_OK) return rc;
  const double *mm = (const double *)ws;
  char *body = (char *)ws + pb_mm_bytes(N, 1);
  const PbPlan p = pb_plan(x, ldx_s, N, C, 1);
  PerturbArgs pa;
  for (int a = 0; a < PB_MAXA; ++a) pa.da[a] = a < n_alpha ? dalpha_host[a] : 0.0;
  dim3 block3(PB_BLOCK);
  bool launched = false;

  if (block == 1 && n_levels == 1) {
    double *partial_q = (double *)body;
    double *partial_w =
        (double *)(body + align_up((size_t)num_cus() * 8 * (size_t)pb_cols_pad_max(C) * n_alpha * sizeof(double), 256));
    dim3 grid(p.gx, p.chunks);
#define TXM_PC(NA_, VEC_, L2_)                                                                               \
  if (!launched && n_alpha == NA_ && p.vec == VEC_ && p.l2 == L2_) {                                         \
    hipLaunchKernelGGL((perturb_cov_kernel<NA_, VEC_, L2_>), grid, block3, 0, st, x, ldx_s, u, N, C, pa, mm, \
                       mean, partial_q, partial_w);                                                          \
    launched = true;                                                                                         \
  }
#define TXM_PC_L(NA_, VEC_) \
  TXM_PC(NA_, VEC_, 0) TXM_PC(NA_, VEC_, 1) TXM_PC(NA_, VEC_, 2) TXM_PC(NA_, VEC_, 3) TXM_PC(NA_, VEC_, 4) \
  TXM_PC(NA_, VEC_, 5) TXM_PC(NA_, VEC_, 6) TXM_PC(NA_, VEC_, 7) TXM_PC(NA_, VEC_, 8)
#define TXM_PC_A(NA_) TXM_PC_L(NA_, 1) TXM_PC_L(NA_, 2)
    TXM_PC_A(1) TXM_PC_A(2) TXM_PC_A(3) TXM_PC_A(4) TXM_PC_A(5) TXM_PC_A(6) TXM_PC_A(7) TXM_PC_A(8)
#undef TXM_PC_A
#undef TXM_PC_L
#undef TXM_PC
    if (!launched) {
      set_error("perturb_cov: no kernel variant");
      return TXM_ERR_UNSUPPORTED;
    }
    TXM_LAUNCH_CHECK();
    hipLaunchKernelGGL(perturb_cov_final_kernel, dim3((unsigned)C + 1, (unsigned)n_alpha), block3, 0, st, partial_q,
                       partial_w, p.gx, p.cols_pad, C, (int)n_alpha, N, pa, mm, var, neff, lnq, var_lnq);
    TXM_LAUNCH_CHECK();
    return TXM_OK;
  }

  const PcBlockPlan q = pc_block_plan(p, N, block);
  double *zt = (double *)body;
  double *wb = (double *)(body + align_up(8 * (size_t)q.nb * (size_t)n_alpha * (size_t)(C + 1), 256));
  dim3 grid(q.gx, p.chunks);
#define TXM_PCB(NA_, VEC_)                                                                                       \
  if (!launched && n_alpha == NA_ && p.vec == VEC_) {                                                            \
    hipLaunchKernelGGL((perturb_block_sums_kernel<NA_, VEC_>), grid, block3, 0, st, x, ldx_s, u, N, C, pa, mm,   \
                       mean, block, q.nb, p.l2, q.Bs, q.G, zt, wb);                                              \
    launched = true;                                                                                             \
  }
#define TXM_PCB_A(NA_) TXM_PCB(NA_, 1) TXM_PCB(NA_, 2)
  TXM_PCB_A(1) TXM_PCB_A(2) TXM_PCB_A(3) TXM_PCB_A(4) TXM_PCB_A(5) TXM_PCB_A(6) TXM_PCB_A(7) TXM_PCB_A(8)
#undef TXM_PCB_A
#undef TXM_PCB
  if (!launched) {
    set_error("perturb_cov: no kernel variant");
    return TXM_ERR_UNSUPPORTED;
  }
  TXM_LAUNCH_CHECK();
  hipLaunchKernelGGL(perturb_block_levels_kernel, dim3((unsigned)C + 1, (unsigned)n_alpha), block3, 0, st, zt, wb, q.nb,
                     N, block, C, (int)n_alpha, (int)n_levels, pa, mm, var, neff, lnq, var_lnq);
  TXM_LAUNCH_CHECK();
  return TXM_OK;
}
