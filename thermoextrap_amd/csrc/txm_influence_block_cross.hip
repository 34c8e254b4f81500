// txm_influence_block_cross.hip -- the blocked (batch-means) delta-method covariance of txm_influence_block.hip ACROSS the
// observable columns (ExtrapModel.derivs_cross_cov(block=...) / predict_cov(block=...) / cross_blocking_curve).
//
// With the block sums of txm_influence_block.hip, z_j[c][k] = sum_{n in block j} p_n psi_k(n, c), the caller wants every block of
//      cov[l][c][i][c'][j'] = sum_j z_j[c][i] z_j[c'][j']          (level-l blocks of B 2^l rows; (C n_f)^2, symmetric)
//      mean[c][k]           = sum_n p_n psi_k(n, c).
//
//   pass 1 is txm_influence_block.hip's (ib_block_sums: the same kernel, the same plan, the same bits): it streams the samples
//     once and leaves the unnormalised zt [nb][M], M = C n_f logical columns, and wb [nb] in the workspace.
//   influence_block_colsum_kernel / _colsum_final_kernel   the column sums of zt and W = sum wb (wb rides as logical column M)
//     in two fixed-order stages; mean = column sum / W.
//   influence_block_merge_kernel   level l > 0: zt[j 2^l] += zt[j 2^l + 2^(l-1)] IN PLACE (a last unpaired block stays), so level
//     l's blocks are the rows j 2^l of zt and the workspace is pass 1's plus the records below.
//   influence_block_gram_kernel    G = sum_b z_b z_b^T on the FP64 matrix pipe (v_mfma_f64_16x16x4_f64; operand layout as
//     txm_influence_cross.hip).  The M columns are cut into T = ceil(M / 16) tiles and those into TM = ceil(T / 4) macro tiles of
//     4 x 4 tiles; grid (macro pairs mi <= mj, block workgroups).  The k-axis of the MFMA is the block axis: lane
//     (m = lane & 15, k = lane >> 4) holds A[m][k] = z_{b0+k}[16 ti + m] and B[k][m] = z_{b0+k}[16 tj + m].  A wave keeps the
//     up to 16 accumulator tiles of its macro pair (128 VGPRs) and takes every fourth 4-block step of its workgroup: 4 A and 4
//     B operands per 16 MFMAs, sixteen independent accumulation chains.  Tiles below the diagonal of a diagonal macro pair and
//     tiles >= T are skipped (wave-uniform); a column >= M or a block >= nb is read at column 0 / row 0 (addresses that exist,
//     so the loads of a step stay unconditional and in flight together) and selected to zero, never used.  At the end the four
//     waves' tiles are added in wave order through LDS: one record of 16 tiles per (workgroup, macro pair).
//   influence_block_gram_sum_kernel   adds the workgroups' records in index order.
//   influence_block_cross_final_kernel   a thread per pair (P, Q), P <= Q, of the M logical columns: reads G at
//     (row <= column) only, divides by W^2 and stores the entry and its mirror.
// No floating-point atomics: two calls give the same bits.  First-order rounding bound per level:
// |cov - exact| <= few eps * sum_b beta_b(c, i) beta_b(c', j'),  beta_b(c, k) = sum_{n in b} p_n B_k(n, c).
#include "txm_influence_block.h"

namespace txm {

constexpr int BX_BLOCK = 256;      // four waves
constexpr int BX_MT = 4;           // tiles a side of a macro tile
constexpr int BX_SHARE = 256;      // blocks a workgroup takes before the grid grows by one workgroup
constexpr int BX_UNR = 2;          // 4-block steps a wave has in flight
constexpr int BX_MAXC = 255;       // as txm_influence_cross_cov
constexpr int BX_REC = BX_MT * BX_MT * 256;  // doubles of one (workgroup, macro pair) record
constexpr int BX_CS_COLS = 64;     // columns of a column-sum workgroup (four row slots)
constexpr int BX_CS_MAXP = 256;    // row workgroups of the column sums at most

// part[blockIdx.y][M + 1]: the sums over the rows blockIdx.y * 4 + slot, + 4 gridDim.y, ... of zt's columns and (column M) wb,
// the four row slots added in slot order
__global__ __launch_bounds__(BX_BLOCK) void influence_block_colsum_kernel(const double *__restrict__ zt,
                                                                          const double *__restrict__ wb, int64_t nb, int M,
                                                                          double *__restrict__ part) {
  __shared__ double red[4][BX_CS_COLS];
  const int tid = threadIdx.x, cl = tid & (BX_CS_COLS - 1), slot = tid >> 6;
  const int col = (int)blockIdx.x * BX_CS_COLS + cl;
  double acc = 0.0;
  if (col <= M) {
    const int64_t stride = (int64_t)gridDim.y * 4;
#pragma unroll 4
    for (int64_t r = (int64_t)blockIdx.y * 4 + slot; r < nb; r += stride) acc += col < M ? zt[(size_t)r * M + col] : wb[r];
  }
  red[slot][cl] = acc;
  __syncthreads();
  if (slot == 0 && col <= M)
    part[(size_t)blockIdx.y * (M + 1) + col] = ((red[0][cl] + red[1][cl]) + red[2][cl]) + red[3][cl];
}

// a thread per logical column: the row workgroups in index order.  wtot[0] = W, mean[col] = column sum / W
__global__ __launch_bounds__(BX_BLOCK) void influence_block_colsum_final_kernel(const double *__restrict__ part, int nparts,
                                                                                int M, double *__restrict__ wtot,
                                                                                double *__restrict__ mean) {
  const int col = (int)blockIdx.x * BX_BLOCK + threadIdx.x;
  if (col > M) return;
  double acc = 0.0, W = 0.0;
  for (int p = 0; p < nparts; ++p) {
    acc += part[(size_t)p * (M + 1) + col];
    W += part[(size_t)p * (M + 1) + M];
  }
  if (col == M)
    wtot[0] = W;
  else
    mean[col] = W == 0.0 ? 0.0 : acc / W;
}

// level l = log2(step) > 0: row j step of zt [nb][M] takes its partner row j step + step / 2 (if there is one)
__global__ __launch_bounds__(BX_BLOCK) void influence_block_merge_kernel(double *zt, int64_t nb, int64_t M, int64_t step,
                                                                         int64_t nbl) {
  const int64_t half = step >> 1, total = nbl * M, gsz = (int64_t)gridDim.x * BX_BLOCK;
  for (int64_t e = (int64_t)blockIdx.x * BX_BLOCK + threadIdx.x; e < total; e += gsz) {
    const int64_t j = e / M, c = e - j * M, r = j * step;
    if (r + half < nb) zt[(size_t)r * M + c] += zt[(size_t)(r + half) * M + c];
  }
}

// The block loop of the Gram pass for one wave: wave wg of NW takes the 4-block steps wg, wg + NW, ... (wave-uniform bounds).
// A column >= M or a block >= nbl is read at an address that exists (column 0, row 0) and selected to zero; the tiles
// ta >= nta, tb >= ntb (tile index >= T) and, on a diagonal macro pair, ta > tb are skipped.
template <bool DIAG>
__device__ __forceinline__ void bx_accumulate(const double *__restrict__ zt, int64_t rs, int64_t nbl, int M, int ca, int cb,
                                              int nta, int ntb, int64_t ib0, int64_t stride, int k4,
                                              inf_v4d (&acc)[BX_MT][BX_MT]) {
  int oa[BX_MT], ob[BX_MT];  // the lane's column of tile t, or 0 where there is none
#pragma unroll
  for (int t = 0; t < BX_MT; ++t) {
    oa[t] = ca + 16 * t < M ? ca + 16 * t : 0;
    ob[t] = cb + 16 * t < M ? cb + 16 * t : 0;
  }
  for (int64_t ib = ib0; ib < nbl; ib += BX_UNR * stride) {
    double za[BX_UNR][BX_MT], zb[BX_UNR][BX_MT];
    bool ok[BX_UNR];
#pragma unroll
    for (int s = 0; s < BX_UNR; ++s) {
      const int64_t row = ib + s * stride + k4;
      ok[s] = row < nbl;
      const double *p = zt + (size_t)(ok[s] ? row : 0) * rs;
#pragma unroll
      for (int t = 0; t < BX_MT; ++t) za[s][t] = p[oa[t]];
      if (!DIAG) {
#pragma unroll
        for (int t = 0; t < BX_MT; ++t) zb[s][t] = p[ob[t]];
      }
    }
#pragma unroll
    for (int s = 0; s < BX_UNR; ++s) {
#pragma unroll
      for (int t = 0; t < BX_MT; ++t) {
        za[s][t] = (ok[s] && ca + 16 * t < M) ? za[s][t] : 0.0;
        zb[s][t] = DIAG ? za[s][t] : ((ok[s] && cb + 16 * t < M) ? zb[s][t] : 0.0);
      }
#pragma unroll
      for (int ta = 0; ta < BX_MT; ++ta) {
        if (ta < nta) {
#pragma unroll
          for (int tb = DIAG ? ta : 0; tb < BX_MT; ++tb)
            if (tb < ntb) acc[ta][tb] = __builtin_amdgcn_mfma_f64_16x16x4f64(za[s][ta], zb[s][tb], acc[ta][tb], 0, 0, 0);
        }
      }
    }
  }
}

// zt: nbl rows of M columns, rs doubles apart.  partial [gridDim.y block workgroups][gridDim.x macro pairs][BX_REC]
__global__ __launch_bounds__(BX_BLOCK) void influence_block_gram_kernel(const double *__restrict__ zt, int64_t rs, int64_t nbl,
                                                                        int M, int T, int TM, double *__restrict__ partial) {
  __shared__ double red[4 * 256];
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, m = lane & 15, k4 = lane >> 4;
  int mi, mj;
  inf_pair((int)blockIdx.x, TM, mi, mj);  // macro pair (mi <= mj)
  // logical columns of this lane's A rows and B columns in tile 0 of the macro pair; tiles of the pair that exist
  const int ca = 16 * BX_MT * mi + m, cb = 16 * BX_MT * mj + m;
  const int nta = min(BX_MT, T - BX_MT * mi), ntb = min(BX_MT, T - BX_MT * mj);

  inf_v4d acc[BX_MT][BX_MT];
#pragma unroll
  for (int ta = 0; ta < BX_MT; ++ta)
#pragma unroll
    for (int tb = 0; tb < BX_MT; ++tb) acc[ta][tb] = inf_v4d{0.0, 0.0, 0.0, 0.0};

  const int64_t stride = (int64_t)gridDim.y * 4 * 4, ib0 = ((int64_t)blockIdx.y * 4 + wave) * 4;
  if (mi == mj)
    bx_accumulate<true>(zt, rs, nbl, M, ca, cb, nta, ntb, ib0, stride, k4, acc);
  else
    bx_accumulate<false>(zt, rs, nbl, M, ca, cb, nta, ntb, ib0, stride, k4, acc);

  // the four waves' tiles in wave order.  D layout: column = lane & 15, row = (lane >> 4) + 4 * reg
  double *dst = partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * BX_REC;
#pragma unroll
  for (int ta = 0; ta < BX_MT; ++ta)
#pragma unroll
    for (int tb = 0; tb < BX_MT; ++tb) {
#pragma unroll
      for (int g = 0; g < 4; ++g) red[wave * 256 + (k4 + 4 * g) * 16 + m] = acc[ta][tb][g];
      __syncthreads();
      dst[(ta * BX_MT + tb) * 256 + tid] = ((red[tid] + red[256 + tid]) + red[512 + tid]) + red[768 + tid];
      __syncthreads();
    }
}

// G[e] = sum over the nblk workgroups, in index order, of partial[blk][e]      (e < per_blk = macro pairs * BX_REC)
__global__ __launch_bounds__(BX_BLOCK) void influence_block_gram_sum_kernel(const double *__restrict__ partial, int nblk,
                                                                            size_t per_blk, double *__restrict__ G) {
  inf_sum_records(partial, nblk, per_blk, G);
}

// cov [M][M]; a thread per (P, Q), the threads with P <= Q store both
__global__ __launch_bounds__(BX_BLOCK) void influence_block_cross_final_kernel(const double *__restrict__ G,
                                                                               const double *__restrict__ wtot, int M, int TM,
                                                                               double *__restrict__ cov) {
  const size_t Ms = (size_t)M, e = (size_t)blockIdx.x * BX_BLOCK + threadIdx.x;
  if (e >= Ms * Ms) return;
  const size_t P = e / Ms, Q = e % Ms;
  if (P > Q) return;
  const int ti = (int)(P >> 4), tj = (int)(Q >> 4);
  const double g = G[(size_t)inf_pair_index(ti / BX_MT, tj / BX_MT, TM) * BX_REC +
                     ((ti % BX_MT) * BX_MT + (tj % BX_MT)) * 256 + (P & 15) * 16 + (Q & 15)];
  const double W = wtot[0];
  const double v = W == 0.0 ? 0.0 : g / (W * W);
  cov[P * Ms + Q] = v;
  cov[Q * Ms + P] = v;
}

// ---------------------------------------------------------------------------
// host side

struct BxPlan {
  int M, T, TM, pairs, grid_y, cs_parts;
  int64_t nb;
  size_t off_part, off_w, off_partial, off_G, total;  // workspace offsets in doubles (zt at 0, wb at nb M)
};

// block workgroups of the Gram pass over nbl blocks: one per BX_SHARE blocks, up to about four workgroups per CU in all
// (two waves per SIMD, two rounds)
static int bx_grid_y(int64_t nbl, int pairs) {
  int64_t cap = (int64_t)num_cus() * 4 / pairs;
  if (cap < 1) cap = 1;
  const int64_t gy = cdiv(nbl, BX_SHARE);
  return (int)(gy > cap ? cap : gy);
}

static BxPlan bx_plan(int64_t N, int64_t C, int n_f, int64_t block) {
  BxPlan p{};
  p.M = (int)(C * n_f);
  p.T = (p.M + 15) / 16;
  p.TM = (p.T + BX_MT - 1) / BX_MT;
  p.pairs = p.TM * (p.TM + 1) / 2;
  p.nb = cdiv(N, block);
  p.grid_y = bx_grid_y(p.nb, p.pairs);  // level 0 has the most blocks
  const int64_t cs = cdiv(p.nb, 64);
  p.cs_parts = (int)(cs > BX_CS_MAXP ? BX_CS_MAXP : cs);
  p.off_part = (size_t)p.nb * ((size_t)p.M + 1);  // behind pass 1's zt | wb
  p.off_w = p.off_part + (size_t)p.cs_parts * ((size_t)p.M + 1);
  p.off_partial = p.off_w + 8;
  p.off_G = p.off_partial + (size_t)p.grid_y * p.pairs * BX_REC;
  p.total = p.off_G + (size_t)p.pairs * BX_REC;
  return p;
}

static bool bx_args_ok(int64_t N, int64_t C, int n_f, int n_q, int64_t block, int n_levels) {
  return N >= 1 && C >= 1 && C <= BX_MAXC && n_f >= 1 && n_f <= TXM_MAXK && n_q >= 1 && n_q <= TXM_MAXK && block >= 1 &&
         n_levels >= 1 && n_levels <= 32;
}

}  // namespace txm

using namespace txm;

extern "C" size_t txm_influence_block_cross_cov_ws_bytes(int64_t N, int64_t C, int n_f, int n_q, int64_t block, int n_levels) {
  if (!bx_args_ok(N, C, n_f, n_q, block, n_levels)) return 0;
  return bx_plan(N, C, n_f, block).total * sizeof(double) + 256;
}

extern "C" int txm_influence_block_cross_cov(const double *x, int64_t ldx_s, const double *u, const double *w, int64_t N,
                                             int64_t C, int n_f, int n_q, double center_u, const double *center_x,
                                             const double *a, const double *b, int64_t block, int n_levels, double *cov,
                                             double *mean, void *ws, size_t ws_bytes, txm_stream stream) {
  if (const int rc = inf_check_args("influence_block_cross_cov", x && u && center_x && a && b && cov && mean && ws, N, C, BX_MAXC,
                                    " (the result has (C n_f)^2 entries a level)", n_f, n_q, ldx_s >= C, "row pitch ldx_s < C",
                                    center_u))
    return rc;
  if (const int rc = inf_check_block("influence_block_cross_cov", block, n_levels)) return rc;
  if (ws_bytes < txm_influence_block_cross_cov_ws_bytes(N, C, n_f, n_q, block, n_levels)) {
    set_error("influence_block_cross_cov: workspace too small");
    return TXM_ERR_WORKSPACE;
  }
  const BxPlan p = bx_plan(N, C, n_f, block);
  hipStream_t st = (hipStream_t)stream;
  double *base = (double *)ws;
  double *zt = base, *wb = base + (size_t)p.nb * p.M, *part = base + p.off_part, *wtot = base + p.off_w;
  double *partial = base + p.off_partial, *G = base + p.off_G;
  const int rc = ib_block_sums(x, ldx_s, u, w, N, C, n_f, n_q, center_u, center_x, a, b, block, zt, wb, st);
  if (rc != TXM_OK) return rc;

  const dim3 blk(BX_BLOCK);
  hipLaunchKernelGGL(influence_block_colsum_kernel, dim3((unsigned)cdiv(p.M + 1, BX_CS_COLS), (unsigned)p.cs_parts), blk, 0, st,
                     zt, wb, p.nb, p.M, part);
  TXM_LAUNCH_CHECK();
  hipLaunchKernelGGL(influence_block_colsum_final_kernel, dim3((unsigned)cdiv(p.M + 1, BX_BLOCK)), blk, 0, st, part, p.cs_parts,
                     p.M, wtot, mean);
  TXM_LAUNCH_CHECK();

  const size_t per_blk = (size_t)p.pairs * BX_REC, MM = (size_t)p.M * p.M;
  for (int l = 0; l < n_levels; ++l) {
    const int64_t step = (int64_t)1 << l, nbl = (p.nb + step - 1) >> l;
    if (l > 0 && (step >> 1) < p.nb) {  // (otherwise: a single block that has no partner any more)
      int64_t mg = cdiv(nbl * p.M, BX_BLOCK);
      if (mg > (int64_t)num_cus() * 16) mg = (int64_t)num_cus() * 16;
      hipLaunchKernelGGL(influence_block_merge_kernel, dim3((unsigned)mg), blk, 0, st, zt, p.nb, (int64_t)p.M, step, nbl);
      TXM_LAUNCH_CHECK();
    }
    const int gy = bx_grid_y(nbl, p.pairs);  // <= p.grid_y: nbl only shrinks
    hipLaunchKernelGGL(influence_block_gram_kernel, dim3((unsigned)p.pairs, (unsigned)gy), blk, 0, st, zt, step * (int64_t)p.M,
                       nbl, p.M, p.T, p.TM, partial);
    TXM_LAUNCH_CHECK();
    hipLaunchKernelGGL(influence_block_gram_sum_kernel, dim3((unsigned)cdiv((int64_t)per_blk, BX_BLOCK)), blk, 0, st, partial, gy,
                       per_blk, G);
    TXM_LAUNCH_CHECK();
    hipLaunchKernelGGL(influence_block_cross_final_kernel, dim3((unsigned)cdiv((int64_t)MM, BX_BLOCK)), blk, 0, st, G, wtot, p.M,
                       p.TM, cov + (size_t)l * MM);
    TXM_LAUNCH_CHECK();
  }
  return TXM_OK;
}
