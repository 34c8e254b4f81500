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
//     txm_influence_cross.hip; the body is bx_gram of txm_block_gram.h, shared with txm_mbar_block.hip).  The M columns are cut into T = ceil(M / 16) tiles and those into TM = ceil(T / 4) macro tiles of
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
#include "txm_block_gram.h"
#include "txm_influence_block.h"

namespace txm {

constexpr int BX_MAXC = 255;       // as txm_influence_cross_cov
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

// zt: nbl rows of M columns, rs doubles apart.  partial [gridDim.y block workgroups][gridDim.x macro pairs][BX_REC]
__global__ __launch_bounds__(BX_BLOCK) void influence_block_gram_kernel(const double *__restrict__ zt, int64_t rs, int64_t nbl,
                                                                        int M, int T, int TM, double *__restrict__ partial) {
  bx_gram(zt, rs, nbl, M, T, TM, partial);  // txm_block_gram.h
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
  const double g = bx_gram_entry(G, P, Q, TM);
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
