// txm_mbar_block.hip -- blocked (batch-means) MBAR error bars for correlated series kept whole (MBARModel.predict_with_error /
// predict_with_covariance / free_energy / free_energy_covariance (block=...), blocking_curve).
//
// Every first-order influence of an MBAR estimate is linear in the row
//   t_n = (W_n1 .. W_nK, {W_na, y_n,(a,0) .. y_n,(a,C-1)} for each target a),      M = K + n_alpha (C + 1) columns,
// with W_nk = p_kn / N_k (p_kn the softmax of txm_mbar_eval at the solution's g), W_na = e^{-a ut_n - logDt_n - lnw_a} (lnw:
// txm_mbar_cov's output, so the weight is ONE exponential and never above 1) and y_n,(a,c) = W_na (x_nc - mean_ac) (mean:
// txm_mbar_predict's output; x is centred on the mean itself, no pivot, no correction term).  State s is cut into blocks of
// block[s] records (a last short one is kept; blocks never straddle two states) and the call returns per level l
//   Gamma_l = sum_beta Tc_beta Tc_beta^T,   Tc_beta = T_beta - (len_beta / n_s) sum_{beta' in s} T_beta',   T_beta = sum_{n in beta} t_n
// for the blocks of block[s] 2^l records.  The covariance of two estimates is l^T Gamma l' (thermoextrap_amd/_mbar_host.py).
//
//   mbar_block_sums_kernel   grid (unit workgroups, K).  A unit is a level-0 block, or -- block[s] > MK_SEG -- one of the
//       block's pieces of MK_SEG records.  The workgroup walks the unit's records in tiles of 64 FROM THE UNIT'S START:
//       phase 1  txm_mbar_cov's: four lanes per record, the softmax p_kn of all K states (no positive exponent) into
//                P[record][k], the NA target weights into V[record][a]; records past the unit's end get zeros.
//       phase 2  VALU.  Lane (c = tid mod CP, g = tid / CP), CP the power of two >= C + 1: column c < C of x, or the column
//                of ones (c == C: the sums of W_na); sub-group g takes the tile's records g, g + 256 / CP, ... in order and
//                adds V[record][a] d to its NA sums.  Lane (k = tid mod 64, g4 = tid / 64) adds P[record][k] of the records
//                g4, g4 + 4, ...  (The contraction is (NA x records) x (records x (C + 1)): at most 8 rows, so the FP64
//                MFMA's 16 x 16 tile would run half empty while x is read once either way; the pass is bound by the K + NA
//                exponentials per record of phase 1 and by the read of x.)
//       At the unit's end the sub-groups are added in index order through LDS and the M sums written: the order of every
//       addition is fixed by the unit's start, its length and C alone -- not by the grid.
//   mbar_block_pieces_kernel   T_beta = its pieces in index order (states with block[s] > MK_SEG only).
//   mbar_block_chunk_kernel / _total_kernel   per state the column sums of its T_beta: chunks of MK_CHUNK blocks in index
//       order, then the chunks in index order.
//   mbar_block_centre_kernel   Tc_beta in place.  The centring comes BEFORE the Gram: the W_nk block sums have means far
//       above their spread.  A state with ONE block is set to exactly 0.0 (its centred sum is T - (n/n) T).
//   mbar_block_merge_kernel    level l from level l - 1: within each state the pairs of the level below, a last unpaired
//       block stays; never across a state boundary.  Tc is linear, so merged centred sums are the centred sums of the
//       merged blocks; a state left with one block is set to exactly 0.0.  The levels ping-pong between two compact
//       arrays (all states' rows contiguous), so the Gram pass sees one matrix of rows M apart.
//   mbar_block_gram_kernel / _gram_sum_kernel   bx_gram of txm_block_gram.h: v_mfma_f64_16x16x4_f64, block axis = k-axis,
//       upper-triangle tiles, workgroup records added in index order.
//   mbar_block_final_kernel    a thread per (P <= Q): the entry and its mirror.
// No atomics: two calls under the same plan give the same bits and Gamma is exactly symmetric.
//
// Workspace: no size query; txm_mbar_block_cov_plan gives the bytes (the Gram pass takes as many block workgroups as
// records fit, at least one).
#include <cmath>
#include <cstring>
#include <vector>

#include "txm_block_gram.h"
#include "txm_mbar.h"

namespace txm {

constexpr int MK_TILE = 64;        // records per tile
constexpr int MK_LDP = MB_MAXK + 1;  // row pitch of P (all K states + one pad double)
constexpr int MK_SEG = 4096;       // records per unit at most: longer blocks are summed in pieces
constexpr int MK_CHUNK = 1024;     // blocks per chunk of the per-state column sums
constexpr int MK_MAXC = 255;

struct MkState {
  int64_t n, block, nb, boff;  // records, block length, level-0 blocks, first row in T
  int64_t pieces, poff;        // pieces per block (1: the block is the unit), first row in the piece array
  int64_t choff, nch;          // first chunk, chunks
};
constexpr size_t MK_HEAD_BYTES = MB_HEAD_BYTES + MB_MAXK * sizeof(MkState);
static_assert(MB_MAXK * sizeof(MkState) <= MB_EXTRA_BYTES, "txm_mbar.h: mb_stage_head's buffer holds the block table");

// grid (unit workgroups, K)
template <int NA>
__global__ __launch_bounds__(MB_BLOCK) void mbar_block_sums_kernel(const txm_mbar_state *__restrict__ tab,
                                                                   const MkState *__restrict__ mk, int K, int C, int cp_log2,
                                                                   const double *__restrict__ gk,
                                                                   const double *__restrict__ a0k,
                                                                   const double *__restrict__ logD, double upiv,
                                                                   const MbarTargets ta, const double *__restrict__ lnw,
                                                                   const double *__restrict__ mean, int n_alpha, int M,
                                                                   double *__restrict__ T, double *__restrict__ part) {
  __shared__ double P[MK_TILE * MK_LDP];  // after a unit's last tile: the sub-groups' sums (NA * 256 + 256 doubles)
  __shared__ double V[MK_TILE * MB_MAXA];
  __shared__ double sg[MB_MAXK], sa[MB_MAXK];
  const int tid = threadIdx.x, s = blockIdx.y;
  const double *__restrict__ x = tab[s].x;
  const double *__restrict__ u = tab[s].u;
  const int64_t n = tab[s].n, ldx = tab[s].ldx_s, off = mb_state_offset(tab, s);
  const MkState st = mk[s];
  if (tid < K) {
    sg[tid] = gk[tid];
    sa[tid] = a0k[tid];
  }
  // phase 1 roles
  const int j1 = tid >> 2, q = tid & 3;
  double al1[2], l1[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int a = q + 4 * t < n_alpha ? q + 4 * t : n_alpha - 1;
    al1[t] = ta.a[a];
    l1[t] = lnw[a];
  }
  // phase 2 roles
  const int cp = 1 << cp_log2, c = tid & (cp - 1), g = tid >> cp_log2, nsub = MB_BLOCK >> cp_log2;
  const bool is_x = c < C, is_one = c == C;
  const int k2 = tid & 63, g4 = tid >> 6;
  double mu[NA];
#pragma unroll
  for (int a = 0; a < NA; ++a) mu[a] = is_x ? mean[(size_t)(a < n_alpha ? a : n_alpha - 1) * C + c] : 0.0;
  double *red = P, *redw = P + NA * MB_BLOCK;
  __syncthreads();

  const int64_t units = st.nb * st.pieces;
  for (int64_t un = blockIdx.x; un < units; un += gridDim.x) {
    const int64_t jb = un / st.pieces, pc = un - jb * st.pieces;
    const int64_t bend = (jb + 1) * st.block < n ? (jb + 1) * st.block : n;
    const int64_t start = jb * st.block + pc * MK_SEG;
    int64_t len = (bend < start + MK_SEG ? bend : start + MK_SEG) - start;  // <= 0: a piece behind a short last block
    len = len < 0 ? 0 : len;
    double acc[NA], accw = 0.0;
#pragma unroll
    for (int a = 0; a < NA; ++a) acc[a] = 0.0;
    for (int64_t t0 = 0; t0 < len; t0 += MK_TILE) {
      {
        const bool ok = t0 + j1 < len;
        const int64_t i = start + t0 + j1;
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
          P[j1 * MK_LDP + k] = e;
        }
        sum += __shfl_xor(sum, 1);
        sum += __shfl_xor(sum, 2);
        const double inv = ok ? 1.0 / sum : 0.0;
        for (int k = q; k < K; k += 4) P[j1 * MK_LDP + k] *= inv;
#pragma unroll
        for (int t = 0; t < 2; ++t)
          if (q + 4 * t < NA) V[j1 * MB_MAXA + q + 4 * t] = ok ? exp(fma(-al1[t], ut, nld) - l1[t]) : 0.0;
      }
      __syncthreads();
      const int tl = len - t0 < MK_TILE ? (int)(len - t0) : MK_TILE;
      if (is_x || is_one) {
#pragma unroll 4
        for (int j = g; j < tl; j += nsub) {
          const double xv = is_x ? x[(start + t0 + j) * ldx + c] : 0.0;
#pragma unroll
          for (int a = 0; a < NA; ++a) acc[a] = fma(V[j * MB_MAXA + a], is_x ? xv - mu[a] : 1.0, acc[a]);
        }
      }
      if (k2 < K)
        for (int j = g4; j < tl; j += 4) accw += P[j * MK_LDP + k2];
      __syncthreads();
    }
    // the sub-groups in index order
#pragma unroll
    for (int a = 0; a < NA; ++a) red[(g * NA + a) * cp + c] = acc[a];
    redw[g4 * 64 + k2] = accw;
    __syncthreads();
    double *dst = st.pieces == 1 ? T + (size_t)(st.boff + jb) * M : part + (size_t)(st.poff + un) * M;
    for (int e = tid; e < n_alpha * (C + 1); e += MB_BLOCK) {
      const int a = e / (C + 1), cc = e - a * (C + 1);
      double v = red[a * cp + cc];
      for (int h = 1; h < nsub; ++h) v += red[(h * NA + a) * cp + cc];
      dst[K + a * (C + 1) + (cc == C ? 0 : 1 + cc)] = v;
    }
    if (tid < K) dst[tid] = (((redw[tid] + redw[64 + tid]) + redw[128 + tid]) + redw[192 + tid]) / (double)tab[tid].n;
    __syncthreads();
  }
}

// the state of row r of the level-0 array (boff ascending)
__device__ __forceinline__ int mk_row_state(const MkState *__restrict__ mk, int K, int64_t r) {
  int s = 0;
  while (s + 1 < K && r >= mk[s + 1].boff) ++s;
  return s;
}

// grid-stride over the level-0 rows; a thread per column
__global__ __launch_bounds__(MB_BLOCK) void mbar_block_pieces_kernel(const MkState *__restrict__ mk, int K, int64_t nbtot,
                                                                     int M, const double *__restrict__ part,
                                                                     double *__restrict__ T) {
  for (int64_t r = blockIdx.x; r < nbtot; r += gridDim.x) {
    const int s = mk_row_state(mk, K, r);
    const int64_t pieces = mk[s].pieces;
    if (pieces == 1) continue;
    const double *src = part + (size_t)(mk[s].poff + (r - mk[s].boff) * pieces) * M;
    for (int m = threadIdx.x; m < M; m += MB_BLOCK) {
      double v = src[m];
      for (int64_t p = 1; p < pieces; ++p) v += src[(size_t)p * M + m];
      T[(size_t)r * M + m] = v;
    }
  }
}

// grid (chunks of all states, column groups of 256): csum[chunk][m] = the chunk's rows in index order
__global__ __launch_bounds__(MB_BLOCK) void mbar_block_chunk_kernel(const MkState *__restrict__ mk, int K, int M,
                                                                    const double *__restrict__ T,
                                                                    double *__restrict__ csum) {
  const int64_t ch = blockIdx.x;
  const int m = (int)blockIdx.y * MB_BLOCK + threadIdx.x;
  if (m >= M) return;
  int s = 0;
  while (s + 1 < K && ch >= mk[s + 1].choff) ++s;
  const int64_t j0 = (ch - mk[s].choff) * MK_CHUNK;
  const int64_t j1 = j0 + MK_CHUNK < mk[s].nb ? j0 + MK_CHUNK : mk[s].nb;
  const double *src = T + (size_t)mk[s].boff * M + m;
  double v = 0.0;
#pragma unroll 4
  for (int64_t j = j0; j < j1; ++j) v += src[(size_t)j * M];
  csum[(size_t)ch * M + m] = v;
}

// grid (K, column groups of 256): tot[s][m] = the state's chunks in index order
__global__ __launch_bounds__(MB_BLOCK) void mbar_block_total_kernel(const MkState *__restrict__ mk, int M,
                                                                    const double *__restrict__ csum,
                                                                    double *__restrict__ tot) {
  const int s = blockIdx.x;
  const int m = (int)blockIdx.y * MB_BLOCK + threadIdx.x;
  if (m >= M) return;
  const double *src = csum + (size_t)mk[s].choff * M + m;
  double v = 0.0;
  for (int64_t h = 0; h < mk[s].nch; ++h) v += src[(size_t)h * M];
  tot[(size_t)s * M + m] = v;
}

// Tc_beta = T_beta - (len_beta / n_s) tot_s in place; exactly 0.0 for a state with one block
__global__ __launch_bounds__(MB_BLOCK) void mbar_block_centre_kernel(const MkState *__restrict__ mk, int K, int64_t nbtot,
                                                                     int M, const double *__restrict__ tot,
                                                                     double *__restrict__ T) {
  for (int64_t r = blockIdx.x; r < nbtot; r += gridDim.x) {
    const int s = mk_row_state(mk, K, r);
    const MkState st = mk[s];
    const int64_t jb = r - st.boff;
    const int64_t len = (jb + 1) * st.block < st.n ? st.block : st.n - jb * st.block;
    const double frac = (double)len / (double)st.n;
    for (int m = threadIdx.x; m < M; m += MB_BLOCK) {
      const size_t at = (size_t)r * M + m;
      T[at] = st.nb == 1 ? 0.0 : T[at] - frac * tot[(size_t)s * M + m];
    }
  }
}

__host__ __device__ __forceinline__ int64_t mk_level_blocks(int64_t nb, int l) { return (nb + (((int64_t)1) << l) - 1) >> l; }

// level l >= 1 from level l - 1 (both compact: state after state); grid-stride over the rows of level l
__global__ __launch_bounds__(MB_BLOCK) void mbar_block_merge_kernel(const MkState *__restrict__ mk, int K, int l, int64_t nbl,
                                                                    int M, const double *__restrict__ src,
                                                                    double *__restrict__ dst) {
  for (int64_t r = blockIdx.x; r < nbl; r += gridDim.x) {
    int s = 0;
    int64_t doff = 0, soff = 0;  // the state's first row at level l and at level l - 1
    for (;; ++s) {
      const int64_t cnt = mk_level_blocks(mk[s].nb, l);
      if (r < doff + cnt || s + 1 == K) break;
      doff += cnt;
      soff += mk_level_blocks(mk[s].nb, l - 1);
    }
    const int64_t cnt = mk_level_blocks(mk[s].nb, l), prev = mk_level_blocks(mk[s].nb, l - 1), j = r - doff;
    const double *a = src + (size_t)(soff + 2 * j) * M;
    const bool pair = 2 * j + 1 < prev;
    for (int m = threadIdx.x; m < M; m += MB_BLOCK)
      dst[(size_t)r * M + m] = cnt == 1 ? 0.0 : (pair ? a[m] + a[(size_t)M + m] : a[m]);
  }
}

// zt: nbl rows of M columns, M doubles apart.  partial [gridDim.y block workgroups][gridDim.x macro pairs][BX_REC]
__global__ __launch_bounds__(BX_BLOCK) void mbar_block_gram_kernel(const double *__restrict__ zt, int64_t nbl, int M, int T,
                                                                   int TM, double *__restrict__ partial) {
  bx_gram(zt, (int64_t)M, nbl, M, T, TM, partial);  // txm_block_gram.h
}

__global__ __launch_bounds__(BX_BLOCK) void mbar_block_gram_sum_kernel(const double *__restrict__ partial, int nblk,
                                                                       size_t per_blk, double *__restrict__ G) {
  inf_sum_records(partial, nblk, per_blk, G);
}

// gamma [M][M]; a thread per (P, Q), the threads with P <= Q store both
__global__ __launch_bounds__(BX_BLOCK) void mbar_block_final_kernel(const double *__restrict__ G, int M, int TM,
                                                                    double *__restrict__ gamma) {
  const size_t Ms = (size_t)M, e = (size_t)blockIdx.x * BX_BLOCK + threadIdx.x;
  if (e >= Ms * Ms) return;
  const size_t P = e / Ms, Q = e % Ms;
  if (P > Q) return;
  const double v = bx_gram_entry(G, P, Q, TM);
  gamma[P * Ms + Q] = v;
  gamma[Q * Ms + P] = v;
}

// ---------------------------------------------------------------------------
// host side

struct MkPlan {
  int M, T, TM, pairs, gy;
  int64_t nbtot, nb1, prows, nchunks, max_units;
  size_t off_l1, off_part, off_csum, off_tot, off_partial, off_G, total;  // doubles behind the head (T at 0)
  size_t bytes;
  MkState st[MB_MAXK];
};

static int mk_check_shape(const char *who, const int64_t *n_host, const int64_t *block_host, int32_t K, int64_t C,
                          int32_t n_alpha, int32_t n_levels) {
  TXM_REQUIRE(K >= 1 && K <= MB_MAXK, "%s: K = %d states outside [1, %d]", who, (int)K, MB_MAXK);
  TXM_REQUIRE(C >= 1 && C <= MK_MAXC, "%s: C = %lld outside [1, %d]", who, (long long)C, MK_MAXC);
  TXM_REQUIRE(n_alpha >= 1 && n_alpha <= MB_MAXA, "%s: n_alpha = %d outside [1, %d]", who, (int)n_alpha, MB_MAXA);
  TXM_REQUIRE(n_levels >= 1 && n_levels <= 32, "%s: n_levels = %d outside [1, 32]", who, (int)n_levels);
  TXM_REQUIRE(n_host && block_host, "%s: null pointer", who);
  for (int32_t s = 0; s < K; ++s) {
    TXM_REQUIRE(n_host[s] >= 1, "%s: state %d has n = %lld samples (need >= 1)", who, (int)s, (long long)n_host[s]);
    TXM_REQUIRE(block_host[s] >= 1, "%s: state %d has block = %lld < 1", who, (int)s, (long long)block_host[s]);
  }
  return TXM_OK;
}

// The layout and the launch plan from the bytes the caller has: everything but the Gram pass's block workgroups is fixed by
// the shapes; those are as many as records fit, at most bx_grid_y's.  TXM_OK or TXM_ERR_WORKSPACE (bytes: the smallest).
static int mk_plan(const int64_t *n_host, const int64_t *block_host, int32_t K, int64_t C, int32_t n_alpha, int32_t n_levels,
                   size_t ws_bytes, MkPlan *p) {
  p->M = (int)(K + n_alpha * (C + 1));
  p->T = (p->M + 15) / 16;
  p->TM = (p->T + BX_MT - 1) / BX_MT;
  p->pairs = p->TM * (p->TM + 1) / 2;
  p->nbtot = p->nb1 = p->prows = p->nchunks = p->max_units = 0;
  for (int32_t s = 0; s < K; ++s) {
    MkState &st = p->st[s];
    st.n = n_host[s];
    st.block = block_host[s] < n_host[s] ? block_host[s] : n_host[s];  // (a longer block is the whole state)
    st.nb = cdiv(st.n, st.block);
    st.boff = p->nbtot;
    st.pieces = cdiv(st.block, MK_SEG);
    st.poff = p->prows;
    st.nch = cdiv(st.nb, MK_CHUNK);
    st.choff = p->nchunks;
    p->nbtot += st.nb;
    p->nb1 += mk_level_blocks(st.nb, 1);
    if (st.pieces > 1) p->prows += st.nb * st.pieces;
    p->nchunks += st.nch;
    const int64_t units = st.nb * st.pieces;
    p->max_units = units > p->max_units ? units : p->max_units;
  }
  const size_t M = (size_t)p->M;
  p->off_l1 = (size_t)p->nbtot * M;
  p->off_part = p->off_l1 + (n_levels > 1 ? (size_t)p->nb1 * M : 0);
  p->off_csum = p->off_part + (size_t)p->prows * M;
  p->off_tot = p->off_csum + (size_t)p->nchunks * M;
  p->off_G = p->off_tot + (size_t)K * M;
  p->off_partial = p->off_G + (size_t)p->pairs * BX_REC;
  const size_t rec_bytes = (size_t)p->pairs * BX_REC * sizeof(double);
  const size_t fixed = MK_HEAD_BYTES + p->off_partial * sizeof(double);
  p->gy = 0;
  p->bytes = fixed + rec_bytes;  // the smallest plan: one block workgroup
  if (ws_bytes < p->bytes) return TXM_ERR_WORKSPACE;
  const int64_t fit = (int64_t)((ws_bytes - fixed) / rec_bytes), want = bx_grid_y(p->nbtot, p->pairs);
  p->gy = (int)(fit < want ? fit : want);
  p->bytes = fixed + (size_t)p->gy * rec_bytes;
  return TXM_OK;
}

}  // namespace txm

using namespace txm;

extern "C" int txm_mbar_block_cov_plan(const int64_t *n_host, const int64_t *block_host, int32_t K, int64_t C,
                                       int32_t n_alpha, int32_t n_levels, size_t ws_bytes, int64_t *plan_host) {
  if (const int rc = mk_check_shape("mbar_block_cov_plan", n_host, block_host, K, C, n_alpha, n_levels)) return rc;
  TXM_REQUIRE(plan_host, "mbar_block_cov_plan: null pointer");
  MkPlan p;
  const int rc = mk_plan(n_host, block_host, K, C, n_alpha, n_levels, ws_bytes, &p);
  plan_host[0] = p.M;
  plan_host[1] = p.nbtot;
  plan_host[2] = p.prows;
  plan_host[3] = p.pairs;
  plan_host[4] = p.gy;
  plan_host[5] = (int64_t)p.bytes;  // refused: the smallest workspace the call takes
  plan_host[6] = (int64_t)MK_HEAD_BYTES;  // where the level-0 array starts in ws
  if (rc != TXM_OK)
    set_error("mbar_block_cov_plan: workspace too small (%zu bytes, the smallest plan needs %zu)", ws_bytes, p.bytes);
  return rc;
}

extern "C" int txm_mbar_block_cov(const txm_mbar_state *states_host, int32_t K, int64_t C, double upiv,
                                  const double *alpha0_host, const double *g_host, const double *logD,
                                  const double *alpha_host, int32_t n_alpha, const double *mean, const double *lnw,
                                  const int64_t *block_host, int32_t n_levels, double *gamma, int64_t *nblocks, void *ws,
                                  size_t ws_bytes, txm_stream stream) {
  TXM_REQUIRE(K >= 1 && K <= MB_MAXK && states_host, "mbar_block_cov: K = %d states outside [1, %d] or a null state table",
              (int)K, MB_MAXK);
  int64_t n_host[MB_MAXK];
  for (int32_t s = 0; s < K; ++s) n_host[s] = states_host[s].n;
  if (const int rc = mk_check_shape("mbar_block_cov", n_host, block_host, K, C, n_alpha, n_levels)) return rc;
  if (const int rc = mb_check_states(states_host, K, true, true, C, "mbar_block_cov", nullptr, nullptr)) return rc;
  TXM_REQUIRE(alpha0_host && g_host && logD && alpha_host && mean && lnw && gamma && nblocks && ws,
              "mbar_block_cov: null pointer");
  if (const int rc = mb_check_finite("mbar_block_cov", K, alpha0_host, g_host, n_alpha, alpha_host, upiv)) return rc;
  MkPlan p;
  if (mk_plan(n_host, block_host, K, C, n_alpha, n_levels, ws_bytes, &p) != TXM_OK) {
    set_error("mbar_block_cov: workspace too small (%zu bytes, the smallest plan needs %zu)", ws_bytes, p.bytes);
    return TXM_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  // one staging copy: state table, g, alpha0 (the head of txm_mbar_eval), then the block table
  MbarHead h;
  if (const int rc = mb_stage_head(ws, states_host, K, g_host, alpha0_host, MK_HEAD_BYTES, p.st, (size_t)K * sizeof(MkState), st,
                                   &h))
    return rc;
  std::vector<int64_t> counts((size_t)n_levels * K);
  for (int l = 0; l < n_levels; ++l)
    for (int32_t s = 0; s < K; ++s) counts[(size_t)l * K + s] = mk_level_blocks(p.st[s].nb, l);
  TXM_HIP(hipMemcpyAsync(nblocks, counts.data(), counts.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
  const txm_mbar_state *tab = h.tab;
  const double *gk = h.gk, *a0k = h.a0k;
  const MkState *mk = (const MkState *)((char *)ws + MB_HEAD_BYTES);
  double *base = (double *)((char *)ws + MK_HEAD_BYTES);
  double *T = base, *L1 = base + p.off_l1, *part = base + p.off_part, *csum = base + p.off_csum, *tot = base + p.off_tot;
  double *G = base + p.off_G, *partial = base + p.off_partial;
  const MbarTargets ta = mb_targets(alpha_host, n_alpha);

  int cp_log2 = 1;
  while ((1 << cp_log2) < C + 1) ++cp_log2;  // <= 8: C + 1 <= 256
  const int64_t cap = mb_blocks_per_state(K);
  const int64_t gx = p.max_units > cap ? cap : p.max_units;
  const dim3 block(MB_BLOCK);
#define TXM_MK(NA_)                                                                                                        \
  hipLaunchKernelGGL((mbar_block_sums_kernel<NA_>), dim3((unsigned)gx, (unsigned)K), block, 0, st, tab, mk, (int)K, (int)C, \
                     cp_log2, gk, a0k, logD, upiv, ta, lnw, mean, (int)n_alpha, p.M, T, part)
  TXM_MB_NA_DISPATCH(n_alpha, TXM_MK)
#undef TXM_MK
  TXM_LAUNCH_CHECK();
  const int64_t rows_cap = (int64_t)num_cus() * 16;
  const unsigned grows = (unsigned)(p.nbtot > rows_cap ? rows_cap : p.nbtot);
  const unsigned gcols = (unsigned)cdiv(p.M, MB_BLOCK);
  if (p.prows > 0) {
    hipLaunchKernelGGL(mbar_block_pieces_kernel, dim3(grows), block, 0, st, mk, (int)K, p.nbtot, p.M, part, T);
    TXM_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(mbar_block_chunk_kernel, dim3((unsigned)p.nchunks, gcols), block, 0, st, mk, (int)K, p.M, T, csum);
  TXM_LAUNCH_CHECK();
  hipLaunchKernelGGL(mbar_block_total_kernel, dim3((unsigned)K, gcols), block, 0, st, mk, p.M, csum, tot);
  TXM_LAUNCH_CHECK();
  hipLaunchKernelGGL(mbar_block_centre_kernel, dim3(grows), block, 0, st, mk, (int)K, p.nbtot, p.M, tot, T);
  TXM_LAUNCH_CHECK();

  const size_t per_blk = (size_t)p.pairs * BX_REC, MM = (size_t)p.M * p.M;
  double *lev[2] = {T, L1};
  for (int l = 0; l < n_levels; ++l) {
    int64_t nbl = 0;
    for (int32_t s = 0; s < K; ++s) nbl += mk_level_blocks(p.st[s].nb, l);
    if (l > 0) {
      hipLaunchKernelGGL(mbar_block_merge_kernel, dim3((unsigned)(nbl > rows_cap ? rows_cap : nbl)), block, 0, st, mk, (int)K,
                         l, nbl, p.M, lev[(l - 1) & 1], lev[l & 1]);
      TXM_LAUNCH_CHECK();
    }
    int gy = bx_grid_y(nbl, p.pairs);
    gy = gy > p.gy ? p.gy : gy;
    hipLaunchKernelGGL(mbar_block_gram_kernel, dim3((unsigned)p.pairs, (unsigned)gy), dim3(BX_BLOCK), 0, st, lev[l & 1], nbl,
                       p.M, p.T, p.TM, partial);
    TXM_LAUNCH_CHECK();
    hipLaunchKernelGGL(mbar_block_gram_sum_kernel, dim3((unsigned)cdiv((int64_t)per_blk, BX_BLOCK)), dim3(BX_BLOCK), 0, st,
                       partial, gy, per_blk, G);
    TXM_LAUNCH_CHECK();
    hipLaunchKernelGGL(mbar_block_final_kernel, dim3((unsigned)cdiv((int64_t)MM, BX_BLOCK)), dim3(BX_BLOCK), 0, st, G, p.M,
                       p.TM, gamma + (size_t)l * MM);
    TXM_LAUNCH_CHECK();
  }
  return TXM_OK;
}
