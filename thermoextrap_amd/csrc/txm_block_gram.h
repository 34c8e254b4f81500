// txm_block_gram.h -- the Gram pass over block sums that txm_influence_block_cross.hip and txm_mbar_block.hip share:
// G = sum_b z_b z_b^T on the FP64 matrix pipe (v_mfma_f64_16x16x4_f64), the block axis as the k-axis of the MFMA.
//
// The M columns are cut into T = ceil(M / 16) tiles and those into TM = ceil(T / 4) macro tiles of 4 x 4 tiles; grid (macro
// pairs mi <= mj, block workgroups).  Lane (m = lane & 15, k = lane >> 4) holds A[m][k] = z_{b0+k}[16 ti + m] and
// B[k][m] = z_{b0+k}[16 tj + m].  A wave keeps the up to 16 accumulator tiles of its macro pair (128 VGPRs) and takes every
// fourth 4-block step of its workgroup: 4 A and 4 B operands per 16 MFMAs, sixteen independent accumulation chains.  Tiles
// below the diagonal of a diagonal macro pair and tiles >= T are skipped (wave-uniform); a column >= M or a block >= nbl is
// read at column 0 / row 0 (addresses that exist, so the loads of a step stay unconditional and in flight together) and
// selected to zero, never used.  At the end the four waves' tiles are added in wave order through LDS: one record of 16
// tiles per (workgroup, macro pair); inf_sum_records adds the workgroups' records in index order.  No atomics.
// The __global__ kernels that call bx_gram stay in the two files; both are built in VGPR form (_build.py).
#pragma once
#include "txm_influence_common.h"

namespace txm {

constexpr int BX_BLOCK = 256;      // four waves
constexpr int BX_MT = 4;           // tiles a side of a macro tile
constexpr int BX_SHARE = 256;      // blocks a workgroup takes before the grid grows by one workgroup
constexpr int BX_UNR = 2;          // 4-block steps a wave has in flight
constexpr int BX_REC = BX_MT * BX_MT * 256;  // doubles of one (workgroup, macro pair) record

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

// The body of a Gram kernel (BX_BLOCK threads; grid (macro pairs, block workgroups)).  zt: nbl rows of M columns, rs doubles
// apart.  partial [gridDim.y block workgroups][gridDim.x macro pairs][BX_REC]
__device__ __forceinline__ void bx_gram(const double *__restrict__ zt, int64_t rs, int64_t nbl, int M, int T, int TM,
                                        double *__restrict__ partial) {
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

// the entry of G for the logical columns P <= Q of a record array [macro pairs][BX_REC]
__device__ __forceinline__ double bx_gram_entry(const double *__restrict__ G, size_t P, size_t Q, int TM) {
  const int ti = (int)(P >> 4), tj = (int)(Q >> 4);
  return G[(size_t)inf_pair_index(ti / BX_MT, tj / BX_MT, TM) * BX_REC + ((ti % BX_MT) * BX_MT + (tj % BX_MT)) * 256 +
           (P & 15) * 16 + (Q & 15)];
}

// block workgroups of the Gram pass over nbl blocks: one per BX_SHARE blocks, up to about four workgroups per CU in all
// (two waves per SIMD, two rounds)
static inline int bx_grid_y(int64_t nbl, int pairs) {
  int64_t cap = (int64_t)num_cus() * 4 / pairs;
  if (cap < 1) cap = 1;
  const int64_t gy = cdiv(nbl, BX_SHARE);
  return (int)(gy > cap ? cap : (gy < 1 ? 1 : gy));
}

}  // namespace txm
