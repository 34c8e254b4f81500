// txm_mbar.h -- what the MBAR translation units share: the workspace head that every (f-5) entry point lays out the same
// way, the by-value target block and the exact max pass of predict (defined in txm_mbar.hip, launched from
// txm_mbar_cov.hip as well).
#pragma once
#include "txm_common.h"

namespace txm {

constexpr int MB_BLOCK = 256;
constexpr int MB_MAXK = 64;
constexpr int MB_REGK = 8;   // K <= MB_REGK: register kernel
constexpr int MB_MAXA = 8;   // targets per predict call
constexpr int MB_TILE = MB_BLOCK / 4;  // samples per LDS tile (four lanes per sample)

// workspace head: the state table, g[MB_MAXK], alpha0[MB_MAXK] (one host-to-device copy), then M[MB_MAXA]
constexpr size_t MB_TAB_BYTES = MB_MAXK * sizeof(txm_mbar_state) + 2 * MB_MAXK * sizeof(double);
constexpr size_t MB_HEAD_BYTES = MB_TAB_BYTES + 256;

struct MbarTargets {
  double a[MB_MAXA];
};

// partial [state][gridDim.x][MB_MAXA]: per-block maxima of -a ut_n - logD_n; grid (blocks, K)
__global__ __launch_bounds__(MB_BLOCK) void mbar_max_kernel(const txm_mbar_state *__restrict__ tab, const double *__restrict__ logD, double upiv,
                                const MbarTargets ta, double *__restrict__ partial);
// one block: M[MB_MAXA] = the maxima over the nblk partial rows
__global__ __launch_bounds__(MB_BLOCK) void mbar_max_final_kernel(const double *__restrict__ partial, int nblk, double *__restrict__ M);

}  // namespace txm
