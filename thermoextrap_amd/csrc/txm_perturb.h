// txm_perturb.h -- what txm_perturb.hip and txm_perturb_cov.hip share: the extremes pre-pass that fixes the reference
// point uref of the weights e^{-da (u - uref)}, the launch plan of the sample kernels and the head of the workspace.
// Both files take uref from the same kernels in the same order, so their weights are the same numbers.
#pragma once
#include "txm_common.h"

namespace txm {

constexpr int PB_BLOCK = 256;
constexpr int PB_MAXA = 8;

// extremes of u over the samples of replicate blockIdx.y with a positive count (all samples when freq == NULL):
// part[rep][gridDim.x][2]
static __global__ __launch_bounds__(PB_BLOCK) void minmax_kernel(const double *__restrict__ u, int64_t N,
                                                                 const int64_t *__restrict__ freq,
                                                                 double *__restrict__ part) {
  double lo = INFINITY, hi = -INFINITY;
  const int64_t *f = freq ? freq + (int64_t)blockIdx.y * N : nullptr;
  for (int64_t i = (int64_t)blockIdx.x * PB_BLOCK + threadIdx.x; i < N; i += (int64_t)gridDim.x * PB_BLOCK) {
    if (f && f[i] <= 0) continue;
    const double v = u[i];
    lo = v < lo ? v : lo;
    hi = v > hi ? v : hi;
  }
  __shared__ double sl[PB_BLOCK], sh[PB_BLOCK];
  sl[threadIdx.x] = lo;
  sh[threadIdx.x] = hi;
  __syncthreads();
  for (int off = PB_BLOCK / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) {
      sl[threadIdx.x] = sl[threadIdx.x + off] < sl[threadIdx.x] ? sl[threadIdx.x + off] : sl[threadIdx.x];
      sh[threadIdx.x] = sh[threadIdx.x + off] > sh[threadIdx.x] ? sh[threadIdx.x + off] : sh[threadIdx.x];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double *dst = part + 2 * ((size_t)blockIdx.y * gridDim.x + blockIdx.x);
    dst[0] = sl[0];
    dst[1] = sh[0];
  }
}

// mm[rep][2]; thread per replicate
static __global__ __launch_bounds__(PB_BLOCK) void minmax_final_kernel(const double *__restrict__ part, int nblk,
                                                                       int64_t nrep, double *__restrict__ mm) {
  const int64_t rep = (int64_t)blockIdx.x * PB_BLOCK + threadIdx.x;
  if (rep >= nrep) return;
  const double *p = part + 2 * (size_t)rep * nblk;
  double lo = INFINITY, hi = -INFINITY;
  for (int b = 0; b < nblk; ++b) {
    lo = p[2 * b] < lo ? p[2 * b] : lo;
    hi = p[2 * b + 1] > hi ? p[2 * b + 1] : hi;
  }
  if (lo > hi) lo = hi = 0.0;  // a replicate without samples: its averages are 0/0 whatever the reference point
  mm[2 * rep] = lo;
  mm[2 * rep + 1] = hi;
}

// blocks per replicate of the extremes pre-pass: all replicates together stay within 8 blocks per CU
static inline int pb_mm_blocks(int64_t N, int64_t nrep) {
  int64_t g = cdiv(N, PB_BLOCK * 8);
  const int64_t cap = (int64_t)num_cus() * 8 / nrep;
  if (g > cap) g = cap;
  return g < 1 ? 1 : (int)g;
}

struct PerturbArgs {
  double da[PB_MAXA];
};

struct PbPlan {
  int vec, l2, chunks, gx;
  int64_t cols_pad;
};

static inline PbPlan pb_plan(const double *x, int64_t ldx_s, int64_t N, int64_t C, int64_t nrep) {
  PbPlan p;
  const bool v2 = (C % 2 == 0) && (ldx_s % 2 == 0) && ((reinterpret_cast<uintptr_t>(x) & 15) == 0);
  p.vec = v2 ? 2 : 1;
  int64_t lanes = cdiv(C, p.vec);
  p.l2 = 0;
  while ((1 << p.l2) < lanes && p.l2 < 8) ++p.l2;
  const int cpc = (1 << p.l2) * p.vec;
  p.chunks = (int)cdiv(C, cpc);
  p.cols_pad = (int64_t)p.chunks * cpc;
  int64_t want = cdiv(N, (int64_t)(PB_BLOCK >> p.l2) * 4);
  int64_t cap = (int64_t)num_cus() * 8 / (nrep > 8 ? 8 : nrep);
  if (cap < 1) cap = 1;
  if (want > cap) want = cap;
  if (want < 1) want = 1;
  p.gx = (int)want;
  return p;
}

// the widest cols_pad pb_plan can choose for C columns (VEC 1: the next power of two, whole 512s beyond one chunk)
static inline int64_t pb_cols_pad_max(int64_t C) {
  int64_t cols_pad = 1;
  while (cols_pad < C) cols_pad <<= 1;
  if (cols_pad > 512) cols_pad = cdiv(C, 512) * 512;
  return cols_pad;
}

// head of the workspace: mm[nrep][2], then the pre-pass partials [nrep][pb_mm_blocks][2]
static inline size_t pb_mm_bytes(int64_t N, int64_t nrep) {
  return align_up((size_t)nrep * 2 * sizeof(double), 256) +
         align_up((size_t)nrep * pb_mm_blocks(N, nrep) * 2 * sizeof(double), 256);
}

// the two launches of the pre-pass into a workspace that starts with pb_mm_bytes(N, nrep) bytes: mm = (double *)ws after them
static inline int pb_launch_minmax(const double *u, int64_t N, const int64_t *freq, int64_t nrep, void *ws,
                                   hipStream_t st) {
  double *mm = (double *)ws;
  double *mpart = (double *)((char *)ws + align_up((size_t)nrep * 2 * sizeof(double), 256));
  const int gmm = pb_mm_blocks(N, nrep);
  hipLaunchKernelGGL(minmax_kernel, dim3(gmm, (unsigned)nrep), dim3(PB_BLOCK), 0, st, u, N, freq, mpart);
  TXM_LAUNCH_CHECK();
  hipLaunchKernelGGL(minmax_final_kernel, dim3((unsigned)cdiv(nrep, PB_BLOCK)), dim3(PB_BLOCK), 0, st, mpart, gmm,
                     nrep, mm);
  TXM_LAUNCH_CHECK();
  return TXM_OK;
}

}  // namespace txm
