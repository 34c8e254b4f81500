// txm_pivot.h -- pivot estimation kernels shared by the reduce and resample
// translation units (static: one copy per TU, no relocatable device code).
#pragma once
#include "txm_common.h"

namespace txm {

constexpr int RED_BLOCK = 256;
constexpr int PIVOT_SAMPLES = 1024;

// ---------------------------------------------------------------------------
// pivot: block b = 0 -> u, b >= 1 -> column b-1.  pivot[b] = mean of a strided
// subsample.  Any value near the mean works; exactness is irrelevant.
static __global__ void pivot_kernel(const double *__restrict__ x, int64_t ldx_s, int64_t ldx_c,
                             const double *__restrict__ u, int64_t ldu_s, int64_t N,
                             double *__restrict__ pivot) {
  const int b = blockIdx.x;
  const int64_t ns = N < PIVOT_SAMPLES ? N : PIVOT_SAMPLES;
  const int64_t step = N / ns;
  double acc = 0.0;
  for (int64_t k = threadIdx.x; k < ns; k += blockDim.x) {
    const int64_t i = k * step;
    acc += (b == 0) ? u[i * ldu_s] : x[i * ldx_s + (int64_t)(b - 1) * ldx_c];
  }
  __shared__ double sh[RED_BLOCK];
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int off = RED_BLOCK / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double p = sh[0] / (double)ns;
    // a non-finite pivot (inf/nan in the subsample) would poison every sum;
    // fall back to 0 and let the data speak for itself.
    if (!(p - p == 0.0)) p = 0.0;
    pivot[b] = p;
  }
}

// batched variant (S state points, blockIdx.y = state): pivot[s][1 + C]
static __global__ void pivot_batch_kernel(const txm_state_ptrs *__restrict__ batch, int64_t ldx_s, int64_t N,
                                          int64_t C, double *__restrict__ pivot) {
  const int b = blockIdx.x;
  const txm_state_ptrs bs = batch[blockIdx.y];
  const int64_t ns = N < PIVOT_SAMPLES ? N : PIVOT_SAMPLES;
  const int64_t step = N / ns;
  double acc = 0.0;
  for (int64_t k = threadIdx.x; k < ns; k += blockDim.x) {
    const int64_t i = k * step;
    acc += (b == 0) ? bs.u[i] : bs.x[i * ldx_s + (int64_t)(b - 1)];
  }
  __shared__ double sh[RED_BLOCK];
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int off = RED_BLOCK / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double p = sh[0] / (double)ns;
    if (!(p - p == 0.0)) p = 0.0;
    pivot[(int64_t)blockIdx.y * (1 + C) + b] = p;
  }
}

// 1-D series variant: pivot[r] for row r of u2d.
static __global__ void pivot_rows_kernel(const double *__restrict__ u, int64_t ldu_r, int64_t N,
                                  double *__restrict__ pivot) {
  const int r = blockIdx.x;
  const int64_t ns = N < PIVOT_SAMPLES ? N : PIVOT_SAMPLES;
  const int64_t step = N / ns;
  double acc = 0.0;
  for (int64_t k = threadIdx.x; k < ns; k += blockDim.x) acc += u[(int64_t)r * ldu_r + k * step];
  __shared__ double sh[RED_BLOCK];
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int off = RED_BLOCK / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double p = sh[0] / (double)ns;
    if (!(p - p == 0.0)) p = 0.0;
    pivot[r] = p;
  }
}

// ---------------------------------------------------------------------------
// Weighted pivots (the reduce entry points with w != NULL; the kernels above stay what they are for the unweighted calls
// and for the bootstrap calls of txm_resample.hip).  The sums are accumulated about the pivot and an off-pivot of delta weighted sigmas costs
// about (1 + delta)^order in accuracy, so with weights the pivot has to sit near the WEIGHTED mean: reweighting weights
// exp(-dbeta u) or a mask put it many weighted sigmas from the unweighted one.  Rule, per series (one block each):
//   1. weighted mean of ns = min(N, 1024) samples spread evenly over the series, rows floor(k N / ns) -- NOT the stride
//      N / ns of the kernels above, which never sees the last N - ns (N / ns) rows (for 1024 < N < 2048 it is the first
//      1024 rows): with a sorted series and the weight at its end those rows can pass any test among themselves and still
//      lie tens of weighted sigmas out.  Rows of weight zero are skipped (a finite value there never matters).  Taken
//      when the weight sum is finite and positive and the subsample is the whole series (ns == N) or carries a Kish
//      effective count (sum w)^2 / sum w^2 of at least PIVOT_MIN_ESS rows -- within ~ 1 / sqrt(32) weighted sigmas;
//   2. else the weighted mean of ALL rows (the block walks the series: the price of a subsample that saw too little
//      weight, paid only then);
//   3. else (total weight zero or non-finite) the unweighted mean of the subsample; non-finite -> 0, as above.
constexpr double PIVOT_MIN_ESS = 32.0;

__device__ __forceinline__ bool pivot_finite(double v) { return v - v == 0.0; }

// sums of (a, b, c) over the block, returned to every thread; fixed order
__device__ inline void pivot_block_sum3(double &a, double &b, double &c, double (*sh)[RED_BLOCK]) {
  __syncthreads();  // (readers of an earlier call are done)
  sh[0][threadIdx.x] = a;
  sh[1][threadIdx.x] = b;
  sh[2][threadIdx.x] = c;
  __syncthreads();
  for (int off = RED_BLOCK / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) {
      sh[0][threadIdx.x] += sh[0][threadIdx.x + off];
      sh[1][threadIdx.x] += sh[1][threadIdx.x + off];
      sh[2][threadIdx.x] += sh[2][threadIdx.x + off];
    }
    __syncthreads();
  }
  a = sh[0][0];
  b = sh[1][0];
  c = sh[2][0];
}

// val(i): sample i of the block's series.  Every thread of the block returns the same pivot.
template <class Val>
__device__ inline double weighted_pivot(Val val, const double *__restrict__ w, int64_t N) {
  __shared__ double sh[3][RED_BLOCK];
  const int64_t ns = N < PIVOT_SAMPLES ? N : PIVOT_SAMPLES;
  double sw = 0.0, sww = 0.0, swv = 0.0;
  for (int64_t k = threadIdx.x; k < ns; k += RED_BLOCK) {
    const int64_t i = k * N / ns;  // < N; k < 1024, so the product fits for any N an array can have
    const double wi = w[i];
    if (wi != 0.0) {
      sw += wi;
      sww = fma(wi, wi, sww);
      swv = fma(wi, val(i), swv);
    }
  }
  pivot_block_sum3(sw, sww, swv, sh);
  double p = swv / sw;
  if (pivot_finite(sw) && sw > 0.0 && (ns == N || sw * sw >= PIVOT_MIN_ESS * sww) && pivot_finite(p)) return p;
  if (ns < N) {  // the subsample saw too little of the weight: every row
    sw = sww = swv = 0.0;
    for (int64_t i = threadIdx.x; i < N; i += RED_BLOCK) {
      const double wi = w[i];
      if (wi != 0.0) {
        sw += wi;
        swv = fma(wi, val(i), swv);
      }
    }
    pivot_block_sum3(sw, sww, swv, sh);
    p = swv / sw;
    if (pivot_finite(sw) && sw > 0.0 && pivot_finite(p)) return p;
  }
  sw = sww = swv = 0.0;  // no usable weight at all: the unweighted estimate
  for (int64_t k = threadIdx.x; k < ns; k += RED_BLOCK) swv += val(k * N / ns);
  pivot_block_sum3(sw, sww, swv, sh);
  p = swv / (double)ns;
  return pivot_finite(p) ? p : 0.0;
}

static __global__ __launch_bounds__(RED_BLOCK) void pivot_w_kernel(const double *__restrict__ x, int64_t ldx_s, int64_t ldx_c,
                                                                   const double *__restrict__ u, const double *__restrict__ w,
                                                                   int64_t N, double *__restrict__ pivot) {
  const int b = blockIdx.x;
  const double *base = (b == 0) ? u : x + (int64_t)(b - 1) * ldx_c;
  const int64_t ld = (b == 0) ? 1 : ldx_s;
  const double p = weighted_pivot([&](int64_t i) { return base[i * ld]; }, w, N);
  if (threadIdx.x == 0) pivot[b] = p;
}

static __global__ __launch_bounds__(RED_BLOCK) void pivot_batch_w_kernel(const txm_state_ptrs *__restrict__ batch, int64_t ldx_s,
                                                                         int64_t N, int64_t C, double *__restrict__ pivot) {
  const int b = blockIdx.x;
  const txm_state_ptrs bs = batch[blockIdx.y];
  const double *base = (b == 0) ? bs.u : bs.x + (b - 1);
  const int64_t ld = (b == 0) ? 1 : ldx_s;
  const double p = weighted_pivot([&](int64_t i) { return base[i * ld]; }, bs.w, N);
  if (threadIdx.x == 0) pivot[(int64_t)blockIdx.y * (1 + C) + b] = p;
}

static __global__ __launch_bounds__(RED_BLOCK) void pivot_rows_w_kernel(const double *__restrict__ u, int64_t ldu_r,
                                                                        const double *__restrict__ w, int64_t N,
                                                                        double *__restrict__ pivot) {
  const double *base = u + (int64_t)blockIdx.x * ldu_r;
  const double p = weighted_pivot([&](int64_t i) { return base[i]; }, w, N);
  if (threadIdx.x == 0) pivot[blockIdx.x] = p;
}

}  // namespace txm
