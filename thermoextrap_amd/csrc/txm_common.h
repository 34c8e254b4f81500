// txm_common.h -- shared host/device helpers for libtxmom (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <atomic>

#include "../../include/txmom.h"

#define TXM_MAXK (TXM_MAX_ORDER + 1)
#define TXM_WAVE 64

namespace txm {

// thread-local last error
void set_error(const char *fmt, ...);
int hip_fail(hipError_t e, const char *what, const char *file, int line);

#define TXM_HIP(call)                                                     \
  do {                                                                    \
    hipError_t _e = (call);                                               \
    if (_e != hipSuccess) return txm::hip_fail(_e, #call, __FILE__, __LINE__); \
  } while (0)

#define TXM_LAUNCH_CHECK()                                                \
  do {                                                                    \
    hipError_t _e = hipGetLastError();                                    \
    if (_e != hipSuccess) return txm::hip_fail(_e, "kernel launch", __FILE__, __LINE__); \
  } while (0)

#define TXM_REQUIRE(cond, ...)                                            \
  do {                                                                    \
    if (!(cond)) {                                                        \
      txm::set_error(__VA_ARGS__);                                        \
      return TXM_ERR_INVALID;                                             \
    }                                                                     \
  } while (0)

static inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
static inline size_t align_up(size_t a, size_t b) { return (a + b - 1) / b * b; }

// Number of CUs of the current device (cached by txm_init; 256 on MI355X).
int num_cus();

// hipFuncAttributeMaxDynamicSharedMemorySize belongs to (function, device): set it once per device the calling
// process launches on (`mask` is the call site's static bit set of devices already served).
#define TXM_SET_MAX_LDS(func, bytes)                                                                   \
  do {                                                                                                 \
    static std::atomic<uint64_t> lds_mask_{0};                                                         \
    int dev_ = 0;                                                                                      \
    TXM_HIP(hipGetDevice(&dev_));                                                                      \
    const uint64_t bit_ = (uint64_t)1 << (dev_ & 63);                                                  \
    if (!(lds_mask_.load(std::memory_order_relaxed) & bit_)) {                                         \
      TXM_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(func),                                \
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)(bytes)));          \
      lds_mask_.fetch_or(bit_, std::memory_order_relaxed);                                             \
    }                                                                                                  \
  } while (0)

// ---- pivot-sum -> central moment shift (device + host) --------------------
// S0[j] = sum w du^j, S1[j] = sum w dx du^j about the pivot (pu, px), j < K.
// Writes one cmomy state [2][K]:  [0][0]=W, [0][1]=<u>, [1][0]=<x>,
// [a][b] = <(x-<x>)^a (u-<u>)^b>.
template <int K>
__host__ __device__ inline void pivot_sums_to_state(const double *S0, const double *S1, double pu,
                                                    double px, double *state) {
  const double W = S0[0];
  const double inv = 1.0 / W;
  const double du = (K > 1) ? S0[1] * inv : 0.0;  // <u> - pu
  const double dx = S1[0] * inv;                  // <x> - px
  double m0[K], m1[K];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    m0[j] = S0[j] * inv;
    m1[j] = S1[j] * inv;
  }
  // binomial shift of the u variable by -du:  sum_j C(b,j) (-du)^(b-j) m[j]
#pragma unroll
  for (int b = K - 1; b >= 0; --b) {
    double a0 = 0.0, a1 = 0.0, p = 1.0, c = 1.0;  // p = (-du)^(b-j), c = C(b, j)
    // iterate j from b down to 0
#pragma unroll
    for (int j = b; j >= 0; --j) {
      a0 += c * p * m0[j];
      a1 += c * p * (m1[j] - dx * m0[j]);
      p *= -du;
      c = c * (double)j / (double)(b - j + 1);  // C(b, j-1) = C(b,j) * j / (b-j+1)
    }
    state[b] = a0;
    state[K + b] = a1;
  }
  state[0] = W;
  if (K > 1) state[1] = pu + du;
  state[K] = px + dx;
}

// Total weight EXACTLY zero (every w_i = 0; a bootstrap replicate whose frequency row is all zeros, or that drew only
// samples of weight zero): the empty state, all zeros -- what push_vals and resample_data give and what cmomy returns --
// instead of the 0 / 0 of the shift.  Any other weight sum takes pivot_sums_to_state unchanged (the same bits).
template <int K>
__host__ __device__ inline void pivot_sums_to_state_or_empty(const double *S0, const double *S1, double pu, double px,
                                                             double *state) {
  if (S0[0] == 0.0) {
#pragma unroll
    for (int q = 0; q < 2 * K; ++q) state[q] = 0.0;
    return;
  }
  pivot_sums_to_state<K>(S0, S1, pu, px, state);
}

// The bootstrap kernels (txm_resample*.hip) address a sample row of x through UNSIGNED 32-BIT BYTE offsets from a
// wave-uniform base: the widest is the FP64 kernel's lane_xoff = (3 * 256 * ldx_s + column) * 8, where in the plain and the
// batched launch the base is the unshifted x and `column` runs up to C - 1 (the listed launch folds its column group into
// the base; the int8 kernels' own offsets span at most 31 rows and the C columns).  It stays below 2^32 iff
// 768 * ldx_s + C <= 2^29: TXM_RESAMPLE_PITCH_OK (include/txmom.h); txm_resample_vals[_batched] refuse anything else.
static_assert(TXM_RESAMPLE_PITCH_OK(699050, 512) && !TXM_RESAMPLE_PITCH_OK(699050, 513) && !TXM_RESAMPLE_PITCH_OK(699051, 1) &&
                  ((uint64_t)(768 * (int64_t)699050 + 511) * 8 < ((uint64_t)1 << 32)) && ((uint64_t)(768 * (int64_t)699050 + 512) * 8 == ((uint64_t)1 << 32)),
              "include/txmom.h: TXM_RESAMPLE_PITCH_OK");

}  // namespace txm
