// txm_influence_common.h -- what the four delta-method files share (txm_influence.hip, txm_influence_block.hip,
// txm_influence_cross.hip, txm_influence_block_cross.hip): the host's dispatch over a template order, the argument checks
// of the entry points (one text per condition, the entry point's name in front), the column-lane layout of the row-major
// sample passes, and the pair indexing and record sums of the two Gram passes.  Every __global__ kernel stays in its own file.
#pragma once
#include <type_traits>

#include "txm_common.h"

namespace txm {

// ---- host: f(std::integral_constant<int, K>) for the K of [1, TXM_MAXK] that equals k ------------------------------------
template <int K = 1, class F>
static inline int inf_dispatch(int k, const char *what, F &&f) {
  if constexpr (K > TXM_MAXK) {
    set_error("%s out of range", what);
    return TXM_ERR_INVALID;
  } else {
    return k == K ? f(std::integral_constant<int, K>{}) : inf_dispatch<K + 1>(k, what, f);
  }
}

// ---- host: argument checks, in the order the entry points have always tested them ----------------------------------------
static inline int inf_check_orders(const char *name, int n_f, int n_q) {
  TXM_REQUIRE(n_f >= 1 && n_f <= TXM_MAXK, "%s: n_f=%d outside [1, %d]", name, n_f, TXM_MAXK);
  TXM_REQUIRE(n_q >= 1 && n_q <= TXM_MAXK, "%s: n_q=%d outside [1, %d]", name, n_q, TXM_MAXK);
  return TXM_OK;
}

// one state: `ptrs` all pointers non-null, C <= max_c (`c_note` says what grows with C), `pitch_ok` or `pitch_msg`
static inline int inf_check_args(const char *name, bool ptrs, int64_t N, int64_t C, int max_c, const char *c_note, int n_f,
                                 int n_q, bool pitch_ok, const char *pitch_msg, double center_u) {
  TXM_REQUIRE(ptrs, "%s: null pointer", name);
  TXM_REQUIRE(N >= 1 && C >= 1, "%s: need N >= 1 and C >= 1 (N=%lld C=%lld)", name, (long long)N, (long long)C);
  TXM_REQUIRE(C <= max_c, "%s: C > %d unsupported%s", name, max_c, c_note);
  if (const int rc = inf_check_orders(name, n_f, n_q)) return rc;
  TXM_REQUIRE(pitch_ok, "%s: %s", name, pitch_msg);
  TXM_REQUIRE(center_u == center_u, "%s: center_u is NaN", name);
  return TXM_OK;
}

static inline int inf_check_block(const char *name, int64_t block, int n_levels) {
  TXM_REQUIRE(block >= 1, "%s: block=%lld < 1", name, (long long)block);
  TXM_REQUIRE(n_levels >= 1 && n_levels <= 32, "%s: n_levels=%d outside [1, 32]", name, n_levels);
  return TXM_OK;
}

// S states: the shape, then every state of the table; weighted and n_max (the longest state) come back
static inline int inf_check_batch(const char *name, bool ptrs, const txm_inf_state *states_host, int64_t S, int64_t ldx_s,
                                  int64_t C, int max_c, const char *c_note, int n_f, int n_q, bool &weighted, int64_t &n_max) {
  TXM_REQUIRE(ptrs, "%s: null pointer", name);
  TXM_REQUIRE(S >= 1 && S <= 65535, "%s: S=%lld outside [1, 65535]", name, (long long)S);
  TXM_REQUIRE(C >= 1 && C <= max_c, "%s: C=%lld outside [1, %d]%s", name, (long long)C, max_c, c_note);
  if (const int rc = inf_check_orders(name, n_f, n_q)) return rc;
  TXM_REQUIRE(ldx_s >= C, "%s: row pitch ldx_s < C", name);
  weighted = states_host[0].w != nullptr;
  n_max = 0;
  for (int64_t s = 0; s < S; ++s) {
    const txm_inf_state &h = states_host[s];
    TXM_REQUIRE(h.x && h.u, "%s: state %lld has a null pointer", name, (long long)s);
    TXM_REQUIRE((h.w != nullptr) == weighted, "%s: weights for all states or for none", name);
    TXM_REQUIRE(h.n >= 1, "%s: state %lld has n=%lld < 1", name, (long long)s, (long long)h.n);
    if (h.n > n_max) n_max = h.n;
  }
  return TXM_OK;
}

// ---- host: the lanes of a row in the row-major sample passes --------------------------------------------------------------
constexpr int INF_VEC2_MAXQ = 6;  // the largest n_q that takes two columns per lane

// two columns per lane (16-byte loads) while the sums of both columns fit the register file at two waves per SIMD
static inline bool inf_vec2_ok(const double *x, int64_t ldx_s, int64_t C, int n_q) {
  return (C % 2 == 0) && (ldx_s % 2 == 0) && ((reinterpret_cast<uintptr_t>(x) & 15) == 0) && n_q <= INF_VEC2_MAXQ;
}

// 2^lpr_log2 lanes (at most 256) of `vec` columns each cover cols_per_chunk columns; `chunks` of them cover C
struct InfLanes {
  int vec, lpr_log2, cols_per_chunk, chunks;
};

static inline InfLanes inf_lanes(bool vec2, int64_t C) {
  InfLanes p{};
  p.vec = vec2 ? 2 : 1;
  const int64_t lanes = cdiv(C, p.vec);
  while ((1 << p.lpr_log2) < lanes && p.lpr_log2 < 8) ++p.lpr_log2;
  p.cols_per_chunk = (1 << p.lpr_log2) * p.vec;
  p.chunks = (int)cdiv(C, p.cols_per_chunk);
  return p;
}

// ---- device: the Gram passes (256 threads, FP64 MFMA tiles of 16 x 16) ----------------------------------------------------
typedef double inf_v4d __attribute__((ext_vector_type(4)));

// pair p of the upper triangle of a T x T grid in row order: (0,0) (0,1) ... (0,T-1) (1,1) ...
__device__ __forceinline__ void inf_pair(int p, int T, int &i, int &j) {
  i = 0;
  while (p >= T - i) {
    p -= T - i;
    ++i;
  }
  j = i + p;
}

__host__ __device__ __forceinline__ int inf_pair_index(int i, int j, int T) { return i * T - i * (i - 1) / 2 + (j - i); }

// G[e] = sum over the nblk workgroups, in index order, of partial[blk][e]      (e < per_blk)
__device__ __forceinline__ void inf_sum_records(const double *__restrict__ partial, int nblk, size_t per_blk,
                                                double *__restrict__ G) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= per_blk) return;
  double acc = 0.0;
  for (int b = 0; b < nblk; ++b) acc += partial[(size_t)b * per_blk + e];
  G[e] = acc;
}

}  // namespace txm
