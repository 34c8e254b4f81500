// txm_mbar.h -- what the MBAR translation units share:
//   * the workspace head that every (f-5) entry point lays out the same way, the by-value target block and the exact max
//     pass of predict (kernels defined in txm_mbar.hip, launched through mb_max_pass from the other files as well);
//   * mb_state_offset: a state's first sample in the pooled logD (device);
//   * the preamble of an entry point, as static inline host code, each step written once:
//       mb_check_state / mb_check_states   the state table (txm_mbar_boot.hip's bt_check takes the per-state half)
//       mb_check_finite                    alpha0 / g, the targets, the pivot
//       mb_stage_head, mb_head             the head (or its leading bytes) in one hipMemcpyAsync; where its parts lie
//       mb_targets                         the MbarTargets fill
//       mb_blocks_per_state, mb_max_pass   the two launches of the max pass under a workgroup cap
//       mb_na_class, TXM_MB_NA_DISPATCH    the n_alpha -> {1, 2, 4, 8} class of the kernels templated on NA
//     A check whose text differs between entry points stays at its call site (the null-pointer lists, the joint
//     "K ... or a null state table" of txm_mbar_cov and txm_mbar_block_cov, the bootstrap's own finiteness texts).
#pragma once
#include <cmath>
#include <cstring>

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
// the most an entry point stages behind MB_HEAD_BYTES (txm_mbar_block_cov's table of 64-byte MkState entries)
constexpr size_t MB_EXTRA_BYTES = MB_MAXK * 64;

struct MbarTargets {
  double a[MB_MAXA];
};

// partial [state][gridDim.x][MB_MAXA]: per-block maxima of -a ut_n - logD_n; grid (blocks, K)
__global__ __launch_bounds__(MB_BLOCK) void mbar_max_kernel(const txm_mbar_state *__restrict__ tab, const double *__restrict__ logD, double upiv,
                                const MbarTargets ta, double *__restrict__ partial);
// one block: M[MB_MAXA] = the maxima over the nblk partial rows
__global__ __launch_bounds__(MB_BLOCK) void mbar_max_final_kernel(const double *__restrict__ partial, int nblk, double *__restrict__ M);

// the first sample of state s in the pooled logD
__device__ inline int64_t mb_state_offset(const txm_mbar_state *tab, int s) {
  int64_t off = 0;
  for (int t = 0; t < s; ++t) off += tab[t].n;
  return off;
}

// ---- the preamble of an entry point (host) ----------------------------------------------------------------------------
// One state's entry: u, n >= 1 and, with need_x, x and the row pitch.  joint_ux: a null u or x is reported in one text
// (txm_mbar_cov, _cross_cov, _block_cov) instead of one each.
static inline int mb_check_state(const txm_mbar_state &st, int32_t s, bool need_x, bool joint_ux, int64_t C, const char *what) {
  if (need_x && joint_ux) TXM_REQUIRE(st.u && st.x, "%s: state %d has a null u or x", what, (int)s);
  TXM_REQUIRE(st.u, "%s: state %d has a null u", what, (int)s);
  TXM_REQUIRE(st.n >= 1, "%s: state %d has n = %lld samples (need >= 1)", what, (int)s, (long long)st.n);
  if (need_x) {
    TXM_REQUIRE(st.x, "%s: state %d has a null x", what, (int)s);
    TXM_REQUIRE(st.ldx_s >= C, "%s: state %d has row pitch ldx_s = %lld < C = %lld", what, (int)s, (long long)st.ldx_s,
                (long long)C);
  }
  return TXM_OK;
}

// The table, K and every state; ntot / nmax (either may be null): the pooled and the longest state's samples.
static inline int mb_check_states(const txm_mbar_state *states_host, int32_t K, bool need_x, bool joint_ux, int64_t C,
                                  const char *what, int64_t *ntot, int64_t *nmax) {
  TXM_REQUIRE(states_host, "%s: null state table", what);
  TXM_REQUIRE(K >= 1 && K <= MB_MAXK, "%s: K = %d states outside [1, %d]", what, (int)K, MB_MAXK);
  int64_t tot = 0, mx = 0;
  for (int32_t s = 0; s < K; ++s) {
    if (const int rc = mb_check_state(states_host[s], s, need_x, joint_ux, C, what)) return rc;
    tot += states_host[s].n;
    mx = states_host[s].n > mx ? states_host[s].n : mx;
  }
  if (ntot) *ntot = tot;
  if (nmax) *nmax = mx;
  return TXM_OK;
}

// alpha0 / g of the K states (g_host null: the call takes neither), the n_alpha targets (alpha_host null: not looked at),
// the pivot.
static inline int mb_check_finite(const char *what, int32_t K, const double *alpha0_host, const double *g_host, int32_t n_alpha,
                                  const double *alpha_host, double upiv) {
  if (g_host)
    for (int32_t k = 0; k < K; ++k)
      TXM_REQUIRE(std::isfinite(alpha0_host[k]) && std::isfinite(g_host[k]), "%s: alpha0 / g of state %d not finite", what,
                  (int)k);
  if (alpha_host)
    for (int32_t a = 0; a < n_alpha; ++a) TXM_REQUIRE(std::isfinite(alpha_host[a]), "%s: target %d not finite", what, (int)a);
  TXM_REQUIRE(std::isfinite(upiv), "%s: pivot not finite", what);
  return TXM_OK;
}

struct MbarHead {
  const txm_mbar_state *tab;
  const double *gk, *a0k;
  double *M;
};

// where the parts of the head lie in a workspace
static inline MbarHead mb_head(void *ws) {
  MbarHead h;
  h.tab = (const txm_mbar_state *)ws;
  h.gk = (const double *)((char *)ws + MB_MAXK * sizeof(txm_mbar_state));
  h.a0k = h.gk + MB_MAXK;
  h.M = (double *)((char *)ws + MB_TAB_BYTES);
  return h;
}

// Stages the head of the workspace in ONE hipMemcpyAsync of head_bytes: the state table (zero-padded to MB_MAXK), g and
// alpha0 (null: left zero -- txm_mbar_cross_cov copies only the table), the slot of M and, with `extra`, extra_bytes of it
// behind MB_HEAD_BYTES.  Only the head_bytes that travel are zeroed.  (txm_mbar_predict copies its K table entries
// straight from the caller and stages nothing.)
static inline int mb_stage_head(void *ws, const txm_mbar_state *states_host, int32_t K, const double *g_host,
                                const double *alpha0_host, size_t head_bytes, const void *extra, size_t extra_bytes,
                                hipStream_t st, MbarHead *h) {
  unsigned char head[MB_HEAD_BYTES + MB_EXTRA_BYTES];
  TXM_REQUIRE(head_bytes <= sizeof(head) && (!extra || MB_HEAD_BYTES + extra_bytes <= head_bytes),
              "mbar: a workspace head of %zu bytes with %zu extra does not fit the staging buffer", head_bytes, extra_bytes);
  memset(head, 0, head_bytes);
  memcpy(head, states_host, (size_t)K * sizeof(txm_mbar_state));
  if (g_host) memcpy(head + MB_MAXK * sizeof(txm_mbar_state), g_host, (size_t)K * sizeof(double));
  if (alpha0_host)
    memcpy(head + MB_MAXK * sizeof(txm_mbar_state) + MB_MAXK * sizeof(double), alpha0_host, (size_t)K * sizeof(double));
  if (extra) memcpy(head + MB_HEAD_BYTES, extra, extra_bytes);
  TXM_HIP(hipMemcpyAsync(ws, head, head_bytes, hipMemcpyHostToDevice, st));
  *h = mb_head(ws);
  return TXM_OK;
}

// unused targets repeat the last one
static inline MbarTargets mb_targets(const double *alpha_host, int32_t n_alpha) {
  MbarTargets ta;
  for (int a = 0; a < MB_MAXA; ++a) ta.a[a] = alpha_host[a < n_alpha ? a : n_alpha - 1];
  return ta;
}

static inline int64_t mb_blocks_per_state(int64_t K) {
  int64_t cap = (int64_t)num_cus() * 8 / K;  // at most num_cus * 8 blocks over all states
  return cap < 1 ? 1 : cap;
}

// The exact per-target maximum of the exponent, M[a] = max_n (-a ut_n - logD_n): at most `cap` workgroups per state
// write their maxima to `partial`, one block reduces them (a maximum is exact in any order: M does not depend on cap).
static inline int mb_max_pass(const txm_mbar_state *tab, int32_t K, int64_t nmax, int64_t cap, const double *logD, double upiv,
                              const MbarTargets &ta, double *partial, double *M, hipStream_t st) {
  int64_t gm = cdiv(nmax, (int64_t)MB_BLOCK * 8);
  gm = gm > cap ? cap : (gm < 1 ? 1 : gm);
  hipLaunchKernelGGL(mbar_max_kernel, dim3((unsigned)gm, (unsigned)K), dim3(MB_BLOCK), 0, st, tab, logD, upiv, ta, partial);
  TXM_LAUNCH_CHECK();
  hipLaunchKernelGGL(mbar_max_final_kernel, dim3(1), dim3(MB_BLOCK), 0, st, partial, (int)(gm * K), M);
  TXM_LAUNCH_CHECK();
  return TXM_OK;
}

// the instantiation of a kernel templated on NA that serves n_alpha targets
static inline int mb_na_class(int32_t n_alpha) { return n_alpha <= 1 ? 1 : (n_alpha <= 2 ? 2 : (n_alpha <= 4 ? 4 : 8)); }

// LAUNCH(NA) for the class of n_alpha
#define TXM_MB_NA_DISPATCH(n_alpha, LAUNCH) \
  switch (txm::mb_na_class(n_alpha)) {      \
    case 1: LAUNCH(1); break;               \
    case 2: LAUNCH(2); break;               \
    case 4: LAUNCH(4); break;               \
    default: LAUNCH(8);                     \
  }

}  // namespace txm
