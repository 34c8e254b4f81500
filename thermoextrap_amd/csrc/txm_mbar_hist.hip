// txm_mbar_hist.hip -- reweighted histograms over the pooled samples and every sum their asymptotic covariance needs
// (MBARModel.histogram).  With 1_b(n) the indicator "sample n is in bin b", the columns
//   W_nk = p_kn / N_k              (sampled state k; p_kn the softmax of txm_mbar_eval at the solution's g)
//   W_na = v_an / sum_n v_an       (target a; v_an = e^{-a ut_n - logDt_n - M_a}, the weight of txm_mbar_predict)
// and the class nbins for every sample whose index is outside [0, nbins), the call gives per target
//   T_kab = sum_n W_nk W_na 1_b(n)  (k < K)     H_ab = sum_n W_na 1_b(n)     S_ab = sum_n W_na^2 1_b(n)
// as out [n_alpha][K + 2][nbins + 1].  For indicator columns these ARE the Gram matrix and the b vectors of the covariance
// (thermoextrap_amd/_mbar_host.py mbar_hist_covariance): nothing of size N x nbins is formed.
//
// One pass over u, logD and the bin index behind predict's exact max pass (mbar_max_kernel: M_a, so no exponent is
// positive).  Per target the contraction over the samples is the product of the K + 2 rows {p_k v_a (k < K), v_a, v_a^2}
// with the one-hot of the bin index: FP64 matrix-pipe work whose B operand is a compare in registers.
//
//   mbar_hist_kernel   grid (sample workgroups, bin-tile groups, row tiles).  A workgroup (four waves) walks the states
//       one after the other, and of each state the 64-sample tiles blockIdx.x, blockIdx.x + gridDim.x, ...
//       phase 1  txm_mbar_cov's: four lanes per sample, the softmax p_kn of all K states (K exps per sample; the 16 rows
//                of this workgroup kept, P[sample][row]), the NA target weights V[sample][a] and the sample's class;
//                samples past the state's end get zeros and class -1.
//       phase 2  a wave takes four of the tile's sixteen 4-sample steps.  Lane (m = lane & 15, q = lane >> 4) holds
//                A[m][q] = row m of sample q (p v_a, v_a or v_a^2) and B[q][m] = (class of sample q == column m of the
//                bin tile) -- one v_mfma_f64_16x16x4_f64 per (step, target, bin tile of the group).  ONE phase 1 serves
//                all BT bin tiles of the group: NA x BT = 32 accumulator tiles (256 registers) per wave.  A bin tile that
//                none of the step's four samples falls into is skipped: it would add +0 products, which changes no bits
//                (measured to pay).
//       At the end the four waves' tiles are added in wave order through LDS: one partial per (workgroup, target, row,
//       column).
//   mbar_hist_sum_kernel    a thread per output entry adds the sample workgroups' partials in index order.
//   mbar_hist_norm_kernel   a block per target: sum_n v_an as the sum of row K's nbins + 1 column sums in index order (there
//       is no column of ones), then every entry divided by its normalisation; lnw.
// No atomics: two calls under the same plan give the same bits.  A column no sample fell into only ever adds +0 products
// to +0: it is exactly 0.0.
//
// Workspace: no size query; the launch is planned from ws_bytes (hh_plan; txm_mbar_hist_plan shows it).
#include <cmath>
#include <cstring>

#include "txm_mbar.h"

namespace txm {

typedef double hh_v4d __attribute__((ext_vector_type(4)));

constexpr int HH_TILE = 64;     // samples per tile
constexpr int HH_LDP = 17;      // row pitch of P (16 rows + one pad double)
constexpr int HH_SHARE = 256;   // samples of the longest state per sample workgroup before the rest is strided
constexpr int HH_ACC = 32;      // accumulator tiles per wave: targets (1, 2, 4 or 8) x bin tiles
constexpr int HH_MAXBINS = 1023;  // nbins + 1 columns: at most 64 bin tiles
// the workspace head of the MBAR entry points (state table, g, alpha0, M), then the K device pointers of the bin indices
constexpr size_t HH_HEAD_BYTES = MB_HEAD_BYTES + MB_MAXK * sizeof(void *);
static_assert(MB_MAXK * sizeof(void *) <= MB_EXTRA_BYTES, "txm_mbar.h: mb_stage_head's buffer holds the bin pointers");

// partial [gridDim.x][gridDim.y][gridDim.z][n_alpha][bt][256]
template <int NA, int BT>
__global__ __launch_bounds__(MB_BLOCK) void mbar_hist_kernel(const txm_mbar_state *__restrict__ tab,
                                                             const int32_t *const *__restrict__ bins, int K, int nbins,
                                                             int NT, int bt, const double *__restrict__ gk,
                                                             const double *__restrict__ a0k,
                                                             const double *__restrict__ logD, double upiv,
                                                             const MbarTargets ta, const double *__restrict__ M,
                                                             int n_alpha, double *__restrict__ partial) {
  __shared__ double P[HH_TILE * HH_LDP];
  __shared__ double V[HH_TILE * MB_MAXA];
  __shared__ double sg[MB_MAXK], sa[MB_MAXK];
  __shared__ int cls[HH_TILE];
  __shared__ double red[4 * 256];
  const int tid = threadIdx.x;
  const int rt = blockIdx.z, grp = blockIdx.y;
  const int row0 = 16 * rt;  // logical rows row0 .. row0 + 15: k < K the states, K the row v, K + 1 the row v^2, above zeros
  const int tile0 = grp * bt;
  const int nbt = NT - tile0 < bt ? NT - tile0 : bt;  // bin tiles of this group
  if (tid < K) {
    sg[tid] = gk[tid];
    sa[tid] = a0k[tid];
  }
  for (int e = tid; e < HH_TILE * HH_LDP; e += MB_BLOCK) P[e] = 0.0;
  // phase 1 roles
  const int j = tid >> 2, q = tid & 3;
  double al1[2], M1[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int a = q + 4 * t < NA ? q + 4 * t : NA - 1;
    al1[t] = ta.a[a];
    M1[t] = M[a];
  }
  // phase 2 roles
  const int wave = tid >> 6, lane = tid & 63, m = lane & 15, k4 = lane >> 4;
  const bool is_sq = row0 + m == K + 1;
  hh_v4d acc[NA][BT];
#pragma unroll
  for (int a = 0; a < NA; ++a)
#pragma unroll
    for (int t = 0; t < BT; ++t) acc[a][t] = hh_v4d{0.0, 0.0, 0.0, 0.0};
  __syncthreads();
  int64_t off = 0;
  for (int s = 0; s < K; ++s) {
    const double *__restrict__ u = tab[s].u;
    const int32_t *__restrict__ bin = bins[s];
    const int64_t n = tab[s].n;
    for (int64_t base = (int64_t)blockIdx.x * HH_TILE; base < n; base += (int64_t)gridDim.x * HH_TILE) {
      {
        const int64_t i = base + j;
        const bool ok = i < n;
        const double ut = ok ? u[i] - upiv : 0.0;
        const double nld = ok ? -logD[off + i] : 0.0;
        if (q == 3) {
          int b = -1;  // past the state's end: no column
          if (ok) {
            b = bin[i];
            b = (b < 0 || b >= nbins) ? nbins : b;  // outside the range: the class after the last bin
          }
          cls[j] = b;
        }
        double mx = -INFINITY;
        for (int k = q; k < K; k += 4) mx = fmax(mx, fma(-sa[k], ut, sg[k]));
        mx = fmax(mx, __shfl_xor(mx, 1));
        mx = fmax(mx, __shfl_xor(mx, 2));
        double sum = 0.0;
        for (int k = q; k < K; k += 4) {
          const double e = exp(fma(-sa[k], ut, sg[k]) - mx);  // K < 4 leaves lanes with mx = -inf and no k: no exp taken
          sum += e;
          if (k >= row0 && k < row0 + 16) P[j * HH_LDP + k - row0] = e;
        }
        sum += __shfl_xor(sum, 1);
        sum += __shfl_xor(sum, 2);
        const double inv = ok ? 1.0 / sum : 0.0;
        for (int k = q; k < K; k += 4)
          if (k >= row0 && k < row0 + 16) P[j * HH_LDP + k - row0] *= inv;
        if (q == 0 && K >= row0 && K < row0 + 16) P[j * HH_LDP + K - row0] = ok ? 1.0 : 0.0;
#pragma unroll
        for (int t = 0; t < 2; ++t)
          if (q + 4 * t < NA) V[j * MB_MAXA + q + 4 * t] = ok ? exp(fma(-al1[t], ut, nld) - M1[t]) : 0.0;
      }
      __syncthreads();
#pragma unroll 1
      for (int st = 0; st < 4; ++st) {
        const int nn = 4 * (4 * wave + st) + k4;
        const double pm = P[nn * HH_LDP + m];
        const int col = cls[nn] - 16 * tile0;  // the sample's class as a column of this group (negative: none)
        const int rel = col - m;               // 16 t: this lane's column of bin tile t is the sample's class
        // the bin tiles of the group that any of the step's four samples (lanes 0, 16, 32, 48) falls into; the others
        // would add +0 products to their accumulators, which changes no bits, and are skipped (wave-uniform)
        const int tsv = col >> 4;
        unsigned hit = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int tk = __builtin_amdgcn_readlane(tsv, 16 * k);
          hit |= (tk >= 0 && tk < BT) ? 1u << tk : 0u;
        }
        if (hit == 0) continue;
        double av[NA];
#pragma unroll
        for (int a = 0; a < NA; ++a) {
          const double va = V[nn * MB_MAXA + a];
          av[a] = is_sq ? va * va : pm * va;
        }
#pragma unroll
        for (int t = 0; t < BT; ++t) {
          if ((hit >> t) & 1u) {
            const double hot = rel == 16 * t ? 1.0 : 0.0;
#pragma unroll
            for (int a = 0; a < NA; ++a) acc[a][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a], hot, acc[a][t], 0, 0, 0);
          }
        }
      }
      __syncthreads();
    }
    off += n;
  }
  // the four waves' tiles in wave order.  D layout: column = lane & 15, row = (lane >> 4) + 4 * reg
  double *dst = partial + (((size_t)blockIdx.x * gridDim.y + grp) * gridDim.z + rt) * ((size_t)n_alpha * bt * 256);
#pragma unroll
  for (int a = 0; a < NA; ++a) {
#pragma unroll
    for (int t = 0; t < BT; ++t) {
      if (a < n_alpha && t < nbt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) red[wave * 256 + (k4 + 4 * r) * 16 + m] = acc[a][t][r];
        __syncthreads();
        dst[((size_t)a * bt + t) * 256 + tid] = ((red[tid] + red[256 + tid]) + red[512 + tid]) + red[768 + tid];
        __syncthreads();
      }
    }
  }
}

// A thread per output entry (a, r, c), r < K + 2, c <= nbins: the nblk sample workgroups' partials in index order.
__global__ __launch_bounds__(MB_BLOCK) void mbar_hist_sum_kernel(const double *__restrict__ partial, int nblk, int G,
                                                                 int RT, int bt, int K, int nbins, int n_alpha,
                                                                 double *__restrict__ out) {
  const size_t e = (size_t)blockIdx.x * MB_BLOCK + threadIdx.x;
  const size_t cols = (size_t)nbins + 1, rows = (size_t)K + 2;
  if (e >= (size_t)n_alpha * rows * cols) return;
  const int a = (int)(e / (rows * cols)), r = (int)((e / cols) % rows), c = (int)(e % cols);
  const int tile = c >> 4, grp = tile / bt, t = tile % bt;
  const size_t rec = (size_t)n_alpha * bt * 256, per_blk = (size_t)G * RT * rec;
  const double *src = partial + ((size_t)grp * RT + (r >> 4)) * rec + ((size_t)a * bt + t) * 256 + (r & 15) * 16 + (c & 15);
  double v = 0.0;
  for (int blk = 0; blk < nblk; ++blk) v += src[(size_t)blk * per_blk];
  out[e] = v;
}

// A block per target.  den = sum_n v_an: row K's column sums added in index order by one lane; then rows k < K over
// N_k den, row K over den, row K + 1 over den^2.
__global__ __launch_bounds__(MB_BLOCK) void mbar_hist_norm_kernel(const txm_mbar_state *__restrict__ tab, int K,
                                                                  int nbins, const double *__restrict__ M,
                                                                  double *__restrict__ out, double *__restrict__ lnw) {
  __shared__ double h[HH_MAXBINS + 1];
  __shared__ double sden;
  const int a = blockIdx.x, cols = nbins + 1;
  double *o = out + (size_t)a * (K + 2) * cols;
  for (int c = threadIdx.x; c < cols; c += MB_BLOCK) h[c] = o[(size_t)K * cols + c];
  __syncthreads();
  if (threadIdx.x == 0) {
    double d = 0.0;
    for (int c = 0; c < cols; ++c) d += h[c];
    sden = d;
    if (lnw) lnw[a] = M[a] + log(d);
  }
  __syncthreads();
  const double den = sden;
  for (int e = threadIdx.x; e < (K + 2) * cols; e += MB_BLOCK) {
    const int r = e / cols;
    const double scale = r < K ? (double)tab[r].n * den : (r == K ? den : den * den);
    o[e] = o[e] / scale;
  }
}

struct HhPlan {
  int64_t bt, groups, rt, gx;
  size_t bytes;
};

// The launch plan from the bytes the caller has: HH_ACC accumulator tiles per wave split between the
// targets and the bin tiles of a group; as many sample workgroups as records fit, at most one per HH_SHARE samples of the
// longest state and about four workgroups per CU in all.  TXM_OK or TXM_ERR_WORKSPACE.
static int hh_plan(int32_t K, int32_t nbins, int32_t n_alpha, int64_t n_max, size_t ws_bytes, HhPlan *p) {
  const int64_t NT = nbins / 16 + 1;  // the bins and the outside class
  const int64_t room = HH_ACC / mb_na_class(n_alpha);
  p->bt = NT < room ? NT : room;
  p->groups = cdiv(NT, p->bt);
  p->rt = cdiv((int64_t)K + 2, 16);
  const size_t rec_bytes = (size_t)(p->groups * p->rt) * (size_t)n_alpha * (size_t)p->bt * 256 * sizeof(double);
  p->gx = 0;
  p->bytes = HH_HEAD_BYTES + rec_bytes;  // the smallest plan: one sample workgroup
  if (ws_bytes < p->bytes) return TXM_ERR_WORKSPACE;
  int64_t gx = (int64_t)((ws_bytes - HH_HEAD_BYTES) / rec_bytes);
  const int64_t share = n_max / HH_SHARE + (n_max % HH_SHARE != 0);
  int64_t cap = (int64_t)num_cus() * 4 / (p->groups * p->rt);
  cap = cap < 1 ? 1 : cap;
  gx = gx > share ? share : gx;
  gx = gx > cap ? cap : gx;
  p->gx = gx < 1 ? 1 : gx;
  p->bytes = HH_HEAD_BYTES + (size_t)p->gx * rec_bytes;
  return TXM_OK;
}

static int hh_check_shape(const char *who, int32_t K, int32_t nbins, int32_t n_alpha) {
  TXM_REQUIRE(K >= 1 && K <= MB_MAXK, "%s: K = %d states outside [1, %d]", who, (int)K, MB_MAXK);
  TXM_REQUIRE(nbins >= 1 && nbins <= HH_MAXBINS, "%s: nbins = %d outside [1, %d]", who, (int)nbins, HH_MAXBINS);
  TXM_REQUIRE(n_alpha >= 1 && n_alpha <= MB_MAXA, "%s: n_alpha = %d outside [1, %d]", who, (int)n_alpha, MB_MAXA);
  return TXM_OK;
}

}  // namespace txm

using namespace txm;

extern "C" int txm_mbar_hist_plan(int32_t K, int32_t nbins, int32_t n_alpha, int64_t n_max, size_t ws_bytes,
                                  int64_t *plan_host) {
  if (const int rc = hh_check_shape("mbar_hist_plan", K, nbins, n_alpha)) return rc;
  TXM_REQUIRE(n_max >= 1, "mbar_hist_plan: n_max = %lld samples (need >= 1)", (long long)n_max);
  TXM_REQUIRE(plan_host, "mbar_hist_plan: null pointer");
  HhPlan p;
  const int rc = hh_plan(K, nbins, n_alpha, n_max, ws_bytes, &p);
  plan_host[0] = p.bt;
  plan_host[1] = p.groups;
  plan_host[2] = p.gx;
  plan_host[3] = (int64_t)p.bytes;  // refused: the smallest workspace the call takes
  if (rc != TXM_OK) set_error("mbar_hist_plan: workspace too small (%zu bytes, the smallest plan needs %zu)", ws_bytes, p.bytes);
  return rc;
}

extern "C" int txm_mbar_hist(const txm_mbar_state *states_host, const int32_t *const *bin_host, int32_t K, int32_t nbins,
                             double upiv, const double *alpha0_host, const double *g_host, const double *logD,
                             const double *alpha_host, int32_t n_alpha, double *out, double *lnw, void *ws,
                             size_t ws_bytes, txm_stream stream) {
  if (const int rc = hh_check_shape("mbar_hist", K, nbins, n_alpha)) return rc;
  int64_t nmax = 0;
  if (const int rc = mb_check_states(states_host, K, false, false, 0, "mbar_hist", nullptr, &nmax)) return rc;
  TXM_REQUIRE(bin_host, "mbar_hist: null table of bin indices");
  for (int32_t s = 0; s < K; ++s) TXM_REQUIRE(bin_host[s], "mbar_hist: state %d has null bin indices", (int)s);
  TXM_REQUIRE(alpha0_host && g_host && logD && alpha_host && out && ws, "mbar_hist: null pointer");
  if (const int rc = mb_check_finite("mbar_hist", K, alpha0_host, g_host, n_alpha, alpha_host, upiv)) return rc;
  HhPlan p;
  if (hh_plan(K, nbins, n_alpha, nmax, ws_bytes, &p) != TXM_OK) {
    set_error("mbar_hist: workspace too small (%zu bytes, the smallest plan needs %zu)", ws_bytes, p.bytes);
    return TXM_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  // one staging copy: state table, g, alpha0 (the head of txm_mbar_eval), the slot of M, the bin pointers
  MbarHead h;
  if (const int rc = mb_stage_head(ws, states_host, K, g_host, alpha0_host, HH_HEAD_BYTES, bin_host, (size_t)K * sizeof(void *), st,
                                   &h))
    return rc;
  const txm_mbar_state *tab = h.tab;
  const double *gk = h.gk, *a0k = h.a0k;
  double *M = h.M;
  const int32_t *const *bins = (const int32_t *const *)((char *)ws + MB_HEAD_BYTES);
  double *partial = (double *)((char *)ws + HH_HEAD_BYTES);
  const MbarTargets ta = mb_targets(alpha_host, n_alpha);
  // exact per-target maximum of the exponent (predict's pass); its per-block maxima lie where the records will, so the
  // blocks are also capped by the bytes of the plan (a maximum is exact in any order: M does not depend on the cap)
  const int64_t fit = (int64_t)((p.bytes - HH_HEAD_BYTES) / ((size_t)K * MB_MAXA * sizeof(double)));
  int64_t capm = mb_blocks_per_state(K);
  capm = capm > fit ? fit : capm;
  if (const int rc = mb_max_pass(tab, K, nmax, capm < 1 ? 1 : capm, logD, upiv, ta, partial, M, st)) return rc;
  const int NT = nbins / 16 + 1;
  const dim3 grid((unsigned)p.gx, (unsigned)p.groups, (unsigned)p.rt), block(MB_BLOCK);
#define TXM_HH(NA_)                                                                                                     \
  hipLaunchKernelGGL((mbar_hist_kernel<NA_, HH_ACC / NA_>), grid, block, 0, st, tab, bins, (int)K, (int)nbins, NT,      \
                     (int)p.bt, gk, a0k, logD, upiv, ta, M, (int)n_alpha, partial)
  TXM_MB_NA_DISPATCH(n_alpha, TXM_HH)
#undef TXM_HH
  TXM_LAUNCH_CHECK();
  const int64_t total = (int64_t)n_alpha * (K + 2) * (nbins + 1);
  hipLaunchKernelGGL(mbar_hist_sum_kernel, dim3((unsigned)cdiv(total, MB_BLOCK)), block, 0, st, partial, (int)p.gx,
                     (int)p.groups, (int)p.rt, (int)p.bt, (int)K, (int)nbins, (int)n_alpha, out);
  TXM_LAUNCH_CHECK();
  hipLaunchKernelGGL(mbar_hist_norm_kernel, dim3((unsigned)n_alpha), block, 0, st, tab, (int)K, (int)nbins, M, out, lnw);
  TXM_LAUNCH_CHECK();
  return TXM_OK;
}
