// txm_lagsum.hip -- symmetrised lag sums of centred series (timeseries.statistical_inefficiency; the reference reaches
// pymbar.timeseries from gpr_active/active_utils.py:244-269):
//
//   R_ab(t) = sum_{i=0}^{n-1-t} (da_i db_{i+t} + db_i da_{i+t}),   da = a - <a>, db = b - <b>
//
// for a list of series pairs out of {u, x_0 .. x_{C-1}} and a block of lags [t0, t0 + nlags).  n T (3C + 1) FMAs for the
// 2C + 1 pairs of a state: matrix-pipe work.  Per wave and per step of four samples at s, one v_mfma_f64_16x16x4_f64 on a
// Toeplitz slice
//        A[m][k] = da[s + k - m]              (16 x 4, one f64 per lane: m = lane & 15, k = lane >> 4)
//        B[k][j] = db[s + k + 16 j + t]       (4 x 16:                   j = lane & 15, k = lane >> 4)
//        D[m][j] += A B                       gathers lag t + 16 j + m of the samples i = s + k - m
// so one accumulator tile (4 f64 per lane) holds 256 lags of one pair and every MFMA is 1024 useful FMAs.  A cross pair
// (x_c, u) is two MFMAs into the same tile (A_x B_u + A_u B_x); an auto pair one, doubled (exactly) at the end.
//
// Three kernels:
//   lag_center_kernel   the series, centred with the caller's means and transposed to one contiguous row each
//                       (d[1 + C][ldd]): the contraction then stages with unit-stride loads (reading a column of the
//                       row-major x per workgroup costs a 128-byte line per 8 useful bytes, per pair and per L2).
//   lag_kernel<NT, X>   a workgroup takes (sample chunk, pair, group of NT lag tiles).  The chunk is walked in stages of
//                       LG_L = 1008 samples: the stage of a is put in LDS between zeros (16 before, 16 behind; zeros
//                       also past the chunk's end), the window of b (LG_L + 256 NT samples from stage start + t, zeros
//                       past n) next to it, and 256 steps (s = stage start + 4 q, q = 0 .. 255: 252 + 4 for the skew
//                       of m) are split over the four waves, 64 consecutive steps each.  Sample i of the stage meets
//                       row m in exactly one step (4 q + k = i - start + m), so it is counted once per lag; the loop
//                       has no bounds handling.  The b window is stored with one pad double per 16 (the lanes of a B
//                       read are 16 doubles apart: 8-way bank conflicts without it); with the step loop unrolled by 4
//                       every LDS offset is an immediate.  Accumulators stay in registers over all stages of a chunk;
//                       at the end the four waves' tiles are added in wave order through LDS and ONE partial per
//                       (chunk, pair, lag) is written.
//   lag_sum_kernel      adds the chunks in index order (no atomics) and doubles the auto pairs.
//
// The chunk length is a function of n alone and a lag's products are accumulated in the same order whichever tile of
// whichever (t0, nlags) block holds it (adding the +-0 products of the zero padding changes no bits): R(t) is bitwise
// reproducible from run to run and across block schedules.
//
// Lag sums of every suffix (timeseries.detect_equilibration; pymbar.timeseries.detect_equilibration loops
// statistical_inefficiency over the origins).  With the series centred once on a pivot p (d = a - p), the origin j * nskip,
// M = n - j nskip and delta = mean(a[j nskip:]) - p,
//   R_j(t) = 2 [Q_j(t) - delta X_j(t) + (M - t) delta^2],   Q_j(t) = sum_{i >= j nskip} d_i d_{i+t},
//                                                           X_j(t) = sum_{i >= j nskip} (d_i + d_{i+t})      (i + t < n)
// Q is the auto lag sum and X the symmetrised cross lag sum of d with a series of ones, both restricted to the "a" index
// i >= j nskip: suffix sums over the segments [j nskip, (j + 1) nskip) of per-segment partials.  Four more kernels:
//   lag_origin_kernel<NT>     the Toeplitz loop of lag_kernel with the chunks cut at the origins (the last segment runs to
//                             n) and two accumulator tile sets from one staging of d: Q += A_d B_d, X += A_d B_1 + A_1 B_d
//                             (three MFMAs per step and tile; the ones are made in the staging loop, 1 inside the segment /
//                             below n and 0 elsewhere; products by 1.0 are exact).  The 16-sample groups of a stage that
//                             lie wholly behind a short segment's end are skipped (they would add +-0 products).
//   lag_origin_segsum_kernel  sum of d over each segment, a fixed tree; lag_origin_delta_kernel adds the segments from the
//                             last to the first: delta_j, and the suffix means p + delta_j.
//   lag_origin_scan_kernel    one thread per (series, lag) walks the segments from the last to the first, keeps the running
//                             Q and X and writes R_j(t) of every origin (0 for t >= M).  Fixed order, no atomics.
// Every delta comes from the segment sums, not from X_j(0), so a lag block needs no other block: R_j(t) has the same bits
// whichever 256-aligned (t0, nlags) block it is computed in.
#include <cstring>
#include <vector>

#include "txm_common.h"

namespace txm {

typedef double lg_v4d __attribute__((ext_vector_type(4)));

constexpr int LG_BLOCK = 256;
constexpr int LG_L = 1008;            // samples per stage: LG_L / 4 + 4 = 256 steps, 64 per wave
constexpr int LG_A = LG_L + 32;       // a stage: 16 zeros, the samples, 16 zeros
constexpr int LG_MAX_CHUNKS = 512;
constexpr int LG_MAX_LAGS = 4096;     // per call
constexpr int LG_MAX_ORIGINS = 4096;  // per call (lag_origin_*)

static inline int64_t lg_chunk_len(int64_t n) {  // a function of n alone
  const int64_t stages = cdiv(n, (int64_t)LG_L * LG_MAX_CHUNKS);
  return (stages < 1 ? 1 : stages) * LG_L;
}
static inline int64_t lg_ldd(int64_t n) { return (n + 15) / 16 * 16; }
static inline int lg_tiles(int32_t nlags) { return nlags % 1024 == 0 ? 4 : (nlags % 512 == 0 ? 2 : 1); }
static inline size_t lg_lds_bytes(int nt, bool cross) {
  const size_t nb = LG_L + 256 * nt;
  const size_t stage = (cross ? 2 : 1) * (LG_A + nb + nb / 16);
  const size_t red = (size_t)4 * nt * 256;
  return (stage > red ? stage : red) * sizeof(double);
}

__global__ __launch_bounds__(LG_BLOCK) void lag_center_kernel(const double *__restrict__ x, int64_t ldx,
                                                              const double *__restrict__ u, int64_t n, int64_t C,
                                                              const double *__restrict__ center,
                                                              double *__restrict__ d, int64_t ldd) {
  __shared__ double tile[32][65];
  const int tid = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * 64;
  if (blockIdx.y == 0 && tid < 64 && r0 + tid < n) d[r0 + tid] = u[r0 + tid] - center[0];
  const int64_t c0 = (int64_t)blockIdx.y * 32;
  if (c0 >= C) return;
#pragma unroll
  for (int pass = 0; pass < 8; ++pass) {
    const int r = (tid >> 5) + 8 * pass, c = tid & 31;
    if (r0 + r < n && c0 + c < C) tile[c][r] = x[(r0 + r) * ldx + c0 + c] - center[1 + c0 + c];
  }
  __syncthreads();
#pragma unroll
  for (int pass = 0; pass < 8; ++pass) {
    const int c = (tid >> 6) + 4 * pass, r = tid & 63;
    if (r0 + r < n && c0 + c < C) d[(1 + c0 + c) * ldd + r0 + r] = tile[c][r];
  }
}

// One workgroup's share of the lag sums: the samples [cb, ce) of the pair (da, db), the NT lag tiles from lag tg on, written
// to dst[NT * 256].  Shared by lag_kernel and lag_batched_kernel: a (chunk, pair, tile group) has the same bits in both.
template <int NT, bool CROSS>
__device__ __forceinline__ void lag_chunk(const double *__restrict__ da, const double *__restrict__ db, int64_t n, int64_t cb,
                                          int64_t ce, int64_t tg, double *__restrict__ dst, double *smem) {
  constexpr int NB = LG_L + 256 * NT;  // the b window of a stage (a multiple of 16)
  constexpr int NBP = NB + NB / 16;    // ... with one pad double per 16
  double *sa0 = smem, *sb0 = sa0 + LG_A, *sa1 = sb0 + NBP, *sb1 = sa1 + LG_A;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int m = lane & 15, k = lane >> 4;
  lg_v4d acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) acc[j] = lg_v4d{0.0, 0.0, 0.0, 0.0};
  // (stages whose whole b window lies past n contribute zeros only)
  for (int64_t c = cb; c < ce && c + tg < n; c += LG_L) {
    const int64_t aend = c + LG_L < ce ? c + LG_L : ce;
    __syncthreads();
    for (int j = tid; j < LG_A; j += LG_BLOCK) {
      const int64_t i = c - 16 + j;
      const bool in = i >= c && i < aend;
      sa0[j] = in ? da[i] : 0.0;
      if (CROSS) sa1[j] = in ? db[i] : 0.0;
    }
    for (int q = tid; q < NB; q += LG_BLOCK) {
      const int64_t i = c + tg + q;
      const bool in = i < n;
      sb0[q + (q >> 4)] = in ? db[i] : 0.0;
      if (CROSS) sb1[q + (q >> 4)] = in ? da[i] : 0.0;
    }
    __syncthreads();
    // step q = 4 g + r reads a at 4 q + k - m + 16 and b at e + 16 (m + 16 j), e = 4 q + k = 16 g + 4 r + k, which the
    // padded layout puts at 17 g + 4 r + k + 17 m + 272 j
    const double *pa0 = sa0 + 16 + k - m, *pa1 = sa1 + 16 + k - m;
    const double *pb0 = sb0 + k + 17 * m, *pb1 = sb1 + k + 17 * m;
    for (int g = 16 * wave; g < 16 * wave + 16; ++g) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double a0 = pa0[16 * g + 4 * r];
        double a1 = 0.0;
        if (CROSS) a1 = pa1[16 * g + 4 * r];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, pb0[17 * g + 4 * r + 272 * j], acc[j], 0, 0, 0);
          if (CROSS) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, pb1[17 * g + 4 * r + 272 * j], acc[j], 0, 0, 0);
        }
      }
    }
  }
  // the four waves' tiles, added in wave order.  D layout: column = lane & 15, row = (lane >> 4) + 4 * reg; the lag of
  // D[row][column] inside its tile is 16 * column + row
  __syncthreads();
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) smem[(wave * NT + j) * 256 + 16 * m + k + 4 * r] = acc[j][r];
  __syncthreads();
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    double v = smem[j * 256 + tid];
#pragma unroll
    for (int w = 1; w < 4; ++w) v += smem[(w * NT + j) * 256 + tid];
    dst[j * 256 + tid] = v;
  }
}

// partial: [chunk][n_pairs][nlags]
template <int NT, bool CROSS>
__global__ __launch_bounds__(LG_BLOCK) void lag_kernel(const double *__restrict__ d, int64_t ldd, int64_t n, int C,
                                                       const int32_t *__restrict__ pairs, int64_t chunk_len,
                                                       int64_t t0, int nlags, double *__restrict__ partial) {
  extern __shared__ double smem[];
  const int p = pairs[blockIdx.y];
  if ((p > C) != CROSS) return;        // the other instance's pair
  const double *__restrict__ da = d + (int64_t)(CROSS ? p - C : p) * ldd;
  const double *__restrict__ db = CROSS ? d : da;
  const int64_t cb = (int64_t)blockIdx.x * chunk_len;
  const int64_t ce = cb + chunk_len < n ? cb + chunk_len : n;
  const int64_t tg = t0 + (int64_t)blockIdx.z * (256 * NT);
  double *dst = partial + ((size_t)blockIdx.x * gridDim.y + blockIdx.y) * nlags + (size_t)blockIdx.z * (256 * NT);
  lag_chunk<NT, CROSS>(da, db, n, cb, ce, tg, dst, smem);
}

__global__ __launch_bounds__(LG_BLOCK) void lag_sum_kernel(const double *__restrict__ partial, int nchunks, int C,
                                                           const int32_t *__restrict__ pairs, int n_pairs, int nlags,
                                                           double *__restrict__ out) {
  const int t = blockIdx.x * LG_BLOCK + threadIdx.x, slot = blockIdx.y;
  double acc = 0.0;
  for (int ch = 0; ch < nchunks; ++ch) acc += partial[((size_t)ch * n_pairs + slot) * nlags + t];
  out[(size_t)slot * nlags + t] = pairs[slot] > C ? acc : 2.0 * acc;
}

// ---- S states in one set of launches (txm_lag_rows_batched, txm_lag_sums_batched) ----
// The head of the rows buffer: one record per state, written by the rows call and read by every kernel of both calls.
struct lg_state_rec {
  int64_t n, ldd, chunk_len, nchunks, row_off;  // row_off: the state's first row, in doubles from the end of the head
  const double *x, *u, *center;                 // (the rows call's operands: only lag_center_batched_kernel reads them)
};
// One (state, pair) of a sums call; part_off: the items before it hold this many chunks (a prefix sum made on the host).
struct lg_item_rec {
  int32_t state, pair;
  int64_t part_off;
};

static inline size_t lg_rows_head(int64_t S) { return align_up((size_t)S * sizeof(lg_state_rec), 256); }

// lag_center_kernel with the state on grid.z: the same subtraction, the rows of state s at rows + row_off.
__global__ __launch_bounds__(LG_BLOCK) void lag_center_batched_kernel(const lg_state_rec *__restrict__ tab, int64_t ldx,
                                                                      int64_t C, double *__restrict__ rows) {
  __shared__ double tile[32][65];
  const lg_state_rec st = tab[blockIdx.z];
  const int64_t n = st.n, ldd = st.ldd;
  const int64_t r0 = (int64_t)blockIdx.x * 64;
  if (r0 >= n) return;                 // past this state's records
  const double *__restrict__ x = st.x, *__restrict__ u = st.u, *__restrict__ center = st.center;
  double *__restrict__ d = rows + st.row_off;
  const int tid = threadIdx.x;
  if (blockIdx.y == 0 && tid < 64 && r0 + tid < n) d[r0 + tid] = u[r0 + tid] - center[0];
  const int64_t c0 = (int64_t)blockIdx.y * 32;
  if (c0 >= C) return;
#pragma unroll
  for (int pass = 0; pass < 8; ++pass) {
    const int r = (tid >> 5) + 8 * pass, c = tid & 31;
    if (r0 + r < n && c0 + c < C) tile[c][r] = x[(r0 + r) * ldx + c0 + c] - center[1 + c0 + c];
  }
  __syncthreads();
#pragma unroll
  for (int pass = 0; pass < 8; ++pass) {
    const int c = (tid >> 6) + 4 * pass, r = tid & 63;
    if (r0 + r < n && c0 + c < C) d[(1 + c0 + c) * ldd + r0 + r] = tile[c][r];
  }
}

// partial: [item][chunk of the item's state][nlags], item i from chunk row items[i].part_off on
template <int NT, bool CROSS>
__global__ __launch_bounds__(LG_BLOCK) void lag_batched_kernel(const lg_state_rec *__restrict__ tab,
                                                               const double *__restrict__ rows,
                                                               const lg_item_rec *__restrict__ items, int C, int64_t t0,
                                                               int nlags, double *__restrict__ partial) {
  extern __shared__ double smem[];
  const lg_item_rec it = items[blockIdx.y];
  const int p = it.pair;
  if ((p > C) != CROSS) return;        // the other instance's pair
  const lg_state_rec st = tab[it.state];
  if ((int64_t)blockIdx.x >= st.nchunks) return;  // a shorter state than the one that sets grid.x
  const double *__restrict__ d = rows + st.row_off;
  const double *__restrict__ da = d + (int64_t)(CROSS ? p - C : p) * st.ldd;
  const double *__restrict__ db = CROSS ? d : da;
  const int64_t n = st.n;
  const int64_t cb = (int64_t)blockIdx.x * st.chunk_len;
  const int64_t ce = cb + st.chunk_len < n ? cb + st.chunk_len : n;
  const int64_t tg = t0 + (int64_t)blockIdx.z * (256 * NT);
  double *dst = partial + ((size_t)it.part_off + blockIdx.x) * nlags + (size_t)blockIdx.z * (256 * NT);
  lag_chunk<NT, CROSS>(da, db, n, cb, ce, tg, dst, smem);
}

// out: [item][nlags]; the chunks of an item in index order, the auto pairs doubled
__global__ __launch_bounds__(LG_BLOCK) void lag_sum_batched_kernel(const double *__restrict__ partial,
                                                                   const lg_state_rec *__restrict__ tab,
                                                                   const lg_item_rec *__restrict__ items, int C, int nlags,
                                                                   double *__restrict__ out) {
  const int t = blockIdx.x * LG_BLOCK + threadIdx.x;
  const lg_item_rec it = items[blockIdx.y];
  const int nchunks = (int)tab[it.state].nchunks;
  const double *__restrict__ p = partial + (size_t)it.part_off * nlags + t;
  double acc = 0.0;
  for (int ch = 0; ch < nchunks; ++ch) acc += p[(size_t)ch * nlags];
  out[(size_t)blockIdx.y * nlags + t] = it.pair > C ? acc : 2.0 * acc;
}

// partial: [segment][series][Q, X][nlags].  Segment j is [j nskip, (j + 1) nskip), the last one runs to n.
template <int NT>
__global__ __launch_bounds__(LG_BLOCK) void lag_origin_kernel(const double *__restrict__ d, int64_t ldd, int64_t n,
                                                              const int32_t *__restrict__ series, int64_t nskip,
                                                              int64_t t0, int nlags, double *__restrict__ partial) {
  constexpr int NB = LG_L + 256 * NT;
  constexpr int NBP = NB + NB / 16;
  extern __shared__ double smem[];
  const double *__restrict__ da = d + (int64_t)series[blockIdx.y] * ldd;
  double *sa0 = smem, *sb0 = sa0 + LG_A, *sa1 = sb0 + NBP, *sb1 = sa1 + LG_A;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int m = lane & 15, k = lane >> 4;
  const int64_t cb = (int64_t)blockIdx.x * nskip;
  const int64_t ce = blockIdx.x + 1 == gridDim.x ? n : cb + nskip;
  const int64_t tg = t0 + (int64_t)blockIdx.z * (256 * NT);
  lg_v4d accq[NT], accx[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) accq[j] = accx[j] = lg_v4d{0.0, 0.0, 0.0, 0.0};
  for (int64_t c = cb; c < ce && c + tg < n; c += LG_L) {
    const int64_t aend = c + LG_L < ce ? c + LG_L : ce;
    __syncthreads();
    for (int j = tid; j < LG_A; j += LG_BLOCK) {
      const int64_t i = c - 16 + j;
      const bool in = i >= c && i < aend;
      sa0[j] = in ? da[i] : 0.0;
      sa1[j] = in ? 1.0 : 0.0;
    }
    for (int q = tid; q < NB; q += LG_BLOCK) {
      const int64_t i = c + tg + q;
      const bool in = i < n;
      sb0[q + (q >> 4)] = in ? da[i] : 0.0;
      sb1[q + (q >> 4)] = in ? 1.0 : 0.0;
    }
    __syncthreads();
    // (the steps of group g read the stage's samples 16 g - 15 .. 16 g + 15: nothing but zeros once 16 g - 15 >= len)
    const int gend = (int)((aend - c + 30) / 16);
    const int glast = gend < 16 * wave + 16 ? gend : 16 * wave + 16;
    const double *pa0 = sa0 + 16 + k - m, *pa1 = sa1 + 16 + k - m;
    const double *pb0 = sb0 + k + 17 * m, *pb1 = sb1 + k + 17 * m;
    for (int g = 16 * wave; g < glast; ++g) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double a0 = pa0[16 * g + 4 * r];
        const double a1 = pa1[16 * g + 4 * r];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          const double b0 = pb0[17 * g + 4 * r + 272 * j];
          const double b1 = pb1[17 * g + 4 * r + 272 * j];
          accq[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, accq[j], 0, 0, 0);
          accx[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, accx[j], 0, 0, 0);
          accx[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, accx[j], 0, 0, 0);
        }
      }
    }
  }
  // the four waves' tiles, added in wave order: Q, then X through the same LDS
  double *dst = partial + ((size_t)blockIdx.x * gridDim.y + blockIdx.y) * 2 * nlags + (size_t)blockIdx.z * (256 * NT);
#pragma unroll
  for (int set = 0; set < 2; ++set) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) smem[(wave * NT + j) * 256 + 16 * m + k + 4 * r] = set ? accx[j][r] : accq[j][r];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      double v = smem[j * 256 + tid];
#pragma unroll
      for (int w = 1; w < 4; ++w) v += smem[(w * NT + j) * 256 + tid];
      dst[(size_t)set * nlags + j * 256 + tid] = v;
    }
  }
}

// segsum: [series][segment]
__global__ __launch_bounds__(LG_BLOCK) void lag_origin_segsum_kernel(const double *__restrict__ d, int64_t ldd, int64_t n,
                                                                     const int32_t *__restrict__ series, int64_t nskip,
                                                                     double *__restrict__ segsum) {
  __shared__ double red[LG_BLOCK];
  const double *__restrict__ da = d + (int64_t)series[blockIdx.y] * ldd;
  const int tid = threadIdx.x;
  const int64_t cb = (int64_t)blockIdx.x * nskip;
  const int64_t ce = blockIdx.x + 1 == gridDim.x ? n : cb + nskip;
  double acc = 0.0;
  for (int64_t i = cb + tid; i < ce; i += LG_BLOCK) acc += da[i];
  red[tid] = acc;
  __syncthreads();
  for (int w = LG_BLOCK / 2; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  if (tid == 0) segsum[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = red[0];
}

// delta, mean_out: [series][origin]
__global__ __launch_bounds__(LG_BLOCK) void lag_origin_delta_kernel(const double *__restrict__ segsum,
                                                                    const double *__restrict__ center,
                                                                    const int32_t *__restrict__ series, int n_series,
                                                                    int n_origins, int64_t n, int64_t nskip,
                                                                    double *__restrict__ delta, double *__restrict__ mean_out) {
  const int s = blockIdx.x * LG_BLOCK + threadIdx.x;
  if (s >= n_series) return;
  const double p = center[series[s]];
  double acc = 0.0;
  for (int j = n_origins - 1; j >= 0; --j) {
    acc += segsum[(size_t)s * n_origins + j];
    const double dl = acc / (double)(n - (int64_t)j * nskip);
    delta[(size_t)s * n_origins + j] = dl;
    if (mean_out) mean_out[(size_t)s * n_origins + j] = p + dl;
  }
}

// out: [series][origin][nlags]
__global__ __launch_bounds__(LG_BLOCK) void lag_origin_scan_kernel(const double *__restrict__ partial,
                                                                   const double *__restrict__ delta, int n_series,
                                                                   int n_origins, int64_t n, int64_t nskip, int64_t t0,
                                                                   int nlags, double *__restrict__ out) {
  const int t = blockIdx.x * LG_BLOCK + threadIdx.x, s = blockIdx.y;
  const int64_t lag = t0 + t;
  double q = 0.0, x = 0.0;
  for (int j = n_origins - 1; j >= 0; --j) {
    const double *__restrict__ p = partial + ((size_t)j * n_series + s) * 2 * nlags + t;
    q += p[0];
    x += p[nlags];
    const int64_t M = n - (int64_t)j * nskip;
    const double dl = delta[(size_t)s * n_origins + j];
    out[((size_t)s * n_origins + j) * nlags + t] = lag < M ? 2.0 * (q - dl * x + (double)(M - lag) * dl * dl) : 0.0;
  }
}

static inline int64_t lgo_origins(int64_t n, int64_t nskip) { return n >= 2 && nskip >= 1 ? cdiv(n - 1, nskip) : 0; }
static bool lgo_shape_ok(int64_t n, int64_t C, int32_t n_series, int64_t nskip, int32_t nlags) {
  const int64_t no = lgo_origins(n, nskip);
  return n >= 2 && n <= ((int64_t)1 << 36) && C >= 0 && C <= 16383 && n_series >= 1 && n_series <= C + 1 && no >= 1 &&
         no <= LG_MAX_ORIGINS && nlags >= 256 && nlags <= LG_MAX_LAGS && nlags % 256 == 0;
}

static bool lg_shape_ok(int64_t n, int64_t C, int32_t n_pairs, int32_t nlags) {
  return n >= 1 && n <= ((int64_t)1 << 36) && C >= 0 && C <= 16383 && n_pairs >= 1 && n_pairs <= 2 * C + 1 && nlags >= 256 &&
         nlags <= LG_MAX_LAGS && nlags % 256 == 0;
}

}  // namespace txm

using namespace txm;

extern "C" size_t txm_lag_sums_ws_bytes(int64_t n, int64_t C, int32_t n_pairs, int32_t nlags) {
  if (!lg_shape_ok(n, C, n_pairs, nlags)) return 0;
  const size_t head = align_up((size_t)n_pairs * sizeof(int32_t), 256);
  const size_t series = (size_t)(1 + C) * (size_t)lg_ldd(n) * sizeof(double);
  const size_t nchunks = (size_t)cdiv(n, lg_chunk_len(n));
  return head + series + nchunks * (size_t)n_pairs * (size_t)nlags * sizeof(double) + 256;
}

extern "C" int txm_lag_sums(const double *x, int64_t ldx_s, const double *u, int64_t n, int64_t C, const double *center,
                            const int32_t *pairs_host, int32_t n_pairs, int64_t t0, int32_t nlags, double *out,
                            void *ws, size_t ws_bytes, txm_stream stream) {
  TXM_REQUIRE(u && center && pairs_host && out && ws, "lag_sums: null pointer");
  TXM_REQUIRE(n >= 1 && n <= ((int64_t)1 << 36), "lag_sums: n = %lld outside [1, 2^36]", (long long)n);
  TXM_REQUIRE(C >= 0 && C <= 16383, "lag_sums: C = %lld outside [0, 16383]", (long long)C);
  TXM_REQUIRE(C == 0 || x, "lag_sums: null x with C = %lld columns", (long long)C);
  TXM_REQUIRE(C == 0 || ldx_s >= C, "lag_sums: row pitch ldx_s = %lld < C = %lld", (long long)ldx_s, (long long)C);
  TXM_REQUIRE(n_pairs >= 1 && n_pairs <= 2 * C + 1, "lag_sums: n_pairs = %d outside [1, 2 C + 1 = %lld]", (int)n_pairs,
              (long long)(2 * C + 1));
  for (int32_t s = 0; s < n_pairs; ++s)
    TXM_REQUIRE(pairs_host[s] >= 0 && pairs_host[s] <= 2 * C, "lag_sums: pair index %d (entry %d) outside [0, 2 C = %lld]",
                (int)pairs_host[s], (int)s, (long long)(2 * C));
  TXM_REQUIRE(t0 >= 0 && t0 % 256 == 0 && t0 <= ((int64_t)1 << 36), "lag_sums: t0 = %lld is not a multiple of 256 in [0, 2^36]",
              (long long)t0);
  TXM_REQUIRE(nlags >= 256 && nlags % 256 == 0 && nlags <= LG_MAX_LAGS,
              "lag_sums: nlags = %d is not a multiple of 256 in [256, %d]", (int)nlags, LG_MAX_LAGS);
  if (ws_bytes < txm_lag_sums_ws_bytes(n, C, n_pairs, nlags)) {
    set_error("lag_sums: workspace too small");
    return TXM_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  const size_t head = align_up((size_t)n_pairs * sizeof(int32_t), 256);
  const int64_t ldd = lg_ldd(n);
  int32_t *pairs = (int32_t *)ws;
  double *d = (double *)((char *)ws + head);
  double *partial = d + (size_t)(1 + C) * ldd;
  TXM_HIP(hipMemcpyAsync(pairs, pairs_host, (size_t)n_pairs * sizeof(int32_t), hipMemcpyHostToDevice, st));
  const int64_t cblocks = C > 0 ? cdiv(C, 32) : 1;
  hipLaunchKernelGGL(lag_center_kernel, dim3((unsigned)cdiv(n, 64), (unsigned)cblocks), dim3(LG_BLOCK), 0, st, x, ldx_s,
                     u, n, C, center, d, ldd);
  TXM_LAUNCH_CHECK();
  const int64_t chunk_len = lg_chunk_len(n);
  const int64_t nchunks = cdiv(n, chunk_len);
  const int nt = lg_tiles(nlags);
  bool any_auto = false, any_cross = false;
  for (int32_t s = 0; s < n_pairs; ++s) (pairs_host[s] > C ? any_cross : any_auto) = true;
  const dim3 grid((unsigned)nchunks, (unsigned)n_pairs, (unsigned)(nlags / (256 * nt))), block(LG_BLOCK);
#define TXM_LG(NT_, X_)                                                                                          \
  hipLaunchKernelGGL((lag_kernel<NT_, X_>), grid, block, lg_lds_bytes(NT_, X_), st, d, ldd, n, (int)C, pairs, \
                     chunk_len, t0, (int)nlags, partial)
  if (any_auto) {
    if (nt == 4) TXM_LG(4, false);
    else if (nt == 2) TXM_LG(2, false);
    else TXM_LG(1, false);
    TXM_LAUNCH_CHECK();
  }
  if (any_cross) {
    if (nt == 4) TXM_LG(4, true);
    else if (nt == 2) TXM_LG(2, true);
    else TXM_LG(1, true);
    TXM_LAUNCH_CHECK();
  }
#undef TXM_LG
  hipLaunchKernelGGL(lag_sum_kernel, dim3((unsigned)(nlags / LG_BLOCK), (unsigned)n_pairs), dim3(LG_BLOCK), 0, st, partial,
                     (int)nchunks, (int)C, pairs, (int)n_pairs, (int)nlags, out);
  TXM_LAUNCH_CHECK();
  return TXM_OK;
}

// ---- the batched entry points ------------------------------------------------------------------------------
namespace txm {
static bool lg_batch_shape_ok(const int64_t *n_host, int64_t S, int64_t C) {
  if (!n_host || S < 1 || S > 65535 || C < 0 || C > 16383) return false;
  for (int64_t s = 0; s < S; ++s)
    if (n_host[s] < 1 || n_host[s] > ((int64_t)1 << 36)) return false;
  return true;
}
static inline size_t lg_items_head(int64_t n_items) { return align_up((size_t)n_items * sizeof(lg_item_rec), 256); }
}  // namespace txm

extern "C" size_t txm_lag_rows_batched_bytes(const int64_t *n_host, int64_t S, int64_t C) {
  if (!lg_batch_shape_ok(n_host, S, C)) return 0;
  size_t rows = 0;
  for (int64_t s = 0; s < S; ++s) rows += (size_t)(1 + C) * (size_t)lg_ldd(n_host[s]);
  return lg_rows_head(S) + rows * sizeof(double);
}

extern "C" int txm_lag_rows_batched(const txm_lag_state *states_host, int64_t S, int64_t ldx_s, int64_t C, void *rows,
                                    size_t rows_bytes, txm_stream stream) {
  TXM_REQUIRE(states_host && rows, "lag_rows_batched: null pointer");
  TXM_REQUIRE(S >= 1 && S <= 65535, "lag_rows_batched: S = %lld outside [1, 65535]", (long long)S);
  TXM_REQUIRE(C >= 0 && C <= 16383, "lag_rows_batched: C = %lld outside [0, 16383]", (long long)C);
  TXM_REQUIRE(C == 0 || ldx_s >= C, "lag_rows_batched: row pitch ldx_s = %lld < C = %lld", (long long)ldx_s, (long long)C);
  static thread_local std::vector<lg_state_rec> tab_host;
  tab_host.resize((size_t)S);
  int64_t off = 0, n_max = 1;
  for (int64_t s = 0; s < S; ++s) {
    const txm_lag_state &h = states_host[s];
    TXM_REQUIRE(h.u && h.center, "lag_rows_batched: null pointer (u or center of state %lld)", (long long)s);
    TXM_REQUIRE(h.n >= 1 && h.n <= ((int64_t)1 << 36), "lag_rows_batched: n = %lld of state %lld outside [1, 2^36]",
                (long long)h.n, (long long)s);
    TXM_REQUIRE(C == 0 || h.x, "lag_rows_batched: null x of state %lld with C = %lld columns", (long long)s, (long long)C);
    const int64_t ldd = lg_ldd(h.n), chunk_len = lg_chunk_len(h.n);
    tab_host[(size_t)s] = lg_state_rec{h.n, ldd, chunk_len, cdiv(h.n, chunk_len), off, h.x, h.u, h.center};
    off += (1 + C) * ldd;
    if (h.n > n_max) n_max = h.n;
  }
  const size_t head = lg_rows_head(S);
  TXM_REQUIRE(rows_bytes == head + (size_t)off * sizeof(double),
              "lag_rows_batched: rows_bytes = %zu is not txm_lag_rows_batched_bytes = %zu", rows_bytes,
              head + (size_t)off * sizeof(double));
  hipStream_t st = (hipStream_t)stream;
  lg_state_rec *tab = (lg_state_rec *)rows;
  TXM_HIP(hipMemcpyAsync(tab, tab_host.data(), (size_t)S * sizeof(lg_state_rec), hipMemcpyHostToDevice, st));
  const int64_t cblocks = C > 0 ? cdiv(C, 32) : 1;
  hipLaunchKernelGGL(lag_center_batched_kernel, dim3((unsigned)cdiv(n_max, 64), (unsigned)cblocks, (unsigned)S),
                     dim3(LG_BLOCK), 0, st, tab, ldx_s, C, (double *)((char *)rows + head));
  TXM_LAUNCH_CHECK();
  return TXM_OK;
}

extern "C" size_t txm_lag_sums_batched_ws_bytes(const int64_t *n_host, int64_t S, int64_t C, const txm_lag_item *items_host,
                                                int64_t n_items, int32_t nlags) {
  if (!lg_batch_shape_ok(n_host, S, C) || !items_host || n_items < 1 || n_items > 65535) return 0;
  if (nlags < 256 || nlags > LG_MAX_LAGS || nlags % 256 != 0) return 0;
  size_t chunks = 0;
  for (int64_t i = 0; i < n_items; ++i) {
    const txm_lag_item &it = items_host[i];
    if (it.state < 0 || it.state >= S || it.pair < 0 || it.pair > 2 * C) return 0;
    chunks += (size_t)cdiv(n_host[it.state], lg_chunk_len(n_host[it.state]));
  }
  return lg_items_head(n_items) + chunks * (size_t)nlags * sizeof(double);
}

extern "C" int txm_lag_sums_batched(const void *rows, size_t rows_bytes, const int64_t *n_host, int64_t S, int64_t C,
                                    const txm_lag_item *items_host, int64_t n_items, int64_t t0, int32_t nlags, double *out,
                                    void *ws, size_t ws_bytes, txm_stream stream) {
  TXM_REQUIRE(rows && n_host && items_host && out && ws, "lag_sums_batched: null pointer");
  TXM_REQUIRE(S >= 1 && S <= 65535, "lag_sums_batched: S = %lld outside [1, 65535]", (long long)S);
  TXM_REQUIRE(C >= 0 && C <= 16383, "lag_sums_batched: C = %lld outside [0, 16383]", (long long)C);
  for (int64_t s = 0; s < S; ++s)
    TXM_REQUIRE(n_host[s] >= 1 && n_host[s] <= ((int64_t)1 << 36), "lag_sums_batched: n = %lld of state %lld outside [1, 2^36]",
                (long long)n_host[s], (long long)s);
  TXM_REQUIRE(n_items >= 1 && n_items <= 65535, "lag_sums_batched: n_items = %lld outside [1, 65535]", (long long)n_items);
  TXM_REQUIRE(t0 >= 0 && t0 % 256 == 0 && t0 <= ((int64_t)1 << 36),
              "lag_sums_batched: t0 = %lld is not a multiple of 256 in [0, 2^36]", (long long)t0);
  TXM_REQUIRE(nlags >= 256 && nlags % 256 == 0 && nlags <= LG_MAX_LAGS,
              "lag_sums_batched: nlags = %d is not a multiple of 256 in [256, %d]", (int)nlags, LG_MAX_LAGS);
  static thread_local std::vector<lg_item_rec> items;
  items.resize((size_t)n_items);
  int64_t chunks = 0, grid_x = 1;
  bool any_auto = false, any_cross = false;
  for (int64_t i = 0; i < n_items; ++i) {
    const txm_lag_item &it = items_host[i];
    TXM_REQUIRE(it.state >= 0 && it.state < S, "lag_sums_batched: state index %d (item %lld) outside [0, S = %lld)",
                (int)it.state, (long long)i, (long long)S);
    TXM_REQUIRE(it.pair >= 0 && it.pair <= 2 * C, "lag_sums_batched: pair index %d (item %lld) outside [0, 2 C = %lld]",
                (int)it.pair, (long long)i, (long long)(2 * C));
    const int64_t nch = cdiv(n_host[it.state], lg_chunk_len(n_host[it.state]));
    items[(size_t)i] = lg_item_rec{it.state, it.pair, chunks};
    chunks += nch;
    if (nch > grid_x) grid_x = nch;
    (it.pair > C ? any_cross : any_auto) = true;
  }
  TXM_REQUIRE(rows_bytes == txm_lag_rows_batched_bytes(n_host, S, C),
              "lag_sums_batched: rows_bytes = %zu is not txm_lag_rows_batched_bytes = %zu of these states", rows_bytes,
              txm_lag_rows_batched_bytes(n_host, S, C));
  const size_t head = lg_items_head(n_items);
  if (ws_bytes < head + (size_t)chunks * (size_t)nlags * sizeof(double)) {
    set_error("lag_sums_batched: workspace too small");
    return TXM_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  const lg_state_rec *tab = (const lg_state_rec *)rows;
  const double *d = (const double *)((const char *)rows + lg_rows_head(S));
  lg_item_rec *items_dev = (lg_item_rec *)ws;
  double *partial = (double *)((char *)ws + head);
  TXM_HIP(hipMemcpyAsync(items_dev, items.data(), (size_t)n_items * sizeof(lg_item_rec), hipMemcpyHostToDevice, st));
  const int nt = lg_tiles(nlags);
  const dim3 grid((unsigned)grid_x, (unsigned)n_items, (unsigned)(nlags / (256 * nt))), block(LG_BLOCK);
#define TXM_LGB(NT_, X_)                                                                                              \
  hipLaunchKernelGGL((lag_batched_kernel<NT_, X_>), grid, block, lg_lds_bytes(NT_, X_), st, tab, d, items_dev, (int)C, \
                     t0, (int)nlags, partial)
  if (any_auto) {
    if (nt == 4) TXM_LGB(4, false);
    else if (nt == 2) TXM_LGB(2, false);
    else TXM_LGB(1, false);
    TXM_LAUNCH_CHECK();
  }
  if (any_cross) {
    if (nt == 4) TXM_LGB(4, true);
    else if (nt == 2) TXM_LGB(2, true);
    else TXM_LGB(1, true);
    TXM_LAUNCH_CHECK();
  }
#undef TXM_LGB
  hipLaunchKernelGGL(lag_sum_batched_kernel, dim3((unsigned)(nlags / LG_BLOCK), (unsigned)n_items), dim3(LG_BLOCK), 0, st,
                     partial, tab, items_dev, (int)C, (int)nlags, out);
  TXM_LAUNCH_CHECK();
  return TXM_OK;
}

extern "C" size_t txm_lag_origin_sums_ws_bytes(int64_t n, int64_t C, int32_t n_series, int64_t nskip, int32_t nlags) {
  if (!lgo_shape_ok(n, C, n_series, nskip, nlags)) return 0;
  const size_t no = (size_t)lgo_origins(n, nskip);
  const size_t head = align_up((size_t)n_series * sizeof(int32_t), 256);
  const size_t rows = (size_t)(1 + C) * (size_t)lg_ldd(n) * sizeof(double);
  const size_t sums = 2 * (size_t)n_series * no * sizeof(double);  // segment sums, deltas
  return head + rows + sums + no * (size_t)n_series * 2 * (size_t)nlags * sizeof(double) + 256;
}

extern "C" int txm_lag_origin_sums(const double *x, int64_t ldx_s, const double *u, int64_t n, int64_t C,
                                   const double *center, const int32_t *series_host, int32_t n_series, int64_t nskip,
                                   int64_t t0, int32_t nlags, double *out, double *mean_out, void *ws, size_t ws_bytes,
                                   txm_stream stream) {
  TXM_REQUIRE(u && center && series_host && out && ws, "lag_origin_sums: null pointer");
  TXM_REQUIRE(n >= 2 && n <= ((int64_t)1 << 36), "lag_origin_sums: n = %lld outside [2, 2^36]", (long long)n);
  TXM_REQUIRE(C >= 0 && C <= 16383, "lag_origin_sums: C = %lld outside [0, 16383]", (long long)C);
  TXM_REQUIRE(C == 0 || x, "lag_origin_sums: null x with C = %lld columns", (long long)C);
  TXM_REQUIRE(C == 0 || ldx_s >= C, "lag_origin_sums: row pitch ldx_s = %lld < C = %lld", (long long)ldx_s, (long long)C);
  TXM_REQUIRE(n_series >= 1 && n_series <= C + 1, "lag_origin_sums: n_series = %d outside [1, 1 + C = %lld]", (int)n_series,
              (long long)(C + 1));
  for (int32_t s = 0; s < n_series; ++s)
    TXM_REQUIRE(series_host[s] >= 0 && series_host[s] <= C, "lag_origin_sums: series index %d (entry %d) outside [0, C = %lld]",
                (int)series_host[s], (int)s, (long long)C);
  TXM_REQUIRE(nskip >= 1, "lag_origin_sums: nskip = %lld < 1", (long long)nskip);
  const int64_t no = lgo_origins(n, nskip);
  TXM_REQUIRE(no <= LG_MAX_ORIGINS, "lag_origin_sums: nskip = %lld gives %lld origins, more than %d (smallest legal nskip: %lld)",
              (long long)nskip, (long long)no, LG_MAX_ORIGINS, (long long)cdiv(n - 1, (int64_t)LG_MAX_ORIGINS));
  TXM_REQUIRE(t0 >= 0 && t0 % 256 == 0 && t0 <= ((int64_t)1 << 36),
              "lag_origin_sums: t0 = %lld is not a multiple of 256 in [0, 2^36]", (long long)t0);
  TXM_REQUIRE(nlags >= 256 && nlags % 256 == 0 && nlags <= LG_MAX_LAGS,
              "lag_origin_sums: nlags = %d is not a multiple of 256 in [256, %d]", (int)nlags, LG_MAX_LAGS);
  if (ws_bytes < txm_lag_origin_sums_ws_bytes(n, C, n_series, nskip, nlags)) {
    set_error("lag_origin_sums: workspace too small");
    return TXM_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  const size_t head = align_up((size_t)n_series * sizeof(int32_t), 256);
  const int64_t ldd = lg_ldd(n);
  int32_t *series = (int32_t *)ws;
  double *d = (double *)((char *)ws + head);
  double *segsum = d + (size_t)(1 + C) * ldd;
  double *delta = segsum + (size_t)n_series * no;
  double *partial = delta + (size_t)n_series * no;
  TXM_HIP(hipMemcpyAsync(series, series_host, (size_t)n_series * sizeof(int32_t), hipMemcpyHostToDevice, st));
  const int64_t cblocks = C > 0 ? cdiv(C, 32) : 1;
  hipLaunchKernelGGL(lag_center_kernel, dim3((unsigned)cdiv(n, 64), (unsigned)cblocks), dim3(LG_BLOCK), 0, st, x, ldx_s,
                     u, n, C, center, d, ldd);
  TXM_LAUNCH_CHECK();
  hipLaunchKernelGGL(lag_origin_segsum_kernel, dim3((unsigned)no, (unsigned)n_series), dim3(LG_BLOCK), 0, st, d, ldd, n,
                     series, nskip, segsum);
  TXM_LAUNCH_CHECK();
  hipLaunchKernelGGL(lag_origin_delta_kernel, dim3((unsigned)cdiv(n_series, LG_BLOCK)), dim3(LG_BLOCK), 0, st, segsum, center,
                     series, (int)n_series, (int)no, n, nskip, delta, mean_out);
  TXM_LAUNCH_CHECK();
  const int nt = lg_tiles(nlags);
  const dim3 grid((unsigned)no, (unsigned)n_series, (unsigned)(nlags / (256 * nt))), block(LG_BLOCK);
#define TXM_LGO(NT_)                                                                                               \
  hipLaunchKernelGGL((lag_origin_kernel<NT_>), grid, block, lg_lds_bytes(NT_, true), st, d, ldd, n, series, nskip, \
                     t0, (int)nlags, partial)
  if (nt == 4) TXM_LGO(4);
  else if (nt == 2) TXM_LGO(2);
  else TXM_LGO(1);
#undef TXM_LGO
  TXM_LAUNCH_CHECK();
  hipLaunchKernelGGL(lag_origin_scan_kernel, dim3((unsigned)(nlags / LG_BLOCK), (unsigned)n_series), dim3(LG_BLOCK), 0, st,
                     partial, delta, (int)n_series, (int)no, n, nskip, t0, (int)nlags, out);
  TXM_LAUNCH_CHECK();
  return TXM_OK;
}
