// txm_influence.hip -- delta-method (infinitesimal-jackknife) covariance of derivative estimates, one pass over the samples
// (ExtrapModel.derivs_cov / predict_with_error, gpr_input method="delta").
//
// For every column c the caller gives the empirical influence functions of n_f estimates as polynomials
//      psi_k(n) = sum_q (a[c][k][q] + b[c][k][q] dx) du^q,     dx = x[n][c] - center_x[c],  du = u[n] - center_u,  q < n_q
// and wants   cov[c][i][j] = sum_n w_n^2 psi_i psi_j / (sum_n w_n)^2,   mean[c][k] = sum_n w_n psi_k / sum_n w_n.
//
// psi_i psi_j is a polynomial in (dx, du) of degree <= 2 in dx and <= 2 (n_q - 1) in du, so the sample pass does not need the
// coefficients at all: it accumulates the shifted power sums
//      T_p[r] = sum_n w_n^2 dx^p du^r   p = 0, 1, 2,  r <= 2 (n_q - 1)          M_p[q] = sum_n w_n dx^p du^q   p = 0, 1,  q < n_q
// (4 n_q - 2 + n_q fused multiply-adds per element at 8 bytes read, against n_f (2 n_q + 1) + n_f (n_f + 1) / 2 for forming
// every psi: 25 against 70 at order 4, which keeps the pass on the HBM side of the FP64 balance point), and a per-column
// epilogue contracts them with the coefficients:
//      sum_n w^2 psi_i psi_j = sum_{q,q'} a_iq a_jq' T_0[q+q'] + (a_iq b_jq' + b_iq a_jq') T_1[q+q'] + b_iq b_jq' T_2[q+q'].
// Every product of the expansion is bounded by the matching product of B_k(n) = sum_q (|a_kq| + |b_kq| |dx|) |du|^q, so the
// first-order rounding bound is that of the direct sum: eps * sum_n p_n^2 B_i B_j.
//
// Kernels (the structure of txm_reduce.hip: per-workgroup partial sums, merged in a fixed order -- no floating-point atomics)
//   influence_rowmajor_kernel : x is (rec, val) row-major; a lane owns VEC fixed columns, whole rows are read coalesced.
//   influence_colmajor_kernel : every series contiguous along the samples; lanes <-> samples, blockIdx.y = series.
//   influence_finalize_kernel : block per column: fixed-order sum of the partials, then the contraction above.
// A row of weight zero is skipped (selected out, not multiplied by zero): it may hold anything.
//
// txm_influence_cov_batched runs the same three bodies for S states in ONE launch each, the state on a grid
// axis (influence_*_batch_kernel).  Every state keeps the plan of its own n -- grid_x_s workgroups, row stride
// grid_x_s * ROWS, partials added over grid_x_s records -- inside a launch as wide as the widest state; the workgroups a
// state does not use leave at once.  So state s gets the bits of the single call on state s.
#include <vector>

#include "txm_influence_common.h"

namespace txm {

constexpr int INF_BLOCK = 256;
constexpr int INF_CH = 8;  // values per pass of the block reductions (8 * 256 doubles of LDS)

typedef double inf_v2d __attribute__((ext_vector_type(2)));

template <int NQ>
struct inf_layout {
  static constexpr int NT = 2 * NQ - 1;       // powers of du in the w^2 sums
  static constexpr int SH = NT + NQ;          // per row: T0 | M0
  static constexpr int PC = 2 * NT + NQ;      // per column: T1 | T2 | M1
  static constexpr int NS = SH + PC;          // one column's record in the partials: T0 | M0 | T1 | T2 | M1
};

// one sample row into a lane's sums: sh = T0 | M0, pc[v] = T1 | T2 | M1 of the lane's v-th column
template <int NQ, int VEC, bool WEIGHTED>
__device__ __forceinline__ void inf_body(double ui, double wi, const double (&xv)[VEC], double cu, const double (&px)[VEC],
                                         double *__restrict__ sh, double (*__restrict__ pc)[inf_layout<NQ>::PC]) {
  constexpr int NT = inf_layout<NQ>::NT;
  const bool live = !WEIGHTED || wi != 0.0;
  const double du = live ? ui - cu : 0.0;
  double dx[VEC], dx2[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    dx[v] = live ? xv[v] - px[v] : 0.0;
    dx2[v] = dx[v] * dx[v];
  }
  double p1 = wi, p2 = wi * wi;  // w du^r, w^2 du^r
#pragma unroll
  for (int r = 0; r < NT; ++r) {
    sh[r] += p2;
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      pc[v][r] = fma(dx[v], p2, pc[v][r]);
      pc[v][NT + r] = fma(dx2[v], p2, pc[v][NT + r]);
    }
    if (r < NQ) {
      sh[NT + r] += p1;
#pragma unroll
      for (int v = 0; v < VEC; ++v) pc[v][2 * NT + r] = fma(dx[v], p1, pc[v][2 * NT + r]);
      p1 *= du;
    }
    p2 *= du;
  }
}

// Thread layout of txm_reduce.hip's row-major kernel: lane_in_row = tid & (LPR - 1) owns columns col0 + {0 .. VEC-1},
// row_in_blk = tid >> lpr_log2; blockIdx.y selects a chunk of LPR * VEC columns; rows are grid-strided, UNR loads in flight.
// partial: [blockIdx.y][blockIdx.x][LPR * VEC columns][NS]
// grid_x: the workgroups along x that work on THIS state (gridDim.x of the single call; the state's own plan in a batch,
// whose launch is as wide as its widest state) -- the row stride and the partials' layout follow it, not the launch.
template <int NQ, int VEC, bool WEIGHTED>
__device__ __forceinline__ void influence_rowmajor_body(
    const double *__restrict__ x, int64_t ldx_s, const double *__restrict__ u, const double *__restrict__ w, int64_t N,
    int64_t C, double cu, const double *__restrict__ cx, int lpr_log2, int grid_x, double *__restrict__ partial) {
  using LY = inf_layout<NQ>;
  constexpr int SH = LY::SH, PC = LY::PC, NS = LY::NS, NV = SH + VEC * PC, UNR = 4;
  const int LPR = 1 << lpr_log2, ROWS = INF_BLOCK >> lpr_log2;
  const int tid = threadIdx.x;
  const int lir = tid & (LPR - 1), rib = tid >> lpr_log2;
  const int64_t col0 = (int64_t)blockIdx.y * (LPR * VEC) + (int64_t)lir * VEC;
  const bool col_ok = col0 < C;  // VEC == 2 requires C even, so col0 + 1 < C too

  double px[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) px[v] = col_ok ? cx[col0 + v] : 0.0;
  double sh[SH], pc[VEC][PC];
#pragma unroll
  for (int q = 0; q < SH; ++q) sh[q] = 0.0;
#pragma unroll
  for (int v = 0; v < VEC; ++v)
#pragma unroll
    for (int q = 0; q < PC; ++q) pc[v][q] = 0.0;

  auto load = [&](int64_t r, double (&xv)[VEC]) {
    if constexpr (VEC == 2) {  // (read once: non-temporal, as the reduction does)
      const inf_v2d t = __builtin_nontemporal_load(reinterpret_cast<const inf_v2d *>(x + r * ldx_s + col0));
      xv[0] = t.x;
      xv[1] = t.y;
    } else {
      xv[0] = x[r * ldx_s + col0];
    }
  };

  if (col_ok) {
    const int64_t stride = (int64_t)grid_x * ROWS;
    int64_t i = (int64_t)blockIdx.x * ROWS + rib;
    for (; i + (UNR - 1) * stride < N; i += UNR * stride) {
      double xv[UNR][VEC], ui[UNR], wi[UNR];
#pragma unroll
      for (int q = 0; q < UNR; ++q) {
        const int64_t r = i + q * stride;
        load(r, xv[q]);
        ui[q] = u[r];
        wi[q] = WEIGHTED ? w[r] : 1.0;
      }
#pragma unroll
      for (int q = 0; q < UNR; ++q) inf_body<NQ, VEC, WEIGHTED>(ui[q], wi[q], xv[q], cu, px, sh, pc);
    }
    for (; i < N; i += stride) {
      double xv[VEC];
      load(i, xv);
      inf_body<NQ, VEC, WEIGHTED>(u[i], WEIGHTED ? w[i] : 1.0, xv, cu, px, sh, pc);
    }
  }

  // fixed-order sum over the ROWS row slots that share a lane_in_row, INF_CH of the lane's NV values per pass
  __shared__ double lds[INF_CH][INF_BLOCK];
  double *dst = partial + ((size_t)blockIdx.y * grid_x + blockIdx.x) * ((size_t)LPR * VEC) * NS;
#pragma unroll
  for (int c0 = 0; c0 < NV; c0 += INF_CH) {
#pragma unroll
    for (int k = 0; k < INF_CH; ++k) {
      const int q = c0 + k;  // compile-time: the sums stay in registers
      if (q < SH)
        lds[k][tid] = sh[q];
      else if (q < NV)
        lds[k][tid] = pc[(q - SH) / PC][(q - SH) % PC];
    }
    __syncthreads();
    for (int e = tid; e < LPR * INF_CH; e += INF_BLOCK) {
      const int k = e >> lpr_log2, l = e & (LPR - 1), q = c0 + k;
      if (q < NV) {
        double acc = 0.0;
        for (int r = 0; r < ROWS; ++r) acc += lds[k][r * LPR + l];
        if (q < SH) {  // T0 | M0: the same for every column of the row
#pragma unroll
          for (int v = 0; v < VEC; ++v) dst[((size_t)l * VEC + v) * NS + q] = acc;
        } else {
          const int v = (q - SH) / PC, j = (q - SH) % PC;
          dst[((size_t)l * VEC + v) * NS + SH + j] = acc;
        }
      }
    }
    __syncthreads();
  }
}

// One state of a batched call as the kernels read it (built on the host from txm_inf_state and the state's own plan).
struct inf_dev_state {
  const double *x, *u, *w;
  int64_t n;
  int64_t grid_x;
};

template <int NQ, int VEC, bool WEIGHTED>
__global__ __launch_bounds__(INF_BLOCK) void influence_rowmajor_kernel(
    const double *__restrict__ x, int64_t ldx_s, const double *__restrict__ u, const double *__restrict__ w, int64_t N,
    int64_t C, double cu, const double *__restrict__ cx, int lpr_log2, double *__restrict__ partial) {
  influence_rowmajor_body<NQ, VEC, WEIGHTED>(x, ldx_s, u, w, N, C, cu, cx, lpr_log2, (int)gridDim.x, partial);
}

// blockIdx.z = state; a workgroup beyond the state's own grid leaves at once.  partial: [state][per_state doubles]
template <int NQ, int VEC, bool WEIGHTED>
__global__ __launch_bounds__(INF_BLOCK) void influence_rowmajor_batch_kernel(
    const inf_dev_state *__restrict__ tab, int64_t ldx_s, int64_t C, const double *__restrict__ cu,
    const double *__restrict__ cx, int lpr_log2, double *__restrict__ partial, size_t per_state) {
  const inf_dev_state s = tab[blockIdx.z];
  if ((int64_t)blockIdx.x >= s.grid_x) return;
  influence_rowmajor_body<NQ, VEC, WEIGHTED>(s.x, ldx_s, s.u, s.w, s.n, C, cu[blockIdx.z], cx + (size_t)blockIdx.z * C,
                                             lpr_log2, (int)s.grid_x, partial + (size_t)blockIdx.z * per_state);
}

// sum of lds[k][0 .. 255] for k < INF_CH in a fixed order: thread (k = tid >> 5, j = tid & 31) adds its eight strided
// entries, then the 32 lanes fold downwards; valid in the threads with (tid & 31) == 0
__device__ __forceinline__ double inf_block_sum(const double (*lds)[INF_BLOCK], int tid) {
  const int k = tid >> 5, j = tid & 31;
  double acc = 0.0;
#pragma unroll
  for (int m = 0; m < INF_BLOCK / 32; ++m) acc += lds[k][j + 32 * m];
#pragma unroll
  for (int off = 16; off > 0; off >>= 1) acc += __shfl_down(acc, off, 32);
  return acc;
}

// one series xs[0 .. N) over grid_x workgroups (see influence_rowmajor_body); dst: this workgroup's record [NS]
template <int NQ, bool WEIGHTED>
__device__ __forceinline__ void influence_series_body(const double *__restrict__ xs, const double *__restrict__ u,
                                                      const double *__restrict__ w, int64_t N, double cu, double cxs,
                                                      int grid_x, double *__restrict__ dst) {
  using LY = inf_layout<NQ>;
  constexpr int SH = LY::SH, PC = LY::PC, NS = LY::NS;
  const int tid = threadIdx.x;
  const double px[1] = {cxs};
  double sh[SH], pc[1][PC];
#pragma unroll
  for (int q = 0; q < SH; ++q) sh[q] = 0.0;
#pragma unroll
  for (int q = 0; q < PC; ++q) pc[0][q] = 0.0;

  const int64_t nthreads = (int64_t)grid_x * INF_BLOCK;
  constexpr int UNR = 4;
  int64_t i = (int64_t)blockIdx.x * INF_BLOCK + tid;
  for (; i + (UNR - 1) * nthreads < N; i += UNR * nthreads) {
    double xv[UNR][1], ui[UNR], wi[UNR];
#pragma unroll
    for (int q = 0; q < UNR; ++q) {
      const int64_t r = i + q * nthreads;
      xv[q][0] = xs[r];
      ui[q] = u[r];
      wi[q] = WEIGHTED ? w[r] : 1.0;
    }
#pragma unroll
    for (int q = 0; q < UNR; ++q) inf_body<NQ, 1, WEIGHTED>(ui[q], wi[q], xv[q], cu, px, sh, pc);
  }
  for (; i < N; i += nthreads) {
    const double xv[1] = {xs[i]};
    inf_body<NQ, 1, WEIGHTED>(u[i], WEIGHTED ? w[i] : 1.0, xv, cu, px, sh, pc);
  }

  __shared__ double lds[INF_CH][INF_BLOCK];
#pragma unroll
  for (int c0 = 0; c0 < NS; c0 += INF_CH) {
#pragma unroll
    for (int k = 0; k < INF_CH; ++k) {
      const int q = c0 + k;
      if (q < SH)
        lds[k][tid] = sh[q];
      else if (q < NS)
        lds[k][tid] = pc[0][q - SH];
    }
    __syncthreads();
    const double tot = inf_block_sum(lds, tid);
    if ((tid & 31) == 0 && c0 + (tid >> 5) < NS) dst[c0 + (tid >> 5)] = tot;
    __syncthreads();
  }
}

// partial: [series][gridDim.x][NS]
template <int NQ, bool WEIGHTED>
__global__ __launch_bounds__(INF_BLOCK) void influence_colmajor_kernel(
    const double *__restrict__ x, int64_t ld_series, const double *__restrict__ u, const double *__restrict__ w, int64_t N,
    double cu, const double *__restrict__ cx, double *__restrict__ partial) {
  const int s = blockIdx.y;
  influence_series_body<NQ, WEIGHTED>(x + (int64_t)s * ld_series, u, w, N, cu, cx[s], (int)gridDim.x,
                                      partial + ((size_t)s * gridDim.x + blockIdx.x) * inf_layout<NQ>::NS);
}

// states of ONE contiguous series each (C == 1, pitch 1): blockIdx.y = state
template <int NQ, bool WEIGHTED>
__global__ __launch_bounds__(INF_BLOCK) void influence_series_batch_kernel(
    const inf_dev_state *__restrict__ tab, const double *__restrict__ cu, const double *__restrict__ cx,
    double *__restrict__ partial, size_t per_state) {
  const inf_dev_state s = tab[blockIdx.y];
  if ((int64_t)blockIdx.x >= s.grid_x) return;
  influence_series_body<NQ, WEIGHTED>(s.x, s.u, s.w, s.n, cu[blockIdx.y], cx[blockIdx.y], (int)s.grid_x,
                                      partial + (size_t)blockIdx.y * per_state + (size_t)blockIdx.x * inf_layout<NQ>::NS);
}

// block per column: sums[NS] = the column's records added over the nblk workgroups in a fixed order, then
// cov[c][i][j], mean[c][k] from the coefficients.  Total weight zero: zeros.
template <int NQ>
__device__ __forceinline__ void influence_finalize_body(const double *__restrict__ partial, int nblk, int cols_per_chunk,
                                                        int n_f, const double *__restrict__ a, const double *__restrict__ b,
                                                        double *__restrict__ cov, double *__restrict__ mean) {
  using LY = inf_layout<NQ>;
  constexpr int NT = LY::NT, NS = LY::NS;
  const int64_t c = blockIdx.x;
  const int tid = threadIdx.x;
  const int chunk = (int)(c / cols_per_chunk), cc = (int)(c % cols_per_chunk);
  double acc[NS];
#pragma unroll
  for (int q = 0; q < NS; ++q) acc[q] = 0.0;
  for (int blk = tid; blk < nblk; blk += INF_BLOCK) {
    const double *src = partial + (((size_t)chunk * nblk + blk) * cols_per_chunk + cc) * NS;
#pragma unroll
    for (int q = 0; q < NS; ++q) acc[q] += src[q];
  }
  __shared__ double lds[INF_CH][INF_BLOCK];
  __shared__ double sums[NS];
#pragma unroll
  for (int c0 = 0; c0 < NS; c0 += INF_CH) {
#pragma unroll
    for (int k = 0; k < INF_CH; ++k)
      if (c0 + k < NS) lds[k][tid] = acc[c0 + k];
    __syncthreads();
    const double tot = inf_block_sum(lds, tid);
    if ((tid & 31) == 0 && c0 + (tid >> 5) < NS) sums[c0 + (tid >> 5)] = tot;
    __syncthreads();
  }
  const double *T0 = sums, *M0 = sums + NT, *T1 = M0 + NQ, *T2 = T1 + NT, *M1 = T2 + NT;
  const double W = M0[0];
  const double *ac = a + (size_t)c * n_f * NQ, *bc = b + (size_t)c * n_f * NQ;
  for (int e = tid; e < n_f * n_f; e += INF_BLOCK) {
    // (i <= j: cov[i][j] and cov[j][i] are the same sum in the same order)
    const int i = min(e / n_f, e % n_f), j = max(e / n_f, e % n_f);
    double s = 0.0;
    for (int q = 0; q < NQ; ++q) {
      const double aiq = ac[i * NQ + q], biq = bc[i * NQ + q];
      for (int p = 0; p < NQ; ++p) {
        const double ajp = ac[j * NQ + p], bjp = bc[j * NQ + p];
        s += aiq * ajp * T0[q + p] + (aiq * bjp + biq * ajp) * T1[q + p] + biq * bjp * T2[q + p];
      }
    }
    cov[(size_t)c * n_f * n_f + e] = W == 0.0 ? 0.0 : s / (W * W);
  }
  for (int k = tid; k < n_f; k += INF_BLOCK) {
    double s = 0.0;
    for (int q = 0; q < NQ; ++q) s += ac[k * NQ + q] * M0[q] + bc[k * NQ + q] * M1[q];
    mean[(size_t)c * n_f + k] = W == 0.0 ? 0.0 : s / W;
  }
}

template <int NQ>
__global__ __launch_bounds__(INF_BLOCK) void influence_finalize_kernel(
    const double *__restrict__ partial, int nblk, int cols_per_chunk, int n_f, const double *__restrict__ a,
    const double *__restrict__ b, double *__restrict__ cov, double *__restrict__ mean) {
  influence_finalize_body<NQ>(partial, nblk, cols_per_chunk, n_f, a, b, cov, mean);
}

// blockIdx.y = state: its partials over its own grid_x workgroups, its slices of a, b, cov, mean
template <int NQ>
__global__ __launch_bounds__(INF_BLOCK) void influence_finalize_batch_kernel(
    const inf_dev_state *__restrict__ tab, const double *__restrict__ partial, size_t per_state, int cols_per_chunk,
    int64_t C, int n_f, const double *__restrict__ a, const double *__restrict__ b, double *__restrict__ cov,
    double *__restrict__ mean) {
  const size_t s = blockIdx.y, sc = s * (size_t)C;
  influence_finalize_body<NQ>(partial + s * per_state, (int)tab[s].grid_x, cols_per_chunk, n_f, a + sc * n_f * NQ,
                              b + sc * n_f * NQ, cov + sc * n_f * n_f, mean + sc * n_f);
}

// ---------------------------------------------------------------------------
// host side

struct InfPlan : InfLanes {
  bool rowmajor;
  int grid_x;
  int64_t ld_series;
};

// One workgroup's share is 4 row slots: 4 * (256 >> lpr_log2) rows (row-major), 4 * 256 samples (series layout); the grid
// grows by a workgroup per share up to 8 per CU and strides the rest.
static InfPlan influence_plan_vec(bool vec2, int64_t ldx_s, int64_t ldx_c, int64_t N, int64_t C) {
  InfPlan p{};
  const int64_t cap = (int64_t)num_cus() * 8;
  p.rowmajor = ldx_c == 1 && !(C == 1 && ldx_s == 1);
  if (p.rowmajor) {
    static_cast<InfLanes &>(p) = inf_lanes(vec2, C);
    int64_t gx = cdiv(N, (int64_t)(INF_BLOCK >> p.lpr_log2) * 4);
    p.grid_x = (int)(gx > cap ? cap : gx);
  } else {
    p.vec = 1;
    p.ld_series = (C == 1) ? 0 : ldx_c;
    p.cols_per_chunk = 1;
    p.chunks = (int)C;
    int64_t gx = cdiv(N, (int64_t)INF_BLOCK * 4);
    if (gx > cap) gx = cap;
    while (gx > 1 && gx * C > (int64_t)num_cus() * 16) gx = (gx + 1) / 2;  // many series fill the chip with fewer blocks each
    p.grid_x = (int)gx;
  }
  if (p.grid_x < 1) p.grid_x = 1;
  return p;
}

static InfPlan influence_plan(const double *x, int64_t ldx_s, int64_t ldx_c, int64_t N, int64_t C, int n_q) {
  return influence_plan_vec(inf_vec2_ok(x, ldx_s, C, n_q), ldx_s, ldx_c, N, C);
}

static size_t influence_ws_bytes_impl(int64_t C, int n_q) {
  const size_t NS = (size_t)(3 * (2 * n_q - 1) + 2 * n_q);
  // row-major: chunks * cols_per_chunk <= C rounded up to a power of two (to a multiple of 512 beyond 512), times the grid cap;
  // series layout: grid_x * C <= max(16 per CU, C)
  int64_t cols_pad = 1;
  while (cols_pad < C) cols_pad <<= 1;
  if (cols_pad > 512) cols_pad = cdiv(C, 512) * 512;
  const size_t rowm = (size_t)num_cus() * 8 * (size_t)cols_pad;
  const size_t colm = (size_t)num_cus() * 16 + (size_t)C;
  return (rowm > colm ? rowm : colm) * NS * sizeof(double) + 256;
}

template <int NQ>
static int influence_launch(const InfPlan &p, const double *x, int64_t ldx_s, const double *u, const double *w, int64_t N,
                            int64_t C, int n_f, double cu, const double *cx, const double *a, const double *b, double *cov,
                            double *mean, double *partial, hipStream_t st) {
  const dim3 block(INF_BLOCK);
  if (p.rowmajor) {
    const dim3 grid(p.grid_x, p.chunks);
#define TXM_INF_RM(VEC, WT)                                                                                              \
  hipLaunchKernelGGL((influence_rowmajor_kernel<NQ, VEC, WT>), grid, block, 0, st, x, ldx_s, u, w, N, C, cu, cx, p.lpr_log2, \
                     partial)
    if (p.vec == 2) {
      if constexpr (NQ <= INF_VEC2_MAXQ) {
        if (w) TXM_INF_RM(2, true); else TXM_INF_RM(2, false);
      } else {
        set_error("influence_cov: no two-column kernel for n_q=%d", NQ);
        return TXM_ERR_UNSUPPORTED;
      }
    } else {
      if (w) TXM_INF_RM(1, true); else TXM_INF_RM(1, false);
    }
#undef TXM_INF_RM
  } else {
    const dim3 grid(p.grid_x, (unsigned)C);
    if (w)
      hipLaunchKernelGGL((influence_colmajor_kernel<NQ, true>), grid, block, 0, st, x, p.ld_series, u, w, N, cu, cx, partial);
    else
      hipLaunchKernelGGL((influence_colmajor_kernel<NQ, false>), grid, block, 0, st, x, p.ld_series, u, w, N, cu, cx, partial);
  }
  TXM_LAUNCH_CHECK();
  hipLaunchKernelGGL((influence_finalize_kernel<NQ>), dim3((unsigned)C), block, 0, st, partial, p.grid_x, p.cols_per_chunk, n_f,
                     a, b, cov, mean);
  TXM_LAUNCH_CHECK();
  return TXM_OK;
}

// p: the plan of the batch's WIDEST state (its grid_x is the launch's); every state's own grid_x sits in tab
template <int NQ>
static int influence_launch_batched(const InfPlan &p, const inf_dev_state *tab, int64_t S, bool weighted, int64_t ldx_s,
                                    int64_t C, int n_f, const double *cu, const double *cx, const double *a, const double *b,
                                    double *cov, double *mean, double *partial, size_t per_state, hipStream_t st) {
  const dim3 block(INF_BLOCK);
  if (p.rowmajor) {
    const dim3 grid(p.grid_x, p.chunks, (unsigned)S);
#define TXM_INF_RMB(VEC, WT)                                                                                               \
  hipLaunchKernelGGL((influence_rowmajor_batch_kernel<NQ, VEC, WT>), grid, block, 0, st, tab, ldx_s, C, cu, cx, p.lpr_log2, \
                     partial, per_state)
    if (p.vec == 2) {
      if constexpr (NQ <= INF_VEC2_MAXQ) {
        if (weighted) TXM_INF_RMB(2, true); else TXM_INF_RMB(2, false);
      } else {
        set_error("influence_cov_batched: no two-column kernel for n_q=%d", NQ);
        return TXM_ERR_UNSUPPORTED;
      }
    } else {
      if (weighted) TXM_INF_RMB(1, true); else TXM_INF_RMB(1, false);
    }
#undef TXM_INF_RMB
  } else {
    const dim3 grid(p.grid_x, (unsigned)S);
    if (weighted)
      hipLaunchKernelGGL((influence_series_batch_kernel<NQ, true>), grid, block, 0, st, tab, cu, cx, partial, per_state);
    else
      hipLaunchKernelGGL((influence_series_batch_kernel<NQ, false>), grid, block, 0, st, tab, cu, cx, partial, per_state);
  }
  TXM_LAUNCH_CHECK();
  hipLaunchKernelGGL((influence_finalize_batch_kernel<NQ>), dim3((unsigned)C, (unsigned)S), block, 0, st, tab, partial,
                     per_state, p.cols_per_chunk, C, n_f, a, b, cov, mean);
  TXM_LAUNCH_CHECK();
  return TXM_OK;
}

// doubles of partials one state of at most n_max samples can need under either column width: the one-column plan has
// the smaller share (so the wider grid) and chunks * cols_per_chunk <= cols_pad for both (influence_ws_bytes_impl)
static size_t influence_batched_state_doubles(int64_t n_max, int64_t C, int n_q) {
  const size_t NS = (size_t)(3 * (2 * n_q - 1) + 2 * n_q);
  int64_t cols_pad = 1;
  while (cols_pad < C) cols_pad <<= 1;
  if (cols_pad > 512) cols_pad = cdiv(C, 512) * 512;
  const InfPlan p1 = influence_plan_vec(false, C, 1, n_max, C);
  return (size_t)p1.grid_x * (size_t)cols_pad * NS;
}

}  // namespace txm

using namespace txm;

extern "C" size_t txm_influence_cov_ws_bytes(int64_t N, int64_t C, int n_q) {
  if (N < 1 || C < 1 || C > 65535 || n_q < 1 || n_q > TXM_MAXK) return 0;
  return influence_ws_bytes_impl(C, n_q);
}

extern "C" int txm_influence_cov(const double *x, int64_t ldx_s, int64_t ldx_c, const double *u, const double *w, int64_t N,
                                 int64_t C, int n_f, int n_q, double center_u, const double *center_x, const double *a,
                                 const double *b, double *cov, double *mean, void *ws, size_t ws_bytes, txm_stream stream) {
  if (const int rc = inf_check_args("influence_cov", x && u && center_x && a && b && cov && mean && ws, N, C, 65535, "", n_f,
                                    n_q, ldx_c == 1 || ldx_s == 1, "need ldx_c == 1 or ldx_s == 1", center_u))
    return rc;
  const InfPlan p = influence_plan(x, ldx_s, ldx_c, N, C, n_q);
  if (p.rowmajor) TXM_REQUIRE(ldx_s >= C, "influence_cov: row pitch ldx_s < C");
  const size_t need = (size_t)p.chunks * p.grid_x * p.cols_per_chunk * (size_t)(3 * (2 * n_q - 1) + 2 * n_q) * sizeof(double);
  if (ws_bytes < txm_influence_cov_ws_bytes(N, C, n_q) || ws_bytes < need) {
    set_error("influence_cov: workspace too small");
    return TXM_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  double *partial = (double *)ws;
  return inf_dispatch(n_q, "influence_cov: n_q", [&](auto Q) {
    return influence_launch<decltype(Q)::value>(p, x, ldx_s, u, w, N, C, n_f, center_u, center_x, a, b, cov, mean, partial, st);
  });
}

extern "C" size_t txm_influence_cov_batched_ws_bytes(int64_t S, int64_t n_max, int64_t C, int n_q) {
  if (S < 1 || S > 65535 || n_max < 1 || C < 1 || C > 65535 || n_q < 1 || n_q > TXM_MAXK) return 0;
  return align_up((size_t)S * sizeof(inf_dev_state), 256) +
         (size_t)S * influence_batched_state_doubles(n_max, C, n_q) * sizeof(double) + 256;
}

extern "C" int txm_influence_cov_batched(const txm_inf_state *states_host, int64_t S, int64_t ldx_s, int64_t C, int n_f,
                                         int n_q, const double *center_u, const double *center_x, const double *a,
                                         const double *b, double *cov, double *mean, void *ws, size_t ws_bytes,
                                         txm_stream stream) {
  bool weighted, vec2 = true;
  int64_t n_max;
  if (const int rc = inf_check_batch("influence_cov_batched", states_host && center_u && center_x && a && b && cov && mean && ws,
                                     states_host, S, ldx_s, C, 65535, "", n_f, n_q, weighted, n_max))
    return rc;
  for (int64_t s = 0; s < S; ++s) vec2 = vec2 && inf_vec2_ok(states_host[s].x, ldx_s, C, n_q);
  // every state under the plan the single call makes for its own n (with the batch's column width); the launch takes
  // the widest state's grid
  static thread_local std::vector<inf_dev_state> tab_host;
  tab_host.resize((size_t)S);
  InfPlan pmax{};
  for (int64_t s = 0; s < S; ++s) {
    const txm_inf_state &h = states_host[s];
    const InfPlan p = influence_plan_vec(vec2, ldx_s, 1, h.n, C);
    tab_host[(size_t)s] = inf_dev_state{h.x, h.u, h.w, h.n, (int64_t)p.grid_x};
    if (s == 0 || p.grid_x > pmax.grid_x) pmax = p;
  }
  const size_t NS = (size_t)(3 * (2 * n_q - 1) + 2 * n_q);
  const size_t per_state = (size_t)pmax.chunks * pmax.grid_x * pmax.cols_per_chunk * NS;
  const size_t tab_bytes = align_up((size_t)S * sizeof(inf_dev_state), 256);
  if (ws_bytes < txm_influence_cov_batched_ws_bytes(S, n_max, C, n_q) || ws_bytes < tab_bytes + (size_t)S * per_state * sizeof(double)) {
    set_error("influence_cov_batched: workspace too small");
    return TXM_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  inf_dev_state *tab = (inf_dev_state *)ws;
  TXM_HIP(hipMemcpyAsync(tab, tab_host.data(), (size_t)S * sizeof(inf_dev_state), hipMemcpyHostToDevice, st));
  double *partial = (double *)((char *)ws + tab_bytes);
  return inf_dispatch(n_q, "influence_cov_batched: n_q", [&](auto Q) {
    return influence_launch_batched<decltype(Q)::value>(pmax, tab, S, weighted, ldx_s, C, n_f, center_u, center_x, a, b, cov, mean,
                                                        partial, per_state, st);
  });
}
