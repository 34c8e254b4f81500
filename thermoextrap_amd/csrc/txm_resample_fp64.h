// txm_resample_fp64.h -- internal interface of the FP64 bootstrap kernel and the finalize kernels
// (txm_resample_fp64.hip), called from txm_resample_vals and the batched entry points (txm_resample.hip).
#pragma once
#include "txm_resample_i8.h"

namespace txm {

constexpr int RS_BLOCK = 256;          // 4 waves
constexpr int RS_WAVES = RS_BLOCK / 64;
constexpr int RS_REPS = 16;            // replicates per wave (MFMA M)

// A field a call site does not set is null or zero: the host fills this in ONE place (fp64_args of txm_resample.hip).
struct ResampleArgs {
  const double *x = nullptr;
  int64_t ldx_s = 0;
  const double *u = nullptr;
  const double *w = nullptr;
  int64_t N = 0;
  int64_t C = 0;
  int64_t nrep = 0;
  const int64_t *freq = nullptr;      // parity mode
  const uint32_t *counts = nullptr;   // scale mode: [nrep][ntiles]
  uint32_t k0 = 0, k1 = 0;            // philox key
  uint32_t rep_base = 0;              // replicate r of the call draws stream replicate rep_base + r (txm_sampler_spec.rep0)
  int64_t ntiles = 0;
  uint32_t last_tile_size = 0;
  const double *pivot = nullptr;      // [1 + C]
  double *part_x = nullptr;           // [n_chunks][nrep_pad][C_pad][K]
  double *part_u = nullptr;           // [n_chunks][nrep_pad][K]
  int n_chunks = 0;                   // multiple of 8
  int n_rbg = 0;                      // replicate-block groups (4 blocks of 16 reps each)
  int64_t tiles_per_chunk = 0;
  int64_t nrep_pad = 0;               // n_rbg * 64
  int64_t C_pad = 0;                  // col groups * NBLK * 16
  // listed mode (precision-guard fallback of the int8 path): chunk c contracts the runs list[c], list[c + n_chunks], ...
  // of sub_tiles tiles each instead of its contiguous share; n_list[0] = number of runs (0: the launch is a no-op)
  const uint32_t *list = nullptr;
  const uint32_t *n_list = nullptr;
  int sub_tiles = 0;
  int64_t col_off = 0;                // x already points at the column group; its pivots start at pivot[1 + col_off]
  // batched mode (txm_resample_vals_batched): blockIdx.z = state s of S state points of one shape.  x/u/w come
  // from batch[s]; pivot, the partial sums, counts / freq rows and the sampler's replicate ids are those of the
  // single-state layout shifted by s (replicate s * nrep + r of one sampler over S * nrep replicates)
  const txm_state_ptrs *batch = nullptr;
  // listed mode of a BATCHED int8 call: the fallback runs of state blockIdx.z, operands from the int8 path's state table
  const I8State *i8states = nullptr;
  // L2-sharing hint (nullptr: off).  The waves that contract one sample chunk -- 4 per workgroup x the replicate
  // groups of the chunk, placed on one XCD by the block map -- read the same samples; left alone they drift apart
  // by many tiles and every one of them streams the chunk from HBM again (measured: 19x the algorithmic bytes).
  // Each wave publishes the number of tiles it has finished in progress[group][slot] and, before the next tile,
  // sleeps (bounded) while it is more than RS_LEAD tiles ahead of the slowest STARTED, UNFINISHED wave of its
  // group.  Purely a performance hint: every wait is bounded and no result depends on it.
  uint32_t *progress = nullptr;       // [groups = n_chunks * colgroups (* S)][64], zeroed by the launcher
};

struct ResamplePlan {
  int nblk, colgroups, n_rbg, n_chunks;
  int64_t tiles_per_chunk, nrep_pad, C_pad, ntiles;
  size_t off_pivot, off_px, off_pu, off_prog, prog_bytes, total;
};

// the bootstrap kernel of a plain (S == 1, a.batch == nullptr) or batched call and its finalize: states land in out
int run_resample(const ResampleArgs &a, const ResamplePlan &p, int K, bool weighted, bool explicit_, double *out,
                 hipStream_t st, int64_t S = 1);
// the bootstrap kernel alone, in listed mode (device sampler, N >= one tile), partial sums left for the caller's finalize;
// the plan is that of a full 32-column group
int run_listed(const ResampleArgs &a, const ResamplePlan &p0, int K, bool weighted, hipStream_t st, int64_t S = 1);
// finalize of one column group of the int8 path (b.states: the S = b.S states of a batched call on grid axis y): the
// per-window slots of b, then the listed-mode sums of f; `summed` as in resample_finalize_i8_kernel
int launch_finalize_i8(const I8Args &b, const ResampleArgs &f, int K, int summed, double *out, int64_t C_total,
                       hipStream_t st);
// ... and of the second sample matrix the group's last pass carried: fy = the listed-mode launch on y, fb_u = x's u-row sums
int launch_finalize_y(const I8Args &b, const ResampleArgs &fy, const double *fb_u, int K, double *out_y, int64_t C_total,
                      hipStream_t st);

}  // namespace txm
