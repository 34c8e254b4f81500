// txm_resample.hip -- sample-level bootstrap of central comoments
// (cmomy.wrap_resample_vals as called from thermoextrap data.py:1803-1810,
// 1354-1366).
//
// out[r] = comoment state of the data with weights w_i * f[r][i].  With the
// pivot-shifted monomials m[i][c][j] = (x_ic - px_c) (u_i - pu)^j this is a
// dense contraction over samples
//        S1[r][c][j] = sum_i f[r][i] * w_i * du_i^j * dx_ic
//        S0[r][j]    = sum_i f[r][i] * w_i * du_i^j
// i.e. ~2*K*(C+1) flop per (replicate, sample) against 8*(C+1) bytes per
// sample read once: FP64-bound for nrep >~ 12, so it runs on the FP64 matrix
// pipe.  Per wave and per 4 samples:
//        A_j (16 reps x 4 samples)  = f * w * du^j      one f64 per lane
//        B   (4 samples x 16 cols)  = dx                one f64 per lane
//        D_j (16 reps x 16 cols)   += A_j * B           v_mfma_f64_16x16x4_f64
// so the power index j rides on the A operand (one multiply per j) and B is
// loaded once per column block; S0 is the row-sum of A_j, kept on the VALU.
// The MFMA broadcasts f over columns and dx over replicates for free, and the
// VALU (Philox draws, LDS histogram, u-row sums) co-executes with the matrix
// pipe of the other resident wave.
//
// f comes either from the Philox stage-3 stream (scale mode; the wave fills a
// private [1024 samples][16 reps] u8 tile in LDS, never touching HBM) or from an
// explicit int64 freq table (parity mode).
//
// This file: the kernel, the three finalize kernels and the launchers that instantiate them (txm_resample_fp64.h).  The
// plans, the path rules and the entry points that drive them are txm_resample.hip.
#include <type_traits>

#include "txm_influence_common.h"  // inf_dispatch: the host's switch over a template order
#include "txm_sampler.h"
#include "txm_resample_fp64.h"

namespace txm {

typedef double v4f64 __attribute__((ext_vector_type(4)));

// (RS_BLOCK, RS_WAVES, RS_REPS: txm_resample_fp64.h -- the plan pads replicates to them)
// f tile of one wave: u8 counts, layout [sample slot 0..1023][rep 0..15] (16 KiB).
// A draw of slot `off` for replicate rr is one ds_add_u32 of (1 << 8*(rr&3)) at byte
// off*16 + (rr & ~3): one shift-add of VALU work per draw.  The contraction reads
// one byte per step (ds_read_u8, immediate offset): no VALU unpacking.
// On gfx950 the FP64 MFMA shares the VALU datapath (tools/mfma_f64_peak4.hip:
// every VALU instruction costs 4.5-8 cycles of matrix-pipe time), so the design
// rule of this kernel is: as few VALU instructions per MFMA as possible.
constexpr int RS_QUARTER = SM_T / 4;                  // 256 samples per lane-group per tile
constexpr int RS_TILE_BYTES = SM_T * RS_REPS;         // 16384 bytes per wave
// steps per register-prefetch group: as many as the VGPR budget (2 waves/SIMD,
// 256 VGPRs) allows next to the K*NBLK accumulator tiles.
constexpr int RS_EXP_BUDGET = 160;
constexpr int rs_group(int K, int NBLK, bool weighted, bool explicit_, int pack = 1) {
  const int per_step = 2 + 2 * NBLK + (weighted ? 2 : 0) + (explicit_ ? 10 : 0);
  for (int g = 8; g > 2; g >>= 1)
    if ((K + pack - 1) / pack * NBLK * 8 + 2 * g * per_step <= RS_EXP_BUDGET) return g;
  return 2;
}

// (ResampleArgs: txm_resample_fp64.h)
constexpr uint32_t RS_LEAD = 1;          // tiles a wave may run ahead of its group
constexpr int RS_THROTTLE_SPINS = 48;    // x ~0.3 us: bound of one wait

// One wave: 16 replicates x (NBLK*16 columns) x one chunk of tiles.
//
// MFMA operand roles for step s of a tile (lane = (row = lane & 15, kk = lane >> 4)):
//   sample    i  = tile_base + kk * 256 + s          (each kk owns a contiguous quarter)
//   A (rep = row, k = kk)   = f[rep][i] * w_i * du_i^j
//   B (k = kk,  col = row)  = x[i][col] - px[col]
// A lane therefore walks CONTIGUOUS samples: u/w/freq come as 16-byte loads of
// 8 consecutive steps, f as one 8-byte LDS read per 8 steps, and the loads of
// group g+1 are issued before the 8*K*NBLK MFMAs of group g (register double
// buffer), so HBM/L2 latency hides under the matrix pipe.
// Stage 3 of the sampler for a FULL tile and the 16 replicates of one wave, with the
// minimum of VALU work (the stream itself is the one oracle/philox_oracle.c defines:
// draw d of (r, t) = 10-bit field d % 12 of Philox call d / 12 -- which lane runs a
// call is free).  Replicates are taken in pairs: calls 0..63 of each go to one wave
// iteration each, and their remaining calls 64..95 (n - 768 draws, ~1/3 of a wave)
// share a third iteration, 32 lanes per replicate.  Fields past the replicate's
// draw count add 0 instead of being branched around.
template <bool ALL_VALID>
__device__ __forceinline__ void tile_calls(uint32_t *tw, uint32_t k0, uint32_t k1, uint32_t r, uint32_t t,
                                           uint32_t c, uint32_t n, uint32_t inc, uint32_t wsel) {
  const uint32_t first = c * 12u;
  if (!ALL_VALID && first >= n) return;  // ALL_VALID: 12 (c + 1) <= n by construction, no branch
  // call index in the second counter word: the tile's and the replicate's share of rounds 1-3 is wave-uniform
  const Philox4 o = philox4x32_10(t, c, r, 3u, k0, k1);
  const uint32_t nd = n - first;
#pragma unroll
  for (int wi = 0; wi < 4; ++wi) {
    const uint32_t word = o.w[wi];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const uint32_t f = (word >> (10 * k)) & 1023u;
      const uint32_t add = ALL_VALID ? inc : (((uint32_t)(wi * 3 + k) < nd) ? inc : 0u);
      atomicAdd(&tw[f * (RS_REPS / 4) + wsel], add);
    }
  }
}

__device__ __forceinline__ void fill_tile_full(const ResampleArgs &a, const uint32_t *counts, uint32_t rid0,
                                               uint32_t *tw, int64_t rep0, int64_t t, int lane) {
#pragma unroll 1
  for (int p = 0; p < RS_REPS / 2; ++p) {
    const int64_t ra = rep0 + 2 * p, rb = ra + 1;
    if (ra >= a.nrep) break;  // wave-uniform
    const uint32_t na = counts[(size_t)ra * a.ntiles + t];
    const uint32_t nb = rb < a.nrep ? counts[(size_t)rb * a.ntiles + t] : 0u;
    const uint32_t wsel = (uint32_t)p >> 1;                  // (2p) >> 2 == (2p+1) >> 2
    const uint32_t inc_a = 1u << (8u * ((2u * p) & 3u)), inc_b = inc_a << 8;
    // iterations 1 and 2: calls 0..63 of each replicate; when n >= 768 (wave-uniform,
    // practically always) every field is a real draw and no select is needed
    if (na >= 768u) tile_calls<true>(tw, a.k0, a.k1, rid0 + (uint32_t)ra, (uint32_t)t, (uint32_t)lane, na, inc_a, wsel);
    else tile_calls<false>(tw, a.k0, a.k1, rid0 + (uint32_t)ra, (uint32_t)t, (uint32_t)lane, na, inc_a, wsel);
    if (nb >= 768u) tile_calls<true>(tw, a.k0, a.k1, rid0 + (uint32_t)rb, (uint32_t)t, (uint32_t)lane, nb, inc_b, wsel);
    else tile_calls<false>(tw, a.k0, a.k1, rid0 + (uint32_t)rb, (uint32_t)t, (uint32_t)lane, nb, inc_b, wsel);
    // iteration 3: calls 64..95 of both, 32 lanes each
    const bool hb = lane >= 32;
    tile_calls<false>(tw, a.k0, a.k1, rid0 + (uint32_t)(hb ? rb : ra), (uint32_t)t, 64u + ((uint32_t)lane & 31u),
                      hb ? nb : na, hb ? inc_b : inc_a, wsel);
    // calls >= 96 (n > 1152, a > 4 sigma event): plain loop
    const uint32_t nmax = na > nb ? na : nb;
    for (uint32_t c0 = 96u; c0 * 12u < nmax; c0 += 64u) {
      tile_calls<false>(tw, a.k0, a.k1, rid0 + (uint32_t)ra, (uint32_t)t, c0 + (uint32_t)lane, na, inc_a, wsel);
      tile_calls<false>(tw, a.k0, a.k1, rid0 + (uint32_t)rb, (uint32_t)t, c0 + (uint32_t)lane, nb, inc_b, wsel);
    }
  }
}

//
// Tiles are always contracted over a full 1024-sample window.  The last
// (partial) tile slides its window back to [N - 1024, N) and gives the samples
// that belong to the previous tile a zero count, so the hot loop has no
// bounds handling at all.  Only data sets shorter than one tile (SMALLN) use
// clamped addresses, in a separate instantiation.
// MODE: RS_PLAIN = one state point, contiguous chunk of tiles; RS_LISTED = the runs of the fallback list;
// RS_BATCHED = state blockIdx.z of a batch.  Compile-time so that the plain kernel carries none of the other modes'
// loop state (scalar registers are what this kernel runs out of first: spilled SGPRs cost vector instructions,
// and every vector instruction here costs FP64-MFMA time).
constexpr int RS_PLAIN = 0, RS_LISTED = 1, RS_BATCHED = 2;
//
// PACK (1, 2 or 4; NBLK == 1): with C <= 16 / PACK value columns the 16 B-operand columns carry PACK powers of du
// per column, B[k][jp * CPK + c] = dx_c * du^jp, and the A operands step by du^PACK: ceil(K / PACK) MFMAs per
// k-step instead of K, so a narrow state does not pay for 16 columns it does not have.
template <int K, int NBLK, bool WEIGHTED, bool EXPLICIT, bool SMALLN, int MODE = RS_PLAIN, int PACK = 1>
__global__ __launch_bounds__(RS_BLOCK, 2) void resample_kernel(const ResampleArgs a) {
  static_assert(PACK == 1 || (NBLK == 1 && (PACK == 2 || PACK == 4)), "power packing needs a single column block");
  constexpr int CPK = 16 / PACK;            // value columns per power slot
  constexpr int KJ = (K + PACK - 1) / PACK;  // accumulator tiles (MFMAs per k-step and column block)
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  // readfirstlane: tell the compiler the wave index is wave-uniform, so everything
  // derived from it (replicate base, LDS tile base, loop bounds) lives in SGPRs
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int row = lane & 15;   // A: replicate within block;  B: column within block
  const int kk = lane >> 4;    // which quarter of the tile this lane group walks
  const int crow = PACK == 1 ? row : row % CPK;  // B: value column within the block
  const int jp = PACK == 1 ? 0 : row / CPK;      // B: power of du folded into this lane's column

  // XCD-aware task map: workgroups that share a sample chunk sit on one XCD
  // (blocks b and b+8 share an XCD) and are dispatched back to back, so the
  // chunk is streamed from HBM once and re-read from that XCD's L2.
  const int b = blockIdx.x;
  const int xcd = b & 7, q = b >> 3;
  const int chunk = (q / a.n_rbg) * 8 + xcd;
  const int rbg = q % a.n_rbg;
  const int colgrp = blockIdx.y;
  const int64_t rep0 = ((int64_t)rbg * RS_WAVES + wave) * RS_REPS;
  const int64_t col0 = (int64_t)colgrp * (NBLK * 16);

  const int64_t t_begin = (int64_t)chunk * a.tiles_per_chunk;
  int64_t t_end = t_begin + a.tiles_per_chunk;
  if (t_end > a.ntiles) t_end = a.ntiles;
  // operands of this launch's state (batched mode: state blockIdx.z)
  const double *X = a.x, *U = a.u, *W = a.w, *PIV = a.pivot;
  const uint32_t *CNT = a.counts;
  const int64_t *FREQ = a.freq;
  double *PX = a.part_x, *PU = a.part_u;
  uint32_t rid0 = a.rep_base;
  if constexpr (MODE == RS_BATCHED) {
    const int64_t sidx = blockIdx.z;
    const txm_state_ptrs bs = a.batch[sidx];
    X = bs.x;
    U = bs.u;
    W = bs.w;
    PIV += sidx * (1 + a.C);
    if (CNT) CNT += (size_t)sidx * a.nrep * a.ntiles;
    if (FREQ) FREQ += (size_t)sidx * a.nrep * a.N;
    PX += (size_t)sidx * a.n_chunks * a.nrep_pad * a.C_pad * K;
    PU += (size_t)sidx * a.n_chunks * a.nrep_pad * K;
    rid0 += (uint32_t)(sidx * a.nrep);
  }
  constexpr bool listed = MODE == RS_LISTED;
  int64_t nruns = 1;
  const uint32_t *LIST = a.list, *NLIST = a.n_list;
  if constexpr (listed) {
    if (a.i8states != nullptr) {  // batched int8 call: state blockIdx.z
      const I8State e = a.i8states[blockIdx.z];
      X = e.x + a.col_off;  // (a.x of a listed launch is x + the column group's offset)
      U = e.u;
      W = e.w;
      PIV = e.pivot;
      CNT = e.counts;
      PX = e.fb_x;
      PU = e.fb_u;
      rid0 = e.rep_base;
      LIST = e.list;
      NLIST = e.n_list;
    }
    nruns = (int64_t)*NLIST;
    if (nruns == 0) return;  // nothing flagged: the finalize kernel does not read this launch's partial sums
  }

  const double pu = PIV[0];
  // Columns beyond C (padding of the last 16-column block) re-read column 0:
  // their sums are finite garbage that the finalize kernel never looks at, which
  // is cheaper than a mask multiply on the FP64 pipe the MFMAs need.
  double px[NBLK];
  int64_t ccol[NBLK];
#pragma unroll
  for (int bl = 0; bl < NBLK; ++bl) {
    const int64_t c = col0 + bl * 16 + crow;
    ccol[bl] = c < a.C ? c : 0;
    px[bl] = PIV[1 + a.col_off + ccol[bl]];
  }

  v4f64 acc[KJ][NBLK];
  double usum[K];
#pragma unroll
  for (int j = 0; j < K; ++j) usum[j] = 0.0;
#pragma unroll
  for (int j = 0; j < KJ; ++j)
#pragma unroll
    for (int bl = 0; bl < NBLK; ++bl) acc[j][bl] = (v4f64){0.0, 0.0, 0.0, 0.0};

  unsigned char *tile = lds_raw + (size_t)wave * RS_TILE_BYTES;
  const int64_t my_rep = rep0 + row;
  const bool rep_ok = my_rep < a.nrep;
  const int64_t last = a.N - 1;

  // register double buffer for one group of RS_GROUP steps
  constexpr int RS_GROUP = SMALLN ? 2 : rs_group(K, NBLK, WEIGHTED, EXPLICIT, PACK);
  struct Grp {
    double u[RS_GROUP];
    double w[RS_GROUP];
    double x[RS_GROUP][NBLK];
    uint32_t fb[RS_GROUP];    // scale mode: u8 counts straight from LDS, one per step
    int64_t fi[EXPLICIT ? RS_GROUP : 1];  // parity mode: raw int64 counts
  };

  uint32_t *pg = nullptr;
  uint32_t tiles_done = 0;
  const int pslot = (rbg * RS_WAVES + wave) & 63;
  if constexpr (MODE == RS_PLAIN && !SMALLN)
    if (a.progress != nullptr) pg = a.progress + ((size_t)(colgrp * a.n_chunks + chunk)) * 64;
  double cnt = 0.0;  // lanes kk == 0, unweighted: the replicate's draws in the contracted tiles (exact integers)
  for (int64_t run = listed ? chunk : 0; run < nruns; run += listed ? a.n_chunks : 1) {
  int64_t tb = t_begin, te = t_end;
  if constexpr (listed) {
    tb = (int64_t)LIST[run];
    te = tb + a.sub_tiles;
    if (te > a.ntiles) te = a.ntiles;
  }
  for (int64_t t = tb; t < te; ++t) {
    const int64_t i_tile = t * SM_T;
    if constexpr (!WEIGHTED && !EXPLICIT)
      if (kk == 0 && rep_ok) cnt += (double)CNT[(size_t)my_rep * a.ntiles + t];
    const uint32_t tsize = (t == a.ntiles - 1) ? a.last_tile_size : (uint32_t)SM_T;
    // window of 1024 samples that is contracted for this tile
    int64_t wbase = i_tile;
    if constexpr (!SMALLN)
      if (wbase > a.N - SM_T) wbase = a.N - SM_T;
    const uint32_t shift = (uint32_t)(i_tile - wbase);  // window slots owned by the previous tile

    if constexpr (!EXPLICIT) {
      // ---- stage 3 of the sampler: fill this wave's private f tile ---------
      // (wave-private LDS: DS ops of one wave execute in order, so only the
      // compiler needs fencing -- no s_barrier, waves of a workgroup drift
      // apart and their VALU/LDS phases overlap other waves' MFMA phases)
      uint4 *z = reinterpret_cast<uint4 *>(tile);
#pragma unroll
      for (int e = 0; e < RS_TILE_BYTES / 16 / 64; ++e) z[e * 64 + lane] = make_uint4(0, 0, 0, 0);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __builtin_amdgcn_wave_barrier();
      uint32_t *tw = reinterpret_cast<uint32_t *>(tile);
      if (tsize == (uint32_t)SM_T) {
        fill_tile_full(a, CNT, rid0, tw, rep0, t, lane);
      } else {
        for (int rr = 0; rr < RS_REPS; ++rr) {
          const int64_t r = rep0 + rr;
          if (r >= a.nrep) break;  // wave-uniform
          const uint32_t n = CNT[(size_t)r * a.ntiles + t];
          sampler_fine_tile(a.k0, a.k1, rid0 + (uint32_t)r, (uint32_t)t, n, tsize, lane, [&](uint32_t off0) {
            const uint32_t off = off0 + shift;
            atomicAdd(&tw[off * (RS_REPS / 4) + ((uint32_t)rr >> 2)], 1u << (8u * ((uint32_t)rr & 3u)));
          });
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
      __builtin_amdgcn_wave_barrier();
    }

    const unsigned char *frow = tile + (kk * RS_QUARTER) * RS_REPS + row;  // + s * 16 per step
    const int64_t ibase = wbase + (int64_t)kk * RS_QUARTER;
    const uint32_t lbase = (uint32_t)kk * RS_QUARTER;  // window slot of this lane's step 0
    // unsigned 32-bit BYTE offsets: base (SGPR pair) + zext(VGPR) is the saddr form of global_load
    const uint32_t lane_uoff = (uint32_t)(kk * RS_QUARTER) * 8u;
    uint32_t lane_xoff[NBLK];
#pragma unroll
    for (int bl = 0; bl < NBLK; ++bl) lane_xoff[bl] = (uint32_t)((kk * RS_QUARTER * a.ldx_s + ccol[bl]) * 8);
    auto ld = [](const void *base, uint32_t byteoff) {
      return *reinterpret_cast<const double *>(reinterpret_cast<const char *>(base) + byteoff);
    };

    // One-step operand lookahead: the A operands (f * w * du^j) and B operands
    // (x - px) of step e+1 are computed into a second register set BEFORE the
    // K*NBLK MFMAs of step e are issued, so the MFMAs of a step go out back to back
    // and no VALU write targets a register an in-flight MFMA still reads.
    struct Ops {
      double a[KJ];
      double b[NBLK];
    };
    auto prep_step = [&](const Grp &G, int e, Ops &o) {
      double av;
      if constexpr (EXPLICIT) av = (double)G.fi[e];
      else av = (double)G.fb[e];
      if constexpr (WEIGHTED) av *= G.w[e];
      const double du = G.u[e] - pu;
#pragma unroll
      for (int bl = 0; bl < NBLK; ++bl) o.b[bl] = G.x[e][bl] - px[bl];
      if constexpr (PACK > 1) {
        double f = (jp & 1) ? du : 1.0;
        if constexpr (PACK == 4) f *= (jp & 2) ? du * du : 1.0;
        o.b[0] *= f;
      }
#pragma unroll
      for (int j = 0; j < K; ++j) {
        if (j % PACK == 0) o.a[j / PACK] = av;
        // S0[0] = sum of counts: accumulated only when weights make it non-trivial
        // (unweighted it is the replicate's draw count, summed from `counts` below)
        if (j > 0 || WEIGHTED || EXPLICIT) usum[j] += av;
        av *= du;
      }
    };
    auto mfma_step = [&](const Ops &o) {
#pragma unroll
      for (int j = 0; j < KJ; ++j)
#pragma unroll
        for (int bl = 0; bl < NBLK; ++bl)
          acc[j][bl] = __builtin_amdgcn_mfma_f64_16x16x4f64(o.a[j], o.b[bl], acc[j][bl], 0, 0, 0);
    };
    auto compute_group = [&](const Grp &G) {
      Ops P, Q;
      prep_step(G, 0, P);
#pragma unroll
      for (int e = 0; e < RS_GROUP; e += 2) {
        if (e + 1 < RS_GROUP) prep_step(G, e + 1, Q);
        __builtin_amdgcn_sched_barrier(0);
        mfma_step(P);
        __builtin_amdgcn_sched_barrier(0);
        if (e + 1 < RS_GROUP) {
          if (e + 2 < RS_GROUP) prep_step(G, e + 2, P);
          __builtin_amdgcn_sched_barrier(0);
          mfma_step(Q);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    };

    // Branch-free on purpose: a conditional around the prefetch loads makes the
    // compiler's s_waitcnt insertion fall back to vmcnt(0) at the join, which
    // serialises loads and MFMAs.
    auto load_group = [&](int g, Grp &G) {
      const int s0 = g * RS_GROUP;
      if constexpr (!SMALLN) {
        // wave-uniform row base (SGPRs, scalar ALU) + a loop-invariant 32-bit lane
        // offset: the loads need no per-step vector address arithmetic
        const double *ur = U + (wbase + s0);
#pragma unroll
        for (int e = 0; e < RS_GROUP; ++e) G.u[e] = ld(ur + e, lane_uoff);
        if constexpr (WEIGHTED) {
          const double *wr = W + (wbase + s0);
#pragma unroll
          for (int e = 0; e < RS_GROUP; ++e) G.w[e] = ld(wr + e, lane_uoff);
        }
#pragma unroll
        for (int e = 0; e < RS_GROUP; ++e) {
          const double *xr = X + (wbase + s0 + e) * a.ldx_s;
#pragma unroll
          for (int bl = 0; bl < NBLK; ++bl) G.x[e][bl] = ld(xr, lane_xoff[bl]);
        }
        if constexpr (EXPLICIT) {
          const int64_t *fp = FREQ + (size_t)(rep_ok ? my_rep : 0) * a.N + ibase + s0;
#pragma unroll
          for (int e = 0; e < RS_GROUP; ++e)
            G.fi[e] = (rep_ok && lbase + (uint32_t)(s0 + e) >= shift) ? fp[e] : 0;
        }
      } else {
        // N < 1024: a single short tile; clamp addresses, zero the missing samples
#pragma unroll
        for (int e = 0; e < RS_GROUP; ++e) {
          const int64_t ii = ibase + s0 + e;
          const int64_t ic = ii <= last ? ii : last;
          G.u[e] = U[ic];
          if constexpr (WEIGHTED) G.w[e] = W[ic];
#pragma unroll
          for (int bl = 0; bl < NBLK; ++bl) G.x[e][bl] = X[ic * a.ldx_s + ccol[bl]];
          if constexpr (EXPLICIT)
            G.fi[e] = (rep_ok && ii <= last) ? FREQ[(size_t)(rep_ok ? my_rep : 0) * a.N + ic] : 0;
        }
      }
      if constexpr (!EXPLICIT) {
#pragma unroll
        for (int e = 0; e < RS_GROUP; ++e) G.fb[e] = frow[(s0 + e) * RS_REPS];
      }
    };
    // groups per lane quarter (even); SMALLN: only those that hold samples
    int ngroups = RS_QUARTER / RS_GROUP;
    if constexpr (SMALLN) {
      const uint32_t q0 = tsize < (uint32_t)RS_QUARTER ? tsize : (uint32_t)RS_QUARTER;
      ngroups = (int)((q0 + RS_GROUP - 1) / RS_GROUP);
      ngroups = (ngroups + 1) & ~1;
    }
    {
      Grp A, B;
      load_group(0, A);
      // sched_barrier: keep "issue the next group's loads, then run this group's
      // MFMAs" in program order (the machine scheduler otherwise sinks the loads
      // next to their uses to save registers and exposes their latency).
      for (int g = 0; g < ngroups; g += 2) {
        load_group(g + 1, B);  // g + 1 < ngroups (even count)
        __builtin_amdgcn_sched_barrier(0);
        compute_group(A);
        __builtin_amdgcn_sched_barrier(0);
        const int g2 = (g + 2 < ngroups) ? g + 2 : g + 1;  // tail: harmless re-load
        load_group(g2, A);
        __builtin_amdgcn_sched_barrier(0);
        compute_group(B);
        __builtin_amdgcn_sched_barrier(0);
      }
    }

    if constexpr (!EXPLICIT) {
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
      __builtin_amdgcn_wave_barrier();
    }
    if (pg != nullptr) {  // kernel argument: uniform
      ++tiles_done;
      if (lane == 0) __hip_atomic_store(&pg[pslot], tiles_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll 1
      for (int spin = 0; spin < RS_THROTTLE_SPINS; ++spin) {
        uint32_t v = __hip_atomic_load(&pg[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (v == 0u) v = 0xffffffffu;  // slot unused or its wave not started yet: not a wave to wait for
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const uint32_t w2 = (uint32_t)__shfl_xor((int)v, o);
          v = w2 < v ? w2 : v;
        }
        if (tiles_done <= v + RS_LEAD) break;
        __builtin_amdgcn_s_sleep(32);
      }
    }
  }
  }
  if (pg != nullptr && lane == 0)  // finished: never hold the others back
    __hip_atomic_store(&pg[pslot], 0xfffffff0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);

  // ---- write partial sums ---------------------------------------------------
  // D layout of v_mfma_f64_16x16x4_f64: col = lane & 15, row = (lane >> 4) + 4 * reg
  double *px_out = PX + ((size_t)chunk * a.nrep_pad + rep0) * a.C_pad * K;
#pragma unroll
  for (int jj = 0; jj < KJ; ++jj)
#pragma unroll
    for (int bl = 0; bl < NBLK; ++bl)
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        const int rrow = kk + 4 * rg;
        const int64_t c = col0 + bl * 16 + crow;
        const int j = jj * PACK + jp;
        if (PACK == 1 || j < K) px_out[((size_t)rrow * a.C_pad + c) * K + j] = acc[jj][bl][rg];
      }
  if (colgrp == 0) {
    if constexpr (!WEIGHTED && !EXPLICIT) usum[0] = cnt;  // other lane groups contribute 0
#pragma unroll
    for (int j = 0; j < K; ++j) {
      double v = usum[j];
      v += __shfl_xor(v, 16);
      v += __shfl_xor(v, 32);
      if (kk == 0) PU[((size_t)chunk * a.nrep_pad + rep0 + row) * K + j] = v;
    }
  }
}

// finalize: thread per (rep, col): fixed-order sum over chunks, shift to the
// cmomy state, out[rep][c][2][K].
template <int K>
__global__ __launch_bounds__(256) void resample_finalize_kernel(
    const double *__restrict__ part_x, const double *__restrict__ part_u, int n_chunks,
    int64_t nrep_pad, int64_t C_pad, int64_t nrep, int64_t C, const double *__restrict__ pivot,
    double *__restrict__ out, int64_t c_off = 0, int64_t C_total = 0) {
  // C columns of this launch are the columns c_off .. c_off + C - 1 of the C_total output columns.
  // Thread = (output e of the block's 32, chunk segment seg of 8): segment seg adds the chunks seg, seg + 8, ... in
  // ascending order, then the eight segments are added in order -- a fixed tree (one thread per output walking all
  // chunks was a chain of dependent-latency loads: 0.3 ms for 400 outputs x 1024 chunks).
  constexpr int NSEG = 8, NOUT = 256 / NSEG;
  __shared__ double sh[NSEG][NOUT][2 * K];
  const int eo = threadIdx.x % NOUT, seg = threadIdx.x / NOUT;
  const int64_t e = (int64_t)blockIdx.x * NOUT + eo;
  const bool live = e < nrep * C;
  const int64_t r = live ? e / C : 0, c = live ? e % C : 0;
  if (C_total == 0) C_total = C;
  // batched mode: blockIdx.y = state; every per-state array follows the previous state's
  const int64_t sidx = blockIdx.y;
  part_x += (size_t)sidx * n_chunks * nrep_pad * C_pad * K;
  part_u += (size_t)sidx * n_chunks * nrep_pad * K;
  pivot += sidx * (1 + C);
  out += (size_t)sidx * nrep * C_total * 2 * K;
  double S0[K], S1[K];
#pragma unroll
  for (int j = 0; j < K; ++j) S0[j] = S1[j] = 0.0;
  if (live)
    for (int ch = seg; ch < n_chunks; ch += NSEG) {
      const double *pu_ = part_u + ((size_t)ch * nrep_pad + r) * K;
      const double *px_ = part_x + (((size_t)ch * nrep_pad + r) * C_pad + c) * K;
#pragma unroll
      for (int j = 0; j < K; ++j) {
        S0[j] += pu_[j];
        S1[j] += px_[j];
      }
    }
#pragma unroll
  for (int j = 0; j < K; ++j) {
    sh[seg][eo][j] = S0[j];
    sh[seg][eo][K + j] = S1[j];
  }
  __syncthreads();
  if (seg != 0 || !live) return;
  for (int g = 1; g < NSEG; ++g)
#pragma unroll
    for (int j = 0; j < K; ++j) {
      S0[j] += sh[g][eo][j];
      S1[j] += sh[g][eo][K + j];
    }
  double st[2 * K];
  pivot_sums_to_state_or_empty<K>(S0, S1, pivot[0], pivot[1 + c_off + c], st);  // weight sum exactly 0: the empty state
  double *o = out + (r * C_total + c_off + c) * 2 * K;
#pragma unroll
  for (int q = 0; q < 2 * K; ++q) o[q] = st[q];
}

// finalize of the int8 path: one slot of partial sums per scaling window, [window][replicate][power][8 digit slots]
// [column] (u-row: [window][replicate][power][8]); windows in ascending order, digits in ascending order -- a fixed order
// that does not depend on the launch geometry.  Windows the precision guard flagged hold nothing: they were contracted
// by the FP64 kernel, whose sums are added behind (same pivot).
template <int K, int CPAD>
__global__ __launch_bounds__(256) void resample_finalize_i8_kernel(
    const double *__restrict__ part_x, const double *__restrict__ part_u, int64_t nwin,
    const uint32_t *__restrict__ wflag, int64_t nrep_pad, int64_t nrep, int64_t C,
    const double *__restrict__ pivot, double *__restrict__ out, int64_t c_off, int64_t C_total,
    const double *__restrict__ fb_x, const double *__restrict__ fb_u, int fb_chunks, int64_t fb_cpad,
    const uint32_t *__restrict__ n_list, const I8State *__restrict__ states = nullptr, const int summed = 0) {
  // summed != 0: the x slots hold the digit sums already -- [window][replicate][power][column] -- written by the narrow kernels and
  // resample_i8g_kernel with the expression below; summed == 1: the u slots too ([window][replicate][power])
  if (states != nullptr) {  // batched int8 call: state blockIdx.y
    const I8State e = states[blockIdx.y];
    part_x = e.part_x; part_u = e.part_u; wflag = e.wflag; pivot = e.pivot; out = e.out;
    fb_x = e.fb_x; fb_u = e.fb_u; n_list = e.n_list;
  }
  // CPAD = columns of a row of part_x (32; 4, 8 or 16 where the narrow-state kernel wrote it)
  constexpr int cpad = CPAD;
  // one workgroup per replicate: thread = (column c < cpad, window segment seg of 256 / cpad).  Segment seg adds the
  // windows seg, seg + nseg, ... in ascending order, then the segments are added in order: a fixed tree that depends on
  // the number of windows (i.e. on N) and on the state's width only, not on the launch geometry.  (One thread per output
  // walking all windows was latency-bound on short series with few outputs: 1600 threads x 611 windows at BASELINE
  // config 2; so were 8 segments for an 8-column state.)
  __shared__ double sh[256][2 * K];
  constexpr int nseg = 256 / cpad;
  const int64_t r = blockIdx.x;
  const int c = threadIdx.x % cpad, seg = threadIdx.x / cpad;
  double S0[K], S1[K];
#pragma unroll
  for (int j = 0; j < K; ++j) S0[j] = S1[j] = 0.0;
  if (c < C) {
    for (int64_t w = seg; w < nwin; w += nseg) {
      if (wflag[w] != 0u) continue;
      if (summed) {  // (uniform) 1: x and u slots digit-summed; 2: x summed, u per digit (resample_i8g_kernel: its u-row digits ride
        // in other waves' columns)
        const double *px_ = part_x + ((size_t)w * nrep_pad + r) * K * cpad + c;
        if (summed == 1) {
          const double *pu_ = part_u + ((size_t)w * nrep_pad + r) * K;
#pragma unroll
          for (int j = 0; j < K; ++j) {
            S0[j] += pu_[j];
            S1[j] += px_[j * cpad];
          }
        } else {
          const double *pu_ = part_u + ((size_t)w * nrep_pad + r) * K * 8;
#pragma unroll
          for (int j = 0; j < K; ++j) {
            const double4 ua = *reinterpret_cast<const double4 *>(pu_ + j * 8), ub = *reinterpret_cast<const double4 *>(pu_ + j * 8 + 4);
            S0[j] += ((((((ua.x + ua.y) + ua.z) + ua.w) + ub.x) + ub.y) + ub.z);  // digit slots 0..6, ascending
            S1[j] += px_[j * cpad];
          }
        }
        continue;
      }
      const double *pu_ = part_u + ((size_t)w * nrep_pad + r) * K * 8;
      const double *px_ = part_x + ((size_t)w * nrep_pad + r) * K * 8 * cpad + c;
#pragma unroll
      for (int j = 0; j < K; ++j) {
        const double4 ua = *reinterpret_cast<const double4 *>(pu_ + j * 8), ub = *reinterpret_cast<const double4 *>(pu_ + j * 8 + 4);
        const double *q = px_ + (size_t)j * 8 * cpad;
        S0[j] += ((((((ua.x + ua.y) + ua.z) + ua.w) + ub.x) + ub.y) + ub.z);  // digit slots 0..6, ascending
        S1[j] += ((((((q[0] + q[cpad]) + q[2 * cpad]) + q[3 * cpad]) + q[4 * cpad]) + q[5 * cpad]) + q[6 * cpad]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < K; ++j) {
    sh[threadIdx.x][j] = S0[j];
    sh[threadIdx.x][K + j] = S1[j];
  }
  __syncthreads();
  if (seg != 0 || c >= C) return;
  for (int g = 1; g < nseg; ++g)
#pragma unroll
    for (int j = 0; j < K; ++j) {
      S0[j] += sh[g * cpad + c][j];
      S1[j] += sh[g * cpad + c][K + j];
    }
  // windows the precision guard handed to the FP64 kernel (same pivot: the sums simply add)
  if (n_list[0] != 0u)
    for (int ch = 0; ch < fb_chunks; ++ch) {
      const double *pu_ = fb_u + ((size_t)ch * nrep_pad + r) * K;
      const double *px_ = fb_x + (((size_t)ch * nrep_pad + r) * fb_cpad + c) * K;
#pragma unroll
      for (int j = 0; j < K; ++j) {
        S0[j] += pu_[j];
        S1[j] += px_[j];
      }
    }
  double st[2 * K];
  pivot_sums_to_state_or_empty<K>(S0, S1, pivot[0], pivot[1 + c_off + c], st);  // weight sum exactly 0: the empty state
  double *o = out + (r * C_total + c_off + c) * 2 * K;
#pragma unroll
  for (int q = 0; q < 2 * K; ++q) o[q] = st[q];
  (void)nrep;
}

// the second sample matrix: per-replicate weighted means  out_y[r][c] = py[c] + S1y / S0  from the per-window slots
// written by the y row set (same fixed tree as above), the sum of weights S0 from the u-row slots (power 0)
__global__ __launch_bounds__(256) void resample_finalize_y_kernel(
    const double *__restrict__ part_y, const double *__restrict__ part_u, int K, int64_t nwin,
    const uint32_t *__restrict__ wflag, int64_t nrep_pad, int64_t C, const double *__restrict__ ypivot,
    double *__restrict__ out_y, int64_t c_off, int64_t C_total, const double *__restrict__ fb_y,
    const double *__restrict__ fb_u, int fb_chunks, int64_t fb_cpad, const uint32_t *__restrict__ n_list) {
  constexpr int NSEG = 8;
  __shared__ double sh[NSEG][32][2];
  const int64_t r = blockIdx.x;
  const int c = threadIdx.x & 31, seg = threadIdx.x >> 5;
  double S0 = 0.0, S1 = 0.0;
  if (c < C) {
    for (int64_t w = seg; w < nwin; w += NSEG) {
      if (wflag[w] != 0u) continue;
      const double *pu_ = part_u + ((size_t)w * nrep_pad + r) * K * 8;
      const double *q = part_y + ((size_t)w * nrep_pad + r) * 8 * I8_CPAD + c;
      const double4 ua = *reinterpret_cast<const double4 *>(pu_), ub = *reinterpret_cast<const double4 *>(pu_ + 4);
      S0 += ((((((ua.x + ua.y) + ua.z) + ua.w) + ub.x) + ub.y) + ub.z);
      S1 += ((((((q[0] + q[I8_CPAD]) + q[2 * I8_CPAD]) + q[3 * I8_CPAD]) + q[4 * I8_CPAD]) + q[5 * I8_CPAD]) + q[6 * I8_CPAD]);
    }
  }
  sh[seg][c][0] = S0;
  sh[seg][c][1] = S1;
  __syncthreads();
  if (seg != 0 || c >= C) return;
  S0 = sh[0][c][0];
  S1 = sh[0][c][1];
  for (int g = 1; g < NSEG; ++g) {
    S0 += sh[g][c][0];
    S1 += sh[g][c][1];
  }
  if (n_list[0] != 0u)
    for (int ch = 0; ch < fb_chunks; ++ch) {
      S0 += fb_u[((size_t)ch * nrep_pad + r) * K];
      S1 += fb_y[((size_t)ch * nrep_pad + r) * fb_cpad + c];
    }
  // as pivot_sums_to_state forms a mean; a replicate of weight sum exactly 0 has no mean: 0, as in the empty state
  out_y[r * C_total + c_off + c] = S0 == 0.0 ? 0.0 : ypivot[1 + c_off + c] + S1 * (1.0 / S0);
}

// ---- launchers: every instantiation of the kernels above is made here --------------------------------------------------
template <int K>
static int run_resample_k(const ResampleArgs &a, const ResamplePlan &p, bool weighted, bool explicit_,
                          double *out, hipStream_t st, int64_t S) {
  dim3 grid((unsigned)(p.n_chunks * p.n_rbg), (unsigned)p.colgroups, (unsigned)S), block(RS_BLOCK);
  const size_t lds = explicit_ ? 0 : (size_t)RS_WAVES * RS_TILE_BYTES;
#define TXM_RS_LAUNCH(NB, WT, EX)                                                                       \
  do {                                                                                                 \
    if (S > 1 || a.batch != nullptr) {                                                                 \
      if (a.N < SM_T)                                                                                  \
        hipLaunchKernelGGL((resample_kernel<K, NB, WT, EX, true, RS_BATCHED>), grid, block, lds, st, a);  \
      else                                                                                             \
        hipLaunchKernelGGL((resample_kernel<K, NB, WT, EX, false, RS_BATCHED>), grid, block, lds, st, a); \
    } else if (a.N < SM_T)                                                                             \
      hipLaunchKernelGGL((resample_kernel<K, NB, WT, EX, true>), grid, block, lds, st, a);             \
    else                                                                                               \
      hipLaunchKernelGGL((resample_kernel<K, NB, WT, EX, false>), grid, block, lds, st, a);            \
  } while (0)
  // narrow states (C <= 8, device sampler, full tiles): PACK powers per B column -> ceil(K / PACK) MFMAs per k-step
  bool packed = false;
  if constexpr (K >= 2 && K <= 6) {
    if (p.nblk == 1 && p.colgroups == 1 && !explicit_ && a.N >= SM_T && a.C <= 8) {
      packed = true;
      const bool bat = S > 1 || a.batch != nullptr;
#define TXM_RS_PACKED(PK)                                                                                      \
  do {                                                                                                         \
    if (bat) {                                                                                                 \
      if (weighted) hipLaunchKernelGGL((resample_kernel<K, 1, true, false, false, RS_BATCHED, PK>), grid, block, lds, st, a); \
      else hipLaunchKernelGGL((resample_kernel<K, 1, false, false, false, RS_BATCHED, PK>), grid, block, lds, st, a);         \
    } else {                                                                                                   \
      if (weighted) hipLaunchKernelGGL((resample_kernel<K, 1, true, false, false, RS_PLAIN, PK>), grid, block, lds, st, a);   \
      else hipLaunchKernelGGL((resample_kernel<K, 1, false, false, false, RS_PLAIN, PK>), grid, block, lds, st, a);           \
    }                                                                                                          \
  } while (0)
      if (a.C <= 4 && K >= 3) TXM_RS_PACKED(4);
      else TXM_RS_PACKED(2);
#undef TXM_RS_PACKED
    }
  }
  if (packed) {
  } else if (p.nblk == 1) {
    if (weighted) { if (explicit_) TXM_RS_LAUNCH(1, true, true); else TXM_RS_LAUNCH(1, true, false); }
    else          { if (explicit_) TXM_RS_LAUNCH(1, false, true); else TXM_RS_LAUNCH(1, false, false); }
  } else {
    if (weighted) { if (explicit_) TXM_RS_LAUNCH(2, true, true); else TXM_RS_LAUNCH(2, true, false); }
    else          { if (explicit_) TXM_RS_LAUNCH(2, false, true); else TXM_RS_LAUNCH(2, false, false); }
  }
#undef TXM_RS_LAUNCH
  TXM_LAUNCH_CHECK();
  const int64_t ne = a.nrep * a.C;
  hipLaunchKernelGGL((resample_finalize_kernel<K>), dim3((unsigned)cdiv(ne, 32), (unsigned)S), dim3(256), 0, st,
                     a.part_x, a.part_u, p.n_chunks, p.nrep_pad, p.C_pad, a.nrep, a.C, a.pivot, out);
  TXM_LAUNCH_CHECK();
  return TXM_OK;
}

// the bootstrap kernel alone, in listed mode (device sampler, N >= one tile), partial sums left for the caller's finalize
template <int K>
static int run_listed_k(const ResampleArgs &a, const ResamplePlan &p, bool weighted, hipStream_t st, int64_t S) {
  dim3 grid((unsigned)(p.n_chunks * p.n_rbg), (unsigned)p.colgroups, (unsigned)S), block(RS_BLOCK);
  const size_t lds = (size_t)RS_WAVES * RS_TILE_BYTES;
  if (p.nblk == 1) {
    if (weighted) hipLaunchKernelGGL((resample_kernel<K, 1, true, false, false, RS_LISTED>), grid, block, lds, st, a);
    else hipLaunchKernelGGL((resample_kernel<K, 1, false, false, false, RS_LISTED>), grid, block, lds, st, a);
  } else {
    if (weighted) hipLaunchKernelGGL((resample_kernel<K, 2, true, false, false, RS_LISTED>), grid, block, lds, st, a);
    else hipLaunchKernelGGL((resample_kernel<K, 2, false, false, false, RS_LISTED>), grid, block, lds, st, a);
  }
  TXM_LAUNCH_CHECK();
  return TXM_OK;
}

int run_listed(const ResampleArgs &a, const ResamplePlan &p0, int K, bool weighted, hipStream_t st, int64_t S) {
  // the plan was made for a full 32-column group; a narrower last group uses one 16-column block
  ResamplePlan p = p0;
  if (a.C <= 16) p.nblk = 1;
  p.colgroups = 1;
  return inf_dispatch(K, "order", [&](auto k) { return run_listed_k<decltype(k)::value>(a, p, weighted, st, S); });
}

int run_resample(const ResampleArgs &a, const ResamplePlan &p, int K, bool weighted, bool explicit_, double *out,
                 hipStream_t st, int64_t S) {
  return inf_dispatch(K, "order", [&](auto k) { return run_resample_k<decltype(k)::value>(a, p, weighted, explicit_, out, st, S); });
}

// f(integral_constant) for the K of 1 .. 8 the int8 path serves (the entry points admit no other) and the row width of
// the group's slots: the 8 x 4 finalize instances
template <int K = 1, class F>
static void finalize_i8_dispatch(int k, int cpad, F &&f) {
  if constexpr (K < 8) {
    if (k != K) return finalize_i8_dispatch<K + 1>(k, cpad, f);
  }
  constexpr std::integral_constant<int, K> kk{};
  if (cpad == 32) f(kk, std::integral_constant<int, 32>{});
  else if (cpad == 16) f(kk, std::integral_constant<int, 16>{});
  else if (cpad == 8) f(kk, std::integral_constant<int, 8>{});
  else f(kk, std::integral_constant<int, 4>{});
}

int launch_finalize_i8(const I8Args &b, const ResampleArgs &f, int K, int summed, double *out, int64_t C_total,
                       hipStream_t st) {
  // (a batched launch takes every per-state pointer from b.states: those of b and f are null, the pivot is passed so)
  const double *pivot = b.states != nullptr ? nullptr : b.pivot;
  finalize_i8_dispatch(K, b.cpad, [&](auto k, auto cp) {
    hipLaunchKernelGGL((resample_finalize_i8_kernel<decltype(k)::value, decltype(cp)::value>),
                       dim3((unsigned)b.nrep, (unsigned)b.S), dim3(256), 0, st, b.part_x, b.part_u, b.nwin, b.wflag, b.nrep_pad,
                       b.nrep, b.C, pivot, out, b.col0, C_total, f.part_x, f.part_u, f.n_chunks, f.C_pad, b.n_list, b.states,
                       summed);
  });
  TXM_LAUNCH_CHECK();
  return TXM_OK;
}

int launch_finalize_y(const I8Args &b, const ResampleArgs &fy, const double *fb_u, int K, double *out_y, int64_t C_total,
                      hipStream_t st) {
  hipLaunchKernelGGL(resample_finalize_y_kernel, dim3((unsigned)b.nrep), dim3(256), 0, st, b.part_y, b.part_u, K, b.nwin,
                     b.wflag, b.nrep_pad, b.C, b.ypivot, out_y, b.col0, C_total, fy.part_x, fb_u, fy.n_chunks, fy.C_pad,
                     b.n_list);
  TXM_LAUNCH_CHECK();
  return TXM_OK;
}
}  // namespace txm
