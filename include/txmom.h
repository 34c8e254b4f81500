/*
 * txmom.h -- C ABI of libtxmom.so: the MI355X (gfx950) moment engine behind
 * thermoextrap's central-(co)moment / bootstrap / derivative hot path.
 *
 * The reference (usnistgov/thermoextrap @ v0.6.0) has NO FFI for this path: its
 * boundary is the Python API of the third-party package cmomy 0.24.0 as called
 * from src/thermoextrap/data.py.  Each entry point below names the cmomy call
 * (and the reference call site, file:line under /root/reference) it replaces;
 * INTEGRATION.md shows the ctypes binding a maintainer would add.
 *
 * Conventions
 *   - return 0 on success, negative txm_status on failure; never throws;
 *     txm_last_error() gives a thread-local message.
 *   - every array pointer is a DEVICE pointer (HBM resident) unless the
 *     parameter name ends in `_host`; the caller owns all buffers; outputs
 *     are caller-allocated and fully overwritten.
 *   - all floating point is IEEE binary64, all indices/counts int64_t,
 *     strides are in ELEMENTS.
 *   - moment-state layout (cmomy convention, verified against the reference's
 *     notebook outputs): trailing dims [xmom = 2][umom = K = order + 1]:
 *        [0][0] = sum of weights   [1][0] = <x>   [0][1] = <u>
 *        [a][b] = <(x-<x>)^a (u-<u>)^b>  otherwise.
 *     1-D states: [0] = sum w, [1] = <u>, [k>=2] = <du^k>.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); all
 *     work is enqueued on it and nothing synchronises unless stated.
 *   - `ws` is scratch in HBM of at least the size the matching *_ws_bytes()
 *     returns; no entry point allocates or frees device memory, so every call
 *     is legal inside hipGraph stream capture.
 */
#ifndef TXMOM_H
#define TXMOM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TXM_ABI_VERSION 2 /* 2: txm_sampler_spec.rep0 */
#define TXM_MAX_ORDER 8 /* K = order + 1 <= 9 */
/* the row pitch ld (doubles) a bootstrap call of C columns may have: 768 * ld + C <= 2^29 (txm_resample_vals, "ROW PITCH");
 * ld <= 699050 for one column, 0 for nothing beyond C = 2^29 */
#define TXM_RESAMPLE_PITCH_OK(ld, C) (768 * (int64_t)(ld) + (int64_t)(C) <= ((int64_t)1 << 29))
#define TXM_SAMPLER_STREAM_VERSION 3 /* 3: one BTRS binomial per tree node (round 4); txm_sampler_stream_version() */

typedef enum txm_status {
  TXM_OK = 0,
  TXM_ERR_INVALID = -1,     /* bad argument (shape, order, null pointer, alignment) */
  TXM_ERR_HIP = -2,         /* a HIP runtime call failed; see txm_last_error() */
  TXM_ERR_WORKSPACE = -3,   /* ws too small */
  TXM_ERR_UNSUPPORTED = -4, /* valid request the library cannot serve */
  TXM_ERR_NO_DEVICE = -5    /* no gfx950 device visible */
} txm_status;

typedef void *txm_stream;

/* ---- runtime ------------------------------------------------------------ */
int txm_abi_version(void);
int txm_sampler_stream_version(void); /* the device sampler stream this build draws (tables are a function of it) */
const char *txm_csrc_sha(void); /* sha256 (16 hex digits) over thermoextrap_amd/csrc/*.hip|*.h this library was compiled from */
const char *txm_last_error(void);
/* Select the device for the calling thread and check it is a gfx950 part. */
int txm_init(int device);
int txm_device_count(int *count_host);
int txm_malloc(void **ptr_host, size_t bytes);
int txm_free(void *ptr);
int txm_memcpy_h2d(void *dst, const void *src_host, size_t bytes, txm_stream stream);
int txm_memcpy_d2h(void *dst_host, const void *src, size_t bytes, txm_stream stream);
int txm_memset(void *dst, int value, size_t bytes, txm_stream stream);
int txm_stream_sync(txm_stream stream);

/* ---- a1/a2: cmomy.wrap_reduce_vals ------------------------------------- */
/* Weighted central comoments of C observables against u, mom = (1, order).
 *   replaces cmomy.wrap_reduce_vals(xv, uv, weight=w, dim=rec, mom=(1, order))
 *   reference call sites: data.py:1632-1640 (DataCentralMomentsVals),
 *   data.py:1194-1203 (DataCentralMoments.from_vals), data.py:530-532,
 *   data.py:487-489 (DataValues*).
 * x[i*ldx_s + c*ldx_c], i < N, c < C.  Either ldx_c == 1 ((rec, val) layout,
 * core/xrutils.py:73-116) or ldx_s == 1 ((val, rec) layout).  w may be NULL.
 * out: [C][2][K].  Total weight zero gives the empty state (all zeros), as cmomy does.
 * The sums are taken about a pivot the library estimates itself: without w the mean of at most 1024 strided samples;
 * with w the WEIGHTED mean of at most 1024 samples spread evenly over the series (rows floor(k N / 1024); rows of weight
 * zero never enter it) -- or the weighted mean of all rows when that subsample is not the whole series and carries less
 * than 32 effective rows of weight -- so that concentrated weights (reweighting, masks) keep the accuracy of the
 * unweighted call.  A row of weight zero may hold any FINITE value; a non-finite one still gives NaN (0 * inf).  txm_push_vals, txm_reduce_vals_batched and txm_reduce_vals_1d
 * follow the same rule.
 */
size_t txm_reduce_vals_ws_bytes(int64_t N, int64_t C, int order);
int txm_reduce_vals(const double *x, int64_t ldx_s, int64_t ldx_c, const double *u,
                    const double *w, int64_t N, int64_t C, int order, double *out, void *ws,
                    size_t ws_bytes, txm_stream stream);

/* ---- the same reduction in pieces: sample shards (SURVEY 8(e) partition (4)) and streaming accumulation ----------
 * The reduce kernels accumulate WEIGHT-SCALED POWER SUMS about a pivot {pivot_u, pivot_x[0..C)}:
 *     sums[c][0][j] = sum_i w_i (u_i - pivot_u)^j          sums[c][1][j] = sum_i w_i (x_ic - pivot_x[c]) (u_i - pivot_u)^j
 * Sums about ONE pivot add exactly like the samples they stand for, so N samples split over ranks (or over time) are:
 * one pivot everybody uses, per-shard sums, one addition in a fixed order, one shift to the cmomy state.
 *   txm_reduce_vals_pivot   the library's own estimate (strided means of at most 1024 samples) for a shard: [1 + C]
 *   txm_reduce_vals_pivot_w the same with weights (w may be NULL): the estimate txm_reduce_vals itself uses for (x, u, w) --
 *                           a weighted reduce about the UNWEIGHTED pivot loses about (1 + delta)^order in accuracy when
 *                           the weighted mean lies delta weighted sigmas from it
 *   txm_reduce_vals_sums    the sums of a shard about a GIVEN pivot: [C][2][K]            (ws: txm_reduce_vals_ws_bytes)
 *   txm_sums_to_state       out[C][2][K] = shift(sums[0] + sums[1] + ... + sums[n - 1]), sums [n][C][2][K], added in index
 *                           order -- an all-gathered stack of per-rank sums gives every rank the same bits
 *   replaces, for a sample-sharded array, the one cmomy.wrap_reduce_vals call of data.py:1632-1640 / 1194-1203.
 * txm_push_vals: cmomy's CentralMomentsData.push_vals(x, u, weight=w) -- accumulate a new chunk of samples into an
 * existing state [C][2][K] in place (a state of zeros is the empty accumulator): the chunk's sums about its own pivot,
 * the old state re-expressed about that pivot, added and shifted back.  (thermoextrap itself never calls push_vals --
 * SURVEY 0.7 -- but it is the streaming form of the reduction above.)  ws: txm_push_vals_ws_bytes. */
int txm_reduce_vals_pivot(const double *x, int64_t ldx_s, int64_t ldx_c, const double *u, int64_t N, int64_t C,
                          double *pivot, txm_stream stream);
int txm_reduce_vals_pivot_w(const double *x, int64_t ldx_s, int64_t ldx_c, const double *u, const double *w, int64_t N,
                            int64_t C, double *pivot, txm_stream stream);
int txm_reduce_vals_sums(const double *x, int64_t ldx_s, int64_t ldx_c, const double *u, const double *w,
                         int64_t N, int64_t C, int order, const double *pivot, double *sums, void *ws,
                         size_t ws_bytes, txm_stream stream);
int txm_sums_to_state(const double *sums, int64_t n, const double *pivot, int64_t C, int order, double *out,
                      txm_stream stream);
size_t txm_push_vals_ws_bytes(int64_t N, int64_t C, int order);
int txm_push_vals(double *state, const double *x, int64_t ldx_s, int64_t ldx_c, const double *u, const double *w,
                  int64_t N, int64_t C, int order, void *ws, size_t ws_bytes, txm_stream stream);

/* 1-D central moments of R independent series, mom = M - 1.
 *   replaces cmomy.wrap_reduce_vals(uv, weight=w, mom=order[+1])
 *   reference call sites: data.py:1183-1191 (x_is_u, mom = order + 1),
 *   data.py:485, 528; lnpi.py:278-282.
 * u[r*ldu_r + i*ldu_s]; ldu_s must be 1.  w (nullable) is shared by all rows.
 * out: [R][M].
 */
size_t txm_reduce_vals_1d_ws_bytes(int64_t N, int64_t R, int M);
int txm_reduce_vals_1d(const double *u, int64_t ldu_r, int64_t ldu_s, const double *w,
                       int64_t N, int64_t R, int M, double *out, void *ws, size_t ws_bytes,
                       txm_stream stream);

/* ---- sampler: cmomy.factory_sampler / IndexSampler ---------------------- */
/* indices[nrep][nsamp] -> freq[nrep][ndat] (histogram; cmomy indices_to_freq).
 *   reference: sampler built at data.py:1028-1037, 1344-1352, 1782-1789;
 *   tests/test_data.py:94-112 feeds explicit indices.
 * Returns TXM_ERR_INVALID if any index is outside [0, ndat) (checked on device,
 * reported after a stream sync).  ws: txm_indices_to_freq_ws_bytes() bytes; it holds the call's
 * error word, so concurrent calls on different streams share no state. */
size_t txm_indices_to_freq_ws_bytes(void);
int txm_indices_to_freq(const int64_t *indices, int64_t nrep, int64_t nsamp, int64_t ndat,
                        int64_t *freq, void *ws, size_t ws_bytes, txm_stream stream);

/* Device multinomial sampler ("scale mode").  The reference draws
 *   indices = rng.choice(ndat, (nrep, ndat), replace=True)   
 * and histograms them, which needs 16*nrep*ndat bytes of tables.  This
 * generates the SAME DISTRIBUTION of frequency tables (multinomial:
 * nsamp draws with replacement per replicate) from a
 * counter-based Philox4x32-10 stream keyed by (seed, stage, replicate, tile)
 * without ever materialising indices; oracle/philox_oracle.c restates the
 * stream bit for bit.  The sampler object is a plain struct (no hidden state).
 * Stream version 3 (round 4; TXM_SAMPLER_STREAM_VERSION): the per-tile draw counts come from recursive binomial
 * splitting over a count-balanced binary tree of tile ranges -- ONE binomial variate per node, Hormann's BTRS
 * (transformed rejection with squeeze, O(1) uniforms) restated with IEEE double + - * / floor in a fixed order so
 * that a CPU and the device produce the same integers, and the version-2 bitwise comparison for nodes with n p < 10;
 * the per-sample counts inside a tile from 10-bit fields (unchanged).  Tables of a given seed differ from versions
 * 1 and 2; the distribution is the same multinomial (BTRS: exact in real arithmetic; here to double rounding, 52-bit
 * uniforms and a < 1e-10 truncation of Stirling's series in the acceptance bound -- the class of
 * numpy.random.Generator.binomial; versions 1 and 2 were exact in integers at 4 x the cost).
 */
typedef struct txm_sampler_spec {
  uint64_t seed;
  int64_t nrep;  /* replicates of this call */
  int64_t ndat;  /* samples being resampled */
  int64_t nsamp; /* draws per replicate; 0 means ndat */
  int64_t rep0;  /* replicate r of this call draws STREAM replicate rep0 + r (rep0 + nrep <= 2^32).  The stream
                    is keyed by (seed, stream replicate, tile) and a replicate's draws depend on nothing else, so
                    the rows [a, b) of an (seed, nrep) table equal the (seed, b - a, rep0 = a) table bit for bit:
                    a rank that owns replicates [a, b) -- or the states [s0, s1) of a collection whose state s owns
                    replicates s * nrep ... -- reproduces its slab of the one-GPU result exactly (the reference
                    runs those loops serially: models.py:614-641).  0 for a whole table. */
} txm_sampler_spec;

/* Per-(replicate, tile) draw counts, tile = 1024 consecutive samples.
 * counts: [nrep][txm_sampler_ntiles(ndat)] uint32.  ndat <= 2^30, nrep <= 2^24; the workspace
 * is no longer used (the tile tree lives in LDS) but the query still returns a
 * valid size and ws_bytes is held to it like everywhere else (TXM_ERR_WORKSPACE). */
int64_t txm_sampler_ntiles(int64_t ndat);
size_t txm_sampler_counts_ws_bytes(const txm_sampler_spec *spec_host);
int txm_sampler_tile_counts(const txm_sampler_spec *spec_host, uint32_t *counts, void *ws,
                            size_t ws_bytes, txm_stream stream);
/* Materialise freq[nrep][ndat] int64 from the stream (testing / small sizes). */
int txm_sampler_freq(const txm_sampler_spec *spec_host, const uint32_t *counts, int64_t *freq,
                     txm_stream stream);

/* Per-SAMPLE draw counts of a slab of replicates as a table in HBM (round 5): what cmomy's freq table holds
 * (indices_to_freq, reached from data.py:1782-1789), at one byte per (replicate, sample), for the replicates
 * [rep_begin, rep_begin + nreps) of the spec only, laid out for the int8 bootstrap kernel's matrix operands:
 *   table[((g * ntiles + t) * 32 + s) * 4096 + q * 1024 + L * 16 + b]
 *     = draws of sample min(1024 t, ndat - 1024) + 32 s + 16 (L >> 5) + b   (0 for the samples a slid last tile
 *       shares with its predecessor)   in replicate rep_begin + 128 g + 32 q + (L & 31)   (0 past the spec's nrep)
 * -- the same Philox calls as txm_sampler_freq, bit for bit.  rep_begin is a multiple of 128; ndat >= 1024;
 * txm_sampler_count_table_bytes(ndat, nreps) = ceil(nreps / 128) * ntiles * 131072.  txm_resample_vals builds and
 * consumes such tables inside its workspace; the entry point exists for tests and for callers that keep a table. */
size_t txm_sampler_count_table_bytes(int64_t ndat, int64_t nreps);
int txm_sampler_count_table(const txm_sampler_spec *spec_host, const uint32_t *counts, int64_t rep_begin,
                            int64_t nreps, uint8_t *table, txm_stream stream);

/* ---- a3/a6: cmomy.wrap_resample_vals ------------------------------------ */
/* Sample-level bootstrap of central comoments: replicate r is the weighted
 * comoment state of the data with weights w_i * freq[r][i].
 *   replaces cmomy.wrap_resample_vals(xv, uv, weight=w, sampler=..., mom=(1, order))
 *   reference call sites: data.py:1803-1810 (DataCentralMomentsVals.resample),
 *   data.py:1354-1366 (DataCentralMoments.from_resample_vals).
 * Exactly one of `freq` (explicit table, [nrep][N] int64: "parity mode") and
 * `spec_host` + `counts` (device sampler: "scale mode") must be given.
 * pivot (nullable): [1 + C] doubles {pivot_u, pivot_x[0..C)} near the means;
 * NULL lets the library estimate one.  Requires ldx_c == 1.
 * out: [nrep][C][2][K]  (rep-major, i.e. already `.transpose(rep_dim, ...)`,
 * data.py:1812).
 * Contract at the edges (tests/test_resample_kernel_gpu.py):
 *   - EMPTY REPLICATE: a replicate whose weight sum  sum_i freq[r][i] w_i  is exactly zero -- a freq row of zeros, or
 *     weights that are zero on every sample the replicate drew -- gets the empty state, all zeros (cmomy's convention;
 *     txm_reduce_vals, txm_push_vals and txm_resample_data do the same), and out_y[r][*] = 0.  Every other replicate
 *     is untouched by that rule.
 *   - ROW PITCH: ldx_s (and opts.ldy_s; ldx_s of the batched entry) must satisfy TXM_RESAMPLE_PITCH_OK(ld, C),
 *     768 * ld + C <= 2^29: the kernels address the rows of one 1024-sample tile through unsigned 32-bit byte offsets
 *     (768 ld + column) * 8, and the column runs over all C columns of the call.  Anything else (a pitch above 699050
 *     doubles at any C; a 600-column window at a pitch of 699050; a tight array of more than 698140 columns) returns
 *     TXM_ERR_UNSUPPORTED before anything is enqueued; copy such a window to a tighter array.
 *   - UNUSED ROWS: a row whose weight w_i is zero, or that no replicate of the call draws (count zero in every row), may
 *     hold any values for which |u_i - pivot_u|^order * |x_ic - pivot_x[c]| is finite -- it enters every sum as
 *     0 * (that product).  NaN, inf or magnitudes whose product overflows (1e150 at order >= 2) are not covered: the
 *     narrow-state kernels form dx du^j before the zero count multiplies it.
 *
 * Scale mode has two kernel families behind it and the library picks one per call:
 *   TXM_PATH_FP64  the contraction on the FP64 matrix pipe (any order, any C);
 *   TXM_PATH_INT8  the same sums on the int8 matrix pipe (orders 0..7, N >= 1024): per SCALING WINDOW -- 262144 samples on
 *                  long series (N >= 2^26), 65536 / 16384 / 4096 on shorter ones, a function of N alone -- every monomial is
 *                  scaled by the window maximum, rounded ONCE to a 51-bit fixed-point integer (error <= 2^-51 of the window
 *                  maximum, unbiased), split into seven signed 8-bit digits and accumulated exactly in int32; 32 columns
 *                  per launch.
 *   The rule of TXM_PATH_AUTO (txm_resample_path; tests/test_abi_cpu.py calls it on both sides of every threshold named here):
 *     - needs N >= 262144 and order <= 7;
 *     - NARROW states, C <= 16 observables in the call: order >= 1, and N >= 786432 at ANY replicate count or, below that,
 *       nrep >= 128 (order 0 stays FP64);
 *     - WIDE states, C > 16 (a last group of 1..16 columns behind full 32-column groups is allowed from order 1; at order 0
 *       it keeps the call on FP64): long series (N >= 786432) from nrep >= 32 at order >= 1 and nrep >= 100 at order 0;
 *       shorter series from nrep >= 64 at order >= 3, 128 at orders 1-2, 384 at order 0.
 *   Inside the int8 path two contraction kernels serve every state and agree BIT FOR BIT (same int32 sums, same flush):
 *     - the kernel that draws the per-sample counts in place (64 replicates per workgroup; orders 0-4 one pass over the
 *       sampler stream, 5-7 two): wide states at orders 3 and 4 without a second matrix at nrep <= 128, replicate counts that
 *       pad badly to 128 (4 * ceil128(nrep) > 5 * ceil64(nrep)), misaligned operands (x not 16-byte aligned or an odd row
 *       pitch); narrow states at nrep <= 64, where 128s pad worse than 64s (ceil128(nrep) > ceil64(nrep)), N < 786432, 9-16
 *       observables (four column quads) at order 4 (one fused pass against two table passes), a row shorter than a whole column quad (C = 1..3 in a
 *       tight array) (txm_resample.hip narrow_table_pays: the sweeps it is read from);
 *     - the count-table kernels (128 replicates per workgroup over ONE table of per-sample counts, txm_sampler_count_table --
 *       wide states: at most three row sets per pass, every call with a second matrix rides it; narrow states: the column
 *       quads and powers of the state in one pass, two for four quads from order 4): all other calls whose workspace holds the
 *       table (txm_resample_vals_ws_bytes_opts).  TXM_PATH_INT8_FUSED / TXM_PATH_INT8_TABLE force one of them;
 *       txm_resample_kernel reports the choice for a shape.
 *                  PRECISION GUARD (data dependent, automatic): the pre-pass also takes, per window, a robust
 *                  typical magnitude of the top-power monomial (the smallest of 64 group means of
 *                  |w du^order dx_c|); a window whose scale exceeds 275 sqrt(n) times it -- a heavy tail, an
 *                  outlier, weights spanning decades: the rounding would no longer stay within 1e-13 of what
 *                  the window contributes -- is contracted by the FP64 kernel instead, in the same call, and
 *                  the two sets of partial sums are added.  Ordinary data flags nothing.
 * txm_resample_path reports the shape-based choice.  The kernel of ONE CALL is chosen by txm_resample_opts.path
 * (TXM_PATH_AUTO = that rule); txm_set_resample_path is a process-wide default for TXM_PATH_AUTO calls kept for tests
 * and A/B timing (initially TXM_PATH_AUTO; the library reads NO environment variable) -- calls that pass a path
 * share no mutable state and are re-entrant per (workspace, stream).
 *
 * txm_resample_opts (HOST struct, NULL = all defaults):
 *   path        TXM_PATH_AUTO / TXM_PATH_FP64 / TXM_PATH_INT8 (/ _INT8_FUSED / _INT8_TABLE: which int8 kernel) for this call.
 *   info        DEVICE pointer to 4 int64 (nullable), written on the stream, no synchronisation:
 *               [0] path taken, [1] scaling windows x column groups, [2] how many of them the precision guard sent
 *               to the FP64 kernel, [3] bit 0: the pre-pass tables came from `prep` (below) instead of being computed; bit 1: the
 *               column groups ran a count-table kernel (else the kernel that draws in place).
 *   prep, prep_bytes, prep_valid
 *               The int8 path's pre-pass (pivot + per-window scale table, guard flags and fallback list) depends on
 *               (x, u, w, pivot, N, C, nrep, order) only -- not on the sampler -- and costs one more read of the samples.
 *               A caller that bootstraps the SAME data repeatedly (the reference caches per data object: data.py:285,
 *               844-942) passes a device buffer of txm_resample_prep_bytes() that it keeps next to the data: a call with
 *               prep_valid == 0 computes the tables into it, later calls with prep_valid == 1 reuse them (one HBM pass
 *               and three launches fewer).  The caller invalidates by passing 0 again; the library keeps no state.
 *   y, ldy_s, out_y
 *               optional second sample matrix y[N][C] (row pitch ldy_s) resampled with the SAME replicate weights:
 *               out_y[nrep][C] = sum_i f_ri w_i y_ic / sum_i f_ri w_i   (the per-replicate mean; DEVICE pointers).
 *               This is VolumeDataCallback's <dx/dq> over the bootstrap sample (reference volume.py:121-134,
 *               dxdqv[sampler.indices].mean): carried by the same pass over the sampler stream instead of a
 *               separate order-0 bootstrap.
 * txm_resample_vals_info is the older synchronising read-back of [0..2] from the workspace of the last call.
 */
#define TXM_PATH_AUTO (-1)
#define TXM_PATH_FP64 0
#define TXM_PATH_INT8 1
#define TXM_PATH_INT8_FUSED 2 /* int8 path, wide states on the kernel that draws the per-sample counts in place (txm_resample_i8t.hip) */
#define TXM_PATH_INT8_TABLE 3 /* int8 path, wide states on the count-table kernel wherever it applies (txm_resample_i8g.hip) */
typedef struct txm_resample_opts {
  int32_t path;
  int32_t prep_valid;
  void *prep;
  size_t prep_bytes;
  int64_t *info;
  const double *y;
  int64_t ldy_s;
  double *out_y;
} txm_resample_opts;
int txm_resample_path(int64_t N, int64_t C, int64_t nrep, int order);
/* The contraction kernel ONE scale-mode call with these options runs when it is handed txm_resample_vals_ws_bytes_opts(N, C,
 * nrep, order, path, has_y) bytes: TXM_PATH_FP64, TXM_PATH_INT8_FUSED or TXM_PATH_INT8_TABLE, OR-ed with TXM_KERNEL_WITH_Y
 * when that kernel carries opts.y as a row set of its own (otherwise y is bootstrapped by a separate order-0 pass behind the
 * call).  `aligned` != 0: x (and y) are 16-byte aligned with an even row pitch >= C rounded up to 4 (the count-table kernel's
 * operand requirement; anything else runs the fused kernel).  What a caller-held pre-pass block (opts.prep) contains depends
 * on exactly this word: WITH_Y blocks hold y's pivot, scales and guard flags, the others do not -- reuse a block
 * (prep_valid = 1) only for calls on the same tensors and (N, C, order) that return the same word here.  Replicate slabs of
 * one bootstrap (spec.rep0) should pass the whole call's kernel as their opts.path, so that a short last slab does not fall on
 * the other side of a replicate-count threshold of the rule. */
#define TXM_KERNEL_WITH_Y 0x100
int txm_resample_kernel(int64_t N, int64_t C, int64_t nrep, int order, int path, int has_y, int aligned);
/* `aligned` for a pair of operands as txm_resample_vals would see them (device or host pointer values: only the address bits and
 * the row pitches are looked at; y may be NULL): 1 when the count-table kernel can take them */
int txm_resample_operands_aligned(const double *x, int64_t ldx_s, int64_t C, const double *y, int64_t ldy_s);
int txm_set_resample_path(int path);
int txm_resample_vals_info(const void *ws, int64_t N, int64_t C, int64_t nrep, int order,
                           int64_t *info_host, txm_stream stream);
size_t txm_resample_prep_bytes(int64_t N, int64_t C, int64_t nrep, int order);
size_t txm_resample_vals_ws_bytes(int64_t N, int64_t C, int64_t nrep, int order);
/* the same for a call that will pass txm_resample_opts.path = `path` and a second matrix iff has_y: the int8 path's count-table
 * kernel (wide states; txm_resample_vals_ws_bytes = path TXM_PATH_AUTO, has_y 0) keeps one byte per (replicate padded to 128,
 * sample) in the workspace -- 12.8 GB per 128 replicates at N = 1e8.  A call given less workspace than this, but at least
 * what TXM_PATH_INT8_FUSED needs, runs the kernel that draws the counts in place: same bits, other speed; less than that is
 * refused (TXM_ERR_WORKSPACE) before anything is enqueued, whichever kernel the call would have taken.  Callers bound the
 * workspace by bootstrapping replicate slabs (spec.rep0): rows [a, b) of a call equal the (b - a)-replicate call at rep0 = a. */
size_t txm_resample_vals_ws_bytes_opts(int64_t N, int64_t C, int64_t nrep, int order, int path, int has_y);
/* extra workspace, BEHIND txm_resample_vals_ws_bytes(), that a call with opts.y needs (ws_bytes >= the sum); a call
 * without opts.y needs none of it (~2 GB at N = 1e8, C = 32, nrep = 1000) */
size_t txm_resample_y_ws_bytes(int64_t N, int64_t C, int64_t nrep);
/* 1 when the int8 kernel can take the shape at all (N >= one sampler tile, order <= 7, ...): what TXM_PATH_INT8 needs;
 * txm_resample_path() is the rule TXM_PATH_AUTO applies on top of it */
int txm_resample_i8_supported(int64_t N, int64_t C, int64_t nrep, int order);
int txm_resample_vals(const double *x, int64_t ldx_s, int64_t ldx_c, const double *u,
                      const double *w, int64_t N, int64_t C, int order, int64_t nrep,
                      const int64_t *freq, const txm_sampler_spec *spec_host,
                      const uint32_t *counts, const double *pivot, double *out,
                      const txm_resample_opts *opts_host, void *ws, size_t ws_bytes, txm_stream stream);

/* ---- (f-1) S state points of one shape in one set of launches ------------- */
/* The reference handles a collection of states with a serial Python loop
 * (StateCollection.resample / map_concat, models.py:614-671; one cmomy call per state).
 * These entry points take S state points that share (N, C, order[, nrep]) -- the 16 lnPi states of
 * BASELINE config 3, the 64 states of the GPR loop of config 5 -- and run ONE launch per kernel with
 * the state on a grid axis.  `states_host` is a HOST array of S device-pointer triples (w NULL for all
 * states or for none); it is copied into the workspace by the call (not stream-capturable).
 *   txm_reduce_vals_batched:   out [S][C][2][K]            (= S x txm_reduce_vals, x row-major, pitch ldx_s)
 *   txm_resample_vals_batched: out [S][nrep][C][2][K]      (= S x txm_resample_vals; FP64 kernel, or the int8 path below)
 *     sampler: ONE spec over S * nrep replicates of ndat = N (state s owns replicates s*nrep ..
 *     (s+1)*nrep - 1 of the stream, so the states' bootstrap samples are independent), with its
 *     counts [S * nrep][ntiles]; or an explicit freq table [S * nrep][N]. */
typedef struct txm_state_ptrs {
  const double *x; /* [N][ldx_s] */
  const double *u; /* [N] */
  const double *w; /* [N] or NULL */
} txm_state_ptrs;
size_t txm_reduce_vals_batched_ws_bytes(int64_t S, int64_t N, int64_t C, int order);
int txm_reduce_vals_batched(const txm_state_ptrs *states_host, int64_t S, int64_t ldx_s, int64_t N,
                            int64_t C, int order, double *out, void *ws, size_t ws_bytes,
                            txm_stream stream);
size_t txm_resample_vals_batched_ws_bytes(int64_t S, int64_t N, int64_t C, int64_t nrep, int order);
int txm_resample_vals_batched(const txm_state_ptrs *states_host, int64_t S, int64_t ldx_s, int64_t N,
                              int64_t C, int order, int64_t nrep, const int64_t *freq,
                              const txm_sampler_spec *spec_host, const uint32_t *counts, double *out,
                              void *ws, size_t ws_bytes, txm_stream stream);
/* The same with per-call options (round 4; txm_resample_vals_batched == opts_host NULL).  Narrow states (C <= 16
 * observables, order >= 1, and N >= 786432 at any replicate count or N >= 262144 from 128 replicates per state -- the rule
 * of the single call, txm_resample_path; or opts.path = TXM_PATH_INT8 wherever txm_resample_i8_supported) run the int8 path of txm_resample_vals with the state on a grid axis of EVERY kernel of it
 * (pre-pass, bootstrap kernel, the precision guard's FP64 fallback, finalize): state s of the batch is, bit for bit, the
 * single call on state s with spec.rep0 + s * nrep.  Fields of txm_resample_opts used: path, info, prep / prep_bytes /
 * prep_valid (ONE block of txm_resample_batched_prep_bytes() for the S states -- their pivots, window tables, guard flags
 * and fallback lists; 0 bytes = the shape never takes the int8 path); y / out_y must be NULL.
 * Reference loops replaced: models.py:635-641, gpr_active/active_utils.py:896-925. */
size_t txm_resample_batched_prep_bytes(int64_t S, int64_t N, int64_t C, int64_t nrep, int order);
/* the kernel a TXM_PATH_AUTO batched call takes (TXM_PATH_FP64 / TXM_PATH_INT8): bind a prep block only for INT8 */
int txm_resample_batched_path(int64_t S, int64_t N, int64_t C, int64_t nrep, int order);
int txm_resample_vals_batched_opts(const txm_state_ptrs *states_host, int64_t S, int64_t ldx_s, int64_t N,
                                   int64_t C, int order, int64_t nrep, const int64_t *freq,
                                   const txm_sampler_spec *spec_host, const uint32_t *counts, double *out,
                                   const txm_resample_opts *opts_host, void *ws, size_t ws_bytes, txm_stream stream);

/* ---- a4/a5: CentralMomentsData.reduce / resample_and_reduce ------------- */
/* Block bootstrap of pre-reduced states: replicate r merges freq[r][i] copies
 * of state i.   data [nrec][C][2][K], freq [nrep][nrec] -> out [nrep][C][2][K]
 *   replaces CentralMomentsData.resample_and_reduce(sampler, dim=rec)
 *   reference call site: data.py:1048-1052 (DataCentralMoments.resample).
 * freq == NULL means nrep = 1 with every count 1, i.e.
 *   CentralMomentsData.reduce(dim=rec)  (data.py:996, DataCentralMoments.reduce). */
size_t txm_resample_data_ws_bytes(int64_t nrec, int64_t C, int order);
int txm_resample_data(const double *data, const int64_t *freq, int64_t nrec, int64_t C,
                      int64_t nrep, int order, double *out, void *ws, size_t ws_bytes,
                      txm_stream stream);

/* ---- a8/a9: cmom()/rmom()/convert.moments_type -------------------------- */
/* n states [2][K]; to_central = 0: central -> raw (CentralMomentsData.rmom(),
 * data.py:845-847); 1: raw -> central (convert.moments_type(to="central"),
 * data.py:1109-1115).  [0][0] (weight) is carried over.  in == out allowed. */
int txm_convert_cov(const double *in, double *out, int64_t n, int order, int to_central,
                    txm_stream stream);
/* n states [M], 1-D moments. */
int txm_convert_1d(const double *in, double *out, int64_t n, int M, int to_central,
                   txm_stream stream);

/* ---- a10/a11: Derivatives.derivs ---------------------------------------- */
/* Table-driven evaluation of the derivative polynomials that the reference
 * builds with sympy + lambdify and evaluates with one xarray isel per symbol
 * (models.py:317-383, beta.py:532-573).  A function is
 *     f = sum_t coef[t] * prod_{k < nfac[t]} atom(fac[t][k])^pow[t][k]   (* optional -log, see flags)
 * where an atom addresses one scalar per output element e = (rep, val):
 *     value = src[atom.src][ rep*atom.s_rep + val*atom.s_val + atom.offset ].
 * Tables are built on the host from the symbolic recursion (thermoextrap_amd/beta.py).
 */
typedef struct txm_atom {
  int32_t src;    /* index into srcs[] */
  int32_t pad;
  int64_t offset; /* element offset of the scalar inside one (rep, val) cell */
  int64_t s_rep;  /* element stride per replicate */
  int64_t s_val;  /* element stride per value column */
} txm_atom;

#define TXM_FUNC_PLAIN 0
#define TXM_FUNC_MINUS_LOG 1 /* f = -log(atoms[log_atom]) + polynomial part */

typedef struct txm_poly_table {
  int32_t n_funcs;           /* number of functions (orders 0..n_funcs-1) */
  int32_t n_atoms;
  int32_t n_terms;           /* total terms over all functions */
  int32_t n_factors;         /* total factors over all terms */
  int32_t log_atom;          /* atom used by TXM_FUNC_MINUS_LOG functions */
  int32_t pad;
  const txm_atom *atoms;     /* [n_atoms]                          (device) */
  const int32_t *func_term0; /* [n_funcs + 1] term range per func  (device) */
  const int32_t *func_flags; /* [n_funcs] TXM_FUNC_*               (device) */
  const double *coef;        /* [n_terms]                          (device) */
  const int32_t *term_fac0;  /* [n_terms + 1] factor range         (device) */
  const int32_t *fac_atom;   /* [n_factors] atom id                (device) */
  const int32_t *fac_pow;    /* [n_factors] integer power, may be negative (device) */
} txm_poly_table;

/* srcs: device array of n_srcs device pointers (const double*).
 * out: [n_funcs][nrep][nval].  The struct itself is read on the host. */
int txm_eval_poly(const txm_poly_table *table_host, const double *const *srcs, int32_t n_srcs,
                  int64_t nrep, int64_t nval, double *out, txm_stream stream);

/* ---- (f-1) ExtrapModel.predict: Taylor series of the derivative table -------- */
/* derivs [n_ord][M] (the output of txm_eval_poly, M = nrep * nval), dalpha [n_alpha] (device):
 *   term[a][k][m] = dalpha[a]^k * (derivs[k][m] * (1 / k!))
 *   mode TXM_TAYLOR_SUM    : out[a][m]    = sum_k term[a][k][m]           (k ascending)
 *   mode TXM_TAYLOR_CUMSUM : out[a][k][m] = sum_{k' <= k} term[a][k'][m]
 *   mode TXM_TAYLOR_TERMS  : out[a][k][m] = term[a][k][m]
 *   replaces ExtrapModel.predict = coefs * dalpha**p summed / cumsummed over the order dim
 *   reference: src/thermoextrap/models.py:479-565 (coefs: models.py:449-477, taylor_series_norm :55-70).
 * One launch over (alpha, rep, val); n_ord <= 16. */
#define TXM_TAYLOR_SUM 0
#define TXM_TAYLOR_CUMSUM 1
#define TXM_TAYLOR_TERMS 2
int txm_predict_taylor(const double *derivs, int32_t n_ord, int64_t M, const double *dalpha,
                       int64_t n_alpha, int32_t mode, double *out, txm_stream stream);

/* ---- (f-2) covariance of the derivatives over bootstrap replicates --------- */
/* vals [n_ord][nrep][nval] -> cov [nval][n_ord][n_ord] with ddof = 1 (numpy.cov),
 * the per-output covariance that gpr_active.input_GP_from_state feeds to the GP
 *   replaces np.cov(resamp_derivs.values[..., k]) for every output k
 *   reference: src/thermoextrap/gpr_active/active_utils.py:134-140.  n_ord <= 16. */
int txm_cov_over_rep(const double *vals, int32_t n_ord, int64_t nrep, int64_t nval, double *cov,
                     txm_stream stream);

/* ---- (f-4) PerturbModel.predict: exponential reweighting ------------------- */
/* out[a][c] = sum_i x[i][c] e^{-dalpha[a] (u_i - uref[a])} / sum_i e^{-dalpha[a] (u_i - uref[a])}
 * for n_alpha perturbations in ONE pass over the samples; uref[a] is the u extreme that
 * makes the largest exponent 0 (min u for dalpha > 0, max u for dalpha < 0), computed by
 * the library -- with freq per replicate, over the samples of positive count, so a replicate
 * that misses the global extreme keeps finite weights.   replaces PerturbModel.predict (reference models.py:1019-1039:
 * exp(dalpha_uv - max) weights, xr.dot / mean).  x row-major (ldx_c == 1); freq (nullable,
 * [nrep][N] int64) adds bootstrap weights -> out [nrep][n_alpha][C]; n_alpha <= 8.
 * dalpha_host: host array.  ws: txm_perturb_ws_bytes. */
size_t txm_perturb_ws_bytes(int64_t N, int64_t C, int32_t n_alpha, int64_t nrep);
int txm_perturb(const double *x, int64_t ldx_s, const double *u, int64_t N, int64_t C,
                const double *dalpha_host, int32_t n_alpha, const int64_t *freq, int64_t nrep,
                double *out, void *ws, size_t ws_bytes, txm_stream stream);

/* ---- (f-5) MBARModel: free energies and reweighted averages over K states --------- */
/* K states (1 <= K <= 64) at alpha0[k], each a sample set (x [n][ldx_s], u [n]); samples are pooled
 * in state order (pooled index = n_0 + ... + n_{s-1} + i) without being copied.  The kernels see u only
 * as ut = u - upiv (one host-chosen pivot, e.g. the pooled mean) and the free energies f only as the
 * shifted log-weights g[k] = ln N_k + f[k] - alpha0[k] * upiv (+ any constant shared by all k):
 *   p[k][n]  = softmax_k(g[k] - alpha0[k] ut_n)            (max subtracted: no positive exponent)
 *   logD[n]  = ln sum_k e^{g[k] - alpha0[k] ut_n}           (the MBAR log-denominator + that constant)
 * replaces MBARModel._default_params / predict (reference models.py:1049-1111: pymbar.MBAR(u_kn, N_k)
 * on u_kn = alpha0_k u_n, then compute_multiple_expectations(x, a * u)["mu"]).
 * `states_host` is a HOST array of K entries; it is copied into the workspace by the call (not
 * stream-capturable).  ws: txm_mbar_ws_bytes(K, C, n_alpha) serves an evaluation and a predict of
 * (C, n_alpha); an evaluation alone needs txm_mbar_ws_bytes(K, 1, 1).  All sums are combined in a
 * fixed order: bitwise reproducible run to run. */
typedef struct txm_mbar_state {
  const double *x; /* [n][ldx_s]; may be NULL for txm_mbar_eval */
  const double *u; /* [n] */
  int64_t n;       /* samples of this state, >= 1 */
  int64_t ldx_s;   /* row pitch of x in elements (>= C) */
} txm_mbar_state;
size_t txm_mbar_ws_bytes(int32_t K, int64_t C, int32_t n_alpha);
/* One evaluation pass over u for the log-weights g_host [K] (host), alpha0_host [K] (host):
 *   out [K + K(K+1)/2 + 1] (device) = S[k] = sum_n p[k][n]  (the objective's gradient is S - N),
 *     H[j][k] = sum_n p[j][n] p[k][n] for j <= k (row-major upper triangle), sum_n logD[n];
 *   logD (nullable, device [sum n]) receives logD[n] of every pooled sample. */
int txm_mbar_eval(const txm_mbar_state *states_host, int32_t K, const double *alpha0_host,
                  const double *g_host, double upiv, double *out, double *logD, void *ws,
                  size_t ws_bytes, txm_stream stream);
/* Reweighted averages for n_alpha <= 8 targets alpha_host (host):
 *   out[a][c] = sum_n x[n][c] e^{-alpha[a] ut_n - logD[n]} / sum_n e^{-alpha[a] ut_n - logD[n]}
 * (out [n_alpha][C], device) with the logD a txm_mbar_eval of the same states and upiv stored; the
 * largest exponent of every target is made exactly 0 by a max pass. */
int txm_mbar_predict(const txm_mbar_state *states_host, int32_t K, int64_t C, double upiv,
                     const double *logD, const double *alpha_host, int32_t n_alpha, double *out,
                     void *ws, size_t ws_bytes, txm_stream stream);

/* The sums over the pooled samples behind MBAR's asymptotic covariance (Shirts & Chodera 2008, eq. 8 and appendix D --
 * pymbar's dA of compute_expectations, df of compute_free_energy_differences) for n_alpha <= 8 targets alpha_host (host).
 * With the columns W_nk = p[k][n] / N_k of the sampled states (p at the log-weights g_host [K], alpha0_host [K]: the
 * solution a txm_mbar_eval wrote `logD` at, same upiv), W_na = w_an / sum_n w_an of the targets
 * (w_an = e^{-alpha[a] ut_n - logD[n]}) and d_nc = x[n][c] - mean[a][c] (mean [n_alpha][C], device: txm_mbar_predict's
 * output for the same targets):
 *   out[a] (device, [n_alpha][1 + K + C (1 + K)]) = Q_a = sum_n W_na^2, B_a[k] = sum_n W_nk W_na (k < K), then per
 *   column c: yy_ac = sum_n W_na^2 d_nc^2, b_ac[k] = sum_n W_nk W_na d_nc (k < K).
 *   lnw (nullable, device [n_alpha]) receives ln sum_n e^{-alpha[a] ut_n - logD[n]} (minus it: the target's free energy
 *   up to the constants the caller put into g and upiv).
 * One pass over u, logD and x behind predict's max pass (no exponent is positive); the contraction runs on the FP64
 * matrix pipe; the denominators ride in the same pass.  Partials are combined in a fixed order: bitwise reproducible.
 * `states_host` is copied into the workspace as by txm_mbar_eval; nothing waits on the host.
 * ws: txm_mbar_cov_ws_bytes(K, C, n_alpha) (0 for arguments out of range). */
size_t txm_mbar_cov_ws_bytes(int32_t K, int64_t C, int32_t n_alpha);
int txm_mbar_cov(const txm_mbar_state *states_host, int32_t K, int64_t C, double upiv, const double *alpha0_host,
                 const double *g_host, const double *logD, const double *alpha_host, int32_t n_alpha,
                 const double *mean, double *out, double *lnw, void *ws, size_t ws_bytes, txm_stream stream);

/* The Gram matrix behind MBAR's covariance ACROSS columns and targets (MBARModel.predict_with_covariance): with
 * y_n,(a,c) = W_na d_nac, d_nac = x[n][c] - mean[a][c], the covariance of two averages is
 *   sum_n y_n,(a,c) y_n,(a',c') + (sqrt(N) b_ac)^T (I_K - sqrt(N) G_s sqrt(N))^+ (sqrt(N) b_a'c')
 * (b of txm_mbar_cov, G_s the Gram matrix of the sampled states); this call gives the first term:
 *   cross_alpha = 0: out (device, [n_alpha][C][C])         = sum_n W_na^2 d_nac d_nac'
 *   cross_alpha = 1: out (device, [n_alpha C][n_alpha C])  = sum_n W_na W_na' d_nac d_na'c'   (index a C + c)
 * It FOLLOWS the txm_mbar_cov call for the same targets: upiv, logD, alpha_host and mean are that call's, lnw (device
 * [n_alpha]) is its output, so that W_na = e^{-alpha[a] ut_n - logD[n] - lnw[a]} is one exponential; ws is that call's
 * workspace (txm_mbar_cov_ws_bytes(K, C, n_alpha) always suffices; there is no size query of its own).  The launch is
 * planned from ws_bytes: more bytes, more sample workgroups, up to one per 256 samples of the longest state and about
 * eight workgroups per CU in all.  1 <= C <= 255, 1 <= n_alpha <= 8, 1 <= K <= 64; bad arguments TXM_ERR_INVALID, fewer
 * bytes than the smallest plan (one sample workgroup) TXM_ERR_WORKSPACE, both before anything is enqueued.
 * The contraction runs on the FP64 matrix pipe; partials are combined in a fixed order: bitwise reproducible, and out is
 * exactly symmetric.
 * txm_mbar_cross_cov_plan: the plan the call would run under (host logic, n_max the longest state): plan_host [4] =
 * column tiles T a side, tile pairs T (T + 1) / 2, sample workgroups, bytes of ws used (when refused: the smallest
 * workspace the call takes). */
int txm_mbar_cross_cov_plan(int32_t K, int64_t C, int32_t n_alpha, int32_t cross_alpha, int64_t n_max,
                            size_t ws_bytes, int64_t *plan_host);
int txm_mbar_cross_cov(const txm_mbar_state *states_host, int32_t K, int64_t C, double upiv, const double *logD,
                       const double *alpha_host, int32_t n_alpha, const double *mean, const double *lnw,
                       int32_t cross_alpha, double *out, void *ws, size_t ws_bytes, txm_stream stream);

/* Reweighted histograms and every sum their asymptotic covariance needs (MBARModel.histogram) for n_alpha <= 8 targets
 * alpha_host (host).  bin_host: HOST array of K device pointers, bin_host[s][i] the int32 bin index of sample i of state s;
 * an index outside [0, nbins) means "outside the range": the sample counts in the normalisation and in the class nbins.
 * With 1_b(n) = (class of sample n == b), b <= nbins, and W_nk, W_na as for txm_mbar_cov (g_host, alpha0_host: the solution
 * a txm_mbar_eval wrote `logD` at, same upiv):
 *   out (device, [n_alpha][K + 2][nbins + 1]): rows k < K  T_kab = sum_n W_nk W_na 1_b(n),
 *                                              row K       H_ab  = sum_n W_na 1_b(n)     (the histogram; sums to 1),
 *                                              row K + 1   S_ab  = sum_n W_na^2 1_b(n).
 *   lnw (nullable, device [n_alpha]): as txm_mbar_cov's.
 * sum_n w_an is taken from row K, as the sum of its nbins + 1 column sums in index order, so Q_a = sum_b S_ab and
 * B_ak = sum_b T_kab are sums of non-negative entries.  A column no sample fell into is exactly 0.0.
 * One pass over u, logD and the bin index behind predict's max pass; x of the states is not read (may be NULL); the
 * contraction runs on the FP64 matrix pipe against the one-hot of the bin index, formed in registers.  No atomics: two
 * calls under the same plan give the same bits.  `states_host` and `bin_host` are copied into the workspace.
 * 1 <= K <= 64, 1 <= nbins <= 1023, 1 <= n_alpha <= 8; bad arguments TXM_ERR_INVALID, fewer bytes than the smallest plan
 * TXM_ERR_WORKSPACE, both before anything is enqueued.
 * There is no size query: the launch is planned from ws_bytes (more bytes, more sample workgroups, up to one per 256
 * samples of the longest state and about four workgroups per CU in all).  txm_mbar_hist_plan: the plan the call would
 * run under (host logic, n_max the longest state): plan_host [4] = bin tiles per workgroup, bin-tile groups, sample
 * workgroups, bytes of ws used (when refused: the smallest workspace the call takes).  Calling it with
 * ws_bytes = SIZE_MAX gives the full plan and its bytes. */
int txm_mbar_hist_plan(int32_t K, int32_t nbins, int32_t n_alpha, int64_t n_max, size_t ws_bytes, int64_t *plan_host);
int txm_mbar_hist(const txm_mbar_state *states_host, const int32_t *const *bin_host, int32_t K, int32_t nbins,
                  double upiv, const double *alpha0_host, const double *g_host, const double *logD,
                  const double *alpha_host, int32_t n_alpha, double *out, double *lnw,
                  void *ws, size_t ws_bytes, txm_stream stream);

/* Blocked (batch-means) MBAR error bars for CORRELATED series kept whole (MBARModel.predict_with_error /
 * predict_with_covariance / free_energy / free_energy_covariance (block=...), blocking_curve) for n_alpha <= 8 targets
 * alpha_host (host).  Every first-order influence of an MBAR estimate is linear in the row
 *   t_n = (W_n1 .. W_nK, {W_na, y_n,(a,0) .. y_n,(a,C-1)} for each target a),     M = K + n_alpha (C + 1) columns
 * (column K + a (C + 1): W_na; column K + a (C + 1) + 1 + c: y_n,(a,c) = W_na (x[n][c] - mean[a][c])) with W_nk, W_na as
 * for txm_mbar_cov (g_host, alpha0_host: the solution a txm_mbar_eval wrote `logD` at, same upiv).  It FOLLOWS the
 * txm_mbar_cov call for the same targets: mean (device [n_alpha][C]) is txm_mbar_predict's output, lnw (device [n_alpha])
 * txm_mbar_cov's, so that W_na = e^{-alpha[a] ut_n - logD[n] - lnw[a]} is one exponential.  State s is cut into level-0
 * blocks of block_host[s] records (HOST array [K], every entry >= 1; a last short block is kept, an entry above n_s means
 * the whole state; blocks never straddle two states); level l merges the pairs of level l - 1 within each state (a last
 * unpaired block stays).  With T_beta = sum_{n in beta} t_n and Tc_beta = T_beta - (len_beta / n_s) sum_{beta' in s} T_beta':
 *   gamma   (device, [n_levels][M][M]) = sum_beta Tc_beta Tc_beta^T over the blocks of level l   (no nb / (nb - 1) factor)
 *   nblocks (device, int64 [n_levels][K]) = the blocks of every state at every level.
 * A state that has ONE block at a level contributes exactly 0.0 to that level.  The covariance of two estimates is
 * l^T gamma l' with l the coefficient vectors of their influences (thermoextrap_amd/_mbar_host.py).
 * One pass over u, logD and x: every level-0 block is summed in an order fixed by its start, its length and C alone (not by
 * the launch); the sums are centred per state BEFORE the Gram pass, which runs on the FP64 matrix pipe with the block axis
 * as the k-axis, upper-triangle tiles only, every entry stored with its mirror.  No atomics: two calls under the same plan
 * give the same bits and every gamma[l] is exactly symmetric.  `states_host` is copied into the workspace.
 * 1 <= K <= 64, 1 <= C <= 255, 1 <= n_alpha <= 8, 1 <= n_levels <= 32; bad arguments TXM_ERR_INVALID, fewer bytes than the
 * smallest plan TXM_ERR_WORKSPACE, both before anything is enqueued.
 * There is no size query.  txm_mbar_block_cov_plan (host logic; n_host [K] the states' sample counts): plan_host [7] = M,
 * level-0 blocks of all states, rows of the piece array (blocks above 4096 records are summed in pieces of 4096),
 * macro-tile pairs of the Gram pass, its block workgroups, bytes of ws used (when refused: the smallest workspace the call
 * takes), byte offset of the level-0 array in ws (after a call with n_levels = 1 it holds Tc [blocks][M], state after
 * state: a diagnostic the tests read).  The workspace holds the block sums, 8 M sum_s ceil(n_s / block_s) bytes (half as
 * much again for n_levels > 1), the pieces, the per-state column sums and the Gram records; more bytes buy more block workgroups of the Gram pass, up to
 * one per 256 blocks and about four per CU in all.  ws_bytes = SIZE_MAX gives the full plan and its bytes. */
int txm_mbar_block_cov_plan(const int64_t *n_host, const int64_t *block_host, int32_t K, int64_t C, int32_t n_alpha,
                            int32_t n_levels, size_t ws_bytes, int64_t *plan_host);
int txm_mbar_block_cov(const txm_mbar_state *states_host, int32_t K, int64_t C, double upiv, const double *alpha0_host,
                       const double *g_host, const double *logD, const double *alpha_host, int32_t n_alpha,
                       const double *mean, const double *lnw, const int64_t *block_host, int32_t n_levels,
                       double *gamma, int64_t *nblocks, void *ws, size_t ws_bytes, txm_stream stream);

/* ---- (f-6) MBARModel.bootstrap: nrep weighted MBAR problems over the same pooled samples ----------- */
/* Extends (f-5) where the reference stops (models.py:1109-1111: MBARModel.resample raises): replicate r
 * gives sample n of state s the integer count c[r][n] of row r of that state's multinomial sampler
 * (spec.ndat = n_s draws out of n_s; spec.nsamp 0 or ndat; counts = the tile counts
 * txm_sampler_tile_counts wrote for the spec, [nrep][txm_sampler_ntiles(n_s)]; every state the same
 * spec.nrep).  The per-sample counts are regenerated from the sampler stream inside the kernels:
 * nothing of size nrep x (sum n) is stored, logD is recomputed from g by predict.
 *   S[r][k] = sum_n c p[k][n],  H[r][j][k] = sum_n c p[j][n] p[k][n],  obj[r] = sum_n c logD[n]
 * with p, logD of (f-5) at the log-weights g[r][.] (DEVICE array [nrep][K]).  `states_host`,
 * `samplers_host`, `alpha0_host` are HOST arrays of K entries (copied into the workspace: not
 * stream-capturable).  A state's tiles are split over waves by a rule of (n_s, K) alone and all sums
 * are combined in index order: bitwise reproducible, and row r depends on (seed, spec.rep0 + r, g[r])
 * only -- not on the other replicates of the call (rows [a, b) of a call equal the call with the
 * samplers' rows [a, b): rep0 + a, counts + a * ntiles). */
typedef struct txm_mbar_boot_state {
  txm_sampler_spec spec;  /* this state's sampler (host copy) */
  const uint32_t *counts; /* device, [spec.nrep][txm_sampler_ntiles(spec.ndat)] */
} txm_mbar_boot_state;
/* 0 for arguments out of range; non-decreasing in n_total (= sum n) and nrep. */
size_t txm_mbar_boot_ws_bytes(int32_t K, int64_t C, int32_t n_alpha, int64_t n_total, int64_t nrep);
/* One weighted evaluation pass for the replicates active[0 .. n_active) (device int32 row indices;
 * NULL: rows 0 .. n_active-1): out [nrep][K + K(K+1)/2 + 1] (device) = S, upper triangle of H
 * (row-major), obj of each listed row; other rows are not written.
 * ws >= txm_mbar_boot_ws_bytes(K, 1, 1, sum n, nrep). */
int txm_mbar_boot_eval(const txm_mbar_state *states_host, const txm_mbar_boot_state *samplers_host,
                       int32_t K, const double *alpha0_host, const double *g, const int32_t *active,
                       int64_t n_active, double upiv, double *out, void *ws, size_t ws_bytes,
                       txm_stream stream);
/* Reweighted averages of every replicate at n_alpha <= 8 targets (host):
 *   out[r][a][c] = sum_n c[r][n] x[n][c] w / sum_n c[r][n] w,  w = e^{-alpha[a] ut_n - logD[r][n]}
 * (out [nrep][n_alpha][C], device).  gref_host [K]: reference log-weights, the SAME in every call whose
 * rows are to agree bit for bit (the point solution's g): the exponents of (r, a) are shifted by
 * Mref[a] - min_k (g[r][k] - gref[k]), Mref[a] the exact maximum of -alpha[a] ut - logD over all pooled
 * samples at gref -- no shifted exponent is positive, and the largest is within
 * (max_k - min_k)(g[r] - gref) plus the gap to the largest drawn sample of 0.
 * ws >= txm_mbar_boot_ws_bytes(K, C, n_alpha, sum n, nrep). */
int txm_mbar_boot_predict(const txm_mbar_state *states_host, const txm_mbar_boot_state *samplers_host,
                          int32_t K, int64_t C, double upiv, const double *alpha0_host, const double *g,
                          const double *gref_host, const double *alpha_host, int32_t n_alpha, double *out,
                          void *ws, size_t ws_bytes, txm_stream stream);

/* ---- (f-7) timeseries: symmetrised lag sums for the statistical inefficiency ----------------------------- */
/* R_ab(t) = sum_{i=0}^{n-1-t} (da_i db_{i+t} + db_i da_{i+t}),  da = a - <a>, db = b - <b>, for n_pairs pairs of the
 * series {u, x_0 .. x_{C-1}} and the lags t0 .. t0 + nlags - 1 (both multiples of 256, nlags <= 4096); lags >= n give 0.
 * The normalised fluctuation correlation function is C(t) = R(t) / (2 (n - t) sigma^2) with sigma^2 = R(0) / (2 n).
 *   replaces pymbar.timeseries.statistical_inefficiency's correlation sums, which the reference takes of every
 *   observable column, of the potential energy and of every (column, energy) pair before it subsamples
 *   (gpr_active/active_utils.py:244-269, DataWrapper.get_data).
 * Pair index 0 is (u, u), 1 + c is (x_c, x_c), 1 + C + c is (x_c, u).  x is [n][ldx_s] row-major (pitch ldx_s >= C); x = NULL
 * with C = 0 is legal.  center (device, [1 + C]): <u>, <x_0> .. <x_{C-1}> -- the means of txm_reduce_vals.
 * `pairs_host` is a HOST array of n_pairs indices; it is copied into the workspace by the call (not stream-capturable).
 * out (device): [n_pairs][nlags].  The sample chunking is a function of n alone, each (chunk, pair, lag) partial is
 * written once and the chunks are added in index order: two runs give the same bits, and R(t) has the same bits whichever
 * 256-aligned (t0, nlags) block it is computed in.  ws also holds the 1 + C centred series as contiguous rows
 * (8 (1 + C) n bytes). */
size_t txm_lag_sums_ws_bytes(int64_t n, int64_t C, int32_t n_pairs, int32_t nlags);
int txm_lag_sums(const double *x, int64_t ldx_s, const double *u, int64_t n, int64_t C, const double *center,
                 const int32_t *pairs_host, int32_t n_pairs, int64_t t0, int32_t nlags, double *out, void *ws,
                 size_t ws_bytes, txm_stream stream);

/* ---- (f-8) timeseries: the lag sums of every suffix, for equilibration detection -------------------------- */
/* For n_series of the series {u, x_0 .. x_{C-1}} (index 0 is u, 1 + c is x_c; any order, a subset) and every origin
 * j nskip, j = 0 .. n_origins - 1, n_origins = ceil((n - 1) / nskip) in [1, 4096]: the auto lag sum of the suffix
 * a[j nskip : n], centred with the suffix's OWN mean m_j,
 *   R_j(t) = 2 sum_{i = j nskip}^{n-1-t} (a_i - m_j)(a_{i+t} - m_j),   t = t0 .. t0 + nlags - 1
 * (t0 and nlags multiples of 256, nlags <= 4096; lags >= n - j nskip give 0), so that origin j's statistical
 * inefficiency follows from R_j exactly as in (f-7) with n - j nskip for n.
 *   replaces the loop of pymbar.timeseries.detect_equilibration, which calls statistical_inefficiency on A_t[t0:] for
 *   every origin t0 in range(0, T - 1, nskip): one pass over the samples here instead of one per origin.
 * center (device, [1 + C]): one pivot p per series, ANY value near the data -- the series are centred on it once and
 *   R_j(t) = 2 [Q_j(t) - delta_j X_j(t) + (n - j nskip - t) delta_j^2],  delta_j = m_j - p,
 * with Q_j, X_j the lag sums of d = a - p with itself and with a series of ones over i >= j nskip.  The expansion loses
 * what delta_j^2 / var(a) is large against: pass the mean of the part of the series that is in equilibrium (engine.py:
 * the second half).  x is [n][ldx_s] row-major (pitch ldx_s >= C); x = NULL with C = 0 is legal.
 * `series_host` is a HOST array of n_series indices; it is copied into the workspace by the call (not stream-capturable).
 * out (device): [n_series][n_origins][nlags].  mean_out (device, [n_series][n_origins], may be NULL): the suffix means
 * p + delta_j.  Each (segment, series, lag) partial is written once and the segments are added from the last to the first
 * in index order, every delta_j comes from per-segment sums of d taken the same way: two runs give the same bits, and
 * R_j(t) has the same bits whichever 256-aligned (t0, nlags) block it is computed in.  ws holds the 1 + C centred series
 * (8 (1 + C) n bytes) and 16 n_origins n_series nlags bytes of partials. */
size_t txm_lag_origin_sums_ws_bytes(int64_t n, int64_t C, int32_t n_series, int64_t nskip, int32_t nlags);
int txm_lag_origin_sums(const double *x, int64_t ldx_s, const double *u, int64_t n, int64_t C, const double *center,
                        const int32_t *series_host, int32_t n_series, int64_t nskip, int64_t t0, int32_t nlags,
                        double *out, double *mean_out, void *ws, size_t ws_bytes, txm_stream stream);

/* ---- (f-9) delta-method covariance of n_f estimates from their influence polynomials -------------------------- */
/* For one state of N samples and C observable columns (operands x, ldx_s, ldx_c, u, w as in txm_reduce_vals; w may be
 * NULL) and, per column, the empirical influence functions of n_f estimates as polynomials in
 * dx = x[n][c] - center_x[c], du = u[n] - center_u:
 *     psi_k(n, c)  = sum_{q < n_q} (a[c][k][q] + b[c][k][q] dx) du^q                          k < n_f <= 9, n_q <= 9
 *     cov[c][i][j] = sum_n w_n^2 psi_i psi_j / (sum_n w_n)^2      (full symmetric n_f x n_f; [i][j] and [j][i] same bits)
 *     mean[c][k]   = sum_n w_n psi_k / sum_n w_n                  (diagnostic: ~ 0 for a correct coefficient set)
 * -- the infinitesimal-jackknife (delta-method) covariance of estimates whose influence functions are psi_k: the
 * first-order term of what a multinomial bootstrap of the samples estimates, for independent samples.  No cmomy /
 * reference call does this; ExtrapModel.derivs_cov builds a, b from the derivative polynomials (symbolic.influence_coefs).
 * center_u is a host scalar; center_x [C], a and b [C][n_f][n_q], cov [C][n_f][n_f] and mean [C][n_f] are device arrays.
 * One pass over x: the kernels accumulate sum w^2 dx^p du^r (p <= 2, r <= 2 (n_q - 1)) and sum w dx^p du^q (p <= 1) per
 * workgroup, the partials are added in a fixed order and contracted with a, b per column -- no atomics, two calls give the
 * same bits.  First-order rounding bound: eps * sum_n p_n^2 B_i(n) B_j(n), B_k = sum_q (|a_kq| + |b_kq| |dx|) |du|^q,
 * p_n = w_n / sum w.  A row of weight zero is skipped and may hold anything; total weight zero gives zeros. */
size_t txm_influence_cov_ws_bytes(int64_t N, int64_t C, int n_q);
int txm_influence_cov(const double *x, int64_t ldx_s, int64_t ldx_c, const double *u, const double *w, int64_t N,
                      int64_t C, int n_f, int n_q, double center_u, const double *center_x, const double *a,
                      const double *b, double *cov, double *mean, void *ws, size_t ws_bytes, txm_stream stream);

/* ---- (f-10) the same for S independent states in one set of launches ------------------------------------------- */
/* S states of C columns each, x row-major with ONE pitch ldx_s (ldx_c == 1) and a sample count PER STATE -- decorrelated
 * time series have different lengths.  `states_host` is a HOST array of S records (w NULL for all states or for none);
 * it is copied into the workspace by the call (not stream-capturable).  center_u [S], center_x [S][C], a and b
 * [S][C][n_f][n_q], cov [S][C][n_f][n_f] and mean [S][C][n_f] are device arrays.  Two launches for all states: the
 * state rides a grid axis of the sample kernel and of the finalize kernel.
 * BITS: state s is computed under the plan txm_influence_cov makes for n_s alone -- its own number of workgroups, row
 * stride and fixed-order sum of the partials inside a launch as wide as the widest state (workgroups a state does not
 * use leave at once).  The batch reads two columns per lane only if EVERY state qualifies (C even, ldx_s even, x
 * 16-byte aligned, n_q <= 6), one column per lane otherwise; C == 1 with ldx_s == 1 takes the series kernel, as the
 * single call does.  State s of the batch therefore equals txm_influence_cov(x_s, ldx_s, 1, u_s, w_s, n_s, ...) BIT FOR
 * BIT whenever that call picks the instantiation the batch picked -- always, unless the states' x pointers differ in
 * 16-byte alignment while C and ldx_s are even and n_q <= 6 (then the aligned states' single calls read two columns
 * per lane and the batch one: same sums, another order).
 * Zero-weight rows are skipped; a state of total weight zero gives zeros for that state only; no floating-point
 * atomics, two calls give the same bits, cov is bitwise symmetric.  S <= 65535, C <= 65535, n >= 1 per state,
 * ldx_s >= C; null pointers, mixed NULL / non-NULL w and a short workspace are refused before anything is enqueued.
 * txm_influence_cov_batched_ws_bytes(S, n_max, C, n_q), n_max = max_s n_s, is host logic: 0 for bad arguments. */
typedef struct txm_inf_state {
  const double *x; /* [n][ldx_s] */
  const double *u; /* [n] */
  const double *w; /* [n] or NULL (for all states or for none) */
  int64_t n;       /* >= 1, may differ from state to state */
} txm_inf_state;
size_t txm_influence_cov_batched_ws_bytes(int64_t S, int64_t n_max, int64_t C, int n_q);
int txm_influence_cov_batched(const txm_inf_state *states_host, int64_t S, int64_t ldx_s, int64_t C, int n_f, int n_q,
                              const double *center_u, const double *center_x, const double *a, const double *b,
                              double *cov, double *mean, void *ws, size_t ws_bytes, txm_stream stream);

/* ---- (f-11) blocked (batch-means) delta-method covariance for correlated samples, with the blocking curve ------ */
/* The operands of (f-9) for x row-major with pitch ldx_s >= C (w may be NULL), a block length `block` = B >= 1 and
 * n_levels in [1, 32].  With p_n = w_n / sum w and psi_k(n, c) as in (f-9), level-l block j covers the rows
 * [j B 2^l, min(N, (j + 1) B 2^l)) -- the last block may be short and is kept -- and
 *     z_j[c][k]          = sum_{n in block j} p_n psi_k(n, c)
 *     cov[l][c][i][j']   = sum_j z_j[c][i] z_j[c][j']      (l < n_levels; full symmetric n_f x n_f, [i][j'] and [j'][i] same bits)
 *     mean[c][k]         = sum_n p_n psi_k(n, c)           (diagnostic: ~ 0)
 * -- batch means / the cluster-robust sandwich estimator with time blocks as clusters: the covariance of the estimates
 * when the samples are a correlated series and B exceeds its correlation time.  There is NO nb / (nb - 1) factor, so
 * block = 1, level 0 is the cov of (f-9); the relative bias is -1 / nb with nb = ceil(N / (B 2^l)) blocks at level l.
 * Levels with a single block are allowed and computed (block > N too: one block).  cov [n_levels][C][n_f][n_f] and
 * mean [C][n_f] are device arrays, the rest as in (f-9).
 * Pass 1 reads the samples once: per level-0 block and column the 2 n_q sums  sum w du^q,  sum w dx du^q  are contracted
 * with a, b once per block into the workspace; every block is summed by one workgroup in a fixed order, so its bits do
 * not depend on the launch width.  Pass 2 (a workgroup per column) adds the total weight in a fixed order and merges the
 * pairs of the level below in place, level by level.  No floating-point atomics; two calls give the same bits.
 * A row of weight zero is selected out and may hold anything; a block of total weight zero contributes zero; total
 * weight zero gives zeros.  First-order rounding bound per level: eps * sum_b beta_bi beta_bj',
 * beta_bk = sum_{n in b} p_n B_k(n), B_k as in (f-9).
 * Workspace: 8 ceil(N / block) (C n_f + 1) + 256 bytes -- txm_influence_block_cov_ws_bytes, host logic, 0 for bad
 * arguments.  Null pointers, N < 1, C outside [1, 65535], n_f or n_q outside [1, 9], ldx_s < C, a NaN center_u,
 * block < 1, n_levels outside [1, 32] and a short workspace are refused before anything is enqueued. */
size_t txm_influence_block_cov_ws_bytes(int64_t N, int64_t C, int n_f, int n_q, int64_t block);
int txm_influence_block_cov(const double *x, int64_t ldx_s, const double *u, const double *w, int64_t N, int64_t C,
                            int n_f, int n_q, double center_u, const double *center_x, const double *a, const double *b,
                            int64_t block, int n_levels, double *cov, double *mean, void *ws, size_t ws_bytes,
                            txm_stream stream);

/* ---- (f-12) delta-method covariance ACROSS the observable columns: every block Cov(estimate i of c, estimate j of c') -- */
/* The operands of (f-9) for x row-major with pitch ldx_s >= C (w may be NULL) and C <= 255.  With p_n = w_n / sum w and
 * psi_k(n, c) as in (f-9),
 *     cov[c][i][c'][j] = sum_n p_n^2 psi_i(n, c) psi_j(n, c')                      c, c' < C;  i, j < n_f <= 9;  n_q <= 9
 * -- the (C n_f) x (C n_f) infinitesimal-jackknife covariance of ALL estimates of ALL columns, which share one u and one
 * set of samples: what a sum over bins, a ratio of two observables or a multi-output model needs.  The device array cov
 * [C][n_f][C][n_f] is symmetric as a (C n_f)^2 matrix, [c][i][c'][j] and [c'][j][c][i] holding the same bits; its blocks
 * c == c' are the cov of (f-9) within the two calls' rounding bounds (another summation order, not the same bits).  There
 * is no `mean` output.  Independent samples are assumed, as in (f-9); the blocked form for a correlated series is (f-13).
 * psi psi' depends on (q, q') only through r = q + q', so the sample pass needs no coefficients: it accumulates the
 * 2 n_q - 1 Gram matrices  G_r = sum_n w_n^2 du^r z_n z_n^T,  z_n = (dx_n0 .. dx_n,C-1, 1),  on the FP64 matrix pipe
 * (v_mfma_f64_16x16x4_f64) in tiles of 16 x 16 over the C + 1 logical columns, upper-triangle tile pairs only, one record
 * per (workgroup, tile pair) in the workspace.  A second kernel adds the workgroups in index order and a third contracts
 * with a, b in one fixed order, reading G at (row <= column) only and storing every entry with its mirror.  No
 * floating-point atomics: two calls give the same bits.  The bits depend on N (the samples' assignment to waves does).
 * A row of weight zero is selected out and may hold anything; total weight zero gives zeros.
 * First-order rounding bound: eps * sum_n p_n^2 B_i(n, c) B_j(n, c'), B_k as in (f-9).
 * Workspace: txm_influence_cross_cov_ws_bytes(N, C, n_f, n_q), host logic, nondecreasing in C, 0 for bad arguments (at
 * most 8 (256 (2 n_q - 1) + 8) (8 workgroups per CU + 2 * tile pairs) + 256 bytes: 76 MB at C = 255, order 8).
 * Null pointers, N < 1, C outside [1, 255], n_f or n_q outside [1, 9], ldx_s < C and a NaN center_u return
 * TXM_ERR_INVALID, a short workspace TXM_ERR_WORKSPACE, all before anything is enqueued. */
size_t txm_influence_cross_cov_ws_bytes(int64_t N, int64_t C, int n_f, int n_q);
int txm_influence_cross_cov(const double *x, int64_t ldx_s, const double *u, const double *w, int64_t N, int64_t C,
                            int n_f, int n_q, double center_u, const double *center_x, const double *a, const double *b,
                            double *cov, void *ws, size_t ws_bytes, txm_stream stream);

/* ---- (f-13) blocked (batch-means) delta-method covariance ACROSS the observable columns, with the blocking curve ---- */
/* The operands of (f-11) with C <= 255.  With p_n, psi_k(n, c), the level-l blocks (the last may be short and is kept;
 * levels with a single block are allowed) and the block sums z_j[c][k] = sum_{n in block j} p_n psi_k(n, c) of (f-11),
 *     cov[l][c][i][c'][j'] = sum_j z_j[c][i] z_j[c'][j']      (l < n_levels;  c, c' < C;  i, j' < n_f)
 *     mean[c][k]           = sum_n p_n psi_k(n, c)            (diagnostic: ~ 0)
 * -- the covariance of ALL estimates of ALL columns of a correlated series whose correlation time `block` exceeds: what
 * a sum over bins, a ratio of two observables or a multi-output model needs.  There is NO nb / (nb - 1) factor: block = 1,
 * level 0 is the cov of (f-12) and the blocks c == c' are the cov[l][c] of (f-11), each within the two calls' rounding
 * bounds (other summation orders, not the same bits).  The device array cov [n_levels][C][n_f][C][n_f] is, level by
 * level, symmetric as a (C n_f)^2 matrix, [c][i][c'][j'] and [c'][j'][c][i] holding the same bits; mean is [C][n_f].
 * Pass 1 is that of (f-11) -- the same kernel under the same plan -- and leaves the unnormalised block sums zt [nb][M],
 * M = C n_f, nb = ceil(N / block), and the block weights in the workspace.  Two small kernels add the columns of zt and
 * the weights in a fixed order (mean, W).  Per level: the pairs of the level below are merged in place
 * (zt[j 2^l] += zt[j 2^l + 2^(l-1)]; a last unpaired block stays), then G = sum_b z_b z_b^T runs on the FP64 matrix pipe
 * (v_mfma_f64_16x16x4_f64, the block axis as the k-axis, four blocks a step) in tiles of 16 x 16 grouped into macro tiles
 * of 4 x 4 tiles, upper-triangle macro pairs and, inside a diagonal one, upper-triangle tiles only; one record of 16
 * tiles per (workgroup, macro pair), the workgroups' records added in index order; a last kernel reads G at
 * (row <= column) only, divides by W^2 and stores every entry with its mirror.  No floating-point atomics: two calls give
 * the same bits.  A row of weight zero is selected out and may hold anything; a block of total weight zero contributes
 * zero; total weight zero gives zeros.  First-order rounding bound per level:
 * eps * sum_b beta_b(c, i) beta_b(c', j'),  beta_b(c, k) = sum_{n in b} p_n B_k(n, c),  B_k as in (f-9).
 * Workspace: txm_influence_block_cross_cov_ws_bytes, host logic, 0 for bad arguments, the same for every n_levels (the
 * merge is in place): pass 1's 8 nb (M + 1) bytes, at most 256 (M + 1) column-sum partials and at most
 * max(4 workgroups per CU, macro pairs) + macro pairs records of 32 KiB (44 MB at M = 2295: 666 macro pairs), + 256.
 * Null pointers, N < 1, C outside [1, 255], n_f or n_q outside [1, 9], ldx_s < C, a NaN center_u, block < 1 and n_levels
 * outside [1, 32] return TXM_ERR_INVALID, a short workspace TXM_ERR_WORKSPACE, all before anything is enqueued. */
size_t txm_influence_block_cross_cov_ws_bytes(int64_t N, int64_t C, int n_f, int n_q, int64_t block, int n_levels);
int txm_influence_block_cross_cov(const double *x, int64_t ldx_s, const double *u, const double *w, int64_t N, int64_t C,
                                  int n_f, int n_q, double center_u, const double *center_x, const double *a,
                                  const double *b, int64_t block, int n_levels, double *cov, double *mean, void *ws,
                                  size_t ws_bytes, txm_stream stream);

/* ---- (f-14) the cross-column covariance of (f-12) for S independent states in one set of launches ---------------- */
/* S states of C <= 255 columns each, x row-major with ONE pitch ldx_s >= C and a sample count PER STATE.  `states_host`
 * is a HOST array of S records of (f-10) (w NULL for all states or for none); it is copied into the workspace by the
 * call (not stream-capturable).  center_u [S], center_x [S][C], a and b [S][C][n_f][n_q] and cov [S][C][n_f][C][n_f] are
 * device arrays.  For state s the definition is (f-12)'s on that state's operands:
 *     cov[s][c][i][c'][j] = sum_n p_n^2 psi_i(n, c) psi_j(n, c')
 * Three launches for all states: the state rides a grid axis of the sample, the sum and the finalize kernel.
 * PLAN: the batch has a plan of its own, a function of (S, C, n_s, compute units) only.  With T = ceil((C + 1) / 16) and
 * pairs = T (T + 1) / 2, a state may have  q = max(1, floor(8 CUs / (pairs S)))  sample workgroups and state s gets
 * grid_x_s = min(ceil(n_s / 256), q) -- txm_influence_cross_cov_batched_grid(S, n_s, C), host logic, 0 for bad arguments.
 * The launch is (pairs, max_s grid_x_s, S); a workgroup beyond its state's grid_x_s leaves at once; every state has its
 * own slice of the workspace for its grid_x_s pairs partial records and its pairs summed records.
 * BITS: inside a state everything is (f-12)'s -- the 4-sample steps of a wave, the wave-order sum, the index-order sum of
 * the records, the finalize's fixed contraction order and the mirror store.  State s therefore equals
 * txm_influence_cross_cov on that state alone BIT FOR BIT whenever both plans give it the same number of sample
 * workgroups: whenever ceil(n_s / 256) <= q (q never exceeds the single call's cap), and always for S == 1.  A state whose
 * budget q binds below its single plan has the same sums added in another order: the rounding bound of (f-12) holds for
 * it, equal bits are not promised.  No floating-point atomics, two calls give the same bits, every cov[s] is bitwise
 * symmetric as a (C n_f)^2 matrix.  Zero-weight rows are selected out and may hold anything; a state of total weight zero
 * gives zeros for that state only.
 * Workspace: txm_influence_cross_cov_batched_ws_bytes(S, n_max, C, n_f, n_q), n_max = max_s n_s, host logic, 0 for bad
 * arguments, nondecreasing in n_max: S (min(ceil(n_max / 256), q) + 1) pairs records of 8 (256 (2 n_q - 1) + 8) bytes, the
 * 256-byte-aligned state table and 256 bytes (30 MB for 64 states of 1e6 samples, 4 columns, order 3, on 256 CUs).
 * Null pointers, S outside [1, 65535], any n < 1, C outside [1, 255], n_f or n_q outside [1, 9], ldx_s < C and mixed
 * NULL / non-NULL w return TXM_ERR_INVALID, a short workspace TXM_ERR_WORKSPACE, all before anything is enqueued and with
 * cov untouched.  center_u is a device array here: a NaN among its entries is NOT checked (it gives NaN for that state). */
size_t txm_influence_cross_cov_batched_ws_bytes(int64_t S, int64_t n_max, int64_t C, int n_f, int n_q);
int txm_influence_cross_cov_batched_grid(int64_t S, int64_t n, int64_t C);
int txm_influence_cross_cov_batched(const txm_inf_state *states_host, int64_t S, int64_t ldx_s, int64_t C, int n_f, int n_q,
                                    const double *center_u, const double *center_x, const double *a, const double *b,
                                    double *cov, void *ws, size_t ws_bytes, txm_stream stream);

/* ---- (f-15) PerturbModel error bars: delta-method variance, Kish n_eff and the free-energy difference of (f-4) ---- */
/* The operands of (f-4) without bootstrap counts, the reweighted means  mean [n_alpha][C]  (device; (f-4)'s output -- the
 * sums are centred on the GIVEN mean, so nothing cancels), a block length `block` = B >= 1 and n_levels in [1, 32].  With
 *     w_na = e^{-dalpha[a] (u_n - uref[a])}   (uref[a] from (f-4)'s own extremes pre-pass: the same weights),
 *     W_a = sum_n w_na,  p_na = w_na / W_a,
 * level-l block j covers the rows [j B 2^l, min(N, (j + 1) B 2^l)) -- the last block may be short and is kept -- and
 *     var[l][a][c]  = sum_j z_j^2,  z_j = sum_{n in block j} p_na (x[n][c] - mean[a][c])
 *     neff[a]       = W_a^2 / sum_n w_na^2                                 (Kish effective sample number)
 *     lnq[a]        = ln(W_a / N) - dalpha[a] uref[a] = ln < e^{-dalpha[a] u} >   (minus the free-energy difference)
 *     var_lnq[l][a] = sum_j (sum_{n in j} p_na - n_j / N)^2,  n_j the rows of block j
 * -- the infinitesimal-jackknife (first-order delta-method) variances of the ratio estimator of (f-4) and of lnq, with
 * time blocks as clusters when B > 1 (batch means: for a correlated series, B beyond its correlation time).  There is NO
 * nb / (nb - 1) factor: block = 1, level 0 is the iid  sum_n p_n^2 (x_n - m)^2  and  var_lnq = 1 / neff - 1 / N.
 * var [n_levels][n_alpha][C], neff [n_alpha], lnq [n_alpha], var_lnq [n_levels][n_alpha] are device arrays; dalpha_host
 * is a host array, n_alpha <= 8.  Levels with a single block are allowed and computed (block > N too: one block).
 * block == 1 && n_levels == 1 (iid): ONE pass in (f-4)'s layout, the n_alpha exponentials of a row shared between its
 * lanes, sum w, sum w^2 and sum (w (x - m))^2 in registers, per-workgroup partials added in a fixed order by a finalize;
 * nothing of size N is stored.  Otherwise (blocked): every level-0 block is summed by one workgroup in a fixed order, so
 * its bits do not depend on the launch width, into the workspace as [nb][n_alpha][C + 1] (the extra slot: sum_{n in b} w)
 * plus [nb][n_alpha][2] (sum w, sum w^2); a second kernel (a workgroup per (column, alpha)) adds W in a fixed order and
 * merges the pairs of the level below in place, level by level.  No floating-point atomics; two calls give the same bits.
 * A row whose weight underflows contributes zero.  First-order rounding bound with kappa_n = 1 + |dalpha (u_n - uref)|
 * (the exponent's rounding is the weight's relative error):  var: eps sum_j (sum_{n in j} p_n kappa_n |x_n - m|)^2,
 * var_lnq: eps sum_j (sum_{n in j} p_n kappa_n + n_j / N)^2, neff and lnq: eps kappa-bar (p-weighted mean) relative / absolute.
 * Workspace: txm_perturb_cov_ws_bytes, host logic, 0 for bad arguments: the pre-pass head, then iid  8 CUs workgroups x
 * (8 n_alpha (padded columns + 2)) bytes, blocked  8 nb n_alpha (C + 1) + 16 nb n_alpha  bytes with nb = ceil(N / block),
 * and 256 bytes.  Null pointers, N < 1, C outside [1, 65535], ldx_s < C, n_alpha outside [1, 8], block < 1 and n_levels
 * outside [1, 32] return TXM_ERR_INVALID, a short workspace TXM_ERR_WORKSPACE, all before anything is enqueued. */
size_t txm_perturb_cov_ws_bytes(int64_t N, int64_t C, int32_t n_alpha, int64_t block, int32_t n_levels);
int txm_perturb_cov(const double *x, int64_t ldx_s, const double *u, int64_t N, int64_t C,
                    const double *dalpha_host, int32_t n_alpha, const double *mean, int64_t block, int32_t n_levels,
                    double *var, double *neff, double *lnq, double *var_lnq, void *ws, size_t ws_bytes,
                    txm_stream stream);

/* ---- (f-16) timeseries: the lag sums of (f-7) for S states in one set of launches, the centred rows kept ---------- */
/* S states of C columns each, x row-major with ONE pitch ldx_s >= C, a record count PER STATE.  Two calls:
 *   txm_lag_rows_batched  centres and transposes all states in ONE launch (the state rides a grid axis; workgroups past a
 *       state's n leave at once) into the caller-held buffer `rows` of exactly txm_lag_rows_batched_bytes(n, S, C) bytes:
 *       a head of one 64-byte record per state, padded to 256 bytes -- n, ldd = 16 ceil(n / 16), the chunk length
 *       1008 ceil(n / (1008 * 512)), the chunk count, the row offset -- then per state [1 + C][ldd] contiguous rows of
 *       a - center, the very values (f-7)'s pre-pass writes: 8 (1 + C) sum_s ldd_s bytes.
 *   txm_lag_sums_batched  the lag sums of n_items (state, pair) items (pair as in (f-7); any order, any subset, a state as
 *       often as it has pairs listed) for the lags t0 .. t0 + nlags - 1, from the rows of the first call: one launch of
 *       the auto instance, one of the cross instance (each only if the kind occurs) and one chunk sum.  The item rides
 *       grid.y, grid.x is the largest chunk count among the listed states, workgroups past their state's chunk count leave
 *       at once.  out (device): [n_items][nlags].  `n_host` (HOST, [S]) must be the record counts the rows were made with.
 * The rows stay valid for any number of sums calls: a scan over lag blocks pays the centring pass once.
 * BITS: every state keeps the chunking of (f-7) for its own n, a workgroup's (chunk, pair, lag tile) work is the same
 * device function in both entry points, the four waves' tiles are added in wave order and the chunks in index order.  Row
 * i of `out` therefore equals txm_lag_sums(x_s, ldx_s, u_s, n_s, C, center_s, {pair_i}, 1, t0, nlags, ...) BIT FOR BIT,
 * whatever else is in the batch and however the items are cut into calls.  No floating-point atomics; two calls give the
 * same bits.
 * `states_host` and `items_host` are HOST arrays; the calls copy their tables into `rows` / `ws` (not stream-capturable).
 * Workspace of the sums call: txm_lag_sums_batched_ws_bytes = the item table (16 bytes per item, padded to 256) plus
 * 8 nlags sum_items chunks(n_state) bytes of partials -- per-item offsets, a prefix sum of the items' chunk counts, not
 * the largest chunk count for every item (1 MB per item and 256 lags at n = 1e6).  The *_bytes functions are host logic
 * and return 0 for bad arguments.
 * Null pointers, S outside [1, 65535], any n outside [1, 2^36], C outside [0, 16383], x == NULL with C > 0, ldx_s < C,
 * n_items outside [1, 65535], an item's state outside [0, S) or pair outside [0, 2 C], t0 not a multiple of 256, nlags not a
 * multiple of 256 in [256, 4096] and a rows_bytes other than txm_lag_rows_batched_bytes(n, S, C) return TXM_ERR_INVALID, a
 * short workspace TXM_ERR_WORKSPACE, all before anything is enqueued. */
typedef struct txm_lag_state {
  const double *x;      /* [n][ldx_s]; NULL iff C == 0 */
  const double *u;      /* [n] */
  const double *center; /* device, [1 + C]: <u>, <x_0> .. <x_{C-1}> */
  int64_t n;
} txm_lag_state;
typedef struct txm_lag_item {
  int32_t state;
  int32_t pair;
} txm_lag_item;
size_t txm_lag_rows_batched_bytes(const int64_t *n_host, int64_t S, int64_t C);
int txm_lag_rows_batched(const txm_lag_state *states_host, int64_t S, int64_t ldx_s, int64_t C, void *rows,
                         size_t rows_bytes, txm_stream stream);
size_t txm_lag_sums_batched_ws_bytes(const int64_t *n_host, int64_t S, int64_t C, const txm_lag_item *items_host,
                                     int64_t n_items, int32_t nlags);
int txm_lag_sums_batched(const void *rows, size_t rows_bytes, const int64_t *n_host, int64_t S, int64_t C,
                         const txm_lag_item *items_host, int64_t n_items, int64_t t0, int32_t nlags, double *out, void *ws,
                         size_t ws_bytes, txm_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* TXMOM_H */
