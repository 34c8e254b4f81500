// txm_resample.hip -- sample-level bootstrap of central comoments, the host side
// (cmomy.wrap_resample_vals as called from thermoextrap data.py:1803-1810,
// 1354-1366): the plans (workspace and pre-pass block layouts), the rules that choose a kernel, the size and path
// queries, and txm_resample_vals / txm_resample_vals_batched[_opts], which drive the five bootstrap kernels --
// the FP64 kernel and the finalize kernels (txm_resample_fp64.hip) and the int8 kernels (txm_resample_i8.hip, _i8t.hip,
// _i8g.hip, _i8gn.hip) behind the count-table generator (txm_count_table.hip).
#include <stdlib.h>

#include "txm_sampler.h"
#include "txm_pivot.h"
#include "txm_resample_fp64.h"
#include "txm_i8g.h"

namespace txm {

// tiles per sample chunk: ntiles / div chunks, at least 8 and at most 1024 of them (rounded to octets by the callers)
static int64_t resample_chunk_tiles(int64_t ntiles, int64_t div) {
  int64_t nc = ntiles / div;
  if (nc > 1024) nc = 1024;
  if (nc < 8) nc = 8;
  if (nc > ntiles) nc = ntiles;
  nc = cdiv(nc, 8) * 8;
  return cdiv(ntiles, nc);
}

static ResamplePlan plan_resample(int64_t N, int64_t C, int64_t nrep, int K) {
  ResamplePlan p;
  p.nblk = C <= 16 ? 1 : 2;
  p.colgroups = (int)cdiv(C, p.nblk * 16);
  p.C_pad = (int64_t)p.colgroups * p.nblk * 16;
  p.n_rbg = (int)cdiv(nrep, RS_WAVES * RS_REPS);
  p.nrep_pad = (int64_t)p.n_rbg * RS_WAVES * RS_REPS;
  p.ntiles = cdiv(N, SM_T);
  // Sample chunks: their number is a function of N ALONE (ntiles / 2, between 8 and 1024).  A replicate's sums are formed
  // per chunk and the chunks are added in a fixed order by resample_finalize_kernel, so with a chunking that does not
  // look at nrep (it used to: "enough workgroups to fill the chip") the rows [a, b) of a bootstrap equal the (b - a)-
  // replicate call with rep0 = a BIT FOR BIT on this kernel too, whatever the slab sizes (multi-GPU replicate slabs).
  p.tiles_per_chunk = resample_chunk_tiles(p.ntiles, 2);
  const int64_t nc = cdiv(cdiv(p.ntiles, p.tiles_per_chunk), 8) * 8;
  p.n_chunks = (int)nc;
  p.off_pivot = 0;
  p.off_px = align_up((size_t)(1 + C) * sizeof(double), 256);
  p.off_pu = p.off_px + align_up((size_t)p.n_chunks * p.nrep_pad * p.C_pad * K * sizeof(double), 256);
  p.off_prog = p.off_pu + align_up((size_t)p.n_chunks * p.nrep_pad * K * sizeof(double), 256);
  p.prog_bytes = (size_t)p.n_chunks * p.colgroups * 64 * sizeof(uint32_t);
  p.total = p.off_prog + align_up(p.prog_bytes, 256);
  return p;
}

// What one state point of the int8 path owns, as offsets: its four pre-pass tables (p_*, inside a pre-pass block: the
// workspace's or the caller's) and its scratch block (s_*, inside the workspace).  A single call has one such pair per
// call (its column groups share the scratch and have a set of tables each), a batched call one per state.
struct I8StateLayout {
  size_t stride, s_px, s_pu, s_fbx, s_fbu, s_stats;     // a state's scratch block in the workspace
  size_t p_stride, p_wt, p_flag, p_list, p_nlist;       // a state's pre-pass block (workspace, or the caller's prep buffer)
};

// int8-sliced path (txm_resample_i8.hip): 64 replicates x all columns per workgroup,
// chunks of whole scaling windows, one workgroup per CU.
struct I8Plan {
  int n_rbg, n_chunks, ngroups;
  int64_t tiles_per_chunk, nrep_pad, ntiles, nwin, win_tiles;
  size_t total;
  // precision-guard fallback: the FP64 kernel's plan / partial sums for one column group
  int sub_tiles;
  size_t off_prog, prog_bytes, off_prep;
  // the per-sample count table of the call's replicates (txm_count_table.hip; wide states: the contraction kernel without a
  // sampler inside, txm_resample_i8g.hip) -- 0 bytes for shapes that never take that kernel
  size_t off_table, table_bytes, off_gprog, total_table;  // (+ sixteen progress words per window: the L2-sharing hint of that kernel)
  // second sample matrix (txm_resample_opts.y) carried by the int8 kernel: its per-window partial sums, the FP64
  // fallback's sums for it, the sums themselves [nrep][C] (2 doubles each) and its pre-pass tables inside the prep block
  size_t off_py, off_fby, prep_ypiv, prep_ywt, prep_yflag;
  // the pre-pass block ("prep": what depends on the data and the shape, not on the sampler):
  //   [pivot (1 + C)] then per 32-column group [window table | guard flags | fallback run list | n_list (256 B)]
  size_t prep_group0, prep_group_stride, prep_total;
  I8StateLayout L;  // the tables of one group (p_*) and the call's scratch (s_*, rows of I8_CPAD columns) at the head of the workspace
  ResamplePlan fb;
};

// window table | guard flags | fallback run list | n_list (256 B); p_stride = their end
static void i8_layout_tables(const I8Plan &p, I8StateLayout &L) {
  L.p_wt = 0;
  L.p_flag = L.p_wt + align_up((size_t)p.nwin * I8_WT_STRIDE * sizeof(double) + 2048, 256);  // + timing slots of debug builds
  L.p_list = L.p_flag + align_up((size_t)p.nwin * sizeof(uint32_t), 256);
  L.p_nlist = L.p_list + align_up((size_t)p.nwin * (size_t)(p.win_tiles / p.sub_tiles) * sizeof(uint32_t), 256);
  L.p_stride = L.p_nlist + 256;
}
// per-window slots of x (rows of cpad columns) and of the u row | the FP64 fallback's sums | prog_bytes of progress words
// (single call; their offset is returned) | the pre-pass statistics; stride = their end.  Needs p.fb.
static size_t i8_layout_scratch(const I8Plan &p, int K, int cpad, size_t prog_bytes, I8StateLayout &L) {
  L.s_px = 0;
  L.s_pu = L.s_px + align_up((size_t)p.nwin * p.nrep_pad * K * 8 * cpad * sizeof(double), 256);
  L.s_fbx = L.s_pu + align_up((size_t)p.nwin * p.nrep_pad * K * 8 * sizeof(double), 256);
  L.s_fbu = L.s_fbx + align_up((size_t)p.fb.n_chunks * p.fb.nrep_pad * p.fb.C_pad * K * sizeof(double), 256);
  const size_t prog = L.s_fbu + align_up((size_t)p.fb.n_chunks * p.fb.nrep_pad * (K + 1) * sizeof(double), 256);  // + the y run's
  L.s_stats = prog + align_up(prog_bytes, 256);
  L.stride = L.s_stats + align_up((size_t)cdiv(p.ntiles, p.win_tiles < 16 ? p.win_tiles : 16) * 100 * sizeof(double), 256);
  return prog;
}

static I8Plan plan_i8(int64_t N, int64_t C, int64_t nrep, int K) {
  I8Plan p;
  p.n_rbg = (int)cdiv(nrep, I8_REPS);
  p.nrep_pad = (int64_t)p.n_rbg * I8_REPS;
  p.ntiles = cdiv(N, SM_T);
  p.ngroups = (int)cdiv(C, I8_CPAD);
  // scaling window = the slot of the partial sums: 256 tiles (262144 samples) on long series, shorter on short ones.
  // A function of N ALONE: the window decides the fixed-point scale of every monomial and the order of the final
  // summation, so a replicate's bits must not depend on nrep / the chunking (txm_sampler_spec.rep0: replicate slabs of
  // a multi-GPU run equal the one-GPU rows bit for bit).
  p.win_tiles = I8_WIN_TILES;
  constexpr int WIN_MIN = 256;
  while (p.win_tiles > 4 && p.ntiles < WIN_MIN * p.win_tiles) p.win_tiles /= 4;  // >= 256 windows where N allows
  p.nwin = cdiv(p.ntiles, p.win_tiles);
  // one workgroup per CU: chunks (whole windows) x replicate groups should fill the CUs once, not 1.1 times
  int64_t nc = (int64_t)num_cus() / p.n_rbg / 8 * 8;
  if (nc < 8) nc = 8;
  if (nc > p.nwin) nc = cdiv(p.nwin, 8) * 8;
  p.tiles_per_chunk = cdiv(p.nwin, nc) * p.win_tiles;
  p.n_chunks = (int)(cdiv(cdiv(p.ntiles, p.tiles_per_chunk), 8) * 8);
  p.sub_tiles = p.win_tiles < I8_SUB_TILES ? (int)p.win_tiles : I8_SUB_TILES;
  p.fb = plan_resample(N, C < I8_CPAD ? C : I8_CPAD, nrep, K);
  p.prog_bytes = (size_t)p.n_chunks * 64 * sizeof(uint32_t);
  // prep block
  i8_layout_tables(p, p.L);
  p.prep_ywt = p.L.p_stride;
  p.prep_yflag = p.prep_ywt + align_up((size_t)p.nwin * I8_WT_STRIDE * sizeof(double), 256);
  p.prep_group_stride = p.prep_yflag + align_up((size_t)p.nwin * sizeof(uint32_t), 256);
  p.prep_ypiv = align_up((size_t)(1 + C) * sizeof(double), 256);
  p.prep_group0 = 2 * p.prep_ypiv;
  p.prep_total = p.prep_group0 + (size_t)p.ngroups * p.prep_group_stride;
  // workspace
  p.off_prog = i8_layout_scratch(p, K, I8_CPAD, p.prog_bytes, p.L);
  p.off_py = p.L.stride;
  p.off_fby = p.off_py + align_up((size_t)p.nwin * p.nrep_pad * 8 * I8_CPAD * sizeof(double), 256);
  p.off_prep = p.off_fby + align_up((size_t)p.fb.n_chunks * p.fb.nrep_pad * p.fb.C_pad * sizeof(double), 256);
  // the count table sits LAST: `total` is the size without it, `total_table` with it -- a call runs the table kernel when
  // the rule (table_kernel_pays) or the caller asks for it AND the workspace it was given reaches total_table
  p.off_gprog = p.off_prep + align_up(p.prep_total, 256);
  p.off_table = p.off_gprog + align_up((size_t)cdiv(p.nwin, 8) * 8 * 16 * sizeof(uint32_t), 256);
  // (narrow states -- C <= 16, order >= 1 -- have a table-fed kernel of their own since round 6: txm_resample_i8gn.hip)
  p.table_bytes = (N >= SM_T && (C > 16 || K >= 2)) ? count_table_bytes(p.ntiles, nrep) : 0;
  p.total = p.off_table;
  p.total_table = p.off_table + align_up(p.table_bytes, 256);
  return p;
}

// the process-wide default of TXM_PATH_AUTO calls (txm_set_resample_path; tests and A/B timing): -1 = the shape rule
// below, TXM_PATH_FP64 / TXM_PATH_INT8 = forced wherever the kernel supports the shape.  No environment variable is read
// anywhere in the library (rounds 1-4 read TXM_I8 / TXM_THROTTLE / TXM_PACK / TXM_I8W); a call that passes
// txm_resample_opts.path does not look at this word either.
static int g_path_override = -1;
static int path_override() { return g_path_override; }
// the path of a call that passes `call_path` (idempotent: an effective path maps to itself)
static int effective_path(int call_path) { return call_path != TXM_PATH_AUTO ? call_path : path_override(); }
// a path word other than TXM_PATH_AUTO
static bool is_path(int path) {
  return path == TXM_PATH_FP64 || path == TXM_PATH_INT8 || path == TXM_PATH_INT8_FUSED || path == TXM_PATH_INT8_TABLE;
}
// what every size and path query answers 0 / TXM_PATH_FP64 on, and every call refuses
static bool shape_ok(int64_t N, int64_t C, int64_t nrep, int order) {
  return N >= 1 && C >= 1 && nrep >= 1 && order >= 0 && order <= TXM_MAX_ORDER;
}

// Wide states on the int8 path: which of its two contraction kernels.  They agree bit for bit (the same int32 sums, the same
// flush), so this is a rule on speed alone -- measured on MI355X, pre-pass block kept, ms per call fused / table
// (tools/i8g_sweep.py, profiles/r05_sweep.txt; N = 1e8, C = 32, nrep = 1000):
//   order 0: 92.5 / 74.1   1: 95.1 / 82.9   2: 115.8 / 99.3   3: 134.2 / 137.2   4: 162.8 / 162.7   5: 231.7 / 174.0
//   6: 259.9 / 217.7   7: 268.2 / 226.4;   with a second matrix (N = 1e7, nrep = 256): order 1: 4.47 / 3.94, 4: 8.36 / 5.97,
//   6: 8.79 / 7.58.
// The table kernel takes at most three row sets per pass and pays the count-table generator (28 ms per 1e11 counts) once per
// call; every call with a second matrix and every order but 3 is faster on it.  Orders 3 and 4 -- four and five row sets, two
// passes against the fused kernel's one -- were ties on the kernel's first cut; after its re-cut (reads a slot ahead, no
// spills; same box, fused / table, profiles/r05_orders34_ab.txt): order 4 168.3 / 163.2 (N = 1e8, nrep = 1000), 37.0 / 35.5
// (2e7), 6.2 / 5.95 (1e7, nrep = 200), 1.55 / 1.42 (1e6, 384), 1.72 / 1.76 (3e6, 128); order 3 145.6 / 145.1, 31.8 / 31.9,
// 5.47 / 5.55, 1.47 / 1.56 -- order 4 moved to the table kernel; order 3 followed once its passes were split 3 + 1 (below).
// Replicates come in groups of 128 there, 64 on the fused kernel: a call whose padding to 128 wastes much more than its
// padding to 64 stays fused (nrep = 64: 1.80 / 2.66 ms; 130: 3.45 / 3.92; 100: 2.87 / 2.93; 200, 256, 1000: the table above).
static bool table_kernel_pays(int64_t nrep, int K, bool has_y) {
  const int64_t pad128 = cdiv(nrep, G_REPS) * G_REPS, pad64 = cdiv(nrep, I8_REPS) * I8_REPS;
  if (4 * pad128 > 5 * pad64) return false;
  if (has_y) return true;
  // order 4 is only ~3 % ahead on the table kernel, and one 128-replicate group is 382 workgroups per 1e8 samples -- 1.5 rounds of
  // the 256 CUs -- where two 64-replicate groups of the fused kernel are 3.0 (a 125-replicate slab, what one of 8 ranks runs in
  // bench.py --mode replicas: 22.6 ms fused, 24.4 table)
  // order 3 likewise since its four row sets go as 3 + 1 (the single-row-set pass takes 256 replicates per workgroup: 101 ms for
  // the two passes against 109 for 2 + 2): 142.2 / 150.1 ms table / fused at N = 1e8, 31.1 / 32.7 at 2e7, 5.4 / 5.5 at 1e7 x 200,
  // 1.27 / 1.32 at 1e6 x 384, 1.59 / 1.50 at 3e6 x 128 (profiles/r05_pass_split_ab.txt)
  if (K == 4 || K == 5) return pad128 >= 2 * G_REPS;
  return true;
}

// ONE statement of "does this call run the count-table kernel" for the call itself, the workspace query and
// txm_resample_kernel (what the host keys a kept pre-pass block on): `eff` is the call's path after the process-wide
// override, `applicable` = i8g_applicable() of the operands.  The call additionally needs the table's bytes in its workspace.
// Narrow states (C <= 16): the table-fed kernel of txm_resample_i8gn.hip (128 replicates per workgroup, no fill phase) against the
// quad-sharing variant of the kernel that draws in place -- bit for bit the same sums, so again a rule on speed alone.  Measured on
// MI355X (tools/narrow_table_sweep.py: N = 1e6 .. 3e7, C = 4 .. 16, orders 1 .. 6, 64 .. 1000 replicates), fused ms / table ms:
//   first sweep (profiles/r06_narrow_table_sweep.txt): 0.6 - 0.9 at 64 replicates (the padding to 128 doubles the work), 0.9 - 1.2
//   with ONE group of 128, 1.0 - 1.27 from two groups on -- the rule took the table kernel there for every long series.
//   Re-swept twice in round 6's second session, because both kernels' window boundary got cheaper in turn:
//   (profiles/r06_narrow_table_sweep2.txt, _sweep3.txt) after the FUSED kernel's chunk groups got their cheaper flush and digit-summed
//   slots (6 % faster at the median, 12 % on short series whose windows are four tiles): from two groups on the two kernels were within
//   +- 5 % on most shapes, the table kernel clearly ahead only on long series at some orders -- a rule of four cases followed;
//   (profiles/r06_narrow_table_sweep4.txt: 560 shapes, N = 1e6, 3e6, 4.5e6, 1e7) after the TABLE kernel got digit-summed slots too
//   (one workgroup per window: a short series' call wrote and re-read as many bytes of per-digit slots as of counts): 0.65 - 1.04 at
//   64 replicates, 0.91 - 1.33 with ONE group of 128 (100, 128 replicates: below 1 only for low orders of the widest states around
//   N = 4.5e6), 0.92 - 1.40 from two groups on (median 1.10; N = 1e6: 0.95 - 1.38) -- four column quads at order 4 included (1e6:
//   1.15 - 1.36, 1e7: 0.96 - 1.11).  A one-line rule followed (mean regret 0.5 % on that sweep; the four-case rule: 6.3 %);
//   (profiles/r06_narrow_table_sweep5.txt: 420 shapes) after the fused instances WITHOUT chunk groups got digit-summed slots as well:
//   four column quads at order 4 -- one fused pass against two table passes -- 16 - 19 % faster on the fused kernel, 0.88 - 1.05 now:
//   the exception of the first rule is back.  The rule below picks the slower kernel by more than 3 % on 19 of the 420 shapes (worst
//   10 %), mean regret 0.4 %.
static bool narrow_table_pays(int64_t N, int64_t C, int64_t nrep, int K) {
  const int64_t pad128 = cdiv(nrep, G_REPS) * G_REPS, pad64 = cdiv(nrep, I8_REPS) * I8_REPS;
  if (N < 786432 || nrep <= I8_REPS || pad128 > pad64) return false;
  return !(i8t_narrow_nq(C, K) == 4 && K == 5);
}
static bool table_call_rule(size_t table_bytes, int eff, int64_t N, int64_t C, int64_t nrep, int K, bool has_y, bool applicable) {
  if (eff == TXM_PATH_FP64 || eff == TXM_PATH_INT8_FUSED || table_bytes == 0 || !applicable) return false;
  if (eff == TXM_PATH_INT8_TABLE) return true;
  return C > 16 ? table_kernel_pays(nrep, K, has_y) : narrow_table_pays(N, C, nrep, K);
}
// ... and of "does that kernel carry the second matrix": the wide table kernel always, the fused one where it has the row set
struct I8KernelChoice { bool table_call, with_y; };
static I8KernelChoice i8_kernel_choice(const I8Plan &q, int eff, int64_t N, int64_t C, int64_t nrep, int K, bool has_y, bool applicable) {
  const bool table = table_call_rule(q.table_bytes, eff, N, C, nrep, K, has_y, applicable);
  return {table, has_y && ((table && C > 16) || i8t_carries_y(C, K))};
}
// what the table-fed kernels ask of the operands (16-byte LDS-DMA pieces): wide states txm_resample_i8g.hip, narrow ones
// txm_resample_i8gn.hip (a second matrix never rides a narrow call: it is bootstrapped on its own)
static bool table_operands_ok(const double *x, int64_t ldx_s, int64_t C, int K, const double *y, int64_t ldy_s) {
  return C > 16 ? i8g_applicable(x, ldx_s, C, y, ldy_s) : i8gn_applicable(x, ldx_s, C, K);
}

static bool use_i8(int64_t N, int64_t C, int64_t nrep, int K, int call_path = TXM_PATH_AUTO) {
  if (!i8_supported(N, C, nrep, K)) return false;
  const int ov = effective_path(call_path);
  if (ov == TXM_PATH_FP64) return false;
  if (ov == TXM_PATH_INT8 || ov == TXM_PATH_INT8_FUSED || ov == TXM_PATH_INT8_TABLE) return true;
  // measured on MI355X (tools/i8_sweep.py, N = 1e7; tools/ab_order.py, N = 1e8): C <= 16 runs one 16-column FP64
  // block and stays ahead; with two blocks the int8 kernel wins from one full replicate group on at order >= 3
  // (order 4: 1.2x at 64 replicates, 1.5x at 128, 1.6x from 400), from 128 replicates at orders 1 and 2 (nrep = 128:
  // 25 vs 32 ms and 29 vs 43 ms; nrep = 1000: 157 vs 254 ms and 181 vs 342 ms) and from ~400 at order 0 (nrep = 200:
  // a tie; 400: 74 vs 80 ms; 1000: 151 vs 176 ms) -- round 3's numbers; the long-series thresholds below are round 4's re-measurement.
  // Narrow states (C <= 16, order >= 1: the quad-sharing variant of the transposing-read kernel with chunk groups, round 4):
  // ahead of the power-packed FP64 kernel at EVERY replicate count from 4 to 200 once the series is long (tools/
  // i8_sweep_narrow.py, N = 1e7, C = 1 .. 16, orders 1 .. 4: 1.5 - 2.4 x with the pre-pass block kept by the data object,
  // 0.93 - 2.1 x on a first call that computes it; profiles/r04_narrow_sweep.txt).  On short series the pre-pass weighs more:
  // N = 3e5: 1.05 - 1.6 x kept, 0.6 - 1.2 x on the first call, ahead on both from 128 replicates.  A rule on (N, nrep) that a
  // replicate slab of a long series never crosses: from 3 x 2^18 samples every slab takes the kernel the whole call takes
  // (N = 1e6: 1.2 - 1.35 x on the first call, 1.9 x kept).
  if (C <= 16) return K >= 2 && (N >= 786432 || (N >= 262144 && nrep >= 128));
  // Wide states, re-measured in round 4 (tools/i8_sweep_narrow.py 1e7 32 ..., profiles/r04_narrow_sweep.txt; pre-pass block kept /
  // first call): N = 1e7, order 4: 2.1 / 1.4 x at 32 replicates, 2.4 / 1.9 at 100; orders 1-2: 1.8-1.9 / 1.0-1.15 at 32, 2.1-2.25 /
  // 1.4-1.6 at 100; order 0: 1.4-1.7 x kept at every count, but a first call only pays from 100 replicates (1.03; 0.72 at 64).
  // N = 3e5: ahead on a first call from 128 replicates only (order 4: 1.17, order 1: 0.86).
  // (a tail group of <= 16 columns runs the narrow-state variant; at order 0, which has none, such a call stays on the FP64 kernel)
  const int64_t ctail = C % I8_CPAD;
  const bool long_series = N >= 786432;
  const int64_t min_rep = long_series ? (K >= 2 ? 32 : 100) : (K >= 4 ? 64 : (K >= 2 ? 128 : 384));  // (short series: round 3's rule)
  return C > 16 && (ctail == 0 || ctail > 16 || K >= 2) && nrep >= min_rep && N >= 262144;
}

}  // namespace txm

using namespace txm;

extern "C" int txm_set_resample_path(int path) {
  TXM_REQUIRE(path == -1 || is_path(path), "set_resample_path: %d is not a path", path);
  g_path_override = path;
  return TXM_OK;
}

namespace txm {
// info [4] on the device: path, windows x groups, windows the guard sent to the FP64 kernel, tables came from prep
__global__ void i8_info_kernel(const unsigned char *prep_groups, size_t group_stride, size_t off_nlist, int ngroups,
                               int64_t nwin, int from_prep, int64_t *info) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    int64_t flagged = 0;
    for (int g = 0; g < ngroups; ++g)
      flagged += reinterpret_cast<const uint32_t *>(prep_groups + (size_t)g * group_stride + off_nlist)[1];
    info[0] = TXM_PATH_INT8;
    info[1] = nwin * ngroups;
    info[2] = flagged;
    info[3] = from_prep;  // bit 0: tables came from the caller's block; bit 1: wide groups ran the count-table kernel
  }
}
__global__ void fp64_info_kernel(int64_t *info) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    info[0] = TXM_PATH_FP64;
    info[1] = info[2] = info[3] = 0;
  }
}
}  // namespace txm
using namespace txm;

extern "C" int txm_resample_vals_info(const void *ws, int64_t N, int64_t C, int64_t nrep, int order,
                                      int64_t *info_host, txm_stream stream) {
  TXM_REQUIRE(ws && info_host, "resample_vals_info: null pointer");
  TXM_REQUIRE(shape_ok(N, C, nrep, order), "resample_vals_info: bad shape");
  info_host[0] = TXM_PATH_FP64;
  info_host[1] = info_host[2] = 0;
  if (!use_i8(N, C, nrep, order + 1)) return TXM_OK;
  const I8Plan q = plan_i8(N, C, nrep, order + 1);
  // the last call's info block sits at the head of the workspace's own prep region's n_list words; read them back
  int64_t flagged = 0;
  for (int g = 0; g < q.ngroups; ++g) {
    uint32_t nl[2] = {0, 0};
    TXM_HIP(hipMemcpyAsync(nl, (const char *)ws + q.off_prep + q.prep_group0 + (size_t)g * q.prep_group_stride + q.L.p_nlist,
                           sizeof(nl), hipMemcpyDeviceToHost, (hipStream_t)stream));
    TXM_HIP(hipStreamSynchronize((hipStream_t)stream));
    flagged += nl[1];
  }
  info_host[0] = TXM_PATH_INT8;
  info_host[1] = q.nwin * q.ngroups;
  info_host[2] = flagged;
  return TXM_OK;
}

extern "C" int txm_resample_path(int64_t N, int64_t C, int64_t nrep, int order) {
  if (!shape_ok(N, C, nrep, order)) return TXM_PATH_FP64;
  return use_i8(N, C, nrep, order + 1) ? TXM_PATH_INT8 : TXM_PATH_FP64;
}

// The contraction kernel ONE device-sampler call with these options runs -- TXM_PATH_FP64, TXM_PATH_INT8_FUSED or
// TXM_PATH_INT8_TABLE -- given a workspace of txm_resample_vals_ws_bytes_opts(same arguments) bytes, | TXM_KERNEL_WITH_Y when
// that kernel carries the second matrix (so that the call's pre-pass block holds y's pivot, scales and guard flags).
// `aligned`: x (and y) 16-byte aligned with an even row pitch >= C rounded up to 4 -- what the table kernel's DMA needs.
// A kept pre-pass block serves exactly the calls that return the same word here (and the same N, C, order, tensors).
extern "C" int txm_resample_kernel(int64_t N, int64_t C, int64_t nrep, int order, int path, int has_y, int aligned) {
  if (!shape_ok(N, C, nrep, order)) return TXM_PATH_FP64;
  const int K = order + 1;
  if (!use_i8(N, C, nrep, K, path)) return TXM_PATH_FP64;
  const I8Plan q = plan_i8(N, C, nrep, K);
  const I8KernelChoice k = i8_kernel_choice(q, effective_path(path), N, C, nrep, K, has_y != 0, aligned != 0);
  return (k.table_call ? TXM_PATH_INT8_TABLE : TXM_PATH_INT8_FUSED) | (k.with_y ? TXM_KERNEL_WITH_Y : 0);
}

// the `aligned` argument of txm_resample_kernel for a given pair of operands (y may be NULL): what the count-table kernel's
// LDS-DMA asks of them -- ONE statement of it, the one the call itself applies (i8g_applicable)
extern "C" int txm_resample_operands_aligned(const double *x, int64_t ldx_s, int64_t C, const double *y, int64_t ldy_s) {
  if (x == nullptr || C < 1) return 0;
  return table_operands_ok(x, ldx_s, C, 2, y, ldy_s) ? 1 : 0;  // (K only decides whether a narrow shape is served at all: txm_resample_kernel's business)
}

// (host only, not part of the public header: the workgroup widths of a two-row-set table pass over Q replicate quarters, for the
// tests of the rule -- n6 six-quarter workgroups, then n4 four-quarter ones from quarter 6 n6 on)
extern "C" void txm_i8g_quarter_split(int Q, int *n6, int *n4) { g_quarter_split(Q, n6, n4); }

extern "C" size_t txm_resample_prep_bytes(int64_t N, int64_t C, int64_t nrep, int order) {
  if (!shape_ok(N, C, nrep, order)) return 0;
  if (!i8_supported(N, C, nrep, order + 1)) return 256;
  return plan_i8(N, C, nrep, order + 1).prep_total;
}

// path / has_y: what the call will pass in txm_resample_opts -- they decide whether the int8 path's count table (one byte
// per replicate and sample, replicates padded to 128) is part of the workspace: TXM_PATH_AUTO / TXM_PATH_INT8 follow the
// library's rule (table_kernel_pays), TXM_PATH_INT8_TABLE always asks for it, TXM_PATH_FP64 / _INT8_FUSED never.  A call
// handed less than this runs the kernel without the table.
extern "C" size_t txm_resample_vals_ws_bytes_opts(int64_t N, int64_t C, int64_t nrep, int order, int path, int has_y) {
  if (!shape_ok(N, C, nrep, order)) return 0;
  size_t n = plan_resample(N, C, nrep, order + 1).total;
  if (i8_supported(N, C, nrep, order + 1)) {
    const I8Plan q = plan_i8(N, C, nrep, order + 1);
    const bool table = table_call_rule(q.table_bytes, effective_path(path), N, C, nrep, order + 1, has_y != 0, true);
    const size_t m = table ? q.total_table : q.total;
    if (m > n) n = m;
  }
  return align_up(n, 256);
}

extern "C" size_t txm_resample_vals_ws_bytes(int64_t N, int64_t C, int64_t nrep, int order) {
  return txm_resample_vals_ws_bytes_opts(N, C, nrep, order, TXM_PATH_AUTO, 0);
}

// the second sample matrix of txm_resample_opts (y -> per-replicate means) runs as an order-0 bootstrap of its own
// behind the main call unless the kernel of the main call carries it: its states [nrep][C][2][1] and its own
// workspace sit behind the main plan's
// (the order-0 pass: the larger of the two paths' plans, never the count table)
static size_t y_main_bytes(int64_t N, int64_t C, int64_t nrep) { return txm_resample_vals_ws_bytes_opts(N, C, nrep, 0, TXM_PATH_INT8_FUSED, 0); }
static size_t y_extra_bytes(int64_t N, int64_t C, int64_t nrep) {
  return align_up((size_t)nrep * C * 2 * sizeof(double), 256) + y_main_bytes(N, C, nrep);
}

// ... and the scratch a call with opts.y needs BEHIND those bytes when the kernel of the main call does not carry the
// second matrix (an order-0 bootstrap of its own: its states and its plan).  Opt-in: at the north-star shape it is
// ~2 GB that a call without opts.y never touches.
extern "C" size_t txm_resample_y_ws_bytes(int64_t N, int64_t C, int64_t nrep) {
  if (N < 1 || C < 1 || nrep < 1) return 0;
  return y_extra_bytes(N, C, nrep);
}

// whether the int8 kernel can take the shape at all (TXM_PATH_INT8 on a shape it cannot take runs the FP64 kernel)
extern "C" int txm_resample_i8_supported(int64_t N, int64_t C, int64_t nrep, int order) {
  if (!shape_ok(N, C, nrep, order)) return 0;
  return i8_supported(N, C, nrep, order + 1) ? 1 : 0;
}

namespace txm {
// y[N][C] -> the mean column of its order-0 replicate states
__global__ void y_means_kernel(const double *__restrict__ st /*[n][2]*/, int64_t n, double *__restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) out[e] = st[2 * e + 1];
}

// ---- one description of a call and the steps every call is made of -----------------------------------------------------
// What txm_resample_vals / txm_resample_vals_batched_opts resolve from their arguments, once.
struct ResampleCall {
  const char *fn = "resample_vals";                   // the entry point's name in error texts
  const double *x = nullptr, *u = nullptr, *w = nullptr;  // operands of a single call ...
  const txm_state_ptrs *states_host = nullptr;        // ... or the S states of a batched one
  int64_t S = 1, ldx_s = 0, N = 0, C = 0, nrep = 0;   // nrep: replicates per state
  int K = 1;
  bool weighted = false;
  const int64_t *freq = nullptr;                      // explicit table, or the sampler's spec and tile counts
  const txm_sampler_spec *spec = nullptr;
  const uint32_t *counts = nullptr;
  const double *pivot = nullptr;                      // the caller's, nullptr: computed
  double *out = nullptr;
  int path = TXM_PATH_AUTO;                           // the options, resolved (take_opts): the EFFECTIVE path, ...
  void *prep = nullptr;
  size_t prep_bytes = 0, ws_bytes = 0;
  bool prep_valid = false;
  int64_t *info = nullptr, ldy_s = 0;
  const double *y = nullptr;
  double *out_y = nullptr;
  void *ws = nullptr;
  hipStream_t st = nullptr;
  bool explicit_() const { return freq != nullptr; }
  bool batched() const { return states_host != nullptr; }
};

static int check_pitch(const char *fn, const char *operand, int64_t ld, int64_t C) {
  if (TXM_RESAMPLE_PITCH_OK(ld, C)) return TXM_OK;  // else the kernels' 32-bit lane offsets would wrap
  set_error("%s: row pitch %sld%s_s = %lld with C = %lld columns exceeds the limit 768 * ld%s_s + C <= 2^29 = 536870912 (32-bit byte offsets inside a sampler tile); copy %s to a tighter array",
            fn, operand[0] == 'y' ? "opts." : "", operand, (long long)ld, (long long)C, operand, operand);
  return TXM_ERR_UNSUPPORTED;
}
// the options of a call (NULL: the defaults): the path word is checked, then resolved
static int take_opts(ResampleCall &c, const txm_resample_opts *opts) {
  const int path = opts ? (int)opts->path : TXM_PATH_AUTO;
  TXM_REQUIRE(path == TXM_PATH_AUTO || is_path(path), "%s: opts.path %d is not a path", c.fn, path);
  c.path = effective_path(path);
  if (opts == nullptr) return TXM_OK;
  c.prep = opts->prep; c.prep_bytes = opts->prep_bytes; c.prep_valid = opts->prep_valid != 0; c.info = opts->info;
  c.y = opts->y; c.ldy_s = opts->ldy_s; c.out_y = opts->out_y;
  return TXM_OK;
}
static int check_workspace(const char *fn, size_t have, size_t need) {
  if (have >= need) return TXM_OK;
  set_error("%s: workspace too small (%zu < %zu)", fn, have, need);
  return TXM_ERR_WORKSPACE;
}
// the sampler of a call spans its S * nrep replicates of N samples (the two entry points word it differently)
static int check_sampler(const ResampleCall &c) {
  const int64_t nrep = c.S * c.nrep;
  TXM_REQUIRE(c.spec->ndat == c.N && c.spec->nrep == nrep, "%s", c.batched() ? "resample_vals_batched: the sampler must span S * nrep replicates of N samples"
                                                                           : "resample_vals: sampler spec does not match N/nrep");
  TXM_REQUIRE(c.spec->rep0 >= 0 && c.spec->rep0 + nrep <= ((int64_t)1 << 32), "%s", c.batched() ? "resample_vals_batched: sampler replicates outside [0, 2^32)"
                                                                                             : "resample_vals: sampler rep0 out of range");
  return TXM_OK;
}
// the pre-pass block: the caller's persistent buffer (tables reused when prep_valid) or scratch in ws
static int bind_prep(const ResampleCall &c, size_t need, unsigned char *&pb, bool &have_tables) {
  have_tables = false;
  if (c.prep == nullptr) return TXM_OK;
  if (c.prep_bytes < need) {
    set_error("%s: prep buffer too small (%zu < %zu)", c.fn, c.prep_bytes, need);
    return TXM_ERR_WORKSPACE;
  }
  pb = (unsigned char *)c.prep;
  have_tables = c.prep_valid;
  return TXM_OK;
}
// piv[1 + C] = the caller's pivot, or the one pivot_kernel computes from (x, u)
static int fill_pivot(const double *given, const double *x, int64_t ldx_s, const ResampleCall &c, double *piv) {
  if (given) {
    TXM_HIP(hipMemcpyAsync(piv, given, sizeof(double) * (size_t)(1 + c.C), hipMemcpyDeviceToDevice, c.st));
  } else {
    hipLaunchKernelGGL(pivot_kernel, dim3((unsigned)(1 + c.C)), dim3(256), 0, c.st, x, ldx_s, (int64_t)1, c.u, (int64_t)1, c.N, piv);
    TXM_LAUNCH_CHECK();
  }
  return TXM_OK;
}
// the sampler words of the kernels' arguments (an explicit table: zeros)
struct SamplerWords { uint32_t k0 = 0, k1 = 0, rep_base = 0; };
static SamplerWords sampler_words(const ResampleCall &c) {
  if (c.explicit_()) return {};
  return {(uint32_t)c.spec->seed, (uint32_t)(c.spec->seed >> 32), (uint32_t)c.spec->rep0};
}
static uint32_t last_tile_size(int64_t N, int64_t ntiles) { return (uint32_t)(N - (ntiles - 1) * SM_T); }

// THE fill of the FP64 kernel's arguments: plan, operands, sampler, partial-sum pointers.  Whatever a launch mode adds
// (progress words, fallback lists, a state table) the caller sets on top; the rest stays null / zero.
static ResampleArgs fp64_args(const ResampleCall &c, const ResamplePlan &p, const double *piv, double *part_x, double *part_u) {
  const SamplerWords s = sampler_words(c);
  ResampleArgs a;
  a.x = c.x; a.ldx_s = c.ldx_s; a.u = c.u; a.w = c.w; a.N = c.N; a.C = c.C; a.nrep = c.nrep;
  a.freq = c.freq; a.counts = c.counts;
  a.k0 = s.k0; a.k1 = s.k1; a.rep_base = s.rep_base;
  a.ntiles = p.ntiles;
  a.last_tile_size = last_tile_size(c.N, p.ntiles);
  a.pivot = piv;
  a.part_x = part_x;
  a.part_u = part_u;
  a.n_chunks = p.n_chunks; a.n_rbg = p.n_rbg; a.tiles_per_chunk = p.tiles_per_chunk;
  a.nrep_pad = p.nrep_pad; a.C_pad = p.C_pad;
  return a;
}
// ... and of what the int8 kernels' arguments take from the call and the state's plan
static I8Args i8_args(const ResampleCall &c, const I8Plan &q, const double *piv) {
  const SamplerWords s = sampler_words(c);
  I8Args b;
  b.x = c.x; b.ldx_s = c.ldx_s; b.u = c.u; b.w = c.w; b.N = c.N; b.nrep = c.nrep; b.C_call = c.C;
  b.counts = c.counts;
  b.k0 = s.k0; b.k1 = s.k1; b.rep_base = s.rep_base;
  b.ntiles = q.ntiles;
  b.last_tile_size = last_tile_size(c.N, q.ntiles);
  b.pivot = piv;
  b.nwin = q.nwin;
  b.n_rbg = q.n_rbg;
  b.nrep_pad = q.nrep_pad;
  b.win_tiles = q.win_tiles;
  b.sub_tiles = q.sub_tiles;
  return b;
}

// ---- the int8 call ------------------------------------------------------------------------------------------------------
// What the column groups of a call share.
struct I8CallState {
  I8KernelChoice kernel;
  unsigned char *pb;       // the pre-pass block
  bool have_tables;        // ... holds the tables already
  bool have_table = false; // the count table of the call's replicates has been generated
};

// One group of 32 columns (they reuse the partial buffers): pre-pass, contraction kernel (one launch, or two at orders 5-7),
// the FP64 kernel in listed mode on the windows the precision guard flags (none on ordinary data), finalize -- then the
// last two for the second matrix where the group's last pass carried it.  b, f: the call's arguments, completed here.
static int resample_i8_group(const ResampleCall &c, const I8Plan &q, I8CallState &cs, int g, I8Args b, ResampleArgs f) {
  const int K = c.K;
  const int64_t C = c.C, nrep = c.nrep, col0 = (int64_t)g * I8_CPAD;
  hipStream_t st = c.st;
  unsigned char *pg = cs.pb + q.prep_group0 + (size_t)g * q.prep_group_stride;
  b.wtab = (double *)(pg + q.L.p_wt);
  b.wflag = (uint32_t *)(pg + q.L.p_flag);
  b.list = (uint32_t *)(pg + q.L.p_list);
  b.n_list = (uint32_t *)(pg + q.L.p_nlist);
  b.ywtab = (double *)(pg + q.prep_ywt);
  b.yflag = (uint32_t *)(pg + q.prep_yflag);
  f.list = b.list; f.n_list = b.n_list;
  b.col0 = col0;
  b.C = C - col0 < I8_CPAD ? C - col0 : I8_CPAD;
  // a tail group of <= 16 columns behind full groups runs the narrow-state variant (its own partial-sum row width) --
  // unless a second matrix rides on the pass, which only the wide variant carries
  const bool narrow_tail = C > I8_CPAD && b.C <= 16 && K >= 2 && !cs.kernel.with_y;
  b.C_call = narrow_tail ? b.C : C;
  b.cpad = i8_cpad(b.C_call, K);
  if (!cs.have_tables)
    if (const int rc = launch_i8_prepass(b, K, st)) return rc;
  const bool table_kernel = cs.kernel.table_call && !narrow_tail;
  if (table_kernel) {
    unsigned char *table = (unsigned char *)c.ws + q.off_table;
    if (!cs.have_table) {
      if (const int rc = launch_count_table(c.counts, nrep, c.N, b.k0, b.k1, b.rep_base, 0, cdiv(nrep, G_REPS), table, st)) return rc;
      cs.have_table = true;
    }
    I8Args bg = b;
    bg.progress = nrep > G_REPS ? (uint32_t *)((char *)c.ws + q.off_gprog) : nullptr;
    if (const int rc = C > 16 ? launch_resample_i8g(bg, K, c.weighted, table, 0, (int)cdiv(nrep, G_REPS), st)
                              : launch_resample_i8gn(bg, K, c.weighted, table, 0, (int)cdiv(nrep, G_REPS), 0, st))
      return rc;
  } else {
    if (const int rc = launch_resample_i8(b, K, c.weighted, q.prog_bytes, st)) return rc;
  }
  f.x = c.x + col0; f.C = b.C; f.col_off = col0;
  if (const int rc = run_listed(f, q.fb, K, c.weighted, st)) return rc;
  // (the slots' layout: digit sums where the fused narrow kernel with chunk groups wrote them, per-digit slots otherwise)
  // (table-fed kernels: always -- txm_resample_i8gn.hip both x and u, txm_resample_i8g.hip x only; the fused kernel: its chunk-group instances)
  // the fused kernel: narrow instances always, the wide one unless a second matrix rides the call (its finalize reads per-digit u slots)
  const int fin_summed = table_kernel ? (C <= 16 ? 1 : 2)
                                      : (i8t_narrow_nq(b.C_call, K) != 0 ? (i8t_partials_summed(b.C_call, K) ? 1 : 0) : b.part_summed);
  if (const int rc = launch_finalize_i8(b, f, K, fin_summed, c.out, C, st)) return rc;
  if (!cs.kernel.with_y) return TXM_OK;
  // the windows the guard flagged (for either matrix): the FP64 kernel in listed mode on y, order 0
  ResampleArgs fy = f;
  fy.x = c.y + col0; fy.ldx_s = c.ldy_s; fy.pivot = b.ypivot;
  fy.part_x = (double *)((char *)c.ws + q.off_fby);
  fy.part_u = f.part_u + (size_t)q.fb.n_chunks * q.fb.nrep_pad * K;  // scratch behind x's u-row sums (unused by the finalize)
  if (const int rc = run_listed(fy, q.fb, 1, c.weighted, st)) return rc;
  return launch_finalize_y(b, fy, f.part_u, K, c.out_y, C, st);
}

// y / out_y: the second sample matrix of txm_resample_opts.  Carried by this call when the int8 kernel can take it
// as a row set of its last pass (*y_done = true); otherwise left to the caller (a separate order-0 bootstrap).
// THE kernel choice of an int8 call from what it was handed (plan, path, operands, workspace): the count-table kernel only
// when the workspace holds the table and the operands suit its DMA; with_y: the kernel carries opts.y as a row set
static I8KernelChoice i8_call_kernel(const ResampleCall &c, const I8Plan &q) {
  return i8_kernel_choice(q, c.path, c.N, c.C, c.nrep, c.K, c.y != nullptr,
                          c.ws_bytes >= q.total_table && table_operands_ok(c.x, c.ldx_s, c.C, c.K, c.y, c.ldy_s));
}
// does this call bootstrap opts.y inside its own kernel (no separate order-0 pass, no extra workspace behind the main plan)?
static bool call_carries_y(const ResampleCall &c) {
  if (c.y == nullptr || c.explicit_() || !use_i8(c.N, c.C, c.nrep, c.K, c.path)) return false;
  return i8_call_kernel(c, plan_i8(c.N, c.C, c.nrep, c.K)).with_y;
}
static int resample_i8_call(const ResampleCall &c, bool *y_done) {
  const int K = c.K;
  const int64_t C = c.C;
  hipStream_t st = c.st;
  const I8Plan q = plan_i8(c.N, C, c.nrep, K);
  // wide states: the per-sample counts of the call's replicates as a table in HBM (built once, shared by the column groups
  // and the passes) and the contraction kernel without a sampler inside (txm_resample_i8g.hip).  Misaligned operands and
  // TXM_PATH_INT8_FUSED keep the kernel that draws in place; narrow states and narrow tail groups always run it.
  I8CallState cs;
  cs.kernel = i8_call_kernel(c, q);
  const bool with_y = cs.kernel.with_y;
  if (const int rc = check_workspace(c.fn, c.ws_bytes, q.total)) return rc;
  if (const int rc = check_sampler(c)) return rc;
  cs.pb = (unsigned char *)c.ws + q.off_prep;
  if (const int rc = bind_prep(c, q.prep_total, cs.pb, cs.have_tables)) return rc;
  double *piv = (double *)cs.pb;
  double *ypiv = (double *)(cs.pb + q.prep_ypiv);
  if (!cs.have_tables) {
    if (const int rc = fill_pivot(c.pivot, c.x, c.ldx_s, c, piv)) return rc;
    if (with_y) {
      if (const int rc = fill_pivot(nullptr, c.y, c.ldy_s, c, ypiv)) return rc;
      // one u pivot for the call (the monomial scales of both matrices are built on it)
      TXM_HIP(hipMemcpyAsync(ypiv, piv, sizeof(double), hipMemcpyDeviceToDevice, st));
    }
  }
  I8Args b = i8_args(c, q, piv);
  b.stats = (double *)((char *)c.ws + q.L.s_stats);
  b.part_x = (double *)((char *)c.ws + q.L.s_px);
  b.part_u = (double *)((char *)c.ws + q.L.s_pu);
  b.n_chunks = q.n_chunks; b.tiles_per_chunk = q.tiles_per_chunk;
  b.y = with_y ? c.y : nullptr;
  b.ldy_s = c.ldy_s;
  b.ypivot = ypiv;
  b.part_y = (double *)((char *)c.ws + q.off_py);
  b.part_summed = i8t_wide_summed(with_y) ? 1 : 0;  // (what the wide fused kernel's instances of this call store: the finalize's mode)
  b.progress = q.n_rbg > 1 ? (uint32_t *)((char *)c.ws + q.off_prog) : nullptr;
  ResampleArgs f = fp64_args(c, q.fb, piv, (double *)((char *)c.ws + q.L.s_fbx), (double *)((char *)c.ws + q.L.s_fbu));
  f.sub_tiles = q.sub_tiles;
  TXM_REQUIRE(q.fb.nrep_pad == q.nrep_pad, "resample_vals: replicate padding of the two kernels differs");
  for (int g = 0; g < q.ngroups; ++g)
    if (const int rc = resample_i8_group(c, q, cs, g, b, f)) return rc;
  if (with_y) *y_done = true;
  // a reused prep block keeps its n_list words; a fresh one inside ws is what txm_resample_vals_info reads back
  if (c.prep != nullptr)
    TXM_HIP(hipMemcpyAsync((char *)c.ws + q.off_prep, cs.pb, q.prep_total, hipMemcpyDeviceToDevice, st));
  if (c.info != nullptr) {
    hipLaunchKernelGGL(i8_info_kernel, dim3(1), dim3(64), 0, st, cs.pb + q.prep_group0, q.prep_group_stride, q.L.p_nlist,
                       q.ngroups, q.nwin, (cs.have_tables ? 1 : 0) | (cs.have_table ? 2 : 0), c.info);
    TXM_LAUNCH_CHECK();
  }
  return TXM_OK;
}

// ---- the FP64 call ------------------------------------------------------------------------------------------------------
static int resample_fp64_call(const ResampleCall &c) {
  hipStream_t st = c.st;
  if (c.info != nullptr) {
    hipLaunchKernelGGL(fp64_info_kernel, dim3(1), dim3(64), 0, st, c.info);
    TXM_LAUNCH_CHECK();
  }
  const ResamplePlan p = plan_resample(c.N, c.C, c.nrep, c.K);
  if (const int rc = check_workspace(c.fn, c.ws_bytes, p.total)) return rc;
  TXM_REQUIRE((int64_t)p.n_chunks * p.n_rbg < ((int64_t)1 << 31), "resample_vals: grid too large");
  double *piv = (double *)((char *)c.ws + p.off_pivot);
  if (const int rc = fill_pivot(c.pivot, c.x, c.ldx_s, c, piv)) return rc;
  if (!c.explicit_())
    if (const int rc = check_sampler(c)) return rc;
  ResampleArgs a = fp64_args(c, p, piv, (double *)((char *)c.ws + p.off_px), (double *)((char *)c.ws + p.off_pu));
  if (p.n_rbg > 1 && a.N >= SM_T) {
    a.progress = (uint32_t *)((char *)c.ws + p.off_prog);
    TXM_HIP(hipMemsetAsync(a.progress, 0, p.prog_bytes, st));
  }
  return run_resample(a, p, c.K, c.weighted, c.explicit_(), c.out, st);
}

// the place that chooses between the int8 and the FP64 call
static int resample_vals_impl(const ResampleCall &c, bool *y_done) {
  *y_done = false;
  if (!c.explicit_() && use_i8(c.N, c.C, c.nrep, c.K, c.path)) return resample_i8_call(c, y_done);
  return resample_fp64_call(c);
}
}  // namespace txm

extern "C" int txm_resample_vals(const double *x, int64_t ldx_s, int64_t ldx_c, const double *u,
                                 const double *w, int64_t N, int64_t C, int order, int64_t nrep,
                                 const int64_t *freq, const txm_sampler_spec *spec,
                                 const uint32_t *counts, const double *pivot, double *out,
                                 const txm_resample_opts *opts, void *ws, size_t ws_bytes, txm_stream stream) {
  TXM_REQUIRE(x && u && out && ws, "resample_vals: null pointer");
  TXM_REQUIRE(N >= 1 && C >= 1 && nrep >= 1, "resample_vals: need N, C, nrep >= 1");
  TXM_REQUIRE(order >= 0 && order <= TXM_MAX_ORDER, "resample_vals: order %d outside [0, %d]", order,
              TXM_MAX_ORDER);
  TXM_REQUIRE(ldx_c == 1 && ldx_s >= C, "resample_vals: x must be (rec, val) row-major (ldx_c == 1)");
  if (const int rc = check_pitch("resample_vals", "x", ldx_s, C)) return rc;  // before anything is enqueued
  TXM_REQUIRE((freq != nullptr) != (spec != nullptr && counts != nullptr),
              "resample_vals: give either freq or (spec, counts)");
  ResampleCall c;
  c.x = x; c.ldx_s = ldx_s; c.u = u; c.w = w; c.weighted = w != nullptr;
  c.N = N; c.C = C; c.nrep = nrep; c.K = order + 1;
  c.freq = freq; c.spec = spec; c.counts = counts; c.pivot = pivot; c.out = out;
  if (const int rc = take_opts(c, opts)) return rc;
  TXM_REQUIRE((c.y == nullptr) == (c.out_y == nullptr), "resample_vals: opts.y and opts.out_y go together");
  TXM_REQUIRE(c.y == nullptr || c.ldy_s >= C, "resample_vals: opts.ldy_s < C");
  if (c.y != nullptr)
    if (const int rc = check_pitch("resample_vals", "y", c.ldy_s, C)) return rc;
  const size_t main_bytes = txm_resample_vals_ws_bytes_opts(N, C, nrep, order, c.path, c.y != nullptr);
  c.ws = ws; c.ws_bytes = ws_bytes < main_bytes ? ws_bytes : main_bytes; c.st = (hipStream_t)stream;
  // The queries are the larger of the two paths' plans rounded up to 256 bytes, so a path's own check cannot hold a call to
  // them: refuse here, before anything is enqueued, whatever is less than the query WITHOUT the count table (a workspace
  // between that and the query with it is the documented way onto the kernel that draws in place) ...
  if (const int rc = check_workspace(c.fn, ws_bytes, txm_resample_vals_ws_bytes_opts(N, C, nrep, order, TXM_PATH_INT8_FUSED, c.y != nullptr)))
    return rc;
  // ... and a second matrix's extra workspace, unless the call's kernel carries y
  if (c.y != nullptr && !call_carries_y(c))
    if (const int rc = check_workspace(c.fn, ws_bytes, main_bytes + y_extra_bytes(N, C, nrep))) return rc;
  bool y_done = false;
  int rc = resample_vals_impl(c, &y_done);
  if (rc != TXM_OK || c.y == nullptr || y_done) return rc;
  // second sample matrix: an order-0 bootstrap on the same sampler draw, then its mean column (behind the main plan: checked above)
  double *ystates = (double *)((char *)ws + main_bytes);
  ResampleCall cy;  // (its own pivot, no pre-pass block, no info, no second matrix)
  cy.x = c.y; cy.ldx_s = c.ldy_s; cy.u = u; cy.w = w; cy.weighted = c.weighted;
  cy.N = N; cy.C = C; cy.nrep = nrep;
  cy.freq = freq; cy.spec = spec; cy.counts = counts; cy.out = ystates; cy.path = c.path;
  cy.ws = (char *)ws + main_bytes + align_up((size_t)nrep * C * 2 * sizeof(double), 256);
  cy.ws_bytes = y_main_bytes(N, C, nrep); cy.st = c.st;
  rc = resample_vals_impl(cy, &y_done);
  if (rc != TXM_OK) return rc;
  hipLaunchKernelGGL(y_means_kernel, dim3((unsigned)cdiv(nrep * C, 256)), dim3(256), 0, c.st, ystates, nrep * C, c.out_y);
  TXM_LAUNCH_CHECK();
  return TXM_OK;
}

// ---- S state points of one shape: the same kernels with the state on grid axis z -----------------------
namespace txm {
struct BatchPlan {
  ResamplePlan one;  // plan of one state (the chunk count is chosen for S states together)
  size_t off_tab, off_pivot, off_px, off_pu, total;
};
static BatchPlan plan_batched(int64_t S, int64_t N, int64_t C, int64_t nrep, int K) {
  BatchPlan b;
  ResamplePlan &p = b.one;
  p = plan_resample(N, C, nrep, K);
  // S states fill the chip together: fewer sample chunks per state (ntiles / 8) -- again a function of N alone, so that
  // the states [s0, s1) of a collection give the same bits whichever call (rank) they are part of
  (void)S;
  p.tiles_per_chunk = resample_chunk_tiles(p.ntiles, 8);
  p.n_chunks = (int)(cdiv(cdiv(p.ntiles, p.tiles_per_chunk), 8) * 8);
  b.off_tab = 0;
  b.off_pivot = align_up((size_t)S * sizeof(txm_state_ptrs), 256);
  b.off_px = b.off_pivot + align_up((size_t)S * (1 + C) * sizeof(double), 256);
  b.off_pu = b.off_px + align_up((size_t)S * p.n_chunks * p.nrep_pad * p.C_pad * K * sizeof(double), 256);
  b.total = b.off_pu + align_up((size_t)S * p.n_chunks * p.nrep_pad * K * sizeof(double), 256);
  return b;
}
}  // namespace txm

// ---- S narrow state points on the int8 path (BASELINE config 5: 64 states x 1e6 samples x 4 observables) ----------------
// The reference loops over states in Python (models.py:635-641, gpr_active/active_utils.py:896-925).  Every kernel of the
// single-state int8 call (pre-pass, transposing-read kernel in its narrow-state variant, FP64 fallback in listed mode,
// finalize) takes the state from a grid axis and its operands from an I8State table, so the batch is the same arithmetic
// on the same per-window slots as S single calls: the same bits (tests/test_batched_gpu.py).
namespace txm {
struct BatchI8Plan {
  I8Plan q;                  // one state's plan: windows, replicate groups, the fallback's chunking
  int cpad, n_chunks;
  int64_t tiles_per_chunk;
  I8StateLayout L;
  size_t off_tab, off_states, off_bargs, off_state0, off_prep, total;
  size_t prep_piv, prep_state0, prep_total;  // the pre-pass block: pivots [S][1 + C], then the states' tables
};
static BatchI8Plan plan_batched_i8(int64_t S, int64_t N, int64_t C, int64_t nrep, int K) {
  BatchI8Plan b;
  b.q = plan_i8(N, C, nrep, K);
  const I8Plan &q = b.q;
  b.cpad = i8_cpad(C, K);
  // chunks of whole windows: the S states fill the chip together (the per-window slots make the sums independent of it)
  int64_t nc = (int64_t)num_cus() / ((int64_t)q.n_rbg * S) / 8 * 8;
  if (nc < 8) nc = 8;
  if (nc > q.nwin) nc = cdiv(q.nwin, 8) * 8;
  b.tiles_per_chunk = cdiv(q.nwin, nc) * q.win_tiles;
  b.n_chunks = (int)(cdiv(cdiv(q.ntiles, b.tiles_per_chunk), 8) * 8);
  // a state's tables as one column group's of the single call; its scratch with rows of cpad columns and no progress words
  I8StateLayout &L = b.L;
  L = q.L;
  i8_layout_scratch(q, K, b.cpad, 0, L);
  b.prep_piv = 0;
  b.prep_state0 = align_up((size_t)S * (1 + C) * sizeof(double), 256);
  b.prep_total = b.prep_state0 + (size_t)S * L.p_stride;
  b.off_tab = 0;
  b.off_states = align_up((size_t)S * sizeof(txm_state_ptrs), 256);
  b.off_bargs = b.off_states + align_up((size_t)S * sizeof(I8State), 256);
  b.off_state0 = b.off_bargs + align_up((size_t)S * sizeof(I8Args), 256);
  b.off_prep = b.off_state0 + (size_t)S * L.stride;
  b.total = b.off_prep + align_up(b.prep_total, 256);
  return b;
}

// which batched calls take the int8 path: narrow states (C <= 16: the quad-sharing variant of the transposing-read kernel)
// from order 2 on, with at least one full replicate group per state and windows long enough for the guard's statistics.
// Measured at BASELINE config 5's work (64e6 samples x 4 observables, order 3, nrep = 100): int8 9.6 ms incl. the pre-pass
// against 11.5 ms on the power-packed FP64 kernel (gpurun_out/r4_c5_probe.log).
static bool use_i8_batched(int64_t S, int64_t N, int64_t C, int64_t nrep, int K, int call_path = TXM_PATH_AUTO) {
  if (!i8_supported(N, C, nrep, K) || i8t_narrow_nq(C, K) == 0) return false;
  const int ov = effective_path(call_path);
  if (ov == TXM_PATH_FP64) return false;
  if (ov == TXM_PATH_INT8 || ov == TXM_PATH_INT8_FUSED || ov == TXM_PATH_INT8_TABLE) return true;
  // A rule on the STATE's shape only -- never on how many states share the launch: the states of a collection must take the
  // same kernel whichever rank (or workspace-bounded group) they are bootstrapped in, or a sharded run would differ from the
  // one-GPU run in the last bits.  The single-state rule for narrow states (use_i8): long series at any replicate count,
  // short ones from 128 replicates (64 x 1e6 x 4, order 3, nrep = 100: 6.7 against 11.6 ms on the FP64 kernel).
  (void)S;
  return K >= 2 && (N >= 786432 || (N >= 262144 && nrep >= 128));
}

__global__ void i8_states_kernel(const txm_state_ptrs *__restrict__ tab, int64_t S, unsigned char *base, unsigned char *pbase,
                                 I8StateLayout L, const double *piv, int64_t C, const uint32_t *counts, int64_t nrep, int64_t ntiles,
                                 double *out, int K, uint32_t rep_base, I8State *__restrict__ states) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  unsigned char *b = base + (size_t)s * L.stride, *pb = pbase + (size_t)s * L.p_stride;
  I8State e;
  e.x = tab[s].x; e.u = tab[s].u; e.w = tab[s].w;
  e.pivot = piv + s * (1 + C);
  e.stats = (double *)(b + L.s_stats);
  e.wtab = (double *)(pb + L.p_wt);
  e.wflag = (uint32_t *)(pb + L.p_flag);
  e.list = (uint32_t *)(pb + L.p_list);
  e.n_list = (uint32_t *)(pb + L.p_nlist);
  e.part_x = (double *)(b + L.s_px);
  e.part_u = (double *)(b + L.s_pu);
  e.fb_x = (double *)(b + L.s_fbx);
  e.fb_u = (double *)(b + L.s_fbu);
  e.counts = counts + (size_t)s * nrep * ntiles;
  e.out = out + (size_t)s * nrep * C * 2 * K;
  e.rep_base = rep_base + (uint32_t)(s * nrep);
  e.pad_ = 0;
  states[s] = e;
}

// the bootstrap kernel's arguments of state s: the call's, with the state's operands
__global__ void i8_batch_args_kernel(const I8Args base, int64_t S, I8Args *__restrict__ out) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const I8State e = base.states[s];
  I8Args r = base;
  r.x = e.x; r.u = e.u; r.w = e.w; r.pivot = e.pivot; r.wtab = e.wtab; r.wflag = e.wflag;
  r.part_x = e.part_x; r.part_u = e.part_u; r.counts = e.counts; r.rep_base = e.rep_base;
  out[s] = r;
}
static int resample_batched_i8(const ResampleCall &c) {
  const int64_t S = c.S, C = c.C;
  const int K = c.K;
  hipStream_t st = c.st;
  const BatchI8Plan b = plan_batched_i8(S, c.N, C, c.nrep, K);
  const I8Plan &q = b.q;
  if (const int rc = check_workspace(c.fn, c.ws_bytes, b.total)) return rc;
  if (const int rc = check_sampler(c)) return rc;
  TXM_REQUIRE((int64_t)b.n_chunks * q.n_rbg < ((int64_t)1 << 31) && S <= 65535, "resample_vals_batched: grid too large");
  // the pre-pass block: pivots, window tables, guard flags, fallback lists of the S states (a short caller-held block is
  // refused here, before the state table goes into the workspace: a refused call writes nothing)
  unsigned char *pb = (unsigned char *)c.ws + b.off_prep;
  bool have_tables;
  if (const int rc = bind_prep(c, b.prep_total, pb, have_tables)) return rc;
  txm_state_ptrs *tab = (txm_state_ptrs *)((char *)c.ws + b.off_tab);
  TXM_HIP(hipMemcpyAsync(tab, c.states_host, (size_t)c.S * sizeof(txm_state_ptrs), hipMemcpyHostToDevice, st));
  double *piv = (double *)(pb + b.prep_piv);
  if (!have_tables) {
    hipLaunchKernelGGL(pivot_batch_kernel, dim3((unsigned)(1 + C), (unsigned)S), dim3(256), 0, st, tab, c.ldx_s, c.N, C, piv);
    TXM_LAUNCH_CHECK();
  }
  I8State *states = (I8State *)((char *)c.ws + b.off_states);
  hipLaunchKernelGGL(i8_states_kernel, dim3((unsigned)cdiv(S, 64)), dim3(64), 0, st, tab, S, (unsigned char *)c.ws + b.off_state0,
                     pb + b.prep_state0, b.L, piv, C, c.counts, c.nrep, q.ntiles, c.out, K, (uint32_t)c.spec->rep0, states);
  TXM_LAUNCH_CHECK();
  const txm_state_ptrs &h0 = c.states_host[0];  // (the kernels read the state table; the call's own operand words are state 0's)
  bool vec_ok = c.ldx_s % 2 == 0;
  for (int64_t s = 0; s < S; ++s) vec_ok = vec_ok && (reinterpret_cast<uintptr_t>(c.states_host[s].x) & 15) == 0;
  I8Args a = i8_args(c, q, piv);
  a.states = states;
  a.S = S;
  a.x = vec_ok ? h0.x : reinterpret_cast<const double *>((uintptr_t)8);  // (the pre-pass reads its alignment only)
  a.u = h0.u; a.w = h0.w; a.C = C;
  a.part_summed = 1;  // (narrow instances always store digit-summed slots; the field is the wide instance's)
  a.cpad = b.cpad;
  a.n_chunks = b.n_chunks; a.tiles_per_chunk = b.tiles_per_chunk;
  I8Args *bargs = (I8Args *)((char *)c.ws + b.off_bargs);
  hipLaunchKernelGGL(i8_batch_args_kernel, dim3((unsigned)cdiv(S, 64)), dim3(64), 0, st, a, S, bargs);
  TXM_LAUNCH_CHECK();
  a.batch_args = bargs;
  if (!have_tables)
    if (const int rc = launch_i8_prepass(a, K, st)) return rc;
  if (const int rc = launch_resample_i8t(a, K, c.weighted, 0, st)) return rc;
  // the windows the precision guard flags, state by state on grid axis z (a state with an empty list: its blocks exit)
  ResampleArgs f = fp64_args(c, q.fb, piv, nullptr, nullptr);
  f.x = h0.x; f.u = h0.u; f.w = h0.w;
  f.sub_tiles = q.sub_tiles;
  f.i8states = states;
  TXM_REQUIRE(q.fb.nrep_pad == q.nrep_pad, "resample_vals_batched: replicate padding of the two kernels differs");
  if (const int rc = run_listed(f, q.fb, K, c.weighted, st, S)) return rc;
  // (batched launches always run the fused narrow kernel)
  if (const int rc = launch_finalize_i8(a, f, K, i8t_partials_summed(C, K) ? 1 : 0, nullptr, C, st)) return rc;
  if (c.info != nullptr) {
    hipLaunchKernelGGL(i8_info_kernel, dim3(1), dim3(64), 0, st, pb + b.prep_state0, b.L.p_stride, b.L.p_nlist, (int)S, q.nwin,
                       have_tables ? 1 : 0, c.info);
    TXM_LAUNCH_CHECK();
  }
  return TXM_OK;
}

static int resample_batched_fp64(const ResampleCall &c) {
  hipStream_t st = c.st;
  if (c.info != nullptr) {
    hipLaunchKernelGGL(fp64_info_kernel, dim3(1), dim3(64), 0, st, c.info);
    TXM_LAUNCH_CHECK();
  }
  const BatchPlan b = plan_batched(c.S, c.N, c.C, c.nrep, c.K);
  if (const int rc = check_workspace(c.fn, c.ws_bytes, b.total)) return rc;
  txm_state_ptrs *tab = (txm_state_ptrs *)((char *)c.ws + b.off_tab);
  TXM_HIP(hipMemcpyAsync(tab, c.states_host, (size_t)c.S * sizeof(txm_state_ptrs), hipMemcpyHostToDevice, st));
  double *piv = (double *)((char *)c.ws + b.off_pivot);
  hipLaunchKernelGGL(pivot_batch_kernel, dim3((unsigned)(1 + c.C), (unsigned)c.S), dim3(256), 0, st, tab, c.ldx_s, c.N, c.C, piv);
  TXM_LAUNCH_CHECK();
  if (!c.explicit_())
    if (const int rc = check_sampler(c)) return rc;
  ResampleArgs a = fp64_args(c, b.one, piv, (double *)((char *)c.ws + b.off_px), (double *)((char *)c.ws + b.off_pu));
  a.batch = tab;
  return run_resample(a, b.one, c.K, c.weighted, c.explicit_(), c.out, st, c.S);
}
}  // namespace txm

extern "C" size_t txm_resample_vals_batched_ws_bytes(int64_t S, int64_t N, int64_t C, int64_t nrep, int order) {
  if (S < 1 || !shape_ok(N, C, nrep, order)) return 0;
  // (the larger of the two paths: which one a call takes may be forced per process, txm_set_resample_path)
  const size_t f = plan_batched(S, N, C, nrep, order + 1).total;
  if (!i8_supported(N, C, nrep, order + 1) || i8t_narrow_nq(C, order + 1) == 0) return f;
  const size_t i = plan_batched_i8(S, N, C, nrep, order + 1).total;
  return i > f ? i : f;
}

// the kernel a TXM_PATH_AUTO batched call takes (the batched counterpart of txm_resample_path): callers that keep a
// pre-pass block bind it only when the call really runs the int8 path
extern "C" int txm_resample_batched_path(int64_t S, int64_t N, int64_t C, int64_t nrep, int order) {
  if (S < 1 || !shape_ok(N, C, nrep, order)) return TXM_PATH_FP64;
  return use_i8_batched(S, N, C, nrep, order + 1) ? TXM_PATH_INT8 : TXM_PATH_FP64;
}

extern "C" size_t txm_resample_batched_prep_bytes(int64_t S, int64_t N, int64_t C, int64_t nrep, int order) {
  if (S < 1 || !shape_ok(N, C, nrep, order)) return 0;
  if (!i8_supported(N, C, nrep, order + 1) || i8t_narrow_nq(C, order + 1) == 0) return 0;
  return plan_batched_i8(S, N, C, nrep, order + 1).prep_total;
}

extern "C" int txm_resample_vals_batched(const txm_state_ptrs *states_host, int64_t S, int64_t ldx_s, int64_t N,
                                         int64_t C, int order, int64_t nrep, const int64_t *freq,
                                         const txm_sampler_spec *spec, const uint32_t *counts, double *out,
                                         void *ws, size_t ws_bytes, txm_stream stream) {
  return txm_resample_vals_batched_opts(states_host, S, ldx_s, N, C, order, nrep, freq, spec, counts, out, nullptr, ws, ws_bytes,
                                        stream);
}

extern "C" int txm_resample_vals_batched_opts(const txm_state_ptrs *states_host, int64_t S, int64_t ldx_s, int64_t N,
                                              int64_t C, int order, int64_t nrep, const int64_t *freq,
                                              const txm_sampler_spec *spec, const uint32_t *counts, double *out,
                                              const txm_resample_opts *opts, void *ws, size_t ws_bytes, txm_stream stream) {
  ResampleCall c;
  c.fn = "resample_vals_batched";
  if (const int rc = take_opts(c, opts)) return rc;
  TXM_REQUIRE(!(c.y || c.out_y), "resample_vals_batched: no second sample matrix on the batched entry");
  TXM_REQUIRE(states_host && out && ws, "resample_vals_batched: null pointer");
  TXM_REQUIRE(S >= 1 && S <= 65535 && N >= 1 && C >= 1 && nrep >= 1, "resample_vals_batched: need S, N, C, nrep >= 1");
  TXM_REQUIRE(order >= 0 && order <= TXM_MAX_ORDER, "resample_vals_batched: order %d outside [0, %d]", order, TXM_MAX_ORDER);
  TXM_REQUIRE(ldx_s >= C, "resample_vals_batched: row pitch ldx_s < C");
  if (const int rc = check_pitch(c.fn, "x", ldx_s, C)) return rc;
  TXM_REQUIRE((freq != nullptr) != (spec != nullptr && counts != nullptr), "resample_vals_batched: give either freq or (spec, counts)");
  c.weighted = states_host[0].w != nullptr;
  for (int64_t s = 0; s < S; ++s) {
    TXM_REQUIRE(states_host[s].x && states_host[s].u, "resample_vals_batched: state %lld has a null pointer", (long long)s);
    TXM_REQUIRE((states_host[s].w != nullptr) == c.weighted, "resample_vals_batched: weights for all states or for none");
  }
  c.states_host = states_host; c.S = S; c.ldx_s = ldx_s;
  c.N = N; c.C = C; c.nrep = nrep; c.K = order + 1;
  c.freq = freq; c.spec = spec; c.counts = counts; c.out = out;
  c.ws = ws; c.ws_bytes = ws_bytes; c.st = (hipStream_t)stream;
  // the query is the larger of the two paths' plans: hold every call to it, before anything is enqueued
  if (const int rc = check_workspace(c.fn, ws_bytes, txm_resample_vals_batched_ws_bytes(S, N, C, nrep, order))) return rc;
  if (!c.explicit_() && use_i8_batched(S, N, C, nrep, c.K, c.path)) return resample_batched_i8(c);
  return resample_batched_fp64(c);
}
