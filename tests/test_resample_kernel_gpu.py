"""Differential tests of the FP64 bootstrap, resample_kernel / resample_finalize_kernel of txm_resample_fp64.hip -- the kernel that
serves order 8, explicit frequency tables, series shorter than one sampler tile and every window the int8 precision guard
hands back, and the yardstick of every int8 test -- against the long-double two-pass definition (oracle.truth_cov_multi) on
the same float64 inputs, on every path of its dispatch: every instantiation <K, NBLK, WEIGHTED, EXPLICIT, SMALLN, MODE, PACK>
the launcher can select in plain and batched mode (the case table is proved complete on the CPU from a restatement of
plan_resample / run_resample), the slid last tile, the three rare branches of the in-kernel sampler stage, chunks of two and
three tiles and chunks that hold none, the segmented sum of the finalize kernel, row pitches, misaligned operands, data
kinds, empty replicates, garbage in unused rows, concentrated weights, the second matrix, and the listed mode behind a forced
int8 call whose every scaling window is flagged (with a second matrix, and at a length where one workgroup walks two runs).

Reference.  In scale mode the frequency rows are those of the CPU restatement of the sampler stream
(oracle.sampler_freq(seed, nrep, N, nsamp, rep0)), never read back from the device: a draw that the kernel's own stage 3
puts into the wrong bin shows up at 1 / N.

Rule (README "Tolerances"): |hip - ref| <= 1e-12 (|ref| + sigma_x^a sigma_u^b) with the weighted standard deviations OF THE
REPLICATE (weights f_r * w), each floored at one ulp of the corresponding weighted mean.  A replicate of total weight zero
is expected as oracle.resample_vals gives it: the empty state, all zeros.  A replicate whose weight sits on ONE distinct
sample is known exactly -- {W, u_i, x_i, zeros} -- and expected as such wherever that sample is the pivot or the data has
one sample (the reference's own mean (f w u) / (f w) carries a long-double rounding whose square is 6e-8 of the scale
ulp(u)^2).  Where such a sample lies OFF the call's pivot (N = 2, one of the two samples drawn) the replicate has no sigma of its
own and takes the off-pivot bound with the data's sigmas.  Cases that pass pivot= on purpose off the replicate's means (the listed cases' replicates that drew an outlier)
take the README's off-pivot bound 4^order * 3e-13.

The tests that need no device (the coverage of the case table, the sampler-branch proof, the share of empty replicates, the
listed cases' pivot distance) carry no gpu mark and run with the CPU suite.  Every GPU case prints its worst scaled error
(run with -s).  Measured ratios: profiles/r13_resample_kernel_gpu_tests.txt.
"""

import ctypes as ct
import functools
import itertools
from pathlib import Path

import numpy as np
import pytest
import torch

from test_reduce_kernels_gpu import (CONCENTRATED, cdiv, dev, dev_off8, dev_pitched, exact_minus, idealgas, kind_data,
                                     kind_shift, plain_weights, wstat)

gpu = pytest.mark.gpu
RTOL = 1e-12
SM_T = 1024                      # samples per sampler tile (txm_sampler.h)
GOLDEN = Path(__file__).resolve().parent / "golden" / "resample_fp64_parent.npz"
WORST: dict = {}
PLAIN, BATCHED = "plain", "batched"


@pytest.fixture(scope="module")
def eng(txm):
    from thermoextrap_amd import engine

    return engine


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    if WORST:
        print("\nworst scaled error per family: " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(WORST.items())))


def off_pivot_rtol(order):
    return 4.0 ** order * 3e-13


# ---- the dispatch, restated (plan_resample, plan_batched of txm_resample.hip; run_resample of txm_resample_fp64.hip) ---------
def chunk_tiles(ntiles, div):
    nc = min(max(ntiles // div, 8), 1024)
    nc = cdiv(min(nc, ntiles), 8) * 8
    return cdiv(ntiles, nc)


def plan(N, C, nrep, order, weighted, explicit, mode):
    K = order + 1
    nblk = 1 if C <= 16 else 2
    colgroups = cdiv(C, nblk * 16)
    ntiles = cdiv(N, SM_T)
    tpc = chunk_tiles(ntiles, 8 if mode == BATCHED else 2)
    used = cdiv(ntiles, tpc)
    packed = 2 <= K <= 6 and nblk == 1 and colgroups == 1 and not explicit and N >= SM_T and C <= 8
    pack = (4 if (C <= 4 and K >= 3) else 2) if packed else 1
    return {"inst": (K, nblk, bool(weighted), bool(explicit), N < SM_T, mode, pack), "colgroups": colgroups, "n_rbg": cdiv(nrep, 64),
            "ntiles": ntiles, "tiles_per_chunk": tpc, "n_chunks": cdiv(used, 8) * 8, "chunks_used": used,
            "last_tile": N - (ntiles - 1) * SM_T, "progress": mode == PLAIN and cdiv(nrep, 64) > 1 and N >= SM_T}


@functools.lru_cache(maxsize=None)
def reachable():
    """Brute force over what decides the launch: {instantiation: some (N, C) that selects it}."""
    seen = {}
    for N, C, order, wt, ex, mode in itertools.product((1023, 1024), range(1, 65), range(9), (False, True), (False, True),
                                                       (PLAIN, BATCHED)):
        seen.setdefault(plan(N, C, 16, order, wt, ex, mode)["inst"], (N, C))
    return seen


# ---- data and reference -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=64)
def gas(N, C, seed=0, state=0):
    rng = np.random.default_rng([13, N, C, seed, state])
    x, u = idealgas(rng, N, C)
    x, u = x + 0.5 * state, u + 1.0 * state
    w = plain_weights(rng, N)
    for a in (x, u, w):
        a.setflags(write=False)
    return x, u, w


@functools.lru_cache(maxsize=256)
def stream_freq(orc, seed, nrep, N, nsamp=0, rep0=0):
    f = orc.sampler_freq(seed, nrep, N, nsamp, rep0=rep0)
    assert f.shape == (nrep, N) and np.all(f.sum(axis=1) == (nsamp or N))
    f.setflags(write=False)
    return f


def rep_scale(x, u, K, F, w):
    """scale[r, c, a, b] = sigma_x[r, c]^a sigma_u[r]^b, the weighted deviations of replicate r (weights F[r] * w), each
    floored at one ulp of the weighted mean; zeros for a replicate of total weight zero.  Rows that carry no weight in any
    replicate may hold anything and are left out."""
    W = F.astype(np.float64) * (1.0 if w is None else np.asarray(w)[None, :])
    used = (W != 0.0).any(axis=0)
    W, xs, us = W[:, used], np.asarray(x)[used], np.asarray(u)[used]
    sc = np.zeros((F.shape[0], x.shape[1], 2, K))
    for r in range(F.shape[0]):
        if W[r].sum() == 0.0:
            continue
        _, su = wstat(us, W[r])
        _, sx = wstat(xs, W[r])
        for b in range(K):
            sc[r, :, 0, b] = su ** b
            sc[r, :, 1, b] = sx * su ** b
    return sc


def truth(orc, x, u, order, F, w=None, shift=None):
    """oracle.truth_cov_multi on the frequency rows F; ``shift`` = (x0[C], u0): on exactly shifted inputs (kind_shift of the
    reduction suite: the reference's own mean is good to N 2^-64 |mean| only).  Replicates of total weight zero: zeros
    (oracle.resample_vals); a data set of ONE sample: exactly {W, u, x, zeros}."""
    K = order + 1
    F = np.ascontiguousarray(F, dtype=np.int64)
    W = F.astype(np.float64) * (1.0 if w is None else np.asarray(w)[None, :])
    empty = W.sum(axis=1) == 0.0
    if len(u) == 1:
        t = np.zeros((F.shape[0], x.shape[1], 2, K))
        t[:, :, 0, 0] = W[:, :1]
        t[:, :, 1, 0] = x[0][None, :]
        if K > 1:
            t[:, :, 0, 1] = u[0]
    else:
        used = (W != 0.0).any(axis=0)                      # garbage rows never reach the reference's arithmetic
        xs = np.where(used[:, None], x, 0.0)
        us = np.where(used, u, 0.0)
        Fz = F.copy()
        Fz[empty] = 0
        Fz[empty, 0] = 1                                   # (a placeholder row; overwritten below)
        if shift is None:
            t = orc.truth_cov_multi(xs, us, order, Fz, w=w)
        else:
            t = orc.truth_cov_multi(exact_minus(xs, np.where(used[:, None], shift[0][None, :], 0.0)),
                                    exact_minus(us, np.where(used, shift[1], 0.0)), order, Fz, w=w)
            t[:, :, 1, 0] += shift[0][None, :]
            if K > 1:
                t[:, :, 0, 1] += shift[1]
        one = (W != 0.0).sum(axis=1) == 1                  # the weight on ONE distinct sample: exactly {W, u_i, x_i, zeros}
        for r in np.flatnonzero(one):
            i = int(np.flatnonzero(W[r])[0])
            t[r] = 0.0
            t[r, :, 0, 0] = W[r, i]
            t[r, :, 1, 0] = x[i]
            if K > 1:
                t[r, :, 0, 1] = u[i]
        if empty.any():
            assert not orc.resample_vals(xs, us, F[empty], order, w=w).any(), "oracle.resample_vals: total weight zero is the empty state"
    t[empty] = 0.0
    return t


def hold(family, name, got, ref, scale, rtol=RTOL, nsamp=None):
    """got, ref, scale: (R, C, 2, K); rtol a number or one per replicate.  Replicates whose scale is all zero are the empty
    state and must be exactly zeros.  nsamp: the unweighted draw count S0[0] every replicate must report exactly."""
    got = np.asarray(got)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.all(np.isfinite(got)), (family, name, "a non-finite entry", int((~np.isfinite(got)).sum()))
    empty = ~scale.reshape(len(scale), -1).any(axis=1)
    if empty.any():
        assert not ref[empty].any() and not got[empty].any(), (family, name, "not the empty state", np.flatnonzero(empty))
    if nsamp is not None:
        assert np.all(got[:, :, 0, 0] == float(nsamp)), (family, name, "S0[0] != nsamp")
    live = ~empty
    rt = np.broadcast_to(np.asarray(rtol, dtype=np.float64), (len(got),))[live]
    if not live.any():
        print(f"\n{family}[{name}]: every replicate empty")
        return
    e = (np.abs(got[live] - ref[live]) / (np.abs(ref[live]) + scale[live])).reshape(int(live.sum()), -1).max(axis=1)
    ratio = float((e / rt).max())
    WORST[family] = max(WORST.get(family, 0.0), float((e / rt * RTOL).max()))
    print(f"\n{family}[{name}]: worst scaled err {float(e.max()):.2e}, worst err / limit {ratio:.3f}"
          + (f", {int(empty.sum())} empty replicates" if empty.any() else ""))
    assert ratio <= 1.0, (family, name, float(e.max()), ratio)


def run_single(eng, xd, ud, order, *, F=None, sampler=None, wd=None, pivot=None, path="fp64", y=None):
    """One txm_resample_vals call; asserts the kernel that served it."""
    out = eng.resample_vals(xd, ud, order, freq=None if F is None else torch.tensor(np.asarray(F)).cuda(), sampler=sampler, w=wd,
                            pivot=pivot, path=path, y=y)
    info = eng.resample_info()
    assert info["path"] == ("int8" if path == "int8" else "fp64"), info
    return out


# ---- the case table ---------------------------------------------------------------------------------------------------
SMALL_N, FULL_N = (1, 2, 777, 1023), (1024, 1025, 2047, 2048 + 5)
NARROW_C, WIDE_C = (1, 3, 4, 5, 8, 9, 16), (17, 32, 33, 64)
NREPS = (1, 15, 16, 17, 63, 65, 130)


def _table():
    """One case per reachable instantiation, the shapes rotating through the smallest ones that reach every edge: a padded
    last column block, two column groups, both PACK widths at their edges, an odd last replicate pair, a wave without a
    replicate, one to three replicate-block groups, both sides of one sampler tile and the shortest and longest tails."""
    cases, i = [], 0
    for mode, wt, ex, small in itertools.product((PLAIN, BATCHED), (False, True), (False, True), (True, False)):
        for order in range(9):
            groups = [NARROW_C, WIDE_C]
            if not small and not ex:                         # by PACK: 4 (K >= 3) / 2, 2, 1
                groups = [(1, 3, 4), (5, 8), (9, 16), WIDE_C]
            for g in groups:
                N = (SMALL_N if small else FULL_N)[(i + order) % 4]
                nrep = NREPS[i % 7] if mode == PLAIN else NREPS[i % 4]            # (batched: three states of up to 17)
                C = g[(i // 2 + order) % len(g)]
                if C == 64 and nrep == 130:
                    nrep = 65
                cases.append((mode, N, C, order, wt, ex, nrep, 7 * (i % 2)))
                i += 1
    # the slid last tile at its shortest and longest tail on each (WEIGHTED, EXPLICIT) pair, one and two column blocks
    for wt, ex, N, C in itertools.product((False, True), (False, True), (1025, 2047), (3, 33)):
        cases.append((PLAIN, N, C, 4, wt, ex, 17, 0))
    return cases


TABLE = _table()


def case_id(c):
    mode, N, C, order, wt, ex, nrep, rep0 = c
    return f"{mode}-N{N}-C{C}-o{order}-{'w' if wt else 'u'}-{'freq' if ex else 'smp'}-R{nrep}-r{rep0}"


def test_case_table_covers_every_reachable_instantiation():
    """The enumeration: N on both sides of one sampler tile, C = 1 .. 64, every order, both weight settings, both sampler
    modes, plain and batched launches -- 324 instantiations of the 864 combinations of the template's parameters.  The
    table names exactly those; what cannot be launched is unreachable in the enumeration, not a gap in the table."""
    reach = reachable()
    have = {plan(N, C, nrep, order, wt, ex, mode)["inst"] for (mode, N, C, order, wt, ex, nrep, rep0) in TABLE}
    assert have == set(reach), (sorted(set(reach) - have)[:5], sorted(have - set(reach))[:5])
    assert len(reach) == 324
    every = set(itertools.product(range(1, 10), (1, 2), (False, True), (False, True), (False, True), (PLAIN, BATCHED), (1, 2, 4)))
    unreachable = every - set(reach)
    assert len(every) == 864 and len(unreachable) == 540
    for (K, nblk, wt, ex, small, mode, pack) in unreachable:       # packing: one block, device sampler, full tiles, K in 2..6
        assert pack > 1 or K > 9, (K, nblk, wt, ex, small, mode, pack)
        assert nblk == 2 or ex or small or K in (1, 7, 8, 9) or (K == 2 and pack == 4)
    # unpacked K = 3, C <= 8, scale mode, N >= 1024 cannot be launched: the unpacked narrow instantiation is C = 9 .. 16's
    for C in range(1, 9):
        for order in range(1, 6):
            assert plan(1024, C, 16, order, False, False, PLAIN)["inst"][6] == (4 if (C <= 4 and order >= 2) else 2)
    assert reach[(3, 1, False, False, False, PLAIN, 1)][1] == 9
    # the shapes the table rotates through are all in use, on both sampler modes
    for ex in (False, True):
        used = [(N, C, nrep) for (mode, N, C, order, wt, e, nrep, rep0) in TABLE if e == ex]
        assert {n for n, _, _ in used} == set(SMALL_N + FULL_N)
        assert {c for _, c, _ in used} == set(NARROW_C + WIDE_C)
        assert {r for _, _, r in used} == set(NREPS)
    assert {(wt, ex, N) for (mode, N, C, order, wt, ex, nrep, rep0) in TABLE if mode == PLAIN and N in (1025, 2047)} \
        == set(itertools.product((False, True), (False, True), (1025, 2047)))
    assert {plan(N, 3, r, 4, False, False, PLAIN)["n_rbg"] for N in (1024,) for r in NREPS} == {1, 2, 3}


@functools.lru_cache(maxsize=8)
def table_reference(orc, mode, N, C, wt, ex, nrep, rep0):
    """Order-8 truth and scale of a table case (a moment does not depend on how many higher ones are asked for): per state
    (x, u, w, F, truth, scale)."""
    S = 3 if mode == BATCHED else 1
    seed = 1000 + N + 64 * C + nrep
    # N = 2: a replicate that drew ONE of the two samples has sigma = 0 and its only sample half the data's spread off the
    # call's pivot -- no accumulation about a shared pivot meets a scale of one ulp there (measured: err / ulp^b of 4e12 at order
    # 3 up to 4e98 at order 8, orders 0 and 1 exact).  The N = 2 cases therefore draw 16 N = 32 times (both samples in every
    # replicate, asserted) and their explicit tables count every sample at least once; the rule itself is the same.  (The replicates left out
    # here are held to the off-pivot bound by test_two_samples_one_drawn.)
    ns = 16 * N if N == 2 else 0
    if ex:
        rng = np.random.default_rng([17, N, C, nrep])
        F = rng.multinomial(N, np.full(N, 1.0 / N), size=S * nrep).astype(np.int64) + (1 if N == 2 else 0)
    else:
        F = stream_freq(orc, seed, S * nrep, N, ns, rep0)
    assert N != 2 or np.all(F > 0)
    out = []
    for s in range(S):
        x, u, w = gas(N, C, 0, s)
        w = w if wt else None
        Fs = F[s * nrep:(s + 1) * nrep]
        out.append((x, u, w, Fs, truth(orc, x, u, 8, Fs, w), rep_scale(x, u, 9, Fs, w)))
    return (seed, ns), F, out


@gpu
@pytest.mark.parametrize("case", TABLE, ids=case_id)
def test_every_instantiation(eng, orc, case):
    mode, N, C, order, wt, ex, nrep, rep0 = case
    K = order + 1
    p = plan(N, C, nrep, order, wt, ex, mode)
    (seed, ns), F, states = table_reference(orc, mode, N, C, wt, ex, nrep, rep0)
    fam = f"{mode} K={p['inst'][0]} nblk={p['inst'][1]} pack={p['inst'][6]}" + (" smalln" if p["inst"][4] else "")
    nsamp = None if (wt or ex) else (ns or N)
    if mode == PLAIN:
        x, u, w, Fs, t, sc = states[0]
        smp = None if ex else eng.DeviceSampler(seed, nrep, N, nsamp=ns, rep0=rep0)
        got = run_single(eng, dev(x), dev(u), order, F=Fs if ex else None, sampler=smp, wd=None if w is None else dev(w))
        hold(fam, case_id(case) + f" inst={p['inst']}", got.cpu().numpy(), t[..., :K], sc[..., :K], nsamp=nsamp)
        return
    S = len(states)
    smp = None if ex else eng.DeviceSampler(seed, S * nrep, N, nsamp=ns, rep0=rep0)
    got = eng.resample_vals_batched([dev(s[0]) for s in states], [dev(s[1]) for s in states], order, nrep=nrep, sampler=smp,
                                    freq=torch.tensor(F).cuda() if ex else None, ws=[dev(s[2]) for s in states] if wt else None,
                                    path="fp64")
    assert eng.batched_info()["path"] == "fp64"
    for s, (x, u, w, Fs, t, sc) in enumerate(states):        # the oracle on the state's own rows, rep0 + s * nrep
        hold(fam, case_id(case) + f" state {s} inst={p['inst']}", got[s].cpu().numpy(), t[..., :K], sc[..., :K], nsamp=nsamp)


# ---- chunking: two and three tiles a chunk, chunks that hold no tile, the finalize's eight segments ------------------------
CHUNK_N = (7 * 1024 + 5, 9 * 1024 + 1, 16 * 1024 + 5)
CHUNK_CASES = [(PLAIN, N, C, order, wt, False) for N in CHUNK_N for C in (3, 33) for order in (2, 8) for wt in (False, True)] \
    + [(PLAIN, N, 3, 2, True, True) for N in CHUNK_N] + [(BATCHED, N, 3, 2, False, False) for N in CHUNK_N]


def test_chunk_cases_reach_what_they_are_for():
    p = [plan(N, 3, 65, 2, False, False, PLAIN) for N in CHUNK_N]
    assert [(q["ntiles"], q["tiles_per_chunk"], q["chunks_used"], q["n_chunks"], q["last_tile"]) for q in p] \
        == [(8, 1, 8, 8, 5), (10, 2, 5, 8, 1), (17, 3, 6, 8, 5)]      # every segment of the finalize; three, then two empty chunks
    assert all(q["progress"] and q["n_rbg"] == 2 for q in p)          # the progress words: more than one replicate-block group
    assert [plan(N, 3, 17, 2, False, False, BATCHED)["tiles_per_chunk"] for N in CHUNK_N] == [1, 2, 3]
    assert plan(9 * 1024 + 1, 33, 65, 8, True, False, PLAIN)["colgroups"] == 2


@gpu
@pytest.mark.parametrize("mode,N,C,order,wt,ex", CHUNK_CASES)
def test_chunking(eng, orc, mode, N, C, order, wt, ex):
    nrep = 65 if mode == PLAIN else 17
    test_every_instantiation(eng, orc, (mode, N, C, order, wt, ex, nrep, 0))


# ---- the in-kernel sampler stage: n < 768, n > 1152 (the c0 >= 96 loop), the odd last replicate of a wave -----------------------
SAMPLER_N, SAMPLER_NREP = 2048 + 5, 17
NSAMPS = ("half", "same", "double", "x16")


def nsamp_of(N, which):
    return {"half": N // 2, "same": 0, "double": 2 * N, "x16": 16 * N}[which]


def sampler_seed(N, which, rep0):
    return 500 + NSAMPS.index(which) + 10 * rep0 + N


@pytest.mark.parametrize("which", NSAMPS)
@pytest.mark.parametrize("rep0", [0, 7])
def test_sampler_cases_reach_the_rare_branches(orc, which, rep0):
    """From the CPU restatement of the tile counts: N // 2 draws leave every full tile below 768 (ALL_VALID = false), 2 N and
    16 N put every full tile above 1152 (the plain loop behind call 96), and 17 replicates end on a pair without a second."""
    N = SAMPLER_N
    cnt = orc.sampler_tile_counts(sampler_seed(N, which, rep0), SAMPLER_NREP, N, nsamp_of(N, which), rep0)
    assert cnt.shape == (SAMPLER_NREP, 3) and SAMPLER_NREP % 2 == 1
    full = cnt[:, :2]
    if which == "half":
        assert full.max() < 768
    elif which == "same":
        assert full.min() >= 768 and full.max() <= 1152 + 64
    else:
        assert full.min() > 1152
    assert np.all(cnt.sum(axis=1) == (nsamp_of(N, which) or N))


@gpu
@pytest.mark.parametrize("which", NSAMPS)
@pytest.mark.parametrize("rep0", [0, 7])
@pytest.mark.parametrize("N,C", [(SAMPLER_N, 3), (SAMPLER_N, 33), (777, 3), (777, 33)])
@pytest.mark.parametrize("wt", [False, True])
def test_sampler_branches_through_the_kernel(eng, orc, which, rep0, N, C, wt):
    order, nrep = 4, SAMPLER_NREP
    ns = nsamp_of(N, which)
    seed = sampler_seed(N, which, rep0)
    x, u, w = gas(N, C, 1)
    w = w if wt else None
    F = stream_freq(orc, seed, nrep, N, ns, rep0)
    got = run_single(eng, dev(x), dev(u), order, sampler=eng.DeviceSampler(seed, nrep, N, nsamp=ns, rep0=rep0),
                     wd=None if w is None else dev(w))
    hold("sampler branches", f"nsamp={which} rep0={rep0} N={N} C={C} w={wt}", got.cpu().numpy(), truth(orc, x, u, order, F, w),
         rep_scale(x, u, order + 1, F, w), nsamp=None if wt else (ns or N))


# ---- layout: a row pitch above C with NaN in the padding, a column window, operands 8 bytes off -----------------------------
@gpu
@pytest.mark.parametrize("variant", ["pitched", "window", "x_off8", "u_off8", "w_off8"])
@pytest.mark.parametrize("N,C", [(777, 3), (2048 + 5, 3), (777, 33), (2048 + 5, 33)])
@pytest.mark.parametrize("ex", [False, True])
def test_layouts(eng, orc, variant, N, C, ex):
    order, nrep = 4, 17
    x, u, w = gas(N, C, 2)
    F = stream_freq(orc, 77, nrep, N)
    xd = {"pitched": lambda: dev_pitched(x, C + 5), "window": lambda: dev_pitched(x, C + 6, 1), "x_off8": lambda: dev_off8(x)}.get(
        variant, lambda: dev(x))()
    ud = dev_off8(u) if variant == "u_off8" else dev(u)
    wd = dev_off8(w) if variant == "w_off8" else dev(w)
    if variant in ("window", "x_off8"):
        assert xd.data_ptr() % 16 == 8
    if variant in ("pitched", "window"):
        assert xd.stride(0) > C
    got = run_single(eng, xd, ud, order, F=F if ex else None, sampler=None if ex else eng.DeviceSampler(77, nrep, N), wd=wd)
    hold("layouts", f"{variant} N={N} C={C} explicit={ex}", got.cpu().numpy(), truth(orc, x, u, order, F, w),
         rep_scale(x, u, order + 1, F, w))


# ---- data kinds -----------------------------------------------------------------------------------------------------------
KIND_N, KIND_C, KIND_ORDER, KIND_NREP = 3000, 3, 4, 17
KIND_CASES = [("idealgas", False), ("u_1e8", False), ("u_1e8", True), ("const_column", True), ("const_column", False),
              ("u_sorted", False), ("half_zero", False), ("half_zero", True), ("counts_1e6", True)]


@gpu
@pytest.mark.parametrize("kind,ex", KIND_CASES)
def test_data_kinds(eng, orc, kind, ex):
    x, u, w = kind_data("idealgas" if kind == "counts_1e6" else kind, N=KIND_N, C=KIND_C)
    F = stream_freq(orc, 31, KIND_NREP, KIND_N)
    if kind == "counts_1e6":                                 # explicit counts up to 1e6 in one row
        F = F.copy()
        F[3] = np.random.default_rng(5).integers(0, 1_000_001, KIND_N)
        F[3, 17] = 1_000_000
    sh = kind_shift(kind, x, u)
    got = run_single(eng, dev(x), dev(u), KIND_ORDER, F=F if ex else None, sampler=None if ex else eng.DeviceSampler(31, KIND_NREP, KIND_N),
                     wd=None if w is None else dev(w))
    hold("data kinds", f"{kind} explicit={ex}", got.cpu().numpy(), truth(orc, x, u, KIND_ORDER, F, w, shift=sh),
         rep_scale(x, u, KIND_ORDER + 1, F, w))


# ---- empty replicates -------------------------------------------------------------------------------------------------------
TWO_N, TWO_NREP, TWO_SEED = 2048, 130, 91
TWO_ROWS = (700, 1500)


def two_sample_data():
    """Weights zero except on two samples, which hold the SAME values, passed as the pivot: every replicate that drew one
    of them is known exactly, {f w, u, x, zeros}, on the bound's own terms (sigma = 0, floored at one ulp)."""
    x, u, _ = gas(TWO_N, 3, 3)
    x, u = x.copy(), u.copy()
    x[TWO_ROWS[1]], u[TWO_ROWS[1]] = x[TWO_ROWS[0]], u[TWO_ROWS[0]]
    w = np.zeros(TWO_N)
    w[list(TWO_ROWS)] = (0.75, 1.5)
    return x, u, w


def test_two_sample_weights_leave_some_replicates_empty(orc):
    """About e^-2 of the replicates draw neither of the two samples that carry weight: between 2 and 60 of the 130."""
    F = stream_freq(orc, TWO_SEED, TWO_NREP, TWO_N)
    n_empty = int((F[:, list(TWO_ROWS)].sum(axis=1) == 0).sum())
    print(f"\n{n_empty} of {TWO_NREP} replicates are empty")
    assert 2 <= n_empty <= 60
    x, u, w = two_sample_data()
    assert not orc.resample_vals(x, u, F[F[:, list(TWO_ROWS)].sum(axis=1) == 0], 4, w=w).any()


def two_sample_truth(x, u, w, F, K):
    t = np.zeros((len(F), x.shape[1], 2, K))
    W = F[:, TWO_ROWS[0]] * w[TWO_ROWS[0]] + F[:, TWO_ROWS[1]] * w[TWO_ROWS[1]]
    live = W != 0.0
    t[live, :, 0, 0] = W[live, None]
    t[live, :, 0, 1] = u[TWO_ROWS[0]]
    t[live, :, 1, 0] = x[TWO_ROWS[0]][None, :]
    sc = np.zeros_like(t)
    for b in range(K):                                      # sigma_x^a sigma_u^b, both one ulp of the mean
        sc[live, :, 0, b] = np.spacing(abs(u[TWO_ROWS[0]])) ** b
        sc[live, :, 1, b] = np.spacing(np.abs(x[TWO_ROWS[0]]))[None, :] * np.spacing(abs(u[TWO_ROWS[0]])) ** b
    return t, sc


@gpu
@pytest.mark.parametrize("path", ["fp64", "int8"])
def test_replicates_that_drew_no_weight_are_the_empty_state(eng, orc, path):
    order = 4
    x, u, w = two_sample_data()
    F = stream_freq(orc, TWO_SEED, TWO_NREP, TWO_N)
    assert eng._L().txm_resample_i8_supported(TWO_N, 3, TWO_NREP, order) == 1
    piv = dev(np.r_[u[TWO_ROWS[0]], x[TWO_ROWS[0]]])
    y = 0.5 * x + 0.25
    got, ym = run_single(eng, dev(x), dev(u), order, sampler=eng.DeviceSampler(TWO_SEED, TWO_NREP, TWO_N), wd=dev(w), pivot=piv,
                         path=path, y=dev(y))
    t, sc = two_sample_truth(x, u, w, F, order + 1)
    hold(f"empty replicates ({path})", "two samples carry the weight", got.cpu().numpy(), t, sc)
    empty = ~t.reshape(len(t), -1).any(axis=1)
    ym = ym.cpu().numpy()
    assert np.all(np.isfinite(ym)) and not ym[empty].any()           # out_y of an empty replicate: 0
    assert np.allclose(ym[~empty], y[TWO_ROWS[0]][None, :], rtol=1e-12, atol=0.0)


@gpu
@pytest.mark.parametrize("N,C", [(777, 3), (2048 + 5, 3), (2048 + 5, 33)])
@pytest.mark.parametrize("wt", [False, True])
def test_an_explicit_row_of_zeros_is_the_empty_state(eng, orc, N, C, wt):
    order, nrep = 4, 17
    x, u, w = gas(N, C, 4)
    w = w if wt else None
    F = stream_freq(orc, 93, nrep, N).copy()
    F[[0, 5, nrep - 1]] = 0
    y = 0.5 * x + 0.25
    got, ym = run_single(eng, dev(x), dev(u), order, F=F, wd=None if w is None else dev(w), y=dev(y))
    sc = rep_scale(x, u, order + 1, F, w)
    assert sorted(np.flatnonzero(~sc.reshape(nrep, -1).any(axis=1))) == [0, 5, nrep - 1]
    hold("empty replicates (explicit)", f"N={N} C={C} w={wt}", got.cpu().numpy(), truth(orc, x, u, order, F, w), sc)
    ym = ym.cpu().numpy()
    assert np.all(np.isfinite(ym)) and not ym[[0, 5, nrep - 1]].any()


# ---- garbage in rows that carry no weight ------------------------------------------------------------------------------------
def weighted_means(x, u, w, used):
    ww = (np.ones(len(u)) if w is None else w) * used
    return np.r_[(ww * np.where(used, u, 0.0)).sum() / ww.sum(), (ww[:, None] * np.where(used[:, None], x, 0.0)).sum(axis=0) / ww.sum()]


@gpu
@pytest.mark.parametrize("N,C,order,big", [(2048 + 5, 3, 4, 1e30), (2048 + 5, 8, 4, 1e30), (2048 + 5, 33, 4, 1e30), (777, 3, 4, 1e30),
                                           (2048 + 5, 3, 8, 1e30), (2048 + 5, 9, 4, 1e150), (2048 + 5, 33, 8, 1e150)])
@pytest.mark.parametrize("how", ["weight_zero", "weight_zero_explicit", "not_drawn"])
def test_garbage_in_unused_rows(eng, orc, N, C, order, big, how):
    """Rows of weight zero -- or, unweighted, rows no replicate of the case drew -- hold +-big in u or x; the pivot is the
    weighted mean of the rows in use.  1e30: |du|^8 |dx| stays finite (the contract of include/txmom.h); 1e150 on unpacked
    instantiations only, whose A operand is the zero count itself."""
    nrep = 3 if how == "not_drawn" else 17                 # (three replicates leave 5 % of the rows undrawn)
    if big > 1e100:
        assert plan(N, C, nrep, order, True, False, PLAIN)["inst"][6] == 1
    x, u, w = gas(N, C, 5)
    x, u = x.copy(), u.copy()
    F = stream_freq(orc, 97, nrep, N)
    rng = np.random.default_rng(6)
    if how == "not_drawn":
        z = np.flatnonzero(~F.any(axis=0))
        assert len(z) >= 2
        w = None
    else:
        w = w.copy()
        z = rng.permutation(N)[: N // 8]
        w[z] = 0.0
    u[z[::2]] = big
    x[z[1::2]] = -big
    used = np.ones(N, dtype=bool)
    used[z] = False
    piv = weighted_means(x, u, w, used)
    ex = how == "weight_zero_explicit"
    got = run_single(eng, dev(x), dev(u), order, F=F if ex else None, sampler=None if ex else eng.DeviceSampler(97, nrep, N),
                     wd=None if w is None else dev(w), pivot=dev(piv))
    hold("garbage rows", f"{how} N={N} C={C} order={order} big={big:g}", got.cpu().numpy(), truth(orc, x, u, order, F, w),
         rep_scale(x, u, order + 1, F, w))


# ---- concentrated weights, the weighted means as pivot= --------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", list(CONCENTRATED))
@pytest.mark.parametrize("ex", [False, True])
def test_concentrated_weights_about_the_weighted_means(eng, orc, kind, ex):
    """The library's own pivot of a weighted bootstrap stays the unweighted strided mean ("What stays
    unweighted"); a caller whose weights select passes the weighted means, and is then held to 1e-12."""
    x, u, w = kind_data(kind, N=KIND_N, C=KIND_C)
    nrep, order = 17, KIND_ORDER
    F = stream_freq(orc, 41, nrep, KIND_N)
    piv = weighted_means(x, u, w, w != 0.0)
    got = run_single(eng, dev(x), dev(u), order, F=F if ex else None, sampler=None if ex else eng.DeviceSampler(41, nrep, KIND_N),
                     wd=dev(w), pivot=dev(piv))
    hold("concentrated weights", f"{kind} explicit={ex}", got.cpu().numpy(), truth(orc, x, u, order, F, w),
         rep_scale(x, u, order + 1, F, w))


# ---- the second matrix on the FP64 path: an order-0 bootstrap behind the call, then y_means_kernel -----------------------------
@gpu
@pytest.mark.parametrize("N,C,wt,ex", [(2048 + 5, 3, True, False), (777, 33, False, True), (9 * 1024 + 1, 33, True, False)])
def test_second_matrix(eng, orc, N, C, wt, ex):
    order, nrep = 3, 17
    x, u, w = gas(N, C, 7)
    w = w if wt else None
    y = gas(N, C, 8)[0] * 3.0 - 1.0
    F = stream_freq(orc, 55, nrep, N)
    got, ym = run_single(eng, dev(x), dev(u), order, F=F if ex else None, sampler=None if ex else eng.DeviceSampler(55, nrep, N),
                         wd=None if w is None else dev(w), y=dev(y))
    hold("second matrix", f"states N={N} C={C}", got.cpu().numpy(), truth(orc, x, u, order, F, w), rep_scale(x, u, order + 1, F, w))
    LD = np.longdouble
    fw = F.astype(LD) * (1 if w is None else w.astype(LD)[None, :])
    want = (fw @ y.astype(LD)) / fw.sum(axis=1)[:, None]
    ysig = np.stack([wstat(y, np.asarray(fw[r], dtype=np.float64))[1] for r in range(nrep)])
    e = float((np.abs(ym.cpu().numpy().astype(LD) - want) / (np.abs(want) + ysig)).max())
    print(f"\nsecond matrix[means N={N} C={C}]: worst scaled err {e:.2e}")
    assert e <= RTOL


# ---- RS_BATCHED with more states than one state's grid ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("wt", [False, True])
def test_batched_seventy_states(eng, orc, wt):
    S, N, C, order, nrep = 70, 1025, 3, 3, 5
    assert S > plan(N, C, nrep, order, wt, False, BATCHED)["n_chunks"] * plan(N, C, nrep, order, wt, False, BATCHED)["n_rbg"]
    F = stream_freq(orc, 61, S * nrep, N, 0, 7)
    st = [gas(N, C, 9, s) for s in range(S)]
    got = eng.resample_vals_batched([dev(a[0]) for a in st], [dev(a[1]) for a in st], order, nrep=nrep,
                                    sampler=eng.DeviceSampler(61, S * nrep, N, rep0=7), ws=[dev(a[2]) for a in st] if wt else None, path="fp64")
    assert eng.batched_info()["path"] == "fp64"
    got = got.cpu().numpy()
    for s, (x, u, w) in enumerate(st):
        w = w if wt else None
        Fs = F[s * nrep:(s + 1) * nrep]
        hold("batched S=70", f"state {s} w={wt}", got[s], truth(orc, x, u, order, Fs, w), rep_scale(x, u, order + 1, Fs, w),
             nsamp=None if wt else N)


# ---- repeatability: the progress words never change a result ------------------------------------------------------------------
@gpu
def test_two_runs_give_equal_bits(eng):
    N, C, order, nrep = 9 * 1024 + 1, 33, 4, 130
    assert plan(N, C, nrep, order, True, False, PLAIN)["progress"] and plan(N, C, nrep, order, True, False, PLAIN)["n_rbg"] == 3
    x, u, w = gas(N, C, 10)
    xd, ud, wd = dev(x), dev(u), dev(w)
    s = eng.DeviceSampler(71, nrep, N)
    a = run_single(eng, xd, ud, order, sampler=s, wd=wd).clone()
    run_single(eng, xd, ud, 2, sampler=s)                    # (another call in between: the workspace is reused)
    b = run_single(eng, xd, ud, order, sampler=s, wd=wd)
    assert torch.equal(a, b)


# ---- RS_LISTED: a forced int8 call whose every scaling window the precision guard flags ------------------------------------------
OUT_U = 5.0e5                    # ~1e5 sigma in u: the outlier of tests/test_guard_gpu.py
WIN = 4 * SM_T                   # plan_i8: scaling windows of 4 tiles on series this short
LISTED_N = 3 * WIN + 1025        # four windows; the last one ends on a slid one-sample tile
LISTED_NREP, LISTED_SEED = 63, 97
LISTED_CASES = [(LISTED_N, C, order, wt) for order in range(8) for C in (8, 32) for wt in (False, True)] \
    + [(LISTED_N, 40, 4, True), (LISTED_N, 40, 0, False), (LISTED_N, 40, 7, False)]
OUT_X = 4.0e4                    # order 0 looks at x alone: the same rows carry an outlier in the first and the last column


def listed_data(N, C):
    """Ideal-gas data with one outlier in u per scaling window, on rows the strided pivot subsample (rows k * (N // 1024),
    pivot_kernel of txm_pivot.h) does not visit."""
    x, u, w = gas(N, C, 11)
    u = u.copy()
    step = N // 1024
    rows = np.array([k * WIN + 515 for k in range(cdiv(N, WIN))])
    assert step >= 2 and np.all(rows % step != 0) and rows[-1] < N
    x = x.copy()
    u[rows] += OUT_U
    x[rows, 0] += OUT_X
    x[rows, C - 1] += OUT_X
    return x, u, w, rows


def strided_pivot(x, u):
    N = len(u)
    idx = np.arange(min(N, 1024)) * (N // min(N, 1024))
    return np.r_[u[idx].mean(), x[idx].mean(axis=0)]


@pytest.mark.parametrize("N,C", sorted({(c[0], c[1]) for c in LISTED_CASES}))
def test_listed_pivot_lies_within_three_replicate_sigmas(orc, N, C):
    """The library's pivot (restated) sees no outlier; for the replicates held to 1e-12 -- those that drew none -- it lies
    within 3 of the replicate's sigmas of the replicate's means.  Replicates that drew one take the off-pivot bound."""
    x, u, w, rows = listed_data(N, C)
    piv = strided_pivot(x, u)
    F = stream_freq(orc, LISTED_SEED, LISTED_NREP, N)
    clean = F[:, rows].sum(axis=1) == 0
    print(f"\nN={N} C={C}: {int(clean.sum())} of {LISTED_NREP} replicates drew no outlier")
    assert clean.sum() >= 1 and cdiv(N, WIN) == len(rows) == 4
    for wt in (None, w):
        for r in np.flatnonzero(clean):
            W = F[r] * (1.0 if wt is None else wt)
            mu, su = wstat(u, W)
            mx, sx = wstat(x, W)
            assert abs(piv[0] - mu) <= 3 * su and np.all(np.abs(piv[1:] - mx) <= 3 * sx)


@gpu
@pytest.mark.parametrize("N,C,order,wt", LISTED_CASES)
def test_listed_mode_every_window_flagged(eng, orc, N, C, order, wt):
    nrep = LISTED_NREP
    x, u, w, rows = listed_data(N, C)
    w = w if wt else None
    F = stream_freq(orc, LISTED_SEED, nrep, N)
    got = run_single(eng, dev(x), dev(u), order, sampler=eng.DeviceSampler(LISTED_SEED, nrep, N), wd=None if w is None else dev(w), path="int8")
    info = eng.resample_info()
    print(f"\nlisted N={N} C={C} order={order}: {info}")
    assert info["windows_fp64"] == info["windows"] == cdiv(N, WIN) * cdiv(C, 32), info     # the listed FP64 kernel's result alone
    drew = F[:, rows].sum(axis=1) > 0
    hold(f"listed nblk={1 if C <= 16 else 2}" + (" + tail group" if C == 40 else ""), f"N={N} C={C} order={order} w={wt}", got.cpu().numpy(),
         truth(orc, x, u, order, F, w), rep_scale(x, u, order + 1, F, w), rtol=np.where(drew, off_pivot_rtol(order), RTOL))


def plan_i8_windows(N):
    """plan_i8 of txm_resample.hip: (tiles per scaling window, windows, fallback runs per flagged window)."""
    ntiles, wt = cdiv(N, SM_T), 256
    while wt > 4 and ntiles < 256 * wt:
        wt //= 4
    return wt, cdiv(ntiles, wt), wt // min(wt, 8)


@gpu
def test_listed_mode_second_matrix(eng, orc):
    """K = 1 in listed mode as the y run: every window flagged, so out_y is the listed FP64 kernel's and
    resample_finalize_y_kernel's alone."""
    N, C, order, nrep = LISTED_N, 32, 3, LISTED_NREP
    x, u, w, rows = listed_data(N, C)
    y = 0.5 * x + 0.25 + gas(N, C, 15)[0]
    F = stream_freq(orc, LISTED_SEED, nrep, N)
    got, ym = run_single(eng, dev(x), dev(u), order, sampler=eng.DeviceSampler(LISTED_SEED, nrep, N), wd=dev(w), path="int8", y=dev(y))
    info = eng.resample_info()
    assert info["windows_fp64"] == info["windows"] == 4, info
    drew = F[:, rows].sum(axis=1) > 0
    hold("listed with y", f"states N={N} C={C}", got.cpu().numpy(), truth(orc, x, u, order, F, w), rep_scale(x, u, order + 1, F, w),
         rtol=np.where(drew, off_pivot_rtol(order), RTOL))
    LD = np.longdouble
    fw = F.astype(LD) * w.astype(LD)[None, :]
    want = (fw @ y.astype(LD)) / fw.sum(axis=1)[:, None]
    ysig = np.stack([wstat(y, np.asarray(fw[r], dtype=np.float64))[1] for r in range(nrep)])
    e = float((np.abs(ym.cpu().numpy().astype(LD) - want) / (np.abs(want) + ysig)).max())
    print(f"\nlisted with y[means]: worst scaled err {e:.2e}")
    assert e <= RTOL


# more flagged runs than fallback chunks: one workgroup of the listed launch walks two runs (run += n_chunks).  The fallback
# plan has ntiles / 2 chunks, at most 1024, and a flagged window gives win_tiles / 8 runs, so it takes more than 8192 tiles
LONG_N, LONG_SEED, LONG_NREP = 8200 * SM_T + 5, 29, 2


@functools.lru_cache(maxsize=1)
def long_listed_data():
    x, u, w = gas.__wrapped__(LONG_N, 1, 16)
    u = u.copy()
    wt, nwin, per = plan_i8_windows(LONG_N)
    rows = np.arange(nwin) * (wt * SM_T) + 517
    assert rows[-1] < LONG_N and np.all(rows % (LONG_N // 1024) != 0)          # off the pivot's strided subsample
    u[rows] += OUT_U
    return x, u, rows


def test_long_listed_case_has_more_runs_than_chunks():
    wt, nwin, per = plan_i8_windows(LONG_N)
    q = plan(LONG_N, 1, LONG_NREP, 1, False, False, PLAIN)
    assert (wt, nwin, per) == (16, 513, 2) and q["n_chunks"] == 912 and q["n_chunks"] < nwin * per <= 2 * q["n_chunks"]
    assert plan_i8_windows(LISTED_N) == (4, 4, 1)
    long_listed_data()


@gpu
def test_listed_mode_one_workgroup_walks_two_runs(eng, orc):
    order = 1
    x, u, rows = long_listed_data()
    F = stream_freq.__wrapped__(orc, LONG_SEED, LONG_NREP, LONG_N)           # (134 MB of rows: not kept in the cache)
    got = run_single(eng, dev(x), dev(u), order, sampler=eng.DeviceSampler(LONG_SEED, LONG_NREP, LONG_N), path="int8")
    info = eng.resample_info()
    print(f"\nlisted N={LONG_N}: {info}")
    assert info["windows_fp64"] == info["windows"] == 513, info
    assert np.all(F[:, rows].sum(axis=1) > 0)
    hold("listed, two runs a workgroup", f"N={LONG_N} C=1 order={order}", got.cpu().numpy(), truth(orc, x, u, order, F),
         rep_scale(x, u, order + 1, F, None), rtol=off_pivot_rtol(order), nsamp=LONG_N)


# ---- N = 2: a replicate that drew one of the two samples ---------------------------------------------------------------------
ONE_OF_TWO = [(3, 2, False, False), (3, 4, True, False), (33, 8, False, False), (33, 3, True, True), (3, 8, True, True), (16, 5, False, True)]


def one_of_two(orc, C, wt):
    x, u, w = gas(2, C, 14)
    w = w if wt else None
    F = stream_freq(orc, 123, 17, 2)
    single = (F > 0).sum(axis=1) == 1
    assert 3 <= single.sum() <= 14
    return x, u, w, F, single


@pytest.mark.parametrize("C,wt", sorted({(c[0], c[2]) for c in ONE_OF_TWO}))
def test_one_of_two_samples_lies_within_three_data_sigmas_of_the_pivot(orc, C, wt):
    """Such a replicate has no spread of its own; its one sample lies half the data's spread from the call's pivot (the mean
    of both samples), which is within 3 of the DATA's weighted sigmas: the premise of the off-pivot bound with those sigmas."""
    x, u, w, F, single = one_of_two(orc, C, wt)
    _, su = wstat(u, w)
    _, sx = wstat(x, w)
    assert np.all(np.abs(u - u.mean()) <= 3 * su) and np.all(np.abs(x - x.mean(axis=0)) <= 3 * sx)


@gpu
@pytest.mark.parametrize("C,order,wt,ex", ONE_OF_TWO)
def test_two_samples_one_drawn(eng, orc, C, order, wt, ex):
    """The replicates of an N = 2 bootstrap that drew ONE sample: known exactly, {f w, u_i, x_i, zeros}, and -- their own sigma
    being zero and their sample off the pivot -- held to the off-pivot bound 4^order 3e-13 with the data's sigmas (the one-ulp
    scale of the rule cannot be met about a pivot the replicates share: 4e12 .. 4e98 of it measured at orders 2 .. 8).  The
    replicates that drew both samples are held to the rule itself."""
    x, u, w, F, single = one_of_two(orc, C, wt)
    t, sc = truth(orc, x, u, order, F, w), rep_scale(x, u, order + 1, F, w)
    _, su = wstat(u, w)
    _, sx = wstat(x, w)
    for b in range(order + 1):
        sc[single, :, 0, b] = su ** b
        sc[single, :, 1, b] = (sx * su ** b)[None, :]
    got = run_single(eng, dev(x), dev(u), order, F=F if ex else None, sampler=None if ex else eng.DeviceSampler(123, 17, 2),
                     wd=None if w is None else dev(w))
    hold("N = 2, one sample drawn", f"C={C} order={order} w={wt} explicit={ex}", got.cpu().numpy(), t, sc,
         rtol=np.where(single, off_pivot_rtol(order), RTOL), nsamp=None if (wt or ex) else 2)


# ---- the row pitch -----------------------------------------------------------------------------------------------------------
def pitch_ok(ld, C):
    """include/txmom.h TXM_RESAMPLE_PITCH_OK"""
    return 768 * ld + C <= 1 << 29


PITCH_EDGES = [(699050, 1), (699050, 3), (699050, 512), (699050, 513), (699050, 600), (699051, 1), (699052, 3), (699000, 600),
               (698141, 698141), (698142, 698142), (66, 64), (1 << 29, 1)]


def fake_call(L, ld, C):
    """txm_resample_vals with pointers that are never followed: the pitch is judged before anything else looks at them."""
    fake = ct.c_void_p(4096)
    return L.txm_resample_vals(fake, ld, 1, fake, None, 1024, C, 0, 1, None, None, None, None, fake, None, fake, 0, None)


def test_pitch_rule_is_what_the_lane_offsets_hold():
    """lane_xoff of resample_kernel is (3 * 256 * ldx_s + column) * 8 in 32 unsigned bits, and in the plain and batched launches
    the column runs up to C - 1 (the base is the unshifted x): the rule is that offset below 2^32 -- for a 600-column window
    of a pitch below 699050 and for a tight array of 698142 columns as much as for a pitch above 699050.  The header's
    macro, the engine's copy rule and the library itself (refusing through the C ABI before it touches a pointer) agree."""
    from thermoextrap_amd import _build, _lib, engine

    _build.build_library()                                   # (as the ABI tests' fixture does: no device needed)
    hdr = (Path(__file__).resolve().parent.parent / "include" / "txmom.h").read_text()
    assert "#define TXM_RESAMPLE_PITCH_OK(ld, C) (768 * (int64_t)(ld) + (int64_t)(C) <= ((int64_t)1 << 29))" in hdr
    L = _lib.load()
    tab = (_lib.StatePtrs * 1)()
    tab[0].x = tab[0].u = 4096
    fake = ct.c_void_p(4096)
    for ld, C in PITCH_EDGES:
        fits = (3 * 256 * ld + (C - 1)) * 8 < 2 ** 32
        assert pitch_ok(ld, C) == fits == engine.resample_pitch_ok(ld, C), (ld, C)
        # refused: TXM_ERR_UNSUPPORTED; accepted: the next check fails (neither freq nor a sampler): TXM_ERR_INVALID
        assert fake_call(L, ld, C) == (-1 if fits else -4), (ld, C, _lib.last_error())
        if not fits:
            assert "536870912" in _lib.last_error()
        rc = L.txm_resample_vals_batched(tab, 1, ld, 1024, C, 0, 1, None, None, None, fake, fake, 0, None)
        assert rc == (-1 if fits else -4), (ld, C, _lib.last_error())
    assert [pitch_ok(*e) for e in PITCH_EDGES] == [True, True, True, False, False, False, False, True, True, False, True, False]


@gpu
def test_a_row_pitch_beyond_the_lane_offsets(eng, orc):
    """N = 1024 rows of pitch 699052 and of pitch 699050 doubles in buffers that really are that large (5.7 GB each, only the
    used columns written).  Pitch 699052, 3 columns, and pitch 699050, 600 columns: the C ABI refuses the call before anything
    is enqueued; the engine copies the window to a tight array and meets the oracle.  Pitch 699050, 3 columns: the largest
    pitch there is runs through the C ABI as it stands and meets the oracle.  (The unchecked kernel read the wrong columns
    -- inside these buffers.)"""
    from thermoextrap_amd import _lib

    L = _lib.load()
    p = lambda t: None if t is None else ct.c_void_p(t.data_ptr())  # noqa: E731
    st = ct.c_void_p(torch.cuda.current_stream().cuda_stream)
    N = 1024

    def raw(xd, pitch, ud, C, order, nrep, s, F, out):
        ws = eng.workspace(L.txm_resample_vals_ws_bytes(N, C, nrep, order))
        return L.txm_resample_vals(p(xd), pitch, 1, p(ud), None, N, C, order, nrep, p(F), None if s is None else ct.byref(s.spec),
                                   None if s is None else p(s.counts), None, p(out), None, p(ws), ws.numel(), st)

    for pitch, C, order, nrep in ((699052, 3, 4, 17), (699050, 600, 1, 3), (699050, 3, 4, 17)):
        x, u, w = gas(N, C, 12)
        wide = torch.empty((N, pitch), dtype=torch.float64, device="cuda")
        wide[:, 5:5 + C] = dev(x)
        xd = wide[:, 5:5 + C]
        assert xd.stride(0) == pitch
        ud = dev(u)
        out = torch.full((nrep, C, 2, order + 1), 7.0, dtype=torch.float64, device="cuda")
        s = eng.DeviceSampler(99, nrep, N)
        F = s.freq()
        Fh = stream_freq(orc, 99, nrep, N)
        t, sc = truth(orc, x, u, order, Fh), rep_scale(x, u, order + 1, Fh, None)
        if pitch_ok(pitch, C):
            assert raw(xd, pitch, ud, C, order, nrep, s, None, out) == 0, _lib.last_error()
            hold("row pitch", f"pitch {pitch} C={C} through the C ABI", out.cpu().numpy(), t, sc, nsamp=N)
            assert raw(xd, pitch, ud, C, order, nrep, None, F, out) == 0, _lib.last_error()
            hold("row pitch", f"pitch {pitch} C={C} through the C ABI, explicit", out.cpu().numpy(), t, sc)
        else:
            for args in ((s, None), (None, F)):
                rc = raw(xd, pitch, ud, C, order, nrep, *args, out)
                assert rc == -4 and "536870912" in _lib.last_error(), (rc, _lib.last_error())      # TXM_ERR_UNSUPPORTED
            tab = (_lib.StatePtrs * 1)()
            tab[0].x, tab[0].u, tab[0].w = xd.data_ptr(), ud.data_ptr(), None
            ws = eng.workspace(L.txm_resample_vals_batched_ws_bytes(1, N, C, nrep, order))
            rc = L.txm_resample_vals_batched(tab, 1, pitch, N, C, order, nrep, p(F), None, None, p(out), p(ws), ws.numel(), st)
            assert rc == -4 and "536870912" in _lib.last_error(), (rc, _lib.last_error())
            torch.cuda.synchronize()
            assert bool((out == 7.0).all())                                                        # nothing was enqueued
        for ex in (False, True):
            got = run_single(eng, xd, ud, order, F=Fh if ex else None, sampler=None if ex else eng.DeviceSampler(99, nrep, N))
            hold("row pitch", f"pitch {pitch} C={C} through the engine explicit={ex}", got.cpu().numpy(), t, sc, nsamp=None if ex else N)
        del wide, xd


# ---- replicates of non-zero weight are bit for bit what they were ------------------------------------------------------------
@gpu
def test_outputs_equal_the_stored_ones_bit_for_bit(eng):
    """The finalize kernels write the empty state for a weight sum of exactly zero and leave every other replicate alone: the
    outputs stored by tests/golden/make_resample_golden.py (written once, with the build before that change) are reproduced
    bit for bit."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("make_resample_golden", GOLDEN.parent / "make_resample_golden.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    g = np.load(GOLDEN)
    got = mod.compute(eng, {k: g[k] for k in g.files if k.startswith("in_")})
    assert sorted(got) == sorted(k for k in g.files if k.startswith("out_")) and len(got) == 3
    for k, v in got.items():
        assert np.array_equal(v, g[k]), k
