"""Differential tests of the reduction family of txm_reduce.hip -- txm_reduce_vals, txm_reduce_vals_1d,
txm_reduce_vals_batched, txm_reduce_vals_pivot[_w] / _sums, txm_sums_to_state, txm_push_vals -- against the long-double
two-pass definition (oracle.truth_cov / truth_1d, weights supported) on the same float64 inputs, on every path of their
dispatch: every reduce_rowmajor_kernel<K, VEC, LPR_LOG2, WEIGHTED> instantiation, a second and third column chunk, the
unrolled main loop on several trips, both load paths of reduce_colmajor_kernel (16-byte pairs and the scalar fallback of a
misaligned series, u or w), the batched launch with and without 16-byte alignment and with more states than one state's
grid, and the sharded / streaming pieces.  tests/test_kernels_gpu.py, test_push_shard_gpu.py and test_batched_gpu.py reach
about ten (VEC, LPR_LOG2) pairs at one order each and one kind of weights (rng.random(N) + 0.05).

Rule (README "Tolerances"): a comoment is held to |hip - ref| <= 1e-12 (|ref| + sigma_x^a sigma_u^b), where the sigmas are
the WEIGHTED standard deviations of the call (the natural scale of a weighted moment: np.std of the unweighted data is
the wrong one as soon as the weights select), each floored at one ulp of the corresponding weighted mean so that a
constant column has a scale.  Where cmomy's conventions matter (total weight zero -> the empty state) the expectation is
oracle.reduce_vals.

Weighted pivot.  With weights the kernels accumulate about the weighted mean of a strided subsample (txm_pivot.h;
`pivot_rule` below restates it).  That is still an estimate: for the concentrated-weight kinds the restated rule's pivot
is asserted, on the CPU, to lie within 3 weighted sigmas of the weighted means, and the moments are held to the README's
model bound for such a pivot, 4^order * 3e-13 (the bound tests/test_fullsize_gpu.py uses for a caller's off-centre pivot).
Every other kind stays at 1e-12.  With the unweighted strided pivot this family had before (N = 20000, 3 observables,
order 4, the parent build on an MI355X; profiles/r12_reduce_kernels_gpu_tests.txt) the concentrated-weight, poisoned
zero-weight-row and zero-total-weight kinds miss these bounds by many orders of magnitude or return NaN.

The tests that need no device (the coverage of the case tables, the pivot rule's distance, the oracle's empty state) carry
no gpu mark and run with the CPU suite.  Every GPU case prints its worst scaled error (run with -s).
"""

import ctypes as ct
import functools
from pathlib import Path

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
RTOL = 1e-12
LD = np.longdouble
GOLDEN = Path(__file__).resolve().parent / "golden" / "reduce_unweighted_parent.npz"
WORST: dict = {}


@pytest.fixture(scope="module")
def eng(txm):
    from thermoextrap_amd import engine

    return engine


@pytest.fixture(scope="module")
def cus(txm):
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    if WORST:
        print("\nworst scaled error per entry point: " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(WORST.items())))


def dev(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64).cuda()      # (a copy: the cached inputs are read-only)


def dev_off8(a):
    """``a`` on the device, 8 bytes past a 16-byte boundary (torch allocations are at least 256-byte aligned)."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    buf = torch.empty(a.size + 1, dtype=torch.float64, device="cuda")
    v = buf[1:].view(a.shape)
    v.copy_(torch.tensor(a))
    assert v.data_ptr() % 16 == 8 and v.is_contiguous()
    return v


def dev_pitched(x, pitch, col0=0):
    """x (N, C) as columns [col0, col0 + C) of rows of ``pitch`` doubles, NaN elsewhere."""
    wide = torch.full((x.shape[0], pitch), float("nan"), dtype=torch.float64, device="cuda")
    wide[:, col0:col0 + x.shape[1]] = dev(x)
    return wide[:, col0:col0 + x.shape[1]]


def dev_series(x, ld):
    """x (N, C) in the (val, rec) layout: a transposed view of a (C, ld) array, NaN behind each series."""
    N, C = x.shape
    buf = torch.full((C, ld), float("nan"), dtype=torch.float64, device="cuda")
    buf[:, :N] = dev(x.T)
    return buf[:, :N].t()


def cdiv(a, b):
    return -(-a // b)


# ---- data ---------------------------------------------------------------------------------------------------------------
def idealgas(rng, N, C):
    """u ~ N(174.85, 5.31^2) (the ideal-gas notebook scale: 3 % relative spread, the cancellation regime), x_c = a_c + b_c u +
    noise -- the generator of tests/test_kernels_gpu.py."""
    u = rng.normal(174.85, 5.31, N)
    a = rng.normal(0.0, 1.0, C)
    b = rng.normal(1e-3, 5e-4, C)
    x = a[None, :] + b[None, :] * u[:, None] + rng.normal(0, 0.05, (N, C))
    return x, u


def plain_weights(rng, N):
    return rng.random(N) + 0.05


CONCENTRATED = {"conc_f0.05_s0.05": (0.05, 3.0, 0.05), "conc_f0.01_s0.1": (0.01, 4.0, 0.1),
                "conc_f0.01_s0.01": (0.01, 4.0, 0.01), "conc_f0.001_s0.001": (0.001, 4.0, 0.001)}
# 1024 < N < 2048: a subsample of stride N // 1024 = 1 is the FIRST 1024 rows, not the series (and for any N a stride of
# N // 1024 leaves up to a third of the rows, the last ones, unseen).  u sorted ascending and the weight in the rows past
# 1024: a mask on 30 rows, or reweighting weights exp(3 (u - max u)).  A weighted mean of the first 1024 rows -- whether
# taken because "stride 1" was read as "the whole series", or because those rows pass the effective-count test among
# themselves (they do for the exp kinds: ~33 rows) -- sits 40 to 75 weighted sigma out.  The weighted rule therefore
# spreads its samples over the whole series.
TAIL = {"tail_mask_N1500": 1500, "tail_mask_N2047": 2047, "tail_exp_N1500": 1500, "tail_exp_N2047": 2047}
KINDS = ["idealgas", "u_1e8", "const_column", "u_sorted", "half_zero", "zero_rows_1e150", *CONCENTRATED, "stride_miss",
         "total_zero", *TAIL]
KIND_N, KIND_C, KIND_ORDER = 20000, 3, 4


@functools.lru_cache(maxsize=None)
def kind_data(kind, N=KIND_N, C=KIND_C, seed=0):
    """(x, u, w) of one data kind; w is None for the unweighted kinds.  The TAIL kinds have their own N."""
    N = TAIL.get(kind, N)
    rng = np.random.default_rng([KINDS.index(kind), N, C, seed])
    x, u = idealgas(rng, N, C)
    w = None
    if kind == "u_1e8":                                     # mean / sigma = 1e8
        u = 1e8 + rng.normal(0.0, 1.0, N)
        x = 0.2 + 1e-3 * u[:, None] + rng.normal(0, 0.05, (N, C))
        w = plain_weights(rng, N)
    elif kind == "const_column":
        x[:, C // 2] = 0.1 + 1.0 / 3.0
        w = plain_weights(rng, N)
    elif kind == "u_sorted":                                # a strided subsample of a sorted series is still a fair one
        o = np.argsort(u)
        x, u = x[o], u[o]
    elif kind == "half_zero":
        w = plain_weights(rng, N)
        w[rng.permutation(N)[: N // 2]] = 0.0
    elif kind == "zero_rows_1e150":                         # cmomy skips rows of weight zero, whatever they hold
        w = plain_weights(rng, N)
        z = rng.permutation(N)[: N // 8]
        w[z] = 0.0
        u[z[::2]] = 1e150
        x[z[1::2]] = -1e150
    elif kind in CONCENTRATED:                              # a fraction f carries all the weight; it sits `shift` sigma out
        f, shift, s = CONCENTRATED[kind]                    # with spread s sigma (reweighting exp(-dbeta u), a mask)
        idx = rng.choice(N, max(int(f * N), 4), replace=False)
        u[idx] = 174.85 + shift * 5.31 + rng.normal(0, s * 5.31, len(idx))
        x[idx] = 0.3 + 1e-3 * u[idx, None] + rng.normal(0, 0.05 * s, (len(idx), C))
        w = np.zeros(N)
        w[idx] = plain_weights(rng, len(idx))
    elif kind == "stride_miss":                             # a subsample of stride N // 1024 sees no weight at all
        w = plain_weights(rng, N)
        w[np.arange(N) % (N // 1024) == 0] = 0.0
    elif kind == "total_zero":
        w = np.zeros(N)
    elif kind in TAIL:
        o = np.argsort(u)
        x, u = x[o], u[o]
        if "mask" in kind:
            w = np.zeros(N)
            w[1100:1130] = plain_weights(rng, 30)
        else:
            w = np.exp(3.0 * (u - u.max()))
    for a in (x, u, w):
        if a is not None:
            a.setflags(write=False)
    return x, u, w


def kind_rtol(kind, order):
    return 4.0 ** order * 3e-13 if kind in CONCENTRATED else RTOL


# ---- reference and rule -------------------------------------------------------------------------------------------------
def wstat(v, w):
    """Weighted mean and standard deviation along axis 0 (float64 two-pass: a scale, not a reference), the deviation
    floored at one ulp of the mean."""
    v = np.asarray(v, dtype=np.float64)
    ww = np.ones(v.shape[0]) if w is None else np.asarray(w, dtype=np.float64)
    keep = ww != 0.0                                        # rows of weight zero may hold anything
    vv, ww = v[keep], ww[keep]
    m = np.tensordot(ww, vv, axes=(0, 0)) / ww.sum()
    s = np.sqrt(np.tensordot(ww, (vv - m) ** 2, axes=(0, 0)) / ww.sum())
    return m, np.maximum(s, np.spacing(np.abs(m)))


def moment_scale(x, u, order, w=None):
    """scale[c, a, b] = sigma_x[c]^a sigma_u^b with the weighted sigmas of the call."""
    _, sx = wstat(x, w)
    _, su = wstat(u, w)
    sc = np.empty((x.shape[1], 2, order + 1))
    for b in range(order + 1):
        sc[:, 0, b] = su ** b
        sc[:, 1, b] = sx * su ** b
    return sc


def scaled_err(got, ref, scale):
    got = np.asarray(got)
    assert got.shape == ref.shape and np.all(np.isfinite(got)), "shape or a non-finite entry"
    return float((np.abs(got - ref) / (np.abs(ref) + scale)).max())


def hold(entry, name, got, ref, scale, rtol=RTOL):
    if not np.any(scale):                                   # the empty state: exactly zeros
        assert not np.any(ref) and np.array_equal(np.asarray(got), ref), (entry, name, "not the empty state")
        print(f"\n{entry}[{name}]: the empty state")
        return
    e = scaled_err(got, ref, scale)
    WORST[entry] = max(WORST.get(entry, 0.0), e)
    print(f"\n{entry}[{name}]: worst scaled err {e:.2e} (limit {rtol:.1e})")
    assert e <= rtol, (entry, name, e)


def truth_cov(orc, x, u, order, w=None):
    """oracle.truth_cov; a single sample's state is known exactly -- {w, u, x, zeros} -- and is used as such: the
    reference's mean (w u) / w carries a long-double rounding, whose square is 2e-7 of the scale ulp(u)^2 of one sample."""
    if len(u) > 1:
        return orc.truth_cov(x, u, order, w=w)
    t = np.zeros((x.shape[1], 2, order + 1))
    t[:, 0, 0] = 1.0 if w is None else w[0]
    t[:, 1, 0] = x[0]
    if order >= 1:
        t[:, 0, 1] = u[0]
    return t


def truth_rows(orc, rows, mom, w, r0=None):
    """truth_1d per row; ``r0``: per-row shifts, see kind_shift."""
    if rows.shape[1] == 1:                                  # one sample: exactly {w, u, zeros} (see truth_cov)
        t = np.zeros((len(rows), mom + 1))
        t[:, 0] = 1.0 if w is None else w[0]
        t[:, 1:2] = rows[:, :mom]
        return t
    if r0 is None:
        return np.stack([orc.truth_1d(r, mom, w=w) for r in rows])
    t = np.stack([orc.truth_1d(exact_minus(r, s), mom, w=w) for r, s in zip(rows, r0)])
    if mom >= 1:
        t[:, 1] += r0
    return t


def exact_minus(v, v0):
    """v - v0, asserted to be exact (no rounding), so that the moments about the mean are those of v."""
    d = v - v0
    assert np.array_equal(d.astype(LD), v.astype(LD) - np.asarray(v0, dtype=LD)), "the shift is not exact"
    return d


def kind_shift(kind, x, u):
    """(x0[C], u0) or None.  The long-double two-pass reference carries its own error: its mean is good to about
    N 2^-64 |mean|, and a mean off by d moves the odd central moments by d / sigma of their scale.  That is far inside 1e-12
    for the ideal-gas scale (mean / sigma = 33), but for u = 1e8 + N(0, 1) it is 1e-9 (measured: both builds 'miss' the
    unshifted reference by 1.03e-9, identically on every entry point), and for a constant column c, whose scale is one ulp
    of c, the reference's own <x> - c ~ 1e-19 c is 1e-3 of that scale.  Central moments do not change when a constant is
    subtracted from the samples, so for these two kinds the SAME reference is taken on inputs shifted by a constant whose
    subtraction is exact in float64 (asserted), and the shift is added back to the means: 1e8 and the rounded column means
    for u_1e8; c itself for the constant column, whose exact moments -- zeros -- the reference then returns."""
    C = x.shape[1]
    if kind == "u_1e8":
        return np.round(x.mean(axis=0)), 1e8
    if kind == "const_column":
        x0 = np.zeros(C)
        x0[C // 2] = x[0, C // 2]
        return x0, 0.0
    return None


def scale_rows(rows, mom, w):
    _, s = wstat(rows.T, w)
    return s[:, None] ** np.arange(mom + 1)[None, :]


def pivot_rule(v, w):
    """The documented weighted rule for one series (include/txmom.h), written from that text: the weighted
    mean of ns = min(N, 1024) samples spread evenly over the series (rows floor(k N / ns)) when their weight sum is
    positive and they ARE the whole series (N <= 1024) or carry a Kish effective count of at least 32; else the weighted
    mean of every row; else (no weight at all) the unweighted mean of those samples."""
    N = len(v)
    ns = min(N, 1024)
    idx = (np.arange(ns) * N) // ns
    whole = ns == N
    vs, ws = v[idx], w[idx]
    nz = ws != 0.0
    sw, sww = ws[nz].sum(), (ws[nz] ** 2).sum()
    if np.isfinite(sw) and sw > 0.0 and (whole or sw * sw >= 32.0 * sww):
        p = (ws[nz] * vs[nz]).sum() / sw
        if np.isfinite(p):
            return p, "subsample"
    if not whole:
        nz = w != 0.0
        sw = w[nz].sum()
        if np.isfinite(sw) and sw > 0.0:
            p = (w[nz] * v[nz]).sum() / sw
            if np.isfinite(p):
                return p, "all rows"
    p = vs.mean()
    return (p if np.isfinite(p) else 0.0), "unweighted"


# ---- what needs no device -----------------------------------------------------------------------------------------------
def plan_rowmajor(C, pitch, aligned, N, cus=256):
    """plan_rowmajor / grid_x_for of txm_reduce.hip: VEC, log2 lanes per row, column chunks, blocks along the rows, and how
    many trips the 4-row unrolled main loop makes for the slowest row slot."""
    vec = 2 if (C % 2 == 0 and pitch % 2 == 0 and aligned) else 1
    lanes, l2 = cdiv(C, vec), 0
    while (1 << l2) < lanes and l2 < 8:
        l2 += 1
    rows = 256 >> l2
    gx = max(1, min(cdiv(N, rows * 4), cus * 8))
    stride = gx * rows
    return {"vec": vec, "l2": l2, "chunks": cdiv(C, (1 << l2) * vec), "gx": gx, "rows": rows,
            "main_trips": max(0, (N - 1 - 3 * stride) // (4 * stride) + 1) if N > 3 * stride else 0,
            "tail": N % (4 * stride) != 0}


# (C, pitch, first column, aligned base): VEC = 2 from an aligned base with an even pitch, VEC = 1 from an odd C, an odd pitch
# or a pitched single column
ROW_N = 301
ROW_VEC2 = [(C, C + 2 * (i % 2), 0) for i, C in enumerate((2, 4, 8, 16, 32, 64, 128, 256, 512, 514))]
ROW_VEC1 = [(1, 3, 1), (2, 3, 0), (3, 3, 0), (5, 8, 0), (9, 9, 0), (17, 20, 1), (33, 33, 0), (65, 65, 0), (129, 130, 0),
            (257, 257, 0), (513, 513, 0)]
ROW_CASES = [(C, pitch, col0, order, wt) for (C, pitch, col0) in ROW_VEC2 + ROW_VEC1 for order in range(9) for wt in (False, True)]
SMALL_N_CASES = [(N, 3, 3, 0) for N in (1, 2, 3)] + [(50, 3, 3, 0), (20, 16, 16, 0), (100, 2, 2, 0), (1, 2, 2, 0), (2, 16, 16, 0)]


def case_pair(C, pitch, col0):
    p = plan_rowmajor(C, pitch, col0 % 2 == 0, ROW_N)
    return p["vec"], p["l2"]


def test_row_cases_cover_every_instantiation():
    """Every reduce_rowmajor_kernel<K, VEC, LPR_LOG2, WEIGHTED> the library can launch -- 9 x 2 x 9 x 2 -- is named by the
    parametrisation, from the dispatch rule restated above; so are a second and a third column chunk on both load widths."""
    seen = {(order + 1, *case_pair(C, pitch, col0), wt) for (C, pitch, col0, order, wt) in ROW_CASES}
    assert seen == {(K, vec, l2, wt) for K in range(1, 10) for vec in (1, 2) for l2 in range(9) for wt in (False, True)}
    assert [case_pair(*c) for c in ROW_VEC2] == [(2, l2) for l2 in range(9)] + [(2, 8)]
    assert [case_pair(*c) for c in ROW_VEC1] == [(1, l2) for l2 in range(9)] + [(1, 8), (1, 8)]
    assert plan_rowmajor(514, 514, True, ROW_N)["chunks"] == 2 and plan_rowmajor(257, 257, True, ROW_N)["chunks"] == 2
    assert plan_rowmajor(513, 513, True, ROW_N)["chunks"] == 3
    assert plan_rowmajor(1, 3, False, ROW_N)["l2"] == 0                       # the pitched single column
    for N, C, pitch, col0 in SMALL_N_CASES:                                   # fewer rows than one block's row slots
        assert N < plan_rowmajor(C, pitch, True, N)["rows"]
    assert {c[1] for c in SMALL_N_CASES[3:6]} == {3, 16, 2}


def test_col_cases_cover_both_load_paths():
    """Every (N, C) runs the pair loads ("aligned") and the scalar loop of a misaligned series ("x_odd") in both weight
    modes; all but the 240 MB shape also with u, and with w, 8 bytes off."""
    for N in COL_N:
        for C in COL_C:
            for wt in (False, True):
                have = {v for (n, c, t, v) in COL_CASES if (n, c, t) == (N, C, wt)}
                want = {"aligned", "x_odd"} if N * C > 10 ** 7 else {"aligned", "x_odd", "u_off"} | ({"w_off"} if wt else set())
                assert have == want, (N, C, wt, have)
    assert (4099, 300) in {(n, c) for (n, c, *_) in COL_CASES}                # the grid halving of launch_colmajor_cov
    gx = cdiv(4099, 512 * 4)
    assert gx > 1 and gx * 300 <= 256 * 16                                    # (two blocks a series fit; 100001 x 300 halves)
    assert cdiv(100001, 512 * 4) * 300 > 256 * 16


@pytest.mark.parametrize("kind", list(CONCENTRATED) + ["stride_miss", "zero_rows_1e150", "half_zero"] + list(TAIL))
def test_pivot_rule_stays_within_three_weighted_sigmas(kind):
    """delta = |pivot - weighted mean| / sigma_w over u and the columns, from the restated rule: at most 3 -- the premise of
    the 4^order 3e-13 bound the concentrated kinds are held to.  (The unweighted strided pivot sits 60 ... 4000 sigma_w out.)"""
    x, u, w = kind_data(kind)
    delta, old, how = 0.0, 0.0, set()
    for v in [u, *x.T]:
        m, s = wstat(v, w)
        p, h = pivot_rule(v, w)
        how.add(h)
        delta = max(delta, abs(p - m) / s)
        old = max(old, abs(v[np.arange(1024) * (len(v) // 1024)].mean() - m) / s)
    print(f"\n{kind}: delta {delta:.3f} ({sorted(how)}); the unweighted strided pivot: {old:.3g}")
    assert delta <= 3.0
    if "tail_mask" in kind or kind in ("conc_f0.01_s0.01", "conc_f0.001_s0.001"):
        assert how == {"all rows"} and delta < 1e-6          # too little weight in the subsample: the exact weighted mean
    if kind in TAIL:                                        # (the first-1024-rows pivots: unweighted / weighted)
        assert 1024 < len(u) < 2048 and old > 30.0
        sub = slice(0, 1024)
        if w[sub].any():
            assert abs((w[sub] * u[sub]).sum() / w[sub].sum() - wstat(u, w)[0]) / wstat(u, w)[1] > 30.0
    if kind in CONCENTRATED:
        assert old > 50.0
    if kind == "zero_rows_1e150":
        assert old > 1e100


def test_oracle_gives_the_empty_state_for_total_weight_zero(orc):
    x, u, w = kind_data("total_zero")
    assert w is not None and not w.any()
    assert not orc.reduce_vals(x, u, KIND_ORDER, w=w).any()
    assert not orc.reduce_vals_1d(np.stack([u, x[:, 0]]), KIND_ORDER, w=w).any()


# ---- group A: txm_reduce_vals, row-major --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def row_inputs(C, N=ROW_N):
    rng = np.random.default_rng([1, N, C])
    x, u = idealgas(rng, N, C)
    w = plain_weights(rng, N)
    return x, u, w


@functools.lru_cache(maxsize=8)
def row_truth(orc, C, weighted, N=ROW_N):
    """The order-8 truth: a moment does not depend on how many higher ones are asked for, so order k is its first k + 1."""
    x, u, w = row_inputs(C, N)
    t = orc.truth_cov(x, u, 8, w=w if weighted else None)
    sc = moment_scale(x, u, 8, w if weighted else None)
    t.setflags(write=False)
    sc.setflags(write=False)
    return t, sc


def raw_reduce_vals(eng, xt, ls, lc, u, w, N, C, order):
    """txm_reduce_vals through the C ABI with the strides as given (engine.reduce_vals copies a pitched single column into
    a contiguous series, which is the col-major kernel)."""
    from thermoextrap_amd import _lib

    L = _lib.load()
    out = torch.empty((C, 2, order + 1), dtype=torch.float64, device="cuda")
    ws = eng.workspace(L.txm_reduce_vals_ws_bytes(N, C, order))
    p = lambda t: None if t is None else ct.c_void_p(t.data_ptr())  # noqa: E731
    _lib.check(L.txm_reduce_vals(p(xt), ls, lc, p(u), p(w), N, C, order, p(out), p(ws), ws.numel(),
                                 ct.c_void_p(torch.cuda.current_stream().cuda_stream)), "txm_reduce_vals")
    return out


def run_rowmajor(eng, x, u, w, order, pitch, col0):
    N, C = x.shape
    xd = dev_pitched(x, pitch, col0) if (pitch != C or col0) else dev(x)
    assert (xd.data_ptr() % 16 == 0) == (col0 % 2 == 0)
    ud, wd = dev(u), (None if w is None else dev(w))
    if C == 1:
        return raw_reduce_vals(eng, xd, pitch, 1, ud, wd, N, C, order).cpu().numpy()
    assert N == 1 or xd.stride(0) == pitch
    return eng.reduce_vals(xd, ud, order, w=wd).cpu().numpy()


@gpu
@pytest.mark.parametrize("C,pitch,col0,order,weighted", ROW_CASES)
def test_rowmajor_every_instantiation(eng, orc, C, pitch, col0, order, weighted):
    x, u, w = row_inputs(C)
    t, sc = row_truth(orc, C, weighted)
    got = run_rowmajor(eng, x, u, w if weighted else None, order, pitch, col0)
    K = order + 1
    hold("reduce_vals rowmajor", f"C={C} vec/l2={case_pair(C, pitch, col0)} order={order} w={weighted}", got, t[:, :, :K], sc[:, :, :K])


@gpu
@pytest.mark.parametrize("N,C,pitch,col0", SMALL_N_CASES)
@pytest.mark.parametrize("weighted", [False, True])
def test_rowmajor_fewer_rows_than_row_slots(eng, orc, N, C, pitch, col0, weighted):
    x, u, w = row_inputs(C, N)
    w = w if weighted else None
    got = run_rowmajor(eng, x, u, w, 4, pitch, col0)
    hold("reduce_vals rowmajor", f"N={N} C={C} w={weighted}", got, truth_cov(orc, x, u, 4, w), moment_scale(x, u, 4, w))


@gpu
@pytest.mark.parametrize("which", ["C257", "C2"])
@pytest.mark.parametrize("weighted", [False, True])
def test_rowmajor_main_loop_trips(eng, orc, cus, which, weighted):
    """The 4-row unrolled main loop beyond its first trip: rows above the grid cap of num_cus * 8 blocks.  C = 257: one row
    a block, 20011 rows (two trips and a tail on 256 CUs); C = 2: 256 rows a block, N = 4 strides of the capped grid plus a
    tail of 202851 rows (2_300_003 on 256 CUs): a full trip on every slot, a tail row on some."""
    if which == "C257":
        N, C = 20011, 257
        p = plan_rowmajor(C, C, True, N, cus)
        assert (p["vec"], p["l2"], p["chunks"]) == (1, 8, 2) and p["gx"] == min(cdiv(N, 4), cus * 8) and p["tail"]
        assert p["main_trips"] >= 2 or cus * 8 * 8 > N
    else:
        C = 2
        N = cus * 8 * 256 * 4 + 202_851
        p = plan_rowmajor(C, C, True, N, cus)
        assert (p["vec"], p["l2"]) == (2, 0) and p["gx"] == cus * 8 and p["main_trips"] >= 1 and p["tail"]
    x, u, w = row_inputs(C, N)
    w = w if weighted else None
    got = eng.reduce_vals(dev(x), dev(u), 4, w=None if w is None else dev(w)).cpu().numpy()
    hold("reduce_vals rowmajor", f"N={N} C={C} w={weighted} trips={p['main_trips']}", got, orc.truth_cov(x, u, 4, w=w),
         moment_scale(x, u, 4, w))


# ---- group B: txm_reduce_vals, (val, rec) layout and C == 1 -------------------------------------------------------------
COL_N, COL_C = (1, 2, 3, 64, 4099, 100001), (1, 3, 300)
COL_CASES = [(N, C, wt, v) for N in COL_N for C in COL_C for wt in (False, True)
             for v in (("aligned", "x_odd") if N * C > 10 ** 7 else ("aligned", "x_odd", "u_off", "w_off"))
             if wt or v != "w_off"]


@functools.lru_cache(maxsize=2)
def col_inputs(orc, N, C, weighted):
    order = 8 if C == 3 else 4
    rng = np.random.default_rng([2, N, C])
    x, u = idealgas(rng, N, C)
    w = plain_weights(rng, N) if weighted else None
    return x, u, w, order, truth_cov(orc, x, u, order, w), moment_scale(x, u, order, w)


@gpu
@pytest.mark.parametrize("N,C,weighted,variant", COL_CASES)
def test_colmajor_both_load_paths(eng, orc, N, C, weighted, variant):
    """reduce_colmajor_kernel<K, true, WEIGHTED>: 16-byte pair loads when the series, u and w are 16-byte aligned, the
    scalar loop otherwise.  x_odd: an odd series pitch -- every other series starts 8 bytes off (C == 1: the one series
    does); u_off / w_off: u or w 8 bytes off, which sends every series down the scalar loop."""
    x, u, w, order, t, sc = col_inputs(orc, N, C, weighted)
    ld = N + (N + 1) % 2 + (0 if variant == "x_odd" else 1)       # odd for x_odd, else even
    assert ld % 2 == (1 if variant == "x_odd" else 0) and ld >= N
    if C == 1:
        xd = dev_off8(x) if variant == "x_odd" else dev(x)
    else:
        xd = dev_series(x, ld)
        assert xd.stride(0) == 1 and (N == 1 or xd.stride(1) == ld)
    ud = dev_off8(u) if variant == "u_off" else dev(u)
    wd = None if w is None else (dev_off8(w) if variant == "w_off" else dev(w))
    got = eng.reduce_vals(xd, ud, order, w=wd).cpu().numpy()
    hold("reduce_vals colmajor", f"N={N} C={C} w={weighted} {variant}", got, t, sc)


# ---- group C: txm_reduce_vals_1d ----------------------------------------------------------------------------------------
ONE_D_SHAPES = [(1, 1, None), (3, 777, 779), (300, 1000, None), (2, 100001, None)]


def rows_1d(R, N):
    rng = np.random.default_rng([3, R, N])
    return rng.normal(3.0, 1.5, (R, N)) + rng.normal(0.0, 2.0, (R, 1)), plain_weights(rng, N)


def run_1d(eng, rows, mom, w, pitch=None):
    R, N = rows.shape
    if pitch is None:
        rd = dev(rows)
    else:                                                   # an odd row pitch: every other row starts 8 bytes off
        buf = torch.full((R, pitch), float("nan"), dtype=torch.float64, device="cuda")
        buf[:, :N] = dev(rows)
        rd = buf[:, :N]
    return eng.reduce_vals_1d(rd, mom, w=None if w is None else dev(w)).cpu().numpy()


@gpu
@pytest.mark.parametrize("R,N,pitch", ONE_D_SHAPES)
@pytest.mark.parametrize("weighted", [False, True])
def test_1d_shapes(eng, orc, R, N, pitch, weighted):
    rows, w = rows_1d(R, N)
    w = w if weighted else None
    got = run_1d(eng, rows, 4, w, pitch)
    hold("reduce_vals_1d", f"R={R} N={N} w={weighted}", got, truth_rows(orc, rows, 4, w), scale_rows(rows, 4, w))


@gpu
@pytest.mark.parametrize("M", range(1, 10))
@pytest.mark.parametrize("weighted", [False, True])
def test_1d_every_M(eng, orc, M, weighted):
    rows, w = rows_1d(3, 777)
    w = w if weighted else None
    got = run_1d(eng, rows, M - 1, w, 779)
    hold("reduce_vals_1d", f"M={M} w={weighted}", got, truth_rows(orc, rows, M - 1, w), scale_rows(rows, M - 1, w))


# ---- group D: txm_reduce_vals_batched -----------------------------------------------------------------------------------
def batch_states(S, N, C):
    rng = np.random.default_rng([4, S, N, C])
    out = []
    for s in range(S):
        x, u = idealgas(rng, N, C)
        out.append((x + 0.5 * s, u + s, plain_weights(rng, N)))
    return out


def check_batched(eng, orc, sts, order, weighted, name, off8=()):
    xs = [dev_off8(x) if s in off8 else dev(x) for s, (x, u, w) in enumerate(sts)]
    us = [dev(u) for (x, u, w) in sts]
    ws = [dev(w) for (x, u, w) in sts] if weighted else None
    got = eng.reduce_vals_batched(xs, us, order, ws=ws)
    for s, (x, u, w) in enumerate(sts):
        w = w if weighted else None
        sc = moment_scale(x, u, order, w)
        one = eng.reduce_vals(xs[s], us[s], order, w=None if ws is None else ws[s]).cpu().numpy()
        assert scaled_err(got[s].cpu().numpy(), one, sc) < 2e-13, (name, s)          # equals the per-state call
        hold("reduce_vals_batched", f"{name} state {s}", got[s].cpu().numpy(), orc.truth_cov(x, u, order, w=w), sc)


@gpu
@pytest.mark.parametrize("S", [1, 3, 64])
@pytest.mark.parametrize("N,C", [(1000, 4), (5000, 33)])
@pytest.mark.parametrize("weighted", [False, True])
def test_batched(eng, orc, cus, S, N, C, weighted):
    """S states on blockIdx.z; the blocks of one state's grid are divided among the states (S = 3 and 64 exceed the two
    blocks of (1000, 4): one block a state)."""
    p = plan_rowmajor(C, C, True, N, cus)
    assert (p["vec"], p["gx"]) == ((2, 2) if C == 4 else (1, cdiv(N, 16)))
    check_batched(eng, orc, batch_states(S, N, C), 4, weighted, f"S={S} N={N} C={C} w={weighted}")


@gpu
@pytest.mark.parametrize("weighted", [False, True])
def test_batched_one_state_8_bytes_off(eng, orc, weighted):
    """aligned16 == false: state 1's x starts 8 bytes past a 16-byte boundary, so the whole launch takes VEC = 1 although C
    and the pitch are even."""
    check_batched(eng, orc, batch_states(3, 1000, 4), 4, weighted, f"x[1] 8 bytes off w={weighted}", off8=(1,))


# ---- group E: the reduction in pieces -----------------------------------------------------------------------------------
def layout(x, colmajor):
    return dev_series(x, x.shape[0] + 1 + x.shape[0] % 2) if colmajor else dev(x)


@gpu
@pytest.mark.parametrize("colmajor", [False, True])
@pytest.mark.parametrize("weighted", [False, True])
def test_shards_with_a_single_sample_and_a_weightless_shard(eng, orc, colmajor, weighted):
    """reduce_pivot on the first shard -> reduce_sums per shard -> sums_to_state: three unequal shards, one of a single
    sample and (with weights) one whose weights are all zero; the state of all samples, and of the weightless shard alone
    the empty state."""
    N, C, order = 30011, 3, 4
    rng = np.random.default_rng([5, N])
    x, u = idealgas(rng, N, C)
    cuts = [0, 20000, 20001, N]
    w = None
    if weighted:
        w = plain_weights(rng, N)
        w[20001:] = 0.0
    sl = [slice(a, b) for a, b in zip(cuts[:-1], cuts[1:])]
    wd = lambda s: None if w is None else dev(w[s])  # noqa: E731
    piv = eng.reduce_pivot(layout(x[sl[0]], colmajor), dev(u[sl[0]]), wd(sl[0]))
    sums = torch.stack([eng.reduce_sums(layout(x[s], colmajor), dev(u[s]), order, piv, w=wd(s)) for s in sl])
    got = eng.sums_to_state(sums, piv).cpu().numpy()
    hold("sums_to_state", f"3 shards colmajor={colmajor} w={weighted}", got, orc.truth_cov(x, u, order, w=w),
         moment_scale(x, u, order, w))
    if weighted:
        assert not sums[2].cpu().numpy()[:, 0, 0].any()
        assert not eng.sums_to_state(sums[2], piv).cpu().numpy().any()               # total weight zero: the empty state
        assert np.array_equal(eng.sums_to_state(sums[:2], piv).cpu().numpy(), got)   # ... and adds nothing


@gpu
@pytest.mark.parametrize("colmajor", [False, True])
@pytest.mark.parametrize("weighted", [False, True])
def test_push_far_chunk_and_push_into_zeros(eng, orc, colmajor, weighted):
    """push_vals into zeros == the reduce of the chunk; then a chunk whose mean lies 1e3 sigma from the accumulated state:
    the old state is re-expressed about the new chunk's pivot, 1e3 sigma away, and the result is the state of both."""
    N1, N2, C, order = 5003, 3001, 3, 4
    rng = np.random.default_rng([6, N1])
    x1, u1 = idealgas(rng, N1, C)
    x2, u2 = idealgas(rng, N2, C)
    u2 = u2 + 1e3 * 5.31
    x2 = x2 + 1e3 * 0.05
    w1 = plain_weights(rng, N1) if weighted else None
    w2 = plain_weights(rng, N2) if weighted else None
    st = torch.zeros((C, 2, order + 1), dtype=torch.float64, device="cuda")
    eng.push_vals(st, layout(x1, colmajor), dev(u1), None if w1 is None else dev(w1))
    hold("push_vals", f"into zeros colmajor={colmajor} w={weighted}", st.cpu().numpy(), orc.truth_cov(x1, u1, order, w=w1),
         moment_scale(x1, u1, order, w1))
    eng.push_vals(st, layout(x2, colmajor), dev(u2), None if w2 is None else dev(w2))
    x, u = np.concatenate([x1, x2]), np.concatenate([u1, u2])
    w = None if w1 is None else np.concatenate([w1, w2])
    hold("push_vals", f"chunk 1e3 sigma away colmajor={colmajor} w={weighted}", st.cpu().numpy(), orc.truth_cov(x, u, order, w=w),
         moment_scale(x, u, order, w))


# ---- group F: data kinds on one shape per layout ------------------------------------------------------------------------
def kind_expectation(orc, kind, x, u, w, order):
    if kind == "total_zero":                                # cmomy's convention: the empty state
        ref = orc.reduce_vals(x, u, order, w=w)
        assert not ref.any()
        return ref, np.zeros_like(ref)
    sh = kind_shift(kind, x, u)
    if sh is None:
        return orc.truth_cov(x, u, order, w=w), moment_scale(x, u, order, w)
    ref = orc.truth_cov(exact_minus(x, sh[0][None, :]), exact_minus(u, sh[1]), order, w=w)
    ref[:, 1, 0] += sh[0]
    ref[:, 0, 1] += sh[1]
    return ref, moment_scale(x, u, order, w)


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("entry", ["rowmajor", "colmajor", "batched", "push_vals", "shards"])
def test_data_kinds(eng, orc, kind, entry):
    x, u, w = kind_data(kind)
    N, C = x.shape
    order = KIND_ORDER
    ref, sc = kind_expectation(orc, kind, x, u, w, order)
    ud, wd = dev(u), (None if w is None else dev(w))
    if entry == "rowmajor":
        got = eng.reduce_vals(dev(x), ud, order, w=wd)
    elif entry == "colmajor":
        got = eng.reduce_vals(dev_series(x, N + 2), ud, order, w=wd)
    elif entry == "batched":                                 # the kind as state 1 of two
        x0, u0, w0 = kind_data("idealgas", N=N, seed=1)
        ws = None if w is None else [dev(plain_weights(np.random.default_rng(9), N)), wd]
        got = eng.reduce_vals_batched([dev(x0), dev(x)], [dev(u0), ud], order, ws=ws)[1]
    elif entry == "push_vals":
        got = eng.push_vals(torch.zeros((C, 2, order + 1), dtype=torch.float64, device="cuda"), dev(x), ud, wd)
    else:                                                    # one weighted pivot of the whole, sums of two halves
        piv = eng.reduce_pivot(dev(x), ud, wd)
        h = N // 2
        sums = torch.stack([eng.reduce_sums(dev(x[a:b]), dev(u[a:b]), order, piv, w=None if w is None else dev(w[a:b]))
                            for a, b in ((0, h), (h, N))])
        got = eng.sums_to_state(sums, piv)
    hold({"rowmajor": "reduce_vals rowmajor", "colmajor": "reduce_vals colmajor", "batched": "reduce_vals_batched",
          "push_vals": "push_vals", "shards": "sums_to_state"}[entry] + (" (concentrated, of 4^order 3e-13)" if kind in CONCENTRATED else ""),
         f"{kind}", got.cpu().numpy(), ref, sc, kind_rtol(kind, order))


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_data_kinds_1d(eng, orc, kind):
    """u and the columns as 1-D series sharing the kind's weights."""
    x, u, w = kind_data(kind)
    rows = np.ascontiguousarray(np.vstack([u[None, :], x.T]))
    mom = KIND_ORDER
    got = run_1d(eng, rows, mom, w)
    if kind == "total_zero":
        ref = orc.reduce_vals_1d(rows, mom, w=w)
        assert not ref.any()
        sc = np.zeros_like(ref)
    else:
        sh = kind_shift(kind, x, u)
        ref = truth_rows(orc, rows, mom, w, None if sh is None else np.r_[sh[1], sh[0]])
        sc = scale_rows(rows, mom, w)
    hold("reduce_vals_1d" + (" (concentrated, of 4^order 3e-13)" if kind in CONCENTRATED else ""), kind, got, ref, sc,
         kind_rtol(kind, mom))


# ---- group G: the unweighted path is bit for bit what it was ------------------------------------------------------------
@gpu
def test_unweighted_outputs_equal_the_stored_ones_bit_for_bit(eng):
    """Unweighted calls launch the same kernels in the same order as before the weighted pivot existed: the outputs stored
    by tests/golden/make_reduce_golden.py (written once, with the build before that change) are reproduced bit for bit."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("make_reduce_golden", GOLDEN.parent / "make_reduce_golden.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    compute = mod.compute
    g = np.load(GOLDEN)
    got = compute(eng, {k: g[k] for k in g.files if k.startswith("in_")})
    assert sorted(got) == sorted(k for k in g.files if k.startswith("out_")) and len(got) >= 3
    for k, v in got.items():
        assert np.array_equal(v, g[k]), k
