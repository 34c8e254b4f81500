"""The small kernels of txm_small.hip -- raw <-> central conversion, merge / block bootstrap of pre-reduced states,
covariance over replicates -- against the long-double references of oracle/tail_oracle.py (pinned to mpmath in
tests/test_tail_oracle_cpu.py), plus two additions to predict_taylor's definition test.

Tolerances (none of them taken from what the kernels return).

* convert_cov / convert_1d: every element within ``1e-12`` of the first-order bound of its own sum,
  ``sum |binom * m * shift powers|`` (README "Tolerances", the rule stated there for derivatives).  A sum of at most
  2 * 9 terms, each a product of a binomial coefficient, a moment and at most 9 factors of the shift, carries
  ``~(9 + 9 + 18) eps = 4e-15`` of that bound.
* resample_data: ``|hip - ref| <= 1e-12 (|ref| + scale)`` with the moment scale ``sigma_x^a sigma_u^b`` of
  test_kernels_gpu.py.  The kernel forms two binomial sums per element (records -> sums about the pivot, sums -> state,
  ~20 eps each relative to their own terms), and adds ``f * P`` over the records (``eps * (nrec / 256 + 8)``).  The
  pivot is the mean of the record means, so the shifts are of the size of the spread of the record means (< 0.5
  sigma for the 50-sample blocks used here) and the terms of those sums stay within ~50 x the scale: ~1e-13 in all.
* cov_over_rep: ``|hip - ref| <= 1e-12 (sigma_a + d_a)(sigma_b + d_b) + 2 d_a d_b`` -- see ``cov_tolerance``.

Worst scaled errors observed on an MI355X (every test prints its own; run with ``-s``):
    convert_cov    to raw 1.1e-15, to central 1.3e-16, round trip 2.3e-16   (of the sum bound)
    convert_1d     to raw 8.6e-16, to central 1.3e-16, round trip 2.4e-16
    resample_data  merge 4.1e-15, bootstrap 5.6e-15, weight-0 records 1.2e-15, weights 1 against 1e6 2.3e-15 (of
                   |ref| + scale); merge against truth_cov of the whole series 3.9e-13 (the records are float64
                   Pebay states, that is their own rounding)
    cov_over_rep   2.5e-15 with the mean at 1e6 sigma, 4.4e-16 without  (of the bound of cov_tolerance / 1e-12)
    Before the fixes that came with these tests: a count row of zeros (or a column of weight-0 records only) gave NaN
    where a merge of nothing is the empty state, and weight-0 records dragged the pivot towards zero -- 8e-11 (order
    4) to 3.6e-4 (order 8) of the scale on ideal-gas data.
"""

import math

import numpy as np
import pytest
import torch

from oracle import tail_oracle as tl

pytestmark = pytest.mark.gpu

RTOL = 1e-12
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def eng(txm):
    from thermoextrap_amd import engine

    return engine


def dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def make_data(rng, N, C, kind):
    """idealgas: u ~ N(174.85, 5.31^2), the mean 33 sigma from zero, so raw -> central is a cancellation; unit: U(0, 1)."""
    if kind == "idealgas":
        u = rng.normal(174.85, 5.31, N)
        x = rng.normal(0.0, 1.0, C)[None, :] + rng.normal(1e-3, 5e-4, C)[None, :] * u[:, None] + rng.normal(0, 0.05, (N, C))
    else:
        u = rng.random(N)
        x = rng.random((N, C))
    return x, u


def bounded_ratio(got, ref, bound):
    got = np.asarray(got)
    assert got.shape == ref.shape
    assert np.all(np.isfinite(got)), "non-finite output"
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    return float(r.max())


# ---------------------------------------------------------------------------
# convert_cov / convert_1d
# ---------------------------------------------------------------------------
NS = [1, 255, 256, 257, 70_000]       # one thread per state, 256 per block: one block, a ragged tail, 274 blocks


def central_states(orc, rng, n, order, kind):
    """n central-form states: 257 real ones (the columns of one reduced data set), repeated with a 1 % jitter on
    every element -- the conversion is algebra on the numbers it is given, any finite input is a valid one."""
    x, u = make_data(rng, 400, 257, kind)
    base = orc.reduce_vals(x, u, order)
    st = base[np.arange(n) % 257] * (1.0 + 0.01 * rng.normal(size=(n, 2, order + 1)))
    st[:, 0, 0] = rng.uniform(1.0, 500.0, n)
    return st


@pytest.mark.parametrize("order", range(9))
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("kind", ["idealgas", "unit"])
def test_convert_cov_both_directions(eng, orc, order, n, kind):
    rng = np.random.default_rng(order * 7 + n)
    cen = central_states(orc, rng, n, order, kind)
    raw_ref, raw_b = tl.convert_cov(cen, False, return_bound=True)
    raw = eng.convert_cov(dev(cen), False).cpu().numpy()
    r1 = bounded_ratio(raw, raw_ref, raw_b)
    # raw -> central on the oracle's raw states (the same float64 input for both sides)
    cen_ref, cen_b = tl.convert_cov(raw_ref, True, return_bound=True)
    back = eng.convert_cov(dev(raw_ref), True).cpu().numpy()
    r2 = bounded_ratio(back, cen_ref, cen_b)
    # round trip on the device: central -> raw -> central, against the states it started from
    trip = eng.convert_cov(eng.convert_cov(dev(cen), False), True).cpu().numpy()
    r3 = bounded_ratio(trip, cen, cen_b)
    print(f"convert_cov order={order} n={n} {kind}: to_raw {r1:.3e} to_central {r2:.3e} round trip {r3:.3e}")
    assert r1 <= RTOL and r2 <= RTOL and r3 <= RTOL
    assert np.array_equal(raw[:, 0, 0], cen[:, 0, 0]) and np.array_equal(back[:, 0, 0], cen[:, 0, 0])   # the weight is carried
    if n == 257:
        ref2 = orc.convert_cov(cen, False)
        assert bounded_ratio(ref2, raw_ref, raw_b) <= RTOL      # the compiled oracle agrees with the long-double one


@pytest.mark.parametrize("order", [0, 3, 8])
def test_convert_cov_leading_batch_dimensions(eng, orc, order):
    rng = np.random.default_rng(order)
    cen = central_states(orc, rng, 3 * 5, order, "idealgas").reshape(3, 5, 2, order + 1)
    for to_c, src in ((False, cen), (True, tl.convert_cov(cen, False))):
        ref, b = tl.convert_cov(src, to_c, return_bound=True)
        got = eng.convert_cov(dev(src), to_c)
        assert got.shape == (3, 5, 2, order + 1)
        assert bounded_ratio(got.cpu().numpy(), ref, b) <= RTOL
        # a non-contiguous view (rep and val swapped): the engine copies it
        got_t = eng.convert_cov(dev(src.transpose(1, 0, 2, 3).copy()).transpose(0, 1), to_c)
        assert torch.equal(got_t, got)


@pytest.mark.parametrize("M", range(1, 11))
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("kind", ["idealgas", "unit"])
def test_convert_1d_both_directions(eng, orc, M, n, kind):
    rng = np.random.default_rng(M * 11 + n)
    _, u = make_data(rng, 400, 1, kind)
    base = orc.reduce_vals_1d(np.stack([u, u[::-1] * 1.01, u ** 2 / u.mean()]), M - 1)
    cen = base[np.arange(n) % 3] * (1.0 + 0.01 * rng.normal(size=(n, M)))
    cen[:, 0] = rng.uniform(1.0, 500.0, n)
    raw_ref, raw_b = tl.convert_1d(cen, False, return_bound=True)
    r1 = bounded_ratio(eng.convert_1d(dev(cen), False).cpu().numpy(), raw_ref, raw_b)
    cen_ref, cen_b = tl.convert_1d(raw_ref, True, return_bound=True)
    back = eng.convert_1d(dev(raw_ref), True).cpu().numpy()
    r2 = bounded_ratio(back, cen_ref, cen_b)
    trip = eng.convert_1d(eng.convert_1d(dev(cen), False), True).cpu().numpy()
    r3 = bounded_ratio(trip, cen, cen_b)
    print(f"convert_1d M={M} n={n} {kind}: to_raw {r1:.3e} to_central {r2:.3e} round trip {r3:.3e}")
    assert r1 <= RTOL and r2 <= RTOL and r3 <= RTOL
    assert np.array_equal(back[:, 0], cen[:, 0])
    if n == 257:
        assert bounded_ratio(orc.convert_1d(raw_ref, True), cen_ref, cen_b) <= RTOL
        batch = dev(cen[:12].reshape(3, 4, M))
        assert torch.equal(eng.convert_1d(batch, False).reshape(12, M), eng.convert_1d(dev(cen[:12]), False))


def test_convert_errors(eng):
    from thermoextrap_amd import TxmError

    z = torch.zeros((4, 2, 10), dtype=torch.float64, device="cuda")
    with pytest.raises(TxmError):
        eng.convert_cov(z, False)                       # order 9 > TXM_MAX_ORDER
    with pytest.raises(ValueError):
        eng.convert_cov(z[:, :1], False)
    with pytest.raises(TxmError):
        eng.convert_1d(torch.zeros((4, 11), dtype=torch.float64, device="cuda"), True)


# ---------------------------------------------------------------------------
# resample_data
# ---------------------------------------------------------------------------
NB = 50                                                    # samples per record
# (nrec, C, nrep): every nrec of {1, 2, 256, 257, 5000}, every C of {1, 5, 32, 300}, every nrep of {1, 7, 300};
# the largest is 5000 x 32 records of 2 x 9 moments = 23 MB
SHAPES = [(1, 1, 1), (2, 5, 7), (256, 32, 7), (257, 300, 1), (257, 1, 300), (5000, 5, 300), (5000, 32, 7), (256, 300, 7), (2, 32, 300)]


def moment_scale(x, u, order):
    sx, su = np.std(x, axis=0), np.std(u)
    sc = np.empty((x.shape[1], 2, order + 1))
    for b in range(order + 1):
        sc[:, 0, b] = su ** b
        sc[:, 1, b] = sx * su ** b
    return sc


_SERIES = {}


def records(orc, nrec, C, order):
    """Records = orc.reduce_vals on consecutive 50-sample blocks of one long series; returns (records, x, u, truth) with
    truth = orc.truth_cov of the whole series.  A state of order k is the leading part of the state of order 8 (no
    moment depends on a higher one), so each series is reduced once, at order 8."""
    if (nrec, C) not in _SERIES:
        x, u = make_data(np.random.default_rng(nrec * 1000 + C), nrec * NB, C, "idealgas")
        rec = np.stack([orc.reduce_vals(x[i * NB:(i + 1) * NB], u[i * NB:(i + 1) * NB], 8) for i in range(nrec)])
        _SERIES[(nrec, C)] = (rec, x, u, orc.truth_cov(x, u, 8))
    rec, x, u, truth = _SERIES[(nrec, C)]
    return np.ascontiguousarray(rec[..., : order + 1]), x, u, np.ascontiguousarray(truth[..., : order + 1])


def origin_of(rec):
    """A fixed point near the data for the oracle's sums (not the kernel's pivot): the first record's means, rounded."""
    C, K = rec.shape[1], rec.shape[-1]
    ou = np.round(rec[0, :, 0, 1], 0) if K > 1 else np.zeros(C)
    return np.stack([ou, np.round(rec[0, :, 1, 0], 2)], axis=1)


def check_data(eng, rec, freq, order, scale, what, origin=None):
    ref = tl.resample_data(rec, np.ones((1, rec.shape[0]), dtype=np.int64) if freq is None else freq, order,
                           origin=origin_of(rec) if origin is None else origin)
    got = eng.resample_data(dev(rec), None if freq is None else dev(freq, torch.int64), order).cpu().numpy()
    assert got.shape == ref.shape
    r = bounded_ratio(got, ref, np.abs(ref) + scale[None])
    print(f"resample_data {what}: order={order} nrec={rec.shape[0]} C={rec.shape[1]} nrep={ref.shape[0]} ratio={r:.3e}")
    assert r <= RTOL, f"{what}: {r:.3e}"
    return got, ref


@pytest.mark.parametrize("order", range(9))
@pytest.mark.parametrize("nrec,C,nrep", SHAPES)
def test_resample_data_shapes(eng, orc, order, nrec, C, nrep):
    rng = np.random.default_rng(order * 1000 + nrec + C)
    rec, x, u, truth = records(orc, nrec, C, order)
    sc = moment_scale(x, u, order)
    # merge (freq = None), also against the extended-precision moments of the whole series
    got, _ = check_data(eng, rec, None, order, sc, "merge")
    if nrec * NB > 2:
        r = bounded_ratio(got[0], truth, np.abs(truth) + sc)
        print(f"resample_data merge vs truth_cov of the series: order={order} nrec={nrec} C={C} ratio={r:.3e}")
        assert r <= RTOL
    # bootstrap counts: multinomial rows, then a row of zeros, an entry > 255, zeros in front
    freq = rng.multinomial(nrec, np.full(nrec, 1.0 / nrec), size=nrep).astype(np.int64)
    freq[0, 0] = 1000
    if nrep > 2:
        freq[1] = 0                                       # a replicate without records: the empty state
        freq[2, : nrec // 2] = 0
        freq[2, -1] = 300
    got, ref = check_data(eng, rec, freq, order, sc, "bootstrap")
    if nrep > 2:
        assert np.array_equal(got[1], np.zeros_like(got[1])) and np.array_equal(ref[1], np.zeros_like(ref[1]))
    if nrec <= 257 and C <= 32:                           # the compiled oracle (sequential pairwise merges in float64)
        live = [r for r in range(nrep) if freq[r].any()]
        ref2 = orc.resample_data(rec, freq, order)
        assert bounded_ratio(ref2[live], ref[live], np.abs(ref[live]) + sc[None]) <= 1e-11


@pytest.mark.parametrize("order", [0, 1, 4, 8])
@pytest.mark.parametrize("nrec,C", [(257, 5), (5000, 1), (2, 32)])
def test_resample_data_zero_and_unequal_weights(eng, orc, order, nrec, C):
    """Records of weight 0 whose moments are all zero (what an empty block reduces to), a column in which every
    record but one has weight 0, and records whose weights are 1 against 1e6."""
    rng = np.random.default_rng(order + nrec)
    rec, x, u, _ = records(orc, nrec, C, order)
    sc = moment_scale(x, u, order)
    freq = rng.multinomial(nrec, np.full(nrec, 1.0 / nrec), size=5).astype(np.int64)
    freq[:, nrec // 2] += 1                               # the one live record of column 0 is in every replicate
    z = rec.copy()
    z[rng.random(nrec) < 0.3] = 0.0                       # whole records empty
    z[:, 0] = 0.0
    z[nrec // 2, 0] = rec[nrec // 2, 0]                   # column 0: one live record
    for f in (None, freq):
        got, _ = check_data(eng, z, f, order, sc, "weight 0", origin=origin_of(rec))   # (record 0 of z may be empty)
        # the merge of copies of one live record is that record, its weight times the count
        want = np.broadcast_to(rec[nrec // 2, 0], got[:, 0].shape).copy()
        want[:, 0, 0] *= 1 if f is None else f[:, nrec // 2]
        assert bounded_ratio(got[:, 0], want, np.abs(want) + sc[0]) <= RTOL
    w = rec.copy()
    w[:, :, 0, 0] = np.where(rng.random((nrec, C)) < 0.5, 1.0, 1e6)
    for f in (None, freq):
        check_data(eng, w, f, order, sc, "weights 1 and 1e6")


def test_resample_data_errors(eng):
    from thermoextrap_amd import TxmError

    d = torch.zeros((4, 3, 2, 3), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        eng.resample_data(d, None, 3)
    with pytest.raises(ValueError):
        eng.resample_data(d, torch.ones((2, 5), dtype=torch.int64, device="cuda"), 2)
    with pytest.raises(TxmError):
        eng.resample_data(torch.zeros((4, 3, 2, 10), dtype=torch.float64, device="cuda"), None, 9)


# ---------------------------------------------------------------------------
# cov_over_rep
# ---------------------------------------------------------------------------
def cov_tolerance(vals, sigma):
    """Bound on ``|hip - ref|`` for the two-pass kernel, per (value, a, b).

    The kernel's mean of series a is ``m_a + d_a`` with ``|d_a| <= g mean|v_a|``, ``g = eps (ceil(nrep / 256) + 8 +
    1)``: every thread adds ceil(nrep / 256) values, the tree has 8 levels, one division.  With ``c_ar = v_ar - m_a``
    (``sum_r c_ar = 0``) the second pass sums ``(c_ar - d_a)(c_br - d_b)``:

        sum_r (c_ar - d_a)(c_br - d_b) = sum_r c_ar c_br + nrep d_a d_b

    so the error of the mean enters in second order only -- the term ``nrep / (nrep - 1) d_a d_b <= 2 d_a d_b``.  What
    is of first order is rounding: each factor is rounded once (``eps |c - d|``), each product once, and the sum in
    ``ceil(nrep / 256) + 8`` steps, all relative to ``sum_r |c_ar - d_a| |c_br - d_b| <= (nrep - 1) (sigma_a + |d_a|)
    (sigma_b + |d_b|)`` (Cauchy-Schwarz).  That is ``(3 + ceil(nrep / 256) + 8) eps <= 51 eps = 1.1e-14`` at nrep =
    10^4, inside the project's 1e-12:

        |hip - ref| <= 1e-12 (sigma_a + d_a)(sigma_b + d_b) + 2 d_a d_b.

    With a mean 1e6 x the spread, d = 5e-9 sigma: the mean-cancellation term is 5e-17 sigma_a sigma_b."""
    n_ord, nrep, nval = vals.shape
    g = EPS * (math.ceil(nrep / 256) + 9)
    d = (g * np.abs(vals).mean(axis=1)).T                  # (nval, n_ord)
    s = sigma + d
    return RTOL * s[:, :, None] * s[:, None, :] + 2.0 * d[:, :, None] * d[:, None, :]


COV_CASES = [(a, r, v) for a in (1, 2, 5, 16) for r in (2, 3, 255, 256, 257, 1000, 10_000) for v in (1, 7, 4096)
             if a * r * v <= 5_300_000]                    # <= 42 MB of input; every value of every axis is present


def test_cov_cases_cover_every_axis_value():
    assert {c[0] for c in COV_CASES} == {1, 2, 5, 16}
    assert {c[1] for c in COV_CASES} == {2, 3, 255, 256, 257, 1000, 10_000}
    assert {c[2] for c in COV_CASES} == {1, 7, 4096}
    assert (16, 10_000, 7) in COV_CASES and (1, 1000, 4096) in COV_CASES


@pytest.mark.parametrize("n_ord,nrep,nval", COV_CASES)
@pytest.mark.parametrize("offset", ["1e6 sigma", "none"])
def test_cov_over_rep(eng, n_ord, nrep, nval, offset):
    rng = np.random.default_rng(n_ord * 100_000 + nrep + nval)
    sig = 10.0 ** rng.uniform(-3, 3, (n_ord, 1, nval))
    mix = rng.normal(size=(n_ord, n_ord)) / np.sqrt(n_ord) + np.eye(n_ord)
    z = np.einsum("ab,brv->arv", mix, rng.normal(size=(n_ord, nrep, nval)))
    vals = sig * z
    if offset != "none":
        vals = vals + 1e6 * sig * rng.choice([-1.0, 1.0], (n_ord, 1, nval))
    ref, sigma = tl.cov_over_rep(vals)
    got = eng.cov_over_rep(dev(vals)).cpu().numpy()
    assert got.shape == (nval, n_ord, n_ord)
    r = bounded_ratio(got, ref, cov_tolerance(vals, sigma) / RTOL)
    print(f"cov_over_rep n_ord={n_ord} nrep={nrep} nval={nval} offset={offset}: ratio={r:.3e}")
    assert r <= RTOL
    assert np.array_equal(got, got.transpose(0, 2, 1)), "the output is not exactly symmetric"
    if nval <= 7 and nrep <= 1000:                        # numpy's own, on centred values
        c = vals - vals.mean(axis=1, keepdims=True)
        want = np.stack([np.atleast_2d(np.cov(c[:, :, v], ddof=1)) for v in range(nval)])
        np.testing.assert_allclose(ref, want, rtol=1e-6, atol=0)


def test_cov_over_rep_errors(eng):
    from thermoextrap_amd import TxmError

    with pytest.raises(TxmError):
        eng.cov_over_rep(torch.zeros((3, 1, 4), dtype=torch.float64, device="cuda"))      # nrep = 1
    with pytest.raises(TxmError):
        eng.cov_over_rep(torch.zeros((17, 5, 4), dtype=torch.float64, device="cuda"))     # n_ord = 17


# ---------------------------------------------------------------------------
# predict_taylor: element counts around a block, and dalpha = 0
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("M", [255, 257])
def test_predict_taylor_block_edges_and_zero_dalpha(eng, M):
    """One thread per element, 256 per block.  At dalpha = 0 the terms beyond k = 0 are exactly 0 (finite inputs:
    no 0 * inf), so the sum is the zeroth derivative bit for bit."""
    rng = np.random.default_rng(M)
    n_ord = 7
    d = rng.normal(size=(n_ord, M)) * 10.0 ** rng.uniform(-5, 5, (n_ord, 1))
    da = np.array([0.0, -0.0, 0.4, -1.3])
    fac = np.array([1.0 / math.factorial(k) for k in range(n_ord)])
    pw = np.stack([np.cumprod(np.r_[1.0, np.full(n_ord - 1, t)]) for t in da])
    terms = pw[:, :, None] * (d * fac[:, None])[None]
    dd = dev(d)
    gt = eng.predict_taylor(dd, da, "terms").cpu().numpy()
    np.testing.assert_allclose(gt, terms, rtol=1e-15)
    assert np.all(gt[:2, 1:] == 0.0) and np.array_equal(gt[0, 0], d[0]) and np.array_equal(gt[1, 0], d[0])
    gs = eng.predict_taylor(dd, da, "sum").cpu().numpy()
    assert np.all(np.isfinite(gs)) and np.array_equal(gs[0], d[0]) and np.array_equal(gs[1], d[0])
    bound = np.abs(terms).sum(axis=1)
    assert np.all(np.abs(gs - np.asarray(terms, dtype=np.longdouble).sum(axis=1).astype(np.float64)) <= 1e-14 * bound)
    gc = eng.predict_taylor(dd, da, "cumsum").cpu().numpy()
    assert np.array_equal(gc[:2], np.broadcast_to(d[0], (2, n_ord, M)))
    assert np.array_equal(gc[:, -1], gs)
