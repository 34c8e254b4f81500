"""The long-double references of oracle/tail_oracle.py, pinned to mpmath at 50 digits (and, where one exists, to the
compiled oracle's counterpart).  No GPU.

The mpmath side is written as scalar loops straight from the definitions -- weighted sample averages of
``x^a u^b`` and ``(x - <x>)^a (u - <u>)^b`` -- so it shares no code and no vectorisation with the module it checks.
The long-double functions must agree with it to 1e-17 of each element's own first-order sum bound (64 mantissa bits
give 1.08e-19 per operation; the sums here have at most a few hundred terms).
"""

import mpmath as mp
import numpy as np
import pytest

from oracle import tail_oracle as tl

mp.mp.dps = 50
TOL = 1e-17


def F(v):
    return mp.mpf(float(v))


def mp_moments(x, u, w, order):
    """(central, raw) states [2][K] of weighted samples, in mpmath."""
    K = order + 1
    W = mp.fsum(F(t) for t in w)
    xa = mp.fsum(F(a) * F(b) for a, b in zip(w, x)) / W
    ua = mp.fsum(F(a) * F(b) for a, b in zip(w, u)) / W
    cen = [[None] * K for _ in range(2)]
    raw = [[None] * K for _ in range(2)]
    for a in range(2):
        for b in range(K):
            raw[a][b] = mp.fsum(F(wi) * F(xi) ** a * F(ui) ** b for wi, xi, ui in zip(w, x, u)) / W
            cen[a][b] = mp.fsum(F(wi) * (F(xi) - xa) ** a * (F(ui) - ua) ** b for wi, xi, ui in zip(w, x, u)) / W
    cen[0][0] = raw[0][0] = W
    cen[1][0] = xa
    if K > 1:
        cen[0][1] = ua
    return cen, raw


def to_f64(m):
    return np.array([[float(v) for v in row] for row in m])


def mp_shift(m, sx, su, K):
    """sum_{i<=a, j<=b} C(a,i) C(b,j) m[i][j] sx^(a-i) su^(b-j) with m[0][0] read as 1, and the sum of |terms|."""
    out = [[None] * K for _ in range(2)]
    bnd = [[None] * K for _ in range(2)]
    for a in range(2):
        for b in range(K):
            terms = []
            for i in range(a + 1):
                for j in range(b + 1):
                    mij = mp.mpf(1) if i + j == 0 else m[i][j]
                    terms.append(mp.binomial(a, i) * mp.binomial(b, j) * mij * sx ** (a - i) * su ** (b - j))
            out[a][b] = mp.fsum(terms)
            bnd[a][b] = mp.fsum(abs(t) for t in terms)
    return out, bnd


def mp_convert_cov(state, to_central):
    """The conversion of one float64 state [2][K], in mpmath, from the binomial theorem."""
    K = state.shape[1]
    m = [[F(v) for v in row] for row in state]
    xa = m[1][0]
    ua = m[0][1] if K > 1 else mp.mpf(0)
    if to_central:
        out, bnd = mp_shift(m, -xa, -ua, K)
        out[1][0], bnd[1][0] = xa, abs(xa)
        if K > 1:
            out[0][1], bnd[0][1] = ua, abs(ua)
    else:
        m[1][0] = mp.mpf(0)
        if K > 1:
            m[0][1] = mp.mpf(0)
        out, bnd = mp_shift(m, xa, ua, K)
    out[0][0] = bnd[0][0] = m[0][0]
    return out, bnd


def assert_mp_close(got, want, bound, tol=TOL, what=""):
    got = np.asarray(got, dtype=np.float64)
    for idx in np.ndindex(got.shape):
        w, b = want, bound
        for k in idx:
            w, b = w[k], b[k]
        # the float64 returned is the rounding of a long double: half an ulp of the value on top of the pin
        lim = tol * b + mp.mpf(2) ** -53 * abs(w)
        assert abs(F(got[idx]) - w) <= lim, f"{what} {idx}: {got[idx]!r} vs {mp.nstr(w, 25)} (bound {mp.nstr(b, 5)})"


def samples(rng, N, kind):
    if kind == "idealgas":
        u = rng.normal(174.85, 5.31, N)
        x = 0.3 + 1e-3 * u + rng.normal(0, 0.05, N)
    else:
        u = rng.random(N)
        x = rng.random(N)
    return x, u, rng.random(N) + 0.05


def test_long_double_is_80_bit():
    assert np.finfo(np.longdouble).eps < 1.1e-19


# ---------------------------------------------------------------------------
# perturb
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,C", [(1, 1), (2, 3), (200, 4)])
@pytest.mark.parametrize("with_freq", [False, True])
def test_perturb_vs_mpmath(N, C, with_freq):
    rng = np.random.default_rng(N + C)
    u = rng.normal(174.85, 5.31, N)
    x = rng.normal(1.0, 2.0, (N, C))
    da = [0.0, -0.0, 0.3, -0.7, 5.0, -200.0]          # the last two: weights down to e^-5000, beyond float64
    freq = None
    if with_freq:
        freq = rng.integers(0, 4, (3, N))
        freq[:, 0] = 1                                 # no empty replicate
        if N > 1:                                      # a replicate without the extreme sample
            k = int(np.argmin(u))
            freq[1, k], freq[1, (k + 1) % N] = 0, 2
        if N > 2:
            freq[2] = 0
            freq[2, 5] = 7                             # a single live sample
    avg, S = tl.perturb(x, u, da, freq)
    rows = [np.ones(N, dtype=np.int64)] if freq is None else list(freq)
    for r, f in enumerate(rows):
        for a, d in enumerate(da):
            e = [-F(d) * F(ui) for ui in u]
            emax = max(ei for ei, fi in zip(e, f) if fi > 0)
            w = [F(fi) * mp.exp(ei - emax) for ei, fi in zip(e, f)]
            den = mp.fsum(w)
            for c in range(C):
                want = mp.fsum(wi * F(xi) for wi, xi in zip(w, x[:, c])) / den
                scale = mp.fsum(wi * abs(F(xi)) for wi, xi in zip(w, x[:, c])) / den
                g, s = (avg[a, c], S[a, c]) if freq is None else (avg[r, a, c], S[r, a, c])
                # |arg| of the exponential reaches 5000: its long-double rounding is |arg| * eps
                assert abs(F(g) - want) <= (5000 * 2.2e-19 + 2.0 ** -53) * scale, (r, a, c)
                assert abs(F(s) - scale) <= 1e-15 * scale
    if freq is None:                                   # 1-D x and a single count row
        a1, s1 = tl.perturb(x[:, 0], u, da)
        assert a1.shape == (len(da),) and np.array_equal(a1, avg[:, 0]) and np.array_equal(s1, S[:, 0])
    else:
        a1, _ = tl.perturb(x, u, da, freq[1])
        assert a1.shape == (len(da), C) and np.array_equal(a1, avg[1])


def test_perturb_zero_dalpha_is_the_mean_and_underflow_is_the_extreme_row():
    rng = np.random.default_rng(3)
    u = rng.normal(0, 1, 100)
    x = rng.normal(size=(100, 2))
    avg, _ = tl.perturb(x, u, [0.0, 1e4, -1e4])
    np.testing.assert_allclose(avg[0], x.mean(0), rtol=1e-15)
    np.testing.assert_allclose(avg[1], x[np.argmin(u)], rtol=1e-12)
    np.testing.assert_allclose(avg[2], x[np.argmax(u)], rtol=1e-12)


# ---------------------------------------------------------------------------
# cov_over_rep
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n_ord,nrep,nval", [(1, 2, 1), (3, 7, 2), (5, 200, 1)])
def test_cov_over_rep_vs_mpmath(n_ord, nrep, nval):
    rng = np.random.default_rng(nrep)
    vals = 1e6 + rng.normal(size=(n_ord, nrep, nval))          # mean 1e6 x spread
    cov, sig = tl.cov_over_rep(vals)
    for v in range(nval):
        mean = [mp.fsum(F(t) for t in vals[a, :, v]) / nrep for a in range(n_ord)]
        for a in range(n_ord):
            for b in range(n_ord):
                want = mp.fsum((F(vals[a, r, v]) - mean[a]) * (F(vals[b, r, v]) - mean[b]) for r in range(nrep)) / (nrep - 1)
                sa, sb = (mp.sqrt(mp.fsum((F(vals[k, r, v]) - mean[k]) ** 2 for r in range(nrep)) / (nrep - 1)) for k in (a, b))
                # long-double mean of values ~1e6: 1e6 * eps_ld on each centred factor
                assert abs(F(cov[v, a, b]) - want) <= 2.0 ** -52 * sa * sb + 4 * 1e6 * 1.1e-19 * (sa + sb)
        np.testing.assert_allclose(sig[v], np.sqrt(np.diag(cov[v])), rtol=1e-15)
        assert np.array_equal(cov[v], cov[v].T)
    np.testing.assert_allclose(cov, np.stack([np.atleast_2d(np.cov(vals[:, :, v] - 1e6, ddof=1)) for v in range(nval)]),
                               rtol=1e-9, atol=1e-12)
    with pytest.raises(ValueError):
        tl.cov_over_rep(vals[:, :1])


# ---------------------------------------------------------------------------
# convert_cov / convert_1d
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("order", range(9))
@pytest.mark.parametrize("kind", ["idealgas", "unit"])
def test_convert_cov_vs_mpmath_and_compiled_oracle(orc, order, kind):
    rng = np.random.default_rng(order)
    x, u, w = samples(rng, 60, kind)
    cen, raw = mp_moments(x, u, w, order)
    cen64, raw64 = to_f64(cen), to_f64(raw)
    # (1) the same float64 input through the mpmath restatement of the formula: value and bound
    for src, to_c in ((cen64, False), (raw64, True)):
        want, bnd = mp_convert_cov(src, to_c)
        got, gb = tl.convert_cov(src[None], to_c, return_bound=True)
        assert_mp_close(got[0], want, bnd, what=f"to_central={to_c}")
        assert_mp_close(gb[0], bnd, bnd, tol=1e-15, what="bound")
        # (2) the compiled oracle computes the same sum in float64: within eps of that bound
        ref = orc.convert_cov(src[None], to_c)[0]
        assert np.all(np.abs(ref - got[0]) <= 1e-14 * gb[0])
    # (3) the definition itself: converting the (rounded) central state gives the raw moments of the samples
    got = tl.convert_cov(cen64, False, return_bound=True)
    assert np.all(np.abs(got[0] - raw64) <= 1e-14 * got[1])
    # leading batch dimensions are carried
    batch = np.broadcast_to(cen64, (2, 3, 2, order + 1))
    assert np.array_equal(tl.convert_cov(batch, False)[1, 2], got[0])


@pytest.mark.parametrize("M", range(1, 11))
@pytest.mark.parametrize("kind", ["idealgas", "unit"])
def test_convert_1d_vs_mpmath_and_compiled_oracle(orc, M, kind):
    rng = np.random.default_rng(M)
    _, u, w = samples(rng, 60, kind)
    W = mp.fsum(F(t) for t in w)
    ua = mp.fsum(F(a) * F(b) for a, b in zip(w, u)) / W
    raw = [mp.fsum(F(wi) * F(ui) ** b for wi, ui in zip(w, u)) / W for b in range(M)]
    cen = [mp.fsum(F(wi) * (F(ui) - ua) ** b for wi, ui in zip(w, u)) / W for b in range(M)]
    raw[0] = cen[0] = W
    if M > 1:
        cen[1] = ua
    cen64 = np.array([float(v) for v in cen])
    raw64 = np.array([float(v) for v in raw])
    for src, to_c in ((cen64, False), (raw64, True)):
        m = [F(v) for v in src]
        mean = m[1] if M > 1 else mp.mpf(0)
        su = -mean if to_c else mean
        want, bnd = [], []
        for b in range(M):
            terms = []
            for j in range(b + 1):
                mj = mp.mpf(1) if j == 0 else (mp.mpf(0) if (j == 1 and not to_c) else m[j])
                terms.append(mp.binomial(b, j) * mj * su ** (b - j))
            want.append(mp.fsum(terms))
            bnd.append(mp.fsum(abs(t) for t in terms))
        want[0] = bnd[0] = m[0]
        if M > 1 and to_c:
            want[1], bnd[1] = m[1], abs(m[1])
        got, gb = tl.convert_1d(src[None], to_c, return_bound=True)
        assert_mp_close(got[0], want, bnd, what=f"1d to_central={to_c}")
        ref = orc.convert_1d(src[None], to_c)[0]
        assert np.all(np.abs(ref - got[0]) <= 1e-14 * gb[0])
    got = tl.convert_1d(cen64, False, return_bound=True)
    assert np.all(np.abs(got[0] - raw64) <= 1e-14 * got[1])


# ---------------------------------------------------------------------------
# resample_data / reduce_data
# ---------------------------------------------------------------------------
def mp_merge(blocks, counts, K, ox=0.0, ou=0.0):
    """Merge of float64 central states [nrec][2][K] with integer counts, in mpmath: raw sums about (ox, ou)."""
    ox, ou = F(ox), F(ou)
    tot = [[mp.mpf(0)] * K for _ in range(2)]
    for st, f in zip(blocks, counts):
        W = F(st[0, 0])
        if W == 0 or f == 0:
            continue
        m = [[F(v) for v in row] for row in st]
        xa = m[1][0]
        ua = m[0][1] if K > 1 else mp.mpf(0)
        m[1][0] = mp.mpf(0)
        if K > 1:
            m[0][1] = mp.mpf(0)
        about, _ = mp_shift(m, xa - ox, ua - ou, K)
        about[0][0] = mp.mpf(1)
        for a in range(2):
            for b in range(K):
                tot[a][b] += f * W * about[a][b]
    Wt = tot[0][0]
    if Wt == 0:
        z = [[mp.mpf(0)] * K for _ in range(2)]
        return z, z
    mm = [[v / Wt for v in row] for row in tot]
    dx = mm[1][0]
    du = mm[0][1] if K > 1 else mp.mpf(0)
    out, bnd = mp_shift(mm, -dx, -du, K)
    out[0][0] = bnd[0][0] = Wt
    out[1][0], bnd[1][0] = ox + dx, abs(ox) + abs(dx)
    if K > 1:
        out[0][1], bnd[0][1] = ou + du, abs(ou) + abs(du)
    return out, bnd


@pytest.mark.parametrize("order", range(9))
@pytest.mark.parametrize("kind", ["idealgas", "unit"])
def test_resample_data_vs_mpmath_and_compiled_oracle(orc, order, kind):
    rng = np.random.default_rng(100 + order)
    nrec, nb, K = 6, 30, order + 1
    x, u, w = samples(rng, nrec * nb, kind)
    blocks = np.stack([to_f64(mp_moments(x[i * nb:(i + 1) * nb], u[i * nb:(i + 1) * nb], w[i * nb:(i + 1) * nb], order)[0])
                       for i in range(nrec)])
    blocks[4] = 0.0                                           # a record of weight 0 with all-zero moments
    freq = np.array([[1, 1, 1, 1, 1, 1], [0, 3, 0, 300, 1, 0], [0, 0, 0, 0, 5, 0], [0, 0, 2, 0, 0, 0]])
    data = blocks[:, None]                                    # C = 1
    # about zero the powers of a mean 33 sigma away cancel: ~33^order * eps_ld relative to the central moment.  The
    # mpmath pin follows the same origin, so both origins are held to the same 1e-17 of the sum bound.
    origins = [None] if kind == "unit" else [None, np.array([[170.0, 0.5]])]
    for origin in origins:
        got, gb = tl.resample_data(data, freq, order, origin=origin, return_bound=True)
        ou, ox = (0.0, 0.0) if origin is None else origin[0]
        for r in range(freq.shape[0]):
            want, bnd = mp_merge(blocks, freq[r], K, ox, ou)
            # the weight-scaled sums carry eps_ld relative to sum |f W m_about|: for moments about zero of a mean 33
            # sigma out that is 33^b times the central scale, which the bound of the re-centralisation sum also has
            assert_mp_close(got[r, 0], want, bnd, tol=20 * TOL, what=f"rep {r} origin {origin is not None}")
            assert_mp_close(gb[r, 0], bnd, bnd, tol=1e-14, what="bound")
        assert np.array_equal(got[2, 0], np.zeros((2, K)))    # only the weight-0 record drawn: the empty state
        red = tl.reduce_data(data, order, origin=origin)
        assert np.array_equal(red, got[0])
    # whole-series truth: merging the blocks gives the moments of the samples the live blocks hold
    live = np.r_[0:4 * nb, 5 * nb:6 * nb]
    cen, _ = mp_moments(x[live], u[live], w[live], order)
    got, gb = tl.resample_data(data, freq[:1], order, origin=origins[-1], return_bound=True)
    assert np.all(np.abs(got[0, 0] - to_f64(cen)) <= 1e-13 * gb[0, 0])
    # compiled oracle (sequential pairwise merges in float64) on the rows that hold weight
    ref = orc.resample_data(data, freq, order)
    sc = np.std(u) ** np.arange(K)
    sc = np.stack([sc, np.std(x) * sc])
    for r in (0, 1, 3):
        mine = tl.resample_data(data, freq[r:r + 1], order, origin=origins[-1])[0, 0]
        assert np.all(np.abs(ref[r, 0] - mine) <= 1e-11 * (np.abs(ref[r, 0]) + sc))
    assert np.array_equal(ref[2, 0], np.zeros((2, K)))
    np.testing.assert_allclose(orc.reduce_data(data, order), ref[0], rtol=1e-13, atol=1e-13)
