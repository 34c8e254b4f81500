"""timeseries.py without a device: the subsampling rule against pymbar's literal while-loop, the host scan over lag blocks
against a restatement of the estimator in numpy.longdouble (mpmath on a small case), and the C ABI's host-side validation.

The restatement (`ref_scan`, `ref_lag_sum`) is the estimator exactly as the module docstring of thermoextrap_amd/timeseries.py
states it, one lag at a time in extended precision; tests/test_timeseries_gpu.py holds the device to it as well."""

import ctypes as ct
import math

import numpy as np
import pytest

LD = np.longdouble


# ---------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------
def ref_centered(A, B=None):
    A = np.asarray(A, dtype=LD)
    B = A if B is None else np.asarray(B, dtype=LD)
    return A - A.mean(dtype=LD), B - B.mean(dtype=LD)


def ref_lag_sum(dA, dB, t):
    """R(t) = sum_{n < N - t} (dA_n dB_{n+t} + dB_n dA_{n+t}) in long double; 0 for t >= N."""
    N = len(dA)
    if t >= N:
        return LD(0)
    if dA is dB:
        return 2 * np.dot(dA[: N - t], dA[t:])
    return np.dot(dA[: N - t], dB[t:]) + np.dot(dB[: N - t], dA[t:])


def ref_scan(A, B=None, fast=False, mintime=3, cache=None):
    """(g, stop lag, visited [(t, C(t), inc)]) of the loop for g, in long double.  `cache` (a dict) keeps the lag sums
    of one pair of series between calls (plain and fast visit many of the same lags) and receives "c_stop": the C(t) <= 0
    the loop ended on, None when the series ran out first."""
    cache = {} if cache is None else cache
    if "cen" not in cache:
        cache["cen"] = ref_centered(A, B)
    dA, dB = cache["cen"]
    N = len(dA)
    sig2 = np.mean(dA * dB, dtype=LD)
    if sig2 == 0:
        raise ValueError("sigma^2 == 0")
    g, t, inc, visited = LD(1), 1, 1, []
    cache["c_stop"] = None
    while t < N - 1:
        if t not in cache:
            cache[t] = ref_lag_sum(dA, dB, t)
        C = cache[t] / (2 * LD(N - t) * sig2)
        if C <= 0 and t > mintime:
            cache["c_stop"] = C
            break
        visited.append((t, C, inc))
        g += 2 * C * (1 - LD(t) / LD(N)) * inc
        t += inc
        if fast:
            inc += 1
    return max(g, LD(1)), t, visited


def g_bound(visited):
    return 1e-11 * (1.0 + float(sum(2 * abs(c) * inc for _, c, inc in visited)))


def numpy_fetch(series):
    """fetch(pairs, t0, nlags) for timeseries.scan_lag_sums out of numpy: pair p of `series` [(A, B or None), ...]."""
    cen = [ref_centered(A, B) for A, B in series]

    def fetch(pairs, t0, nlags):
        return np.array([[float(ref_lag_sum(*cen[p], t)) for t in range(t0, t0 + nlags)] for p in pairs])

    return fetch


# ---------------------------------------------------------------------------
# subsampling
# ---------------------------------------------------------------------------
def literal_subsample(T, g, conservative=False):
    if conservative:
        return list(range(0, T, int(math.ceil(g))))
    idx, n = [], 0
    while True:
        t = int(round(n * g))
        if t >= T:
            break
        if not idx or idx[-1] != t:
            idx.append(t)
        n += 1
    return idx


@pytest.mark.parametrize("conservative", [False, True])
def test_subsample_matches_the_literal_loop(conservative):
    from thermoextrap_amd.timeseries import subsample_correlated_data

    rng = np.random.default_rng(5)
    gs = [1.0, 1.5, 2.0, 2.5, 3.5, 4.5, 0.5, 0.3, 1.0000001, 7.0, 18.0, 33.3333333, 99.5, math.pi, math.e, 1e3 / 3, 12345.678,
          *rng.uniform(1.0, 50.0, 12).tolist()]
    for T in (1, 2, 3, 7, 100, 101, 4099, 100_000):
        for g in gs:
            got = subsample_correlated_data(T, g, conservative=conservative)
            assert got.dtype == np.int64
            assert got.tolist() == literal_subsample(T, g, conservative), (T, g)
    # A_t as an array with g given: only its length counts
    assert subsample_correlated_data(np.zeros(50), 2.5).tolist() == literal_subsample(50, 2.5)
    assert subsample_correlated_data(0, 2.0).size == 0
    with pytest.raises(ValueError):
        subsample_correlated_data(10, 0.0)
    with pytest.raises(ValueError):
        subsample_correlated_data(10)


# ---------------------------------------------------------------------------
# host scan
# ---------------------------------------------------------------------------
def check_scan(series, n, **kw):
    from thermoextrap_amd.timeseries import scan_lag_sums

    calls = []
    base = numpy_fetch(series)

    def fetch(pairs, t0, nlags):
        calls.append((list(pairs), t0, nlags))
        return base(pairs, t0, nlags)

    g, stop = scan_lag_sums(fetch, n, range(len(series)), **kw)
    for p, (A, B) in enumerate(series):
        gr, sr, vis = ref_scan(A, B, fast=kw.get("fast", False), mintime=kw.get("mintime", 3))
        assert stop[p] == sr, (p, stop[p], sr)
        assert abs(g[p] - float(gr)) <= g_bound(vis), (p, g[p], float(gr))
    return g, stop, calls


def _cosine(P, N=12000, seed=0):
    rng = np.random.default_rng(seed)
    return np.cos(2 * np.pi * np.arange(N) / P) + 0.01 * rng.standard_normal(N)


def test_lag_block_schedule():
    from thermoextrap_amd.timeseries import lag_blocks

    assert list(lag_blocks(2)) == [(0, 256)]
    assert list(lag_blocks(257)) == [(0, 256)] and list(lag_blocks(258)) == [(0, 256), (256, 256)]
    b = list(lag_blocks(100_000))
    assert b[:7] == [(0, 256), (256, 256), (512, 512), (1024, 1024), (2048, 2048), (4096, 4096), (8192, 4096)]
    assert all(t0 % 256 == 0 and nl % 256 == 0 and nl <= 4096 for t0, nl in b)
    assert all(b[i + 1][0] == b[i][0] + b[i][1] for i in range(len(b) - 1)) and b[-1][0] < 99_999 <= b[-1][0] + b[-1][1]


def test_scan_stop_lags_around_the_block_edges():
    """Series whose correlation function first turns negative at 255 / 256 / 257 (first block edge), 511 / 512 / 513 and
    1024: a cosine of period P crosses zero at P / 4."""
    periods = [1018, 1022, 1026, 2054, 2058, 2060, 4190]       # (found with the restatement: the mean removal shifts P / 4 a little)
    series = [(_cosine(P), None) for P in periods]
    g, stop, calls = check_scan(series, 12000)
    assert stop.tolist() == [255, 256, 257, 511, 512, 513, 1024]
    # pairs that have stopped are dropped from the next call's list; the scan ends with the last of them
    assert [(len(p), t0, nl) for p, t0, nl in calls] == [(7, 0, 256), (6, 256, 256), (3, 512, 512), (1, 1024, 1024)]


@pytest.mark.parametrize("fast", [False, True])
def test_scan_short_series_run_to_the_end(fast):
    """N = 2 .. 300: t reaches N - 1 before (or just as) the correlation function turns negative."""
    rng = np.random.default_rng(11)
    for n in list(range(2, 40)) + [63, 64, 100, 255, 256, 257, 258, 259, 300]:
        e = rng.standard_normal(n)
        ramp = np.linspace(0.0, 3.0, n) ** 2 + 0.05 * e           # stays correlated to the end
        noise = rng.standard_normal(n)
        check_scan([(ramp, None), (noise, None), (ramp, noise + ramp)], n, fast=fast)


def test_scan_fast_and_mintime():
    rng = np.random.default_rng(3)
    from scipy.signal import lfilter

    a = lfilter([1.0], [1.0, -0.95], rng.standard_normal(6000))
    b = 0.5 * a + lfilter([1.0], [1.0, -0.6], rng.standard_normal(6000))
    alt = np.tile([1.0, -1.0], 3000) + 0.1 * rng.standard_normal(6000)   # C(1) < 0: only mintime keeps the loop going
    for kw in ({}, {"fast": True}, {"mintime": 0}, {"mintime": 1}, {"mintime": 10}, {"fast": True, "mintime": 7}):
        g, stop, _ = check_scan([(a, None), (b, None), (a, b), (alt, None)], 6000, **kw)
        if not kw.get("fast"):                                   # C(t) ~ (-1)^t: the first odd lag past mintime
            mt = kw.get("mintime", 3)
            assert stop[3] == (mt + 1 if mt % 2 == 0 else mt + 2)
    g, _, _ = check_scan([(alt, None)], 6000)
    assert g[0] == 1.0                                           # max(g, 1)


def test_scan_negative_sigma2_and_zero_sigma2():
    from thermoextrap_amd.timeseries import scan_lag_sums

    rng = np.random.default_rng(8)
    from scipy.signal import lfilter

    u = lfilter([1.0], [1.0, -0.9], rng.standard_normal(5000))
    a = -u + 0.3 * rng.standard_normal(5000)                      # anticorrelated pair: sigma_AB^2 < 0, no special case
    g, stop, _ = check_scan([(a, u)], 5000)
    assert g[0] > 5.0
    const = np.full(100, 2.5)
    with pytest.raises(ValueError, match="x\\[0\\]"):
        scan_lag_sums(numpy_fetch([(u[:100], None), (const, None)]), 100, [0, 1], names=["u", "x[0]"])
    with pytest.raises(ValueError):
        ref_scan(const)


def test_scan_max_lag():
    from thermoextrap_amd.timeseries import scan_lag_sums

    s = _cosine(2058)                                             # stops at 512
    f = numpy_fetch([(s, None)])
    g, stop = scan_lag_sums(f, len(s), [0], max_lag=512)
    assert stop[0] == 512
    with pytest.raises(ValueError, match="energy"):
        scan_lag_sums(f, len(s), [0], max_lag=511, names=["energy"])


def test_restatement_against_mpmath():
    """The long-double restatement itself on a small case, against 50-digit arithmetic."""
    import mpmath as mp

    mp.mp.dps = 50
    rng = np.random.default_rng(2)
    from scipy.signal import lfilter

    A = lfilter([1.0], [1.0, -0.8], rng.standard_normal(200)) + 5.0
    B = 0.3 * A + rng.standard_normal(200)
    for pair in ((A, None), (A, B)):
        a = [mp.mpf(float(v)) for v in pair[0]]
        b = a if pair[1] is None else [mp.mpf(float(v)) for v in pair[1]]
        N = len(a)
        ma, mb = mp.fsum(a) / N, mp.fsum(b) / N
        da, db = [v - ma for v in a], [v - mb for v in b]
        s2 = mp.fsum(x * y for x, y in zip(da, db)) / N
        g, t = mp.mpf(1), 1
        while t < N - 1:
            R = mp.fsum(da[n] * db[n + t] + db[n] * da[n + t] for n in range(N - t))
            C = R / (2 * (N - t) * s2)
            if C <= 0 and t > 3:
                break
            g += 2 * C * (1 - mp.mpf(t) / N)
            t += 1
        gr, sr, vis = ref_scan(*pair)
        assert sr == t and abs(float(gr) - float(g)) <= 1e-15 * (1 + sum(2 * abs(float(c)) for _, c, _ in vis))


# ---------------------------------------------------------------------------
# the C ABI without a device
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from thermoextrap_amd import _build, _lib

    _build.build_library()
    return _lib.load()


def test_ws_bytes_and_validation_need_no_device(lib):
    W = lib.txm_lag_sums_ws_bytes
    n, C = 200_000, 5
    base = W(n, C, 1, 256)
    assert base >= 8 * (1 + C) * n                                 # the centred series as contiguous rows
    # partials: one [pairs][nlags] block per chunk of 1008 samples (n <= 1008 * 512)
    chunks = -(-n // 1008)
    assert W(n, C, 11, 256) - base == chunks * 10 * 256 * 8
    assert W(n, C, 1, 1024) - base == chunks * 768 * 8
    assert W(100_000_000, 32, 65, 4096) < 30 << 30
    for bad in ((0, C, 1, 256), (n, -1, 1, 256), (n, C, 0, 256), (n, C, 12, 256), (n, C, 1, 0), (n, C, 1, 255), (n, C, 1, 8192)):
        assert W(*bad) == 0, bad
    assert W(n, 0, 1, 256) > 0 and W(n, 0, 2, 256) == 0

    one = ct.c_void_p(4096)                                        # never dereferenced: validation comes first
    pairs = (ct.c_int32 * 3)(0, 1, 10)
    F = lib.txm_lag_sums

    def call(x=one, ldx=8, u=one, n=1000, C=5, center=one, pl=pairs, npairs=3, t0=0, nlags=256, out=one, ws=one, nws=1 << 40):
        return F(x, ldx, u, n, C, center, pl, npairs, t0, nlags, out, ws, nws, None)

    assert call(u=None) == -1 and b"null" in lib.txm_last_error()
    assert call(out=None) == -1 and call(ws=None) == -1 and call(center=None) == -1 and call(pl=None) == -1
    assert call(x=None) == -1 and b"null x" in lib.txm_last_error()
    assert call(t0=100) == -1 and b"t0" in lib.txm_last_error()
    assert call(t0=-256) == -1
    assert call(nlags=300) == -1 and b"nlags" in lib.txm_last_error()
    assert call(nlags=0) == -1 and call(nlags=8192) == -1
    assert call(pl=(ct.c_int32 * 3)(0, 1, 11), C=5) == -1 and b"pair index 11" in lib.txm_last_error()   # 2 C = 10 is the last
    assert call(pl=(ct.c_int32 * 3)(0, -1, 2)) == -1
    assert call(ldx=4) == -1 and b"pitch" in lib.txm_last_error()
    assert call(n=0) == -1 and call(npairs=0) == -1 and call(npairs=12) == -1
    assert call(pl=(ct.c_int32 * 3)(0, 1, 10), nws=16) == -3 and b"workspace" in lib.txm_last_error()
    # x = NULL with C = 0 is legal: it gets as far as the workspace check
    assert call(x=None, ldx=0, C=0, pl=(ct.c_int32 * 1)(0), npairs=1, nws=16) == -3


def test_module_is_exported_lazily():
    import thermoextrap_amd as txa

    assert txa.timeseries.subsample_correlated_data is txa.subsample_correlated_data
    for name in ("statistical_inefficiency", "statistical_inefficiencies", "normalized_fluctuation_correlation_function", "decorrelate"):
        assert callable(getattr(txa, name)) and name in txa.__all__


def test_inputs_other_than_arrays_raise():
    """The type check comes before anything else a call does once a device is bound; without one the call must raise
    TxmError, not fall back to a host computation."""
    import torch

    import thermoextrap_amd as txa

    if torch.cuda.is_available():
        with pytest.raises(TypeError):
            txa.statistical_inefficiency([1.0, 2.0, 3.0])
    else:
        with pytest.raises(txa.TxmError):
            txa.statistical_inefficiency(np.arange(10.0))
