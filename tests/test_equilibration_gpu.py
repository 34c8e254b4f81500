"""Equilibration detection on the device against the long-double restatement of tests/test_equilibration_cpu.py.

Lag sums of every suffix (engine.lag_origin_sums -> txm_lag_origin_sums), against the direct sum on each suffix centred with
its own mean: |hip - ref| <= 1e-12 * 2 sum_{n=t0}^{T-1-t} (|d_n| + |delta|)(|d_{n+t}| + |delta|) with d = A - p and
delta = mean(A[t0:]) - p of the pivot p the test passed in -- the project's 1e-12 rule on the first-order bound of the
expanded form R = 2 [Q - delta X + (M - t) delta^2].  The suffix means: 1e-13 (|p| + mean |d|).
t, g and Neff: the decisions are discrete, so every case first asserts margins on the restatement alone (every visited
|C_ref(t)| >= 1e-9 at every origin, the two largest Neff_ref more than 1e-9 apart), then equal stop lags,
|g - g_ref| <= 1e-11 (1 + sum 2 |C_ref| inc) per origin, equal t, and Neff to the same relative bound."""

import numpy as np
import pytest
import torch

from test_equilibration_cpu import neff_margin, ref_detect, transient_series
from test_timeseries_cpu import LD, g_bound, ref_centered, ref_lag_sum

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(txm):
    from thermoextrap_amd import engine

    assert engine.LAG_STAGE == 1008
    return engine


def state_with_transient(T, C, seed):
    """u and x (T, C): offset, correlated series with different scales and a decaying transient on each."""
    from scipy.signal import lfilter

    rng = np.random.default_rng(seed)
    n = np.arange(T)
    u = 174.85 + 5.31 * lfilter([1], [1, -0.9], rng.standard_normal(T)) * np.sqrt(1 - 0.81) + 20.0 * np.exp(-n / (0.1 * T + 1))
    x = np.empty((T, C))
    for c in range(C):
        ph = 0.3 + 0.3 * c
        x[:, c] = (0.2 + c) + 1e-3 * u + 0.05 * lfilter([1], [1, -ph], rng.standard_normal(T)) - 0.3 * np.exp(-n / (0.03 * (c + 1) * T + 1))
    return u, x


def series_row(s, u, x):
    return u if s == 0 else x[:, s - 1]


def pitched(x):
    """x on the device as a column slice of a wider matrix (row pitch > C); None for C = 0."""
    T, C = x.shape
    if C == 0:
        return None
    big = torch.zeros((T, C + 3), dtype=torch.float64, device="cuda")
    big[:, :C] = torch.as_tensor(x).cuda()
    xd = big[:, :C]
    assert xd.stride(0) == C + 3
    return xd


def sample_origins(no):
    return sorted({j for j in (0, 1, 2, no // 3, no // 2, no - 3, no - 2, no - 1) if 0 <= j < no})


def sample_lags(t0, nlags, M):
    base = {0, 1, 2, 15, 16, 17, 100, 255, 256, 257, 511, 512, 777, 1023, M - 2, M - 1, M, M + 1}
    return sorted(t for t in base if t0 <= t < t0 + nlags)


worst = {"scaled": 0.0, "mean": 0.0}


def check_origin_sums(eng, u, x, xd, series, nskip, t0, nlags, center):
    """engine.lag_origin_sums on (t0, nlags) against the restatement on sampled (origin, lag) entries; returns (R, means)."""
    T = len(u)
    ud = torch.as_tensor(u).cuda()
    cen_d = torch.as_tensor(center).cuda()
    got, mean = eng.lag_origin_sums(xd, ud, series, nskip, t0, nlags, center=cen_d)
    origins = list(range(0, T - 1, nskip))
    assert got.shape == (len(series), len(origins), nlags) and mean.shape == (len(series), len(origins))
    R, mu = got.cpu().numpy(), mean.cpu().numpy()
    for row, s in enumerate(series):
        A = np.asarray(series_row(s, u, x), dtype=LD)
        p = LD(center[s])
        d = A - p
        ad = np.abs(d)
        for j in sample_origins(len(origins)):
            o = origins[j]
            M = T - o
            m_ref = A[o:].mean(dtype=LD)
            delta = abs(m_ref - p)
            mean_bound = 1e-13 * float(abs(p) + ad[o:].mean(dtype=LD))
            worst["mean"] = max(worst["mean"], abs(mu[row, j] - float(m_ref)) / mean_bound * 1e-13)
            assert abs(mu[row, j] - float(m_ref)) <= mean_bound, (T, nskip, s, j, mu[row, j], float(m_ref))
            dc = ref_centered(A[o:])[0]
            assert (R[row, j, max(M - t0, 0):] == 0.0).all()                       # lags beyond the suffix
            for t in sample_lags(t0, nlags, M):
                if t >= M:
                    assert R[row, j, t - t0] == 0.0
                    continue
                ref = float(ref_lag_sum(dc, dc, t))
                bound = 1e-12 * 2 * float(np.dot(ad[o:T - t] + delta, ad[o + t:] + delta))
                err = abs(R[row, j, t - t0] - ref)
                if bound > 0:
                    worst["scaled"] = max(worst["scaled"], err / bound * 1e-12)
                assert err <= bound, (T, nskip, s, o, t, R[row, j, t - t0], ref, err, bound)
    return got, mean


# T against the stage length of 1008 and the 256-lag tiles; nskip shorter than a stage, equal, one over, not a multiple
SHAPES = [(2, 7, 0), (255, 7, 1), (257, 100, 3), (1009, 1008, 1), (1009, 1009, 0), (1009, 100, 3), (3000, 7, 0), (3000, 1008, 3),
          (3000, 1009, 1), (3000, 1500, 0), (3000, 2500, 1), (20011, 7, 1), (20011, 100, 3), (20011, 1008, 0), (20011, 1009, 3),
          (20011, 1500, 1), (20011, 2500, 3)]


@pytest.mark.parametrize("T,nskip,C", SHAPES)
def test_origin_sums_through_the_abi(eng, T, nskip, C):
    u, x = state_with_transient(T, C, seed=T + nskip)
    xd = pitched(x)
    series = {0: [0], 1: [1, 0], 3: [2, 0, 3]}[C]                                   # a subset, not monotone
    half = np.array([series_row(s, u, x)[T // 2:].mean() for s in range(1 + C)])
    far = half + 3.0 * np.array([series_row(s, u, x).std() for s in range(1 + C)])
    for center in (half, far):
        blocks = {}
        for t0, nlags in ((0, 256), (256, 256), (0, 1024)):
            blocks[(t0, nlags)], mean = check_origin_sums(eng, u, x, xd, series, nskip, t0, nlags, center)
        # bits: two runs; a block of 1024 lags and its four pieces; the tight layout
        ud, cd = torch.as_tensor(u).cuda(), torch.as_tensor(center).cuda()
        again, mean2 = eng.lag_origin_sums(xd, ud, series, nskip, 0, 1024, center=cd)
        assert torch.equal(again, blocks[(0, 1024)]) and torch.equal(mean, mean2)
        four = torch.cat([eng.lag_origin_sums(xd, ud, series, nskip, 256 * k, 256, center=cd)[0] for k in range(4)], dim=2)
        assert torch.equal(four, blocks[(0, 1024)])
        assert torch.equal(four[:, :, :256], blocks[(0, 256)]) and torch.equal(four[:, :, 256:512], blocks[(256, 256)])
        if C:
            tight, _ = eng.lag_origin_sums(torch.as_tensor(x).cuda(), ud, series, nskip, 0, 256, center=cd)
            assert torch.equal(tight, blocks[(0, 256)])
    print(f"origin lag sums: worst scaled error so far {worst['scaled']:.3e} (limit 1e-12), suffix means {worst['mean']:.3e} (limit 1e-13)")


def test_origin_zero_agrees_with_lag_sums(eng):
    """Origin 0 with the full mean as the pivot is txm_lag_sums' auto pair: within the sum of both tolerances."""
    T, C = 20011, 3
    u, x = state_with_transient(T, C, seed=3)
    ud, xd = torch.as_tensor(u).cuda(), torch.as_tensor(x).cuda()
    cen = eng.lag_center(xd, ud)
    a = eng.lag_sums(xd, ud, [0, 1, 2, 3], 0, 1024, center=cen).cpu().numpy()
    b = eng.lag_origin_sums(xd, ud, [0, 1, 2, 3], 1500, 0, 1024, center=cen)[0].cpu().numpy()
    p = cen.cpu().numpy()
    for s in range(1 + C):
        A = np.asarray(series_row(s, u, x), dtype=LD)
        dA = ref_centered(A)[0]
        mid = 1.0 + 2.0 * abs(float(A.mean())) / float(dA.std())
        ad, aA = np.abs(A - LD(p[s])), np.abs(dA)
        delta = abs(A.mean(dtype=LD) - LD(p[s]))
        for t in (0, 1, 17, 255, 256, 1000, 1023):
            tol = 1e-12 * (mid * float(np.dot(aA[:T - t], aA[t:])) + 2 * float(np.dot(ad[:T - t] + delta, ad[t:] + delta)))
            assert abs(a[s, t] - b[s, 0, t]) <= tol, (s, t, a[s, t], b[s, 0, t])


def test_default_pivot_budget_and_errors(eng, txm):
    T, C = 20011, 3
    u, x = state_with_transient(T, C, seed=5)
    ud, xd = torch.as_tensor(u).cuda(), torch.as_tensor(x).cuda()
    cen = eng.lag_origin_center(xd, ud).cpu().numpy()
    half = np.array([series_row(s, u, x)[T // 2:].mean() for s in range(1 + C)])
    assert np.allclose(cen, half, rtol=1e-13, atol=0)
    full, mean = eng.lag_origin_sums(xd, ud, [0, 1, 2, 3], 100, 0, 1024)
    assert torch.equal(full, eng.lag_origin_sums(xd, ud, [0, 1, 2, 3], 100, 0, 1024, center=torch.as_tensor(cen).cuda())[0])
    # a workspace budget below what 1024 lags need: shorter lag blocks, the same bits
    old = eng.WORKSPACE_BUDGET_BYTES
    try:
        eng.WORKSPACE_BUDGET_BYTES = eng._L().txm_lag_origin_sums_ws_bytes(T, C, 4, 100, 512) + 1
        cut, mean2 = eng.lag_origin_sums(xd, ud, [0, 1, 2, 3], 100, 0, 1024)
        eng.WORKSPACE_BUDGET_BYTES = 1
        cut2, _ = eng.lag_origin_sums(xd, ud, [0, 1, 2, 3], 100, 0, 1024)
    finally:
        eng.WORKSPACE_BUDGET_BYTES = old
    assert torch.equal(cut, full) and torch.equal(cut2, full) and torch.equal(mean, mean2)
    with pytest.raises(ValueError, match="smallest legal nskip is 5"):
        eng.lag_origin_sums(xd, ud, [0], 4, 0, 256)
    with pytest.raises(txm.TxmError, match="series index 4"):
        eng.lag_origin_sums(xd, ud, [0, 4], 100, 0, 256)
    with pytest.raises(txm.TxmError, match="t0"):
        eng.lag_origin_sums(xd, ud, [0], 100, 100, 256)


# ---------------------------------------------------------------------------
# detection
# ---------------------------------------------------------------------------
T_DET = 20000
TAUS = (150.0, 300.0, 600.0)                      # of u, x_0, x_1: different, so that t0_max is exercised
SEEDS = {0.5: 101, 0.9: 202}
_data, _caches = {}, {}


def detect_state(phi, a):
    """u and x (T_DET, 2): seeded AR(1) series with phi plus a * sigma * exp(-n / tau), tau per series."""
    if (phi, a) not in _data:
        cols = [transient_series(T_DET, phi, a, tau, seed=SEEDS[phi] + k) + 1.5 * k for k, tau in enumerate(TAUS)]
        _data[(phi, a)] = (cols[0], np.stack(cols[1:], axis=1))
    return _data[(phi, a)]


def detect_reference(phi, a, s, nskip, fast):
    """ref_detect of series s of detect_state(phi, a); the lag sums of a suffix are kept between the cases that share it."""
    u, x = detect_state(phi, a)
    return ref_detect(series_row(s, u, x), fast=fast, nskip=nskip, caches=_caches.setdefault((phi, a, s), {}))


def margins_hold(ref):
    cs = [abs(float(c)) for vis in ref["vis_t"] for _, c, _ in vis] + [abs(float(c)) for c in ref["c_stop_t"] if c is not None]
    return min(cs) >= 1e-9 and neff_margin(ref) > 1e-9


def assert_detection(ref, origins, g_t, neff_t, t0, g, neff, label):
    assert origins.tolist() == ref["origins"], label
    for j in range(len(origins)):
        assert abs(g_t[j] - float(ref["g_t"][j])) <= g_bound(ref["vis_t"][j]), (label, j, g_t[j], float(ref["g_t"][j]))
        rel = g_bound(ref["vis_t"][j]) / float(ref["g_t"][j])
        assert abs(neff_t[j] - float(ref["neff_t"][j])) <= rel * float(ref["neff_t"][j]), (label, j)
    assert t0 == ref["t"], (label, t0, ref["t"])
    j = ref["index"]
    assert g == g_t[j] and neff == neff_t[j], label


@pytest.mark.parametrize("fast", [True, False])
@pytest.mark.parametrize("nskip", [100, 1000])
@pytest.mark.parametrize("a", [0.0, 5.0])
@pytest.mark.parametrize("phi", [0.5, 0.9])
def test_detect_equilibrations(txm, phi, a, nskip, fast):
    """Every (series, origin) of the grid against the restatement.  The seeds were picked on the CPU with the restatement
    alone (tests/test_equilibration_cpu.py's ref_detect) so that no case of the grid fails its margins -- none is skipped --
    and so that the transients are found where the sanity check below expects them."""
    from thermoextrap_amd.timeseries import scan_origin_lag_sums

    u, x = detect_state(phi, a)
    refs = [detect_reference(phi, a, s, nskip, fast) for s in range(3)]
    if not all(margins_hold(r) for r in refs):
        pytest.skip("the restatement's own margin is below 1e-9: the decision is a coin toss")
    e = txm.detect_equilibrations(u, x, fast=fast, nskip=nskip)
    assert e.origins.shape == e.g_t.shape == e.neff_t.shape == (3, len(range(0, T_DET - 1, nskip)))
    # the stop lags: the same scan, asked for them
    from thermoextrap_amd import engine

    ud, xd = torch.as_tensor(u).cuda(), torch.as_tensor(x).cuda()
    cen = engine.lag_origin_center(xd, ud)
    g2, stop, zero = scan_origin_lag_sums(lambda sl, t0, nl: engine.lag_origin_sums(xd, ud, sl, nskip, t0, nl, center=cen)[0].cpu().numpy(),
                                          T_DET, nskip, range(3), fast=fast)
    assert np.array_equal(g2, e.g_t) and not zero.any()
    for s, ref in enumerate(refs):
        assert stop[s].tolist() == ref["stop_t"], (s, stop[s].tolist(), ref["stop_t"])
        assert_detection(ref, e.origins[s], e.g_t[s], e.neff_t[s], int(e.t0[s]), float(e.g[s]), float(e.neff[s]), (phi, a, nskip, fast, s))
        if a > 0:
            assert 0 < e.t0[s] <= 10 * TAUS[s], (s, e.t0[s])
    assert e.t0_max == max(r["t"] for r in refs)
    # one series through pymbar's signature
    t, g, neff = txm.detect_equilibration(x[:, 1], fast, nskip)
    assert t == refs[2]["t"] and abs(g - float(refs[2]["g"])) <= g_bound(refs[2]["vis_t"][refs[2]["index"]])
    assert abs(neff - float(refs[2]["neff"])) <= g_bound(refs[2]["vis_t"][refs[2]["index"]]) / float(refs[2]["g"]) * float(refs[2]["neff"])


def test_detect_equilibration_defaults_and_degenerate_series(txm):
    u, x = detect_state(0.5, 5.0)
    # nskip None: the smallest step with at most max_origins origins
    t, g, neff = txm.detect_equilibration(u, max_origins=50)
    ref = ref_detect(u, fast=True, nskip=400)
    assert len(ref["origins"]) == 50 and t == ref["t"] and abs(g - float(ref["g"])) <= g_bound(ref["vis_t"][ref["index"]])
    with pytest.raises(ValueError, match="smallest legal nskip is 5"):
        txm.detect_equilibration(u, nskip=4)
    with pytest.raises(ValueError):
        txm.detect_equilibration(u[:1])
    assert txm.detect_equilibration(np.full(500, 2.5), nskip=10) == (0, 1.0, 1.0)
    t, g, neff = txm.detect_equilibration(np.array([1.0, 3.0]))
    assert (t, g, neff) == (0, 1.0, 3.0)


def test_constant_tail_away_from_the_pivot(txm, eng):
    """A tail that is constant, shorter than half the series and far from the second-half mean: its suffixes have zero
    variance, which the device's expansion around the pivot reproduces only to rounding.  They must take the fallback
    g = M + 1 (Neff = 1), not a g made of rounding noise, and the answer must be the restatement's."""
    from thermoextrap_amd.timeseries import scan_origin_lag_sums

    head = transient_series(7000, 0.5, 3.0, 200.0, seed=9) + 7.3
    series = np.concatenate([head, np.full(3000, 2.7)])
    ref = ref_detect(series, fast=True, nskip=500)
    assert ref["zero_t"] == [False] * 14 + [True] * 6 and margins_hold(ref)
    e = txm.detect_equilibrations(series, None, nskip=500)
    assert e.g_t[0, 14:].tolist() == [3001.0, 2501.0, 2001.0, 1501.0, 1001.0, 501.0] and (e.neff_t[0, 14:] == 1.0).all()
    assert_detection(ref, e.origins[0], e.g_t[0], e.neff_t[0], int(e.t0[0]), float(e.g[0]), float(e.neff[0]), "constant tail")
    # the same with an explicit pivot 3 sigma off, through the scan
    ud = torch.as_tensor(series).cuda()
    cen = torch.as_tensor([series[5000:].mean() + 3.0 * series.std()]).cuda()

    def fetch(sl, t0, nl):
        R, mean = eng.lag_origin_sums(None, ud, sl, 500, t0, nl, center=cen)
        return (R.cpu().numpy(), (mean - cen[0]).cpu().numpy()) if t0 == 0 else R.cpu().numpy()

    g, stop, zero = scan_origin_lag_sums(fetch, len(series), 500, [0], fast=True)
    assert zero[0].tolist() == ref["zero_t"] and stop[0, :14].tolist() == ref["stop_t"][:14]


def test_mean_out_may_be_null(eng):
    """txm_lag_origin_sums with mean_out = NULL writes the same R and nothing else."""
    import ctypes as ct

    T, C = 3000, 1
    u, x = state_with_transient(T, C, seed=8)
    ud, xd = torch.as_tensor(u).cuda(), torch.as_tensor(x).cuda()
    cen = eng.lag_origin_center(xd, ud)
    want, _ = eng.lag_origin_sums(xd, ud, [1, 0], 100, 0, 256, center=cen)
    L = eng._L()
    sl = (ct.c_int32 * 2)(1, 0)
    out = torch.full_like(want, float("nan"))
    ws = eng.workspace(L.txm_lag_origin_sums_ws_bytes(T, C, 2, 100, 256), tag="lag")
    rc = L.txm_lag_origin_sums(eng._ptr(xd), C, eng._ptr(ud), T, C, eng._ptr(cen), sl, 2, 100, 0, 256, eng._ptr(out), None,
                               eng._ptr(ws), ws.numel(), eng._stream())
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(out, want)


def test_equilibrate(txm):
    from thermoextrap_amd.moments import DeviceDataArray
    from thermoextrap_amd.xrlite import DataArray

    u, x = detect_state(0.9, 5.0)
    w = np.random.default_rng(1).uniform(0.5, 2.0, T_DET)
    ud, xd, wd = torch.as_tensor(u).cuda(), torch.as_tensor(x).cuda(), torch.as_tensor(w).cuda()
    want = txm.detect_equilibrations(u, x, nskip=1000)
    t0 = want.t0_max
    assert t0 > 0
    inputs = {"numpy": (u, x, w), "tensor": (ud, xd, wd),
              "DataArray": (DataArray(u, ("rec",)), DataArray(x, ("rec", "val")), DataArray(w, ("rec",))),
              "DeviceDataArray": (DeviceDataArray(ud, ("rec",)), DeviceDataArray(xd, ("rec", "val")), DeviceDataArray(wd, ("rec",)))}
    for kind, (uu, xx, ww) in inputs.items():
        uo, xo, wo, info = txm.equilibrate(uu, xx, ww, nskip=1000)
        assert info["t0"] == t0 and info["n"] == T_DET - t0 and np.array_equal(info["equilibration"].g_t, want.g_t), kind
        if kind in ("numpy", "DataArray"):
            assert isinstance(uo, DataArray) and uo.dims == ("rec",) and xo.dims == ("rec", "val") and wo.dims == ("rec",)
            vals = (uo.values, xo.values, wo.values)
        else:
            assert isinstance(uo, DeviceDataArray) and uo.dims == ("rec",) and xo.dims == ("rec", "val") and wo.dims == ("rec",)
            vals = (uo.tensor.cpu().numpy(), xo.tensor.cpu().numpy(), wo.tensor.cpu().numpy())
        assert np.array_equal(vals[0], u[t0:]) and np.array_equal(vals[1], x[t0:]) and np.array_equal(vals[2], w[t0:]), kind
    # w is optional; an explicit t0 skips detection; the output feeds decorrelate and then from_vals unchanged
    uo, xo, wo, info = txm.equilibrate(u, x, t0=1234)
    assert wo is None and info["equilibration"] is None and info["t0"] == 1234 and np.array_equal(xo.values, x[1234:])
    with pytest.raises(TypeError):
        txm.equilibrate(u, x, t0=5, nskip=100)
    with pytest.raises(ValueError):
        txm.equilibrate(u, x, t0=T_DET)
    for args in (txm.equilibrate(u, x, w, nskip=1000)[:3], txm.equilibrate(ud, xd, wd, nskip=1000)[:3]):
        ue, xe, we, dinfo = txm.decorrelate(*args)
        assert 10 < dinfo["n"] < (T_DET - t0) // 2
        assert we.dims == ("rec",)
        m = txm.DataCentralMomentsVals.from_vals(xv=xe, uv=ue, order=2, central=True)
        assert np.isfinite(np.asarray(m.dxduave.values)).all()


def _ar1_device(N, phi, gen):
    """An AR(1) series on the device by recursive doubling: y <- y + phi^s shift(y, s), s = 1, 2, 4, ... until phi^s < 1e-9."""
    y = torch.empty(N, dtype=torch.float64, device="cuda").normal_(0.0, 1.0, generator=gen)
    s = 1
    while phi**s >= 1e-9:
        z = y.clone()
        z[s:].add_(y[:-s], alpha=phi**s)
        y = z
        s *= 2
    return y


def test_fullsize_origin_sums_and_detection(txm, eng):
    """T = 1e7, C = 1, 512 origins, generated on the device: AR(0.9) plus a transient on the energy, AR(0.7) plus a slower one
    on the column.  A dozen (origin, lag) entries against the long-double sums; the detected origins lie where the transients
    end; and on the strided sub-problem A[::500] (T = 20000, 500 origins) the detected t0 is the restatement's."""
    T = 10_000_000
    gen = torch.Generator(device="cuda").manual_seed(20261018)
    n = torch.arange(T, dtype=torch.float64, device="cuda")
    u = _ar1_device(T, 0.9, gen) + 5.0 * (1 - 0.81) ** -0.5 * torch.exp(-n / 2.0e5) + 174.85
    x = (_ar1_device(T, 0.7, gen) + 5.0 * (1 - 0.49) ** -0.5 * torch.exp(-n / 4.0e5) + 3.0)[:, None].contiguous()
    del n
    nskip = txm.timeseries.pick_nskip(T)
    assert nskip == 19532
    e = txm.detect_equilibrations(u, x)
    assert e.g_t.shape == (2, 512) and np.isfinite(e.g_t).all() and (e.g_t >= 1.0).all()
    print(f"full size: t0 {e.t0.tolist()}, g {e.g.tolist()}, Neff {e.neff.tolist()}")
    assert 0 < e.t0[0] <= 10 * 2.0e5 and 0 < e.t0[1] <= 10 * 4.0e5 and e.t0_max == e.t0.max()
    # AR(1), C(t) = phi^t, once the transient is gone (origin 256: 25 and 12 tau in): the fast loop's quadrature of it over the
    # lags 1, 2, 4, 7, 11, ... with weights 1, 2, 3, ... (21.9 and 6.70, where the plain loop gives 19 and 5.67); the picked
    # origin keeps a rest of the transient -- that is the trade Neff makes -- so its g is not held to that value
    def g_fast(phi):
        g, t, inc = 1.0, 1, 1
        while phi**t > 1e-12:
            g, t, inc = g + 2.0 * phi**t * inc, t + inc, inc + 1
        return g

    assert abs(e.g_t[0, 256] - g_fast(0.9)) < 0.6 and abs(e.g_t[1, 256] - g_fast(0.7)) < 0.2
    cen = eng.lag_origin_center(x, u)
    got = eng.lag_origin_sums(x, u, [1, 0], nskip, 0, 256, center=cen)[0].cpu().numpy()
    p = cen.cpu().numpy()
    hosts = {0: u.cpu().numpy(), 1: x[:, 0].contiguous().cpu().numpy()}
    worst_here = 0.0
    for row, s, j, lags in ((0, 1, 0, (0, 1, 255)), (0, 1, 17, (2, 100)), (0, 1, 511, (0, 16)), (1, 0, 0, (0, 17)), (1, 0, 3, (1, 64)),
                            (1, 0, 510, (15, 254))):
        A = np.asarray(hosts[s][j * nskip:], dtype=LD)
        dc = ref_centered(A)[0]
        ad = np.abs(A - LD(p[s]))
        delta = abs(A.mean(dtype=LD) - LD(p[s]))
        M = len(A)
        for t in lags:
            ref = float(ref_lag_sum(dc, dc, t))
            bound = 1e-12 * 2 * float(np.dot(ad[:M - t] + delta, ad[t:] + delta))
            err = abs(got[row, j, t] - ref)
            worst_here = max(worst_here, err / bound * 1e-12)
            assert err <= bound, (s, j, t, got[row, j, t], ref, err, bound)
    print(f"full size origin lag sums: worst scaled error {worst_here:.3e} (limit 1e-12)")
    sub = hosts[0][::500].copy()
    ref = ref_detect(sub, fast=True, nskip=40)
    t, g, neff = txm.detect_equilibration(sub, nskip=40)
    assert margins_hold(ref)
    assert len(ref["origins"]) == 500 and t == ref["t"] and abs(g - float(ref["g"])) <= g_bound(ref["vis_t"][ref["index"]])
