"""timeseries.py on the device against the long-double restatement of tests/test_timeseries_cpu.py.

Lag sums: |hip - ref| <= 1e-12 (1 + |mu_a| / sigma_a + |mu_b| / sigma_b) sum_n |dA_n| |dB_{n+t}| -- without the middle
factor the project's usual first-order bound; the middle factor covers the rounding of a - mu for offset series.
g: the stop decision is discrete, so every case first asserts a margin on the reference alone (min |C_ref(t)| >= 1e-9 over
the lags visited after mintime, the stopping lag included), then stop lag == reference and
|g - g_ref| <= 1e-11 (1 + sum 2 |C_ref(t)| inc)."""

import numpy as np
import pytest
import torch

from test_timeseries_cpu import LD, g_bound, literal_subsample, ref_centered, ref_lag_sum, ref_scan

pytestmark = pytest.mark.gpu

STAGE = 1008          # engine.LAG_STAGE: samples per chunk for n <= 1008 * 512


@pytest.fixture(scope="module")
def eng(txm):
    from thermoextrap_amd import engine

    assert engine.LAG_STAGE == STAGE
    return engine


def ar1(phi, seed, N):
    from scipy.signal import lfilter

    return lfilter([1], [1, -phi], np.random.default_rng(seed).standard_normal(N))


def correlated_state(N, C, seed):
    """u and x (N, C) with means, scales and correlation times that differ per column."""
    from scipy.signal import lfilter

    rng = np.random.default_rng(seed)
    u = 174.85 + 5.31 * lfilter([1], [1, -0.9], rng.standard_normal(N)) * np.sqrt(1 - 0.81)
    x = np.empty((N, C))
    for c in range(C):
        ph = 0.3 + 0.65 * c / max(C - 1, 1)
        x[:, c] = (0.2 + c) + 1e-3 * (1 + c % 3) * u + 0.05 * lfilter([1], [1, -ph], rng.standard_normal(N))
    return u, x


def series_of(pair, u, x):
    C = x.shape[1]
    if pair == 0:
        return u, None
    if pair <= C:
        return x[:, pair - 1], None
    return x[:, pair - 1 - C], u


worst = {"scaled": 0.0}


def check_lag_sums(eng, u, x, pairs, t0, nlags, lags=None, xd=None):
    """engine.lag_sums on (t0, nlags) against the restatement on `lags` (default: all of the block)."""
    N, C = x.shape
    ud = torch.as_tensor(u).cuda()
    if xd is None:
        xd = torch.as_tensor(x).cuda() if C else None
    got = eng.lag_sums(xd, ud, pairs, t0, nlags).cpu().numpy()
    assert got.shape == (len(pairs), nlags)
    lags = range(t0, t0 + nlags) if lags is None else lags
    for row, p in enumerate(pairs):
        A, B = series_of(p, u, x)
        dA, dB = ref_centered(A, B)
        sa, sb = float(dA.std()), float(dB.std())
        mid = 1.0 + (abs(float(np.mean(A))) / sa if sa > 0 else 0.0) + (abs(float(np.mean(A if B is None else B))) / sb if sb > 0 else 0.0)
        aA, aB = np.abs(dA), np.abs(dB)
        for t in lags:
            ref = float(ref_lag_sum(dA, dB, t))
            bound = 1e-12 * mid * (float(np.dot(aA[: N - t], aB[t:])) if t < N else 0.0)
            err = abs(got[row, t - t0] - ref)
            if bound > 0:
                worst["scaled"] = max(worst["scaled"], err / bound * 1e-12)
            assert err <= bound, (N, C, p, t, got[row, t - t0], ref, err, bound)
    return got


@pytest.mark.parametrize("N", [1, 2, 3, 255, 256, 257, STAGE - 1, STAGE, STAGE + 1, 2 * STAGE - 1, 2 * STAGE, 2 * STAGE + 1])
@pytest.mark.parametrize("C", [0, 1, 5])
def test_lag_sums_small_n_and_chunk_edges(eng, N, C):
    """Every pair kind, N around the tile, the block and the chunk edges; lags beyond N give exactly 0."""
    u, x = correlated_state(N, C, 100 + N + C)
    got = check_lag_sums(eng, u, x, list(range(2 * C + 1)), 0, 256)
    if N < 256:
        assert (got[:, N:] == 0.0).all()
    if N > 256:
        check_lag_sums(eng, u, x, list(range(2 * C + 1))[::-1], 256, 512 if N > 1024 else 256)   # t0 > 0, another pair order


def test_lag_sums_wide_state_all_blocks(eng):
    """C = 32 (65 pairs) at N = 4099: the first block, a 1024-lag block (four tiles per wave), and a block that runs
    past N."""
    N, C = 4099, 32
    u, x = correlated_state(N, C, 7)
    pairs = list(range(2 * C + 1))
    check_lag_sums(eng, u, x, pairs, 0, 256)
    check_lag_sums(eng, u, x, pairs, 1024, 1024, lags=range(1024, 2048, 5))
    got = check_lag_sums(eng, u, x, [0, 3, 40, 64], 3840, 512)
    assert (got[:, N - 3840:] == 0.0).all() and (got[:, : N - 3840] != 0.0).any()


def test_lag_sums_row_pitch_and_offset_series(eng):
    """x as a column slice of a wider matrix (pitch > C), and one series with mean 1e6 sigma."""
    N, C = 200_000, 5
    u, x = correlated_state(N, C, 9)
    x[:, 2] += 1e6 * x[:, 2].std()
    big = torch.zeros((N, C + 3), dtype=torch.float64, device="cuda")
    big[:, :C] = torch.as_tensor(x).cuda()
    xd = big[:, :C]
    assert xd.stride(0) == C + 3
    pairs = list(range(2 * C + 1))
    lags = [0, 1, 2, 3, 15, 16, 17, 100, 254, 255]
    g0 = check_lag_sums(eng, u, x, pairs, 0, 256, lags=lags, xd=xd)
    g1 = check_lag_sums(eng, u, x, pairs, 0, 256, lags=[0, 255])                     # tight layout: same bits
    assert np.array_equal(g0, g1)
    check_lag_sums(eng, u, x, [0, 3, 8], 4096, 4096, lags=[4096, 4097, 5000, 8191])
    check_lag_sums(eng, u, x, [0, 3, 8], 198_656, 2048, lags=[198_656, 199_990, 199_999, 200_000, 200_001, 200_703])
    check_lag_sums(eng, u, x[:, :1], [0, 1, 2], 512, 512, lags=[512, 777, 1023])
    check_lag_sums(eng, u, x[:, :0], [0], 256, 256, lags=[256, 300, 511])
    print(f"lag sums: worst |hip - ref| / (middle factor x sum |dA||dB|) so far: {worst['scaled']:.3e} (limit 1e-12)")


def test_lag_sums_bits_do_not_depend_on_the_block_schedule(eng):
    N, C = 200_000, 5
    u, x = correlated_state(N, C, 13)
    ud, xd = torch.as_tensor(u).cuda(), torch.as_tensor(x).cuda()
    pairs = list(range(2 * C + 1))
    cen = eng.lag_center(xd, ud)
    one = eng.lag_sums(xd, ud, pairs, 1024, 1024, center=cen)
    four = torch.cat([eng.lag_sums(xd, ud, pairs, 1024 + 256 * k, 256, center=cen) for k in range(4)], dim=1)
    two = torch.cat([eng.lag_sums(xd, ud, pairs, 1024 + 512 * k, 512, center=cen) for k in range(2)], dim=1)
    assert torch.equal(one, four) and torch.equal(one, two)
    again = eng.lag_sums(xd, ud, pairs, 1024, 1024)
    assert torch.equal(one, again)
    # a shorter pair list changes nothing for the pairs it keeps; a big block holds the same bits as its pieces
    sub = eng.lag_sums(xd, ud, [8, 0], 1024, 1024)
    assert torch.equal(sub, one[[8, 0]])
    big = eng.lag_sums(xd, ud, [0, 7], 0, 4096)
    assert torch.equal(big[:, 1024:2048], one[[0, 7]])


@pytest.mark.parametrize("N", [4099, 200_000])
@pytest.mark.parametrize("phi", [0, 0.5, 0.9, 0.99])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_statistical_inefficiency_ar1(txm, seed, phi, N):
    """The AR(1) grid: g and the stop lag of u, x and (x, u), plain and fast, against the restatement.  On these inputs the
    restatement's smallest margin min |C_ref(t)| is 2.2e-6 on the plain path and 2.7e-5 with fast (CPU, long double); its stop
    lags are 4-30 (phi = 0), 7-30 (0.5), 23-105 (0.9) and 238-1018 (0.99) on the plain path."""
    u = ar1(phi, seed, N)
    x = 0.6 * u + 0.8 * ar1(0.7, seed, N) + 3
    refs = {"u": (u, None, {}), "x": (x, None, {}), "xu": (x, u, {})}
    for fast in (False, True):
        res = txm.statistical_inefficiencies(u, x[:, None], fast=fast)
        got = {"u": (res.g_u, res.stop_u), "x": (res.g_x[0], res.stop_x[0]), "xu": (res.g_cross[0], res.stop_cross[0])}
        for name, (A, B, cache) in refs.items():
            gr, sr, vis = ref_scan(A, B, fast=fast, cache=cache)
            cs = [abs(float(c)) for t, c, _ in vis if t > 3]
            if cache["c_stop"] is not None:
                cs.append(abs(float(cache["c_stop"])))
            assert min(cs) >= 1e-9, (name, fast, min(cs))             # the reference's own margin: the stop is not a coin toss
            g, stop = got[name]
            assert stop == sr, (name, fast, stop, sr)
            assert abs(g - float(gr)) <= g_bound(vis), (name, fast, g, float(gr), g_bound(vis))
        assert res.g_max == max(res.g_u, res.g_x[0], res.g_cross[0])
    # the single-pair entry points: the cross pair is the same call; a lone series is centred with the 1-D reduction's mean
    # (the last bit of it may differ from the state's), so its g agrees to rounding
    r2 = txm.statistical_inefficiencies(u, x[:, None])
    assert txm.statistical_inefficiency(x, u) == r2.g_cross[0]
    assert abs(txm.statistical_inefficiency(u) - r2.g_u) <= 1e-11 * r2.g_u and abs(txm.statistical_inefficiency(x) - r2.g_x[0]) <= 1e-11 * r2.g_x[0]


def test_correlation_function_max_lag_and_input_kinds(txm):
    from thermoextrap_amd.moments import DeviceDataArray
    from thermoextrap_amd.xrlite import DataArray

    N = 20_000
    u = ar1(0.95, 4, N) + 10.0
    x = 0.5 * u + ar1(0.5, 5, N)
    dA, dB = ref_centered(x, u)
    s2 = np.mean(dA * dB, dtype=LD)
    c = txm.normalized_fluctuation_correlation_function(x, u, N_max=300)
    cn = txm.normalized_fluctuation_correlation_function(x, u, N_max=300, norm=False)
    assert c.shape == (301,) and abs(c[0] - 1.0) < 1e-14
    for t in (0, 1, 17, 255, 256, 300):
        ref = ref_lag_sum(dA, dB, t) / (2 * LD(N - t))
        assert abs(cn[t] - float(ref)) <= 1e-11 * float(abs(s2)) and abs(c[t] - float(ref / s2)) <= 1e-11
    with pytest.raises(ValueError):
        txm.normalized_fluctuation_correlation_function(x, N_max=N)
    # numpy, device tensors, DataArray and DeviceDataArray give the same g; anything else raises
    g = txm.statistical_inefficiencies(u, x[:, None])
    ud, xd = torch.as_tensor(u).cuda(), torch.as_tensor(x[:, None]).cuda()
    for uu, xx in ((ud, xd), (DataArray(u, ("rec",)), DataArray(x[:, None], ("rec", "val"))),
                   (DeviceDataArray(ud, ("rec",)), DeviceDataArray(xd, ("rec", "val")))):
        h = txm.statistical_inefficiencies(uu, xx)
        assert h.g_max == g.g_max and h.stop_u == g.stop_u
    with pytest.raises(TypeError):
        txm.statistical_inefficiencies(list(u), x[:, None])
    with pytest.raises(ValueError):
        txm.statistical_inefficiencies(u, x)                            # xv must be (rec, val)
    with pytest.raises(ValueError, match="u"):
        txm.statistical_inefficiencies(u, x[:, None], max_lag=10)
    assert txm.statistical_inefficiencies(u, x[:, None], max_lag=int(max(g.stop_u, g.stop_x[0], g.stop_cross[0]))).g_max == g.g_max
    with pytest.raises(ValueError):
        txm.statistical_inefficiency(np.full(100, 3.0))                 # sigma^2 == 0


@pytest.mark.parametrize("kind", ["host", "device"])
@pytest.mark.parametrize("conservative", [False, True])
def test_decorrelate(txm, kind, conservative):
    from thermoextrap_amd.moments import DeviceDataArray
    from thermoextrap_amd.xrlite import DataArray

    N, C, order = 200_000, 5, 3
    u, x = correlated_state(N, C, 21)
    w = np.random.default_rng(1).uniform(0.5, 2.0, N)
    if kind == "host":
        uo, xo, wo, info = txm.decorrelate(u, x, w, conservative=conservative)
        assert isinstance(uo, DataArray) and uo.dims == ("rec",) and xo.dims == ("rec", "val") and wo.dims == ("rec",)
        vals = (uo.values, xo.values, wo.values)
    else:
        uo, xo, wo, info = txm.decorrelate(torch.as_tensor(u).cuda(), DeviceDataArray(torch.as_tensor(x).cuda(), ("rec", "val")),
                                           torch.as_tensor(w).cuda(), conservative=conservative)
        assert isinstance(uo, DeviceDataArray) and uo.dims == ("rec",) and xo.dims == ("rec", "val")
        vals = (uo.tensor.cpu().numpy(), xo.tensor.cpu().numpy(), wo.tensor.cpu().numpy())
    # g: the largest of the 2 C + 1 inefficiencies, each held to the restatement
    ineff = info["inefficiencies"]
    gs = []
    for p in range(2 * C + 1):
        gr, sr, vis = ref_scan(*series_of(p, u, x))
        g = ineff.g_u if p == 0 else (ineff.g_x[p - 1] if p <= C else ineff.g_cross[p - 1 - C])
        assert abs(g - float(gr)) <= g_bound(vis)
        gs.append(g)
    assert info["g"] == max(gs) == ineff.g_max
    # indices: the literal loop with that g; the gather: host indexing, bit for bit
    idx = np.array(literal_subsample(N, info["g"], conservative))
    assert np.array_equal(info["indices"], idx) and info["n"] == len(idx) and 100 < len(idx) < N // 5
    assert np.array_equal(vals[0], u[idx]) and np.array_equal(vals[1], x[idx]) and np.array_equal(vals[2], w[idx])
    # the outputs feed from_vals unchanged, and give what from_vals gives on the host-indexed arrays
    a = txm.DataCentralMomentsVals.from_vals(xv=xo, uv=uo, order=order, central=True)
    b = txm.DataCentralMomentsVals.from_vals(xv=DataArray(x[idx], ("rec", "val")), uv=DataArray(u[idx], ("rec",)), order=order, central=True)
    assert np.array_equal(np.asarray(a.dxduave.values), np.asarray(b.dxduave.values))
    # a given g skips the estimate
    _, x2, _, info2 = txm.decorrelate(u, x, g=7.5)
    assert info2["inefficiencies"] is None and np.array_equal(info2["indices"], literal_subsample(N, 7.5)) and x2.shape == (len(info2["indices"]), C)


def _ar1_device(N, C, phi, gen):
    """AR(1) columns on the device by recursive doubling: y <- y + phi^s shift(y, s), s = 1, 2, 4, ... until phi^s < 1e-9."""
    y = torch.empty((N, C), dtype=torch.float64, device="cuda").normal_(0.0, 1.0, generator=gen)
    s = 1
    while phi**s >= 1e-9:
        z = y.clone()
        z[s:].add_(y[:-s], alpha=phi**s)
        y = z
        s *= 2
    return y


def test_fullsize_lag_sums_and_inefficiencies(txm, eng):
    """N = 1e8, C = 32, generated on the device: u = AR(0.9), x_c = 0.6 u + 0.8 AR(0.7) + 3.  A dozen lags of four pairs
    against the long-double sums; g of all 65 pairs finite, >= 1, near the AR(1) values, stop lags where the correlation
    function meets its noise."""
    N, C = 100_000_000, 32
    gen = torch.Generator(device="cuda").manual_seed(20261017)
    u = _ar1_device(N, 1, 0.9, gen)[:, 0].contiguous()
    x = _ar1_device(N, C, 0.7, gen)
    x.mul_(0.8).add_(u[:, None], alpha=0.6).add_(3.0)
    res = txm.statistical_inefficiencies(u, x)
    g_all = np.concatenate([[res.g_u], res.g_x, res.g_cross])
    stops = np.concatenate([[res.stop_u], res.stop_x, res.stop_cross])
    print(f"full size: g_u {res.g_u:.4f}, g_x {res.g_x.min():.4f} .. {res.g_x.max():.4f}, g_cross {res.g_cross.min():.4f} .. "
          f"{res.g_cross.max():.4f}, stop lags {stops.min()} .. {stops.max()}")
    assert np.isfinite(g_all).all() and (g_all >= 1.0).all()
    # AR(1): g = (1 + phi) / (1 - phi) = 19 for u and for (x, u); x mixes 0.9 and 0.7: 13.69
    assert abs(res.g_u - 19.0) < 0.4 and np.all(np.abs(res.g_cross - 19.0) < 0.4) and np.all(np.abs(res.g_x - 13.69) < 0.3)
    assert stops.min() >= 30 and stops.max() <= 511                      # 0.9^t meets the 1e-4 sqrt(g) noise near t = 60 .. 110
    pairs = [0, 1, C, 1 + C + 7]
    lags = [0, 1, 2, 3, 15, 16, 17, 63, 64, 128, 254, 255]
    got = eng.lag_sums(x, u, pairs, 0, 256).cpu().numpy()
    uh = u.cpu().numpy()
    cols = {c: x[:, c].contiguous().cpu().numpy() for c in (0, C - 1, 7)}
    del x, u
    worst_here = 0.0
    for row, (A, B) in enumerate(((uh, None), (cols[0], None), (cols[C - 1], None), (cols[7], uh))):
        dA, dB = ref_centered(A, B)
        mid = 1.0 + abs(float(np.mean(A))) / float(dA.std()) + abs(float(np.mean(A if B is None else B))) / float(dB.std())
        aA, aB = np.abs(dA), np.abs(dB)
        for t in lags:
            ref = float(ref_lag_sum(dA, dB, t))
            bound = 1e-12 * mid * float(np.dot(aA[: N - t], aB[t:]))
            err = abs(got[row, t] - ref)
            worst_here = max(worst_here, err / bound * 1e-12)
            assert err <= bound, (pairs[row], t, got[row, t], ref, err, bound)
    print(f"full size lag sums: worst scaled error {worst_here:.3e} (limit 1e-12)")
