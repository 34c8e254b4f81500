"""GPU tests of MBARModel.histogram on three overlapping Gaussian states (3000, 2500 and 3500 samples).

The other route to the same numbers is an MBARModel whose observable IS the materialised indicator matrix, through
predict_with_covariance: the solve is the same, the kernels (txm_mbar_predict, txm_mbar_cov, txm_mbar_cross_cov against
txm_mbar_hist) and the host algebra (sums of d d' against the closed form of the class sums) are different.  p is held to
1e-12 and cov to 1e-10 sqrt(Theta_ii Theta_jj), the margin the README gives the same kind of two-route comparison
(q^T cov q against predict_with_error()^2); every case prints the worst seen (run with -s).  One statistical test: std
against the spread of 400 bootstrap replicates of the indicator model, 1 +- 6 / sqrt(2 * 399) for every bin with p > 0.02
(the rule of tests/test_mbar_cov_gpu.py).
"""

import warnings

import numpy as np
import pytest
import torch

from test_mbar_cov_cpu import gauss_problem

pytestmark = pytest.mark.gpu
A0, NS, TARGETS = [1.0, 1.15, 1.3], [3000, 2500, 3500], [1.05, 1.25, 1.4]


def numpy_bins(v, edges):
    """numpy.histogram's assignment: left-closed bins, the last closed on the right; -1 outside."""
    idx = np.searchsorted(edges, v, side="right") - 1
    idx[v == edges[-1]] = len(edges) - 2
    idx[(idx < 0) | (idx >= len(edges) - 1)] = -1
    return idx


def make_model(us, xs):
    import thermoextrap_amd as xtrap

    return xtrap.MBARModel([xtrap.beta.factory_extrapmodel(beta=b, data=xtrap.factory_data_values(uv=u, xv=x, order=1, central=False))
                            for b, x, u in zip(A0, xs, us)])


@pytest.fixture(scope="module")
def world(txm):
    us, xs = gauss_problem(A0, NS, C=1, seed=23)
    xs = [np.stack([x[:, 0], u], axis=1) for x, u in zip(xs, us)]              # column 0 an observable, column 1 the energy
    return {"us": us, "xs": xs, "model": make_model(us, xs)}


def indicator_model(world, vals, edges):
    nb = len(edges) - 1
    ind = []
    for v in vals:
        idx = numpy_bins(v, edges)
        m = np.zeros((len(v), nb))
        m[np.flatnonzero(idx >= 0), idx[idx >= 0]] = 1.0
        ind.append(m)
    return make_model(world["us"], ind), ind


def pooled_edges(vals, nb):
    lo, hi = min(v.min() for v in vals), max(v.max() for v in vals)
    return np.histogram_bin_edges(np.empty(0), bins=nb, range=(lo, hi))


def ragged_edges(vals, nb):
    """nb bins of uneven width that leave a few per cent of the samples outside on either side."""
    q = np.quantile(np.concatenate(vals), [0.02, 0.97])
    w = np.random.default_rng(nb).uniform(0.3, 1.7, nb)
    return q[0] + (q[1] - q[0]) * np.concatenate([[0.0], np.cumsum(w) / w.sum()])


@pytest.mark.parametrize("kind", ["uniform20_column", "ragged40_energy"])
def test_histogram_against_predict_with_covariance_of_the_indicator_matrix(world, kind):
    m = world["model"]
    if kind == "uniform20_column":
        vals = [x[:, 0] for x in world["xs"]]
        edges = pooled_edges(vals, 20)
        h = m.histogram(TARGETS, 20, values=0)
        np.testing.assert_array_equal(h.edges, edges)
        assert np.all(h.outside.values == 0.0)
    else:
        vals = world["us"]
        edges = ragged_edges(vals, 40)
        h = m.histogram(TARGETS, edges, values="u")
        assert np.all(h.outside.values > 0.01)
    ref, _ = indicator_model(world, vals, edges)
    mean, cov = ref.predict_with_covariance(TARGETS)
    _, err = ref.predict_with_error(TARGETS)
    assert h.p.values.shape == mean.values.shape and h.cov.values.shape == cov.values.shape
    dp = float(np.max(np.abs(h.p.values - mean.values)))
    sd = np.sqrt(np.einsum("abb->ab", cov.values))
    scale = sd[:, :, None] * sd[:, None, :]
    live = scale > 0                    # an empty bin has a zero row and column on both routes
    assert live.sum() >= 0.8 * live.size and np.array_equal(h.cov.values[~live], cov.values[~live])
    assert np.array_equal(h.std.values[err.values == 0], err.values[err.values == 0])
    dc = float(np.max(np.abs(h.cov.values - cov.values)[live] / scale[live]))
    ds = float(np.max(np.abs(h.std.values - err.values)[err.values > 0] / err.values[err.values > 0]))
    dsum = float(np.max(np.abs(h.p.values.sum(axis=1) + h.outside.values - 1.0)))
    print(f"\n{kind}: worst |p - mean| {dp:.2e}, |cov - cov'| / sqrt(Theta_ii Theta_jj) {dc:.2e}, |std / err - 1| {ds:.2e}, "
          f"|sum p + outside - 1| {dsum:.2e}")
    assert dp <= 1e-12 and dc <= 1e-10 and ds <= 1e-10 and dsum <= 1e-13
    for a in range(len(TARGETS)):
        assert np.array_equal(h.cov.values[a], h.cov.values[a].T)
    np.testing.assert_allclose(h.n_eff.values, m.effective_samples(TARGETS).values, rtol=1e-12)


def test_std_matches_the_bootstrap_spread(world):
    m = world["model"]
    vals = [x[:, 0] for x in world["xs"]]
    edges = pooled_edges(vals, 20)
    h = m.histogram(TARGETS[:2], 20, values=0, cov=False)
    ref, _ = indicator_model(world, vals, edges)
    rep = ref.bootstrap({"nrep": 400, "seed": 20240917}).predict(TARGETS[:2]).values          # (2, 400, 20)
    big = h.p.values > 0.02
    ratio = h.std.values[big] / rep.std(axis=1, ddof=1)[big]
    print(f"\nstd / bootstrap std over {int(big.sum())} bins with p > 0.02: {ratio.min():.3f} ... {ratio.max():.3f}")
    assert big.sum() >= 10 and np.all(np.abs(ratio - 1.0) <= 6.0 / np.sqrt(2.0 * 399.0)), ratio


def same(h1, h2):
    return (np.array_equal(h1.p.values, h2.p.values) and np.array_equal(h1.std.values, h2.std.values)
            and np.array_equal(h1.outside.values, h2.outside.values) and np.array_equal(h1.n_eff.values, h2.n_eff.values)
            and (h1.cov is None or h2.cov is None or np.array_equal(h1.cov.values, h2.cov.values)))


def test_the_forms_of_values_agree_bit_for_bit(world):
    from thermoextrap_amd import engine

    m, us = world["model"], world["us"]
    edges = ragged_edges(us, 12)
    by_name = m.histogram(TARGETS, edges, values="u")
    for other in (1, (1,), list(us), [torch.as_tensor(u).cuda() for u in us]):
        assert same(by_name, m.histogram(TARGETS, edges, values=other))
    # an int with the pooled range, and the same range given
    auto = m.histogram(TARGETS, 12, values="u")
    lo, hi = min(u.min() for u in us), max(u.max() for u in us)
    assert same(auto, m.histogram(TARGETS, 12, values="u", range=(lo, hi))) and np.all(auto.outside.values == 0.0)
    # integer values with bins=int are the bin indices themselves (-1 and 12: outside)
    idx = [engine.bin_index(torch.as_tensor(u), edges).numpy().astype(np.int64) for u in us]
    idx[0] = np.where(idx[0] < 0, 12, idx[0])
    assert same(by_name, m.histogram(TARGETS, 12, values=idx))
    # without the covariance: the same p and std bits
    lean = m.histogram(TARGETS, edges, values="u", cov=False)
    assert lean.cov is None and same(by_name, lean)
    with pytest.raises(ValueError):
        lean.free_energy(reference=0)
    with pytest.raises(ValueError):
        m.histogram(TARGETS, 1024, values="u")
    with pytest.raises(ValueError):
        m.histogram(TARGETS, edges[::-1], values="u")
    with pytest.raises(IndexError):
        m.histogram(TARGETS, 4, values=2)


def test_more_than_eight_targets_are_two_calls_stitched(world):
    m = world["model"]
    al = list(np.linspace(0.95, 1.45, 11))
    edges = ragged_edges(world["us"], 17)
    whole, a, b = (m.histogram(t, edges, values="u") for t in (al, al[:8], al[8:]))
    for name in ("p", "std", "cov", "outside", "n_eff"):
        got = getattr(whole, name).values
        assert np.array_equal(got, np.concatenate([getattr(a, name).values, getattr(b, name).values])), name
    np.testing.assert_array_equal(whole.p.coords["beta"], al)


def test_free_energy_profiles(world):
    m = world["model"]
    h = m.histogram(TARGETS, ragged_edges([x[:, 0] for x in world["xs"]], 15), values=0)
    p, std, cov = h.p.values, h.std.values, h.cov.values
    assert np.all(p > 0)
    F, dF = h.free_energy()
    assert F.dims == dF.dims == ("beta", "bin")
    assert np.array_equal(F.values, -np.log(p)) and np.array_equal(dF.values, std / p)
    r = 6
    Fr, dFr = h.free_energy(reference=r)
    assert np.all(dFr.values[:, r] == 0.0) and np.all(Fr.values[:, r] == 0.0)
    np.testing.assert_array_equal(Fr.values, F.values - F.values[:, [r]])
    v = np.einsum("abb->ab", cov)
    want = v / p**2 + v[:, [r]] / p[:, [r]]**2 - 2.0 * cov[:, :, r] / (p * p[:, [r]])
    others = np.arange(15) != r
    np.testing.assert_allclose(dFr.values[:, others]**2, want[:, others], rtol=1e-12)
    assert np.all(dFr.values[:, others] > 0)
    Fm, dFm = h.free_energy(reference="max")
    top = np.argmax(p, axis=1)
    for a, t in enumerate(top):
        one_F, one_dF = h.free_energy(reference=int(t))
        assert np.array_equal(Fm.values[a], one_F.values[a]) and np.array_equal(dFm.values[a], one_dF.values[a])
    assert np.all(Fm.values >= 0.0)
    d, dd = h.density()
    w = np.diff(h.edges)
    assert np.array_equal(d.values, p / w) and np.array_equal(dd.values, std / w) and d.dims == ("beta", "bin")


def test_empty_bins_dims_and_coordinates(world):
    m, us = world["model"], world["us"]
    lo, hi = min(u.min() for u in us), max(u.max() for u in us)
    edges = np.concatenate([[lo - 30.0, lo - 20.0, lo - 10.0], np.linspace(lo - 1.0, hi + 1.0, 7), [hi + 10.0]])   # 3 + 6 + 1 bins
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        h = m.histogram(1.2, edges, values="u", alpha_name="b")
        F, dF = h.free_energy()
        Fr, dFr = h.free_energy(reference="max")
        h.density()
    assert h.p.dims == h.std.dims == ("b", "bin") and h.cov.dims == ("b", "bin", "bin_2")
    assert h.outside.dims == h.n_eff.dims == ("b",) and h.p.values.shape == (1, 10) and h.cov.values.shape == (1, 10, 10)
    np.testing.assert_array_equal(h.p.coords["b"], [1.2])
    np.testing.assert_array_equal(h.p.coords["bin"], 0.5 * (edges[:-1] + edges[1:]))
    np.testing.assert_array_equal(h.cov.coords["bin_2"], h.cov.coords["bin"])
    np.testing.assert_array_equal(h.edges, edges)
    empty = np.array([0, 1, 2, 9])
    p = h.p.values[0]
    assert np.all(p[empty] == 0.0) and np.all(h.std.values[0, empty] == 0.0) and np.all(np.delete(p, empty) > 0)
    assert not h.cov.values[0][empty].any() and not h.cov.values[0][:, empty].any()
    assert np.all(np.isposinf(F.values[0, empty])) and np.all(np.isnan(dF.values[0, empty]))
    assert np.all(np.isposinf(Fr.values[0, empty])) and np.all(np.isnan(dFr.values[0, empty]))
    assert np.all(np.isfinite(np.delete(F.values[0], empty))) and np.all(np.isfinite(np.delete(dFr.values[0], empty)))
    assert h.outside.values[0] == 0.0 and abs(p.sum() - 1.0) <= 12 * 2.0 ** -52
    assert 1.0 < h.n_eff.values[0] <= sum(NS)
