"""ExtrapModel.derivs_cov / predict_with_error and gpr_input's method="delta" (DESIGN 4.11): the delta-method covariance of the
derivatives from one pass over the samples, against the same sums in long double (tests/_influence_ref.py, the psi of
test_influence_cpu.py), against its own definition t' V t, and once, statistically, against the device bootstrap."""

from __future__ import annotations

import math

import numpy as np
import pytest

from tests._influence_ref import bound_ld, cov_ld, ld_moments, make_data, psi_ld, series_for

pytestmark = pytest.mark.gpu

ORDER, BETA0 = 4, 0.5
CASES = [(c, m) for c in (True, False) for m in (False, True)]


def _model(txm, x, u, w, order, central, minus_log=False):
    DA = txm.DataArray
    xv = DA(x if x.ndim == 2 else x[:, None], ("rec", "val"))
    data = txm.DataCentralMomentsVals.from_vals(xv=xv, uv=DA(u, ("rec",)), order=order, central=central,
                                                weight=None if w is None else DA(w, ("rec",)))
    m = txm.beta.factory_extrapmodel(beta=BETA0, data=data)
    return m.new_like(minus_log=True) if minus_log else m


@pytest.fixture(scope="module")
def data200():
    return make_data(200, seed=0)


@pytest.mark.parametrize("central,minus_log", CASES)
def test_derivs_cov_matches_long_double(txm, data200, central, minus_log):
    """N = 200, weighted, order 4: V within 1e-12 sum p^2 B_i B_j of the long-double sum over the CPU test's psi."""
    from thermoextrap_amd import symbolic as S

    x, u, w = data200
    V = _model(txm, x, u, w, ORDER, central, minus_log).derivs_cov()
    assert V.dims == ("order", "order_2", "val") and V.shape == (ORDER + 1, ORDER + 1, 1)
    p, dx, du, mom = ld_moments(x, u, w, ORDER)
    a, b = S.influence_coefs(series_for(central), ORDER, mom, minus_log=minus_log)
    ref = cov_ld(psi_ld(a, b, dx, du), p)
    B = bound_ld(a, b, dx, du)
    ratio = float((np.abs(V.values[:, :, 0] - ref) / cov_ld(B, p)).max())
    print(f"central={central} minus_log={minus_log}: worst |V - ref| / sum p^2 B_i B_j = {ratio:.2e}")
    assert ratio <= 1e-12
    # norm=True carries 1 / (i! j!)
    f = np.array([1.0 / math.factorial(i) for i in range(ORDER + 1)])
    Vn = _model(txm, x, u, w, ORDER, central, minus_log).derivs_cov(norm=True)
    np.testing.assert_allclose(Vn.values[:, :, 0], V.values[:, :, 0] * f[:, None] * f[None, :], rtol=1e-15)


def test_lower_order_and_columns(txm):
    """order below the data's; three columns keep their order; the unweighted call."""
    from thermoextrap_amd import symbolic as S

    x, u, _ = make_data(300, seed=2, weighted=False, ncol=3)
    m = _model(txm, x, u, None, ORDER, True)
    V = m.derivs_cov(order=2)
    assert V.shape == (3, 3, 3)
    p, dx, du, mom = ld_moments(x, u, None, 2)
    a, b = S.influence_coefs(series_for(True), 2, mom)
    for c in range(3):
        ref = cov_ld(psi_ld(a[c], b[c], dx[:, c], du), p)
        bnd = cov_ld(bound_ld(a[c], b[c], dx[:, c], du), p)
        assert (np.abs(V.values[:, :, c] - ref) <= 1e-12 * bnd).all()


@pytest.mark.parametrize("minus_log", [False, True])
def test_predict_with_error(txm, data200, minus_log):
    x, u, w = data200
    m = _model(txm, x, u, w, ORDER, True, minus_log)
    alphas = np.array([0.3, 0.5, 0.62])
    pred, std = m.predict_with_error(alphas)
    ref = m.predict(alphas)
    assert pred.dims == ref.dims == std.dims and np.array_equal(pred.values, ref.values)
    V = np.asarray(m.derivs_cov().values[:, :, 0], np.longdouble)
    for i, al in enumerate(alphas):
        t = np.array([np.longdouble(al - BETA0) ** k / math.factorial(k) for k in range(ORDER + 1)])
        var = float(t @ V @ t)
        assert abs(float(std.values[i, 0]) ** 2 - var) <= 1e-12 * var
    pred1, std1 = m.predict_with_error(0.3, order=2)
    assert np.array_equal(pred1.values, m.predict(0.3, order=2).values) and std1.shape == pred1.shape


@pytest.mark.parametrize("minus_log", [False, True])
def test_gp_input_delta(txm, minus_log):
    from thermoextrap_amd import gpr_input as G

    x, u, w = make_data(400, seed=4, ncol=2)
    m = _model(txm, x, u, w, 3, True, minus_log)
    spec = {"nrep": 16, "seed": 3, "device": True}
    xb, yb, cb = G.input_GP_from_state(m, sampler=spec)
    xd, yd, cd = G.input_GP_from_state(m, method="delta")
    assert np.array_equal(xb, xd) and np.array_equal(yb, yd) and cd.shape == cb.shape == (2, 4, 4)
    V = m.derivs_cov().values                                     # (order, order_2, val)
    assert np.array_equal(cd, np.transpose(V, (2, 0, 1)))
    # log scale: T V T'
    xl, yl, cl = G.input_GP_from_state(m, method="delta", log_scale=True)
    xlb, ylb, _ = G.input_GP_from_state(m, sampler=spec, log_scale=True)
    assert np.array_equal(xl, xlb) and np.array_equal(yl, ylb)
    T = G.log_scale_matrix(BETA0, 3)
    for k in range(2):
        np.testing.assert_allclose(cl[k], T @ cd[k] @ T.T, rtol=1e-13, atol=0)
    with pytest.raises(ValueError):
        G.input_GP_from_state(m, method="jackknife")


def test_gp_input_delta_draws_no_sampler(txm, monkeypatch):
    from thermoextrap_amd import gpr_input as G, moments as cm

    x, u, w = make_data(300, seed=5)
    m = _model(txm, x, u, w, 2, True)

    def boom(*a, **k):
        raise AssertionError("a sampler was drawn")

    monkeypatch.setattr(cm, "factory_sampler", boom)
    G.input_GP_from_state(m, method="delta")


def test_gp_input_states_delta(txm):
    from thermoextrap_amd import gpr_input as G

    ms = []
    for s in range(3):
        x, u, w = make_data(300, seed=10 + s, ncol=2)
        data = txm.DataCentralMomentsVals.from_vals(xv=txm.DataArray(x, ("rec", "val")), uv=txm.DataArray(u, ("rec",)), order=2,
                                                    central=True, weight=txm.DataArray(w, ("rec",)))
        ms.append(txm.beta.factory_extrapmodel(beta=0.4 + 0.1 * s, data=data))
    spec = {"nrep": 8, "seed": 1, "device": True}
    xb, yb, cb = G.input_GP_from_states(ms, sampler=spec)
    xd, yd, cd = G.input_GP_from_states(ms, method="delta")
    assert np.array_equal(xb, xd) and cd.shape == cb.shape == (2, 9, 9)
    np.testing.assert_allclose(yd, yb, rtol=1e-13)
    for s, m in enumerate(ms):
        V = np.transpose(m.derivs_cov().values, (2, 0, 1))
        assert np.array_equal(cd[:, 3 * s:3 * s + 3, 3 * s:3 * s + 3], V)
    assert not cd[:, :3, 3:].any()


def test_against_device_bootstrap(txm):
    """N = 1e5, three columns, order 2: every entry of V within 5 se of the covariance over 2000 device-bootstrap replicates,
    se_ij = std_r[(d_i - m_i)(d_j - m_j)] / sqrt(R) from the replicates themselves."""
    R = 2000
    x, u, _ = make_data(100_000, seed=7, weighted=False, ncol=3)
    m = _model(txm, x, u, None, 2, True)
    V = m.derivs_cov().values                                                       # (3, 3, val)
    d = m.resample({"nrep": R, "seed": 1, "device": True}).derivs().transpose("rep", "order", "val").values
    dev = d - d.mean(axis=0)
    prod = dev[:, :, None, :] * dev[:, None, :, :]
    Sm = prod.sum(axis=0) / (R - 1)
    se = prod.std(axis=0, ddof=1) / math.sqrt(R)
    ratio = np.abs(V - Sm) / se
    print("device bootstrap: worst |V - S| / se =", float(ratio.max()), " median se / |S| =", float(np.median(se / np.abs(Sm))))
    assert (ratio <= 5.0).all()


def test_unsupported_kinds_raise(txm):
    DA = txm.DataArray
    x, u, w = make_data(120, seed=8, ncol=2)
    xv, uv = DA(x, ("rec", "val")), DA(u, ("rec",))
    B = txm.beta.factory_extrapmodel
    models = {}
    xd = DA(np.stack([x, 0.1 * x, 0.01 * x], axis=1), ("rec", "deriv", "val"))
    models["xalpha"] = B(BETA0, txm.DataCentralMomentsVals.from_vals(xv=xd, uv=uv, order=2, central=True, deriv_dim="deriv"),
                         xalpha=True)
    models["x_is_u"] = B(BETA0, txm.DataCentralMomentsVals.from_vals(xv=None, uv=uv, order=2, central=True, x_is_u=True),
                         name="u_ave")
    models["reduced"] = B(BETA0, txm.DataCentralMoments.from_vals(xv=xv, uv=uv, order=2, central=True, dim="rec"))
    for central in (False, True):
        models[f"values{central}"] = B(BETA0, txm.factory_data_values(order=2, uv=uv, xv=xv, central=central))
    vals = txm.DataCentralMomentsVals.from_vals(xv=xv, uv=uv, order=2, central=True)
    models["resampled"] = B(BETA0, vals).resample({"nrep": 4, "seed": 0})
    models["volume"] = txm.volume.factory_extrapmodel(volume=5.0, uv=uv, xv=xv, dxdqv=xv, ndim=1)

    class Meta(txm.DataCallback):
        pass

    models["callback"] = B(BETA0, vals.new_like(meta=Meta()))
    funcs = [lambda *a: a[0], lambda *a: -a[2][1], lambda *a: a[2][2]]
    models["callables"] = txm.ExtrapModel(alpha0=BETA0, data=vals, derivatives=txm.Derivatives(funcs), order=2)
    for name, m in models.items():
        with pytest.raises(NotImplementedError):
            m.derivs_cov()
        with pytest.raises(NotImplementedError):
            m.predict_with_error(0.6)
    from thermoextrap_amd import gpr_input as G

    with pytest.raises(NotImplementedError):
        G.input_GP_from_state(models["reduced"], method="delta")
