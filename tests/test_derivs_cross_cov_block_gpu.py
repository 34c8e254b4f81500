"""The blocked cross-column delta-method covariance through the public interface:
ExtrapModel.derivs_cross_cov(block=...), predict_cov(block=...) and cross_blocking_curve -- against the definition restated
in long double through symbolic.influence_coefs (tests/_block_cross_ref.py)

    V^B[i, j, c, c'] = sum_b z_bi(c) z_bj(c'),   z_bk(c) = sum_{n in block b} p_n psi_k(n, c)

under the rule tests/test_influence_cross_gpu.py holds the iid interface to, with the blocked bound:
|V - ref| <= 1e-12 sum_b beta_bi(c) beta_bj(c') + 2^-1022, beta from the same coefficients (through the raw form they cancel
on the host) -- against derivs_cov(block=...), predict_with_error(block=...) and itself, and once against a series whose
long-run covariance is known."""

from __future__ import annotations

import math

import numpy as np
import pytest

from tests._block_cross_ref import AR1_BLOCK, AR1_LIMIT, ar1_columns, ar1_scale, blocked_cross_ld
from tests._influence_ref import LD, make_data

pytestmark = pytest.mark.gpu

TOL = 1e-12
TINY = 2.0**-1022
ORDER, BETA0 = 4, 0.5
_worst: dict = {}


def _model(txm, x, u, w, order, central=True, minus_log=False):
    DA = txm.DataArray
    data = txm.DataCentralMomentsVals.from_vals(xv=DA(x, ("rec", "val")), uv=DA(u, ("rec",)), order=order, central=central,
                                                weight=None if w is None else DA(w, ("rec",)))
    m = txm.beta.factory_extrapmodel(beta=BETA0, data=data)
    return m.new_like(minus_log=True) if minus_log else m


def _cicj(V):
    """(order, order_2, val, val_2) values as [c, i, c', j]."""
    return np.transpose(np.asarray(V.values), (2, 0, 3, 1))


def _compare(group, got, ref, bnd, what):
    ratio = float((np.abs(got - ref) / (TOL * bnd + TINY)).max()) * TOL
    _worst[group] = max(_worst.get(group, 0.0), ratio)
    assert ratio <= TOL, (what, ratio)


def _report(group):
    print(f"{group}: worst |V - ref| / sum_b beta_b beta_b' = {_worst.get(group, 0.0):.2e}")


@pytest.fixture(scope="module")
def data3():
    return make_data(331, seed=0, ncol=3)           # three columns, weighted, N no multiple of the blocks used


@pytest.mark.parametrize("central", [True, False])
@pytest.mark.parametrize("minus_log", [False, True])
@pytest.mark.parametrize("weighted", [True, False])
def test_derivs_cross_cov_block_matches_long_double(txm, data3, central, minus_log, weighted):
    """N = 331, three columns, order 4, blocks of 7 and 64: V within the bound of the long-double restatement, exactly
    symmetric; the blocks c == c' against derivs_cov(block=B) within the two bounds; norm=True carries 1 / (i! j!)."""
    x, u, w = data3
    w = w if weighted else None
    m = _model(txm, x, u, w, ORDER, central, minus_log)
    for block in (7, 64):
        V = m.derivs_cross_cov(block=block)
        assert V.dims == ("order", "order_2", "val", "val_2") and V.shape == (ORDER + 1, ORDER + 1, 3, 3)
        ref, bnd = blocked_cross_ld(x, u, w, ORDER, central, minus_log, block)
        got = _cicj(V)
        _compare("derivs_cross_cov(block)", got, ref, bnd, (central, minus_log, weighted, block))
        assert np.array_equal(got.reshape(15, 15), got.reshape(15, 15).T)
        D = m.derivs_cov(block=block).values                                             # (order, order_2, val)
        for c in range(3):
            assert (np.abs(got[c, :, c, :] - D[:, :, c]) <= 2 * TOL * bnd[c, :, c, :].astype(np.float64) + TINY).all(), c
    f = np.array([1.0 / math.factorial(i) for i in range(ORDER + 1)])
    V, Vn = m.derivs_cross_cov(block=7), m.derivs_cross_cov(norm=True, block=7)
    np.testing.assert_allclose(Vn.values, V.values * f[:, None, None, None] * f[None, :, None, None], rtol=1e-15)
    V2 = m.derivs_cross_cov(order=2, block=7)
    ref2, bnd2 = blocked_cross_ld(x, u, w, 2, central, minus_log, 7)
    assert V2.shape == (3, 3, 3, 3)
    _compare("derivs_cross_cov(block)", _cicj(V2), ref2, bnd2, (central, minus_log, weighted, "order 2"))
    _report("derivs_cross_cov(block)")


def test_block_one_is_the_iid_result(txm, data3):
    x, u, w = data3
    m = _model(txm, x, u, w, ORDER)
    _, bnd = blocked_cross_ld(x, u, w, ORDER, True, False, 1)
    assert (np.abs(_cicj(m.derivs_cross_cov(block=1)) - _cicj(m.derivs_cross_cov())) <= 2 * TOL * bnd.astype(np.float64) + TINY).all()


def test_linearity_in_the_observable(txm):
    """A third column x_2 = x_0 + x_1, no minus_log: V[2,2] = V[0,0] + V[0,1] + V[1,0] + V[1,1] for every (i, j), within
    the bounds of the five blocks."""
    x, u, w = make_data(300, seed=3, ncol=2)
    x3 = np.concatenate([x, (x[:, 0] + x[:, 1])[:, None]], axis=1)
    for central in (True, False):
        V = _cicj(_model(txm, x3, u, w, ORDER, central).derivs_cross_cov(block=16))
        _, bnd = blocked_cross_ld(x3, u, w, ORDER, central, False, 16)
        total = V[0, :, 0, :] + V[0, :, 1, :] + V[1, :, 0, :] + V[1, :, 1, :]
        lim = TOL * (bnd[2, :, 2, :] + bnd[0, :, 0, :] + bnd[0, :, 1, :] + bnd[1, :, 0, :] + bnd[1, :, 1, :]).astype(np.float64)
        # (x_2 as stored is the ROUNDED sum: relative 2^-53 on dx, far inside the bound's 1e-12)
        assert (np.abs(V[2, :, 2, :] - total) <= lim + TINY).all(), central


@pytest.mark.parametrize("minus_log", [False, True])
def test_predict_cov_block(txm, data3, minus_log):
    x, u, w = data3
    m = _model(txm, x, u, w, ORDER, True, minus_log)
    alphas = np.array([0.3, 0.5, 0.62])
    pred, cov = m.predict_cov(alphas, block=7)
    ref = m.predict(alphas)
    assert pred.dims == ref.dims and np.array_equal(pred.values, ref.values)             # bit for bit
    assert cov.dims == (*ref.dims, "val_2") and cov.shape == (3, 3, 3)
    V = np.asarray(m.derivs_cross_cov(block=7).values, LD)                               # (i, j, c, c')
    _, bnd = blocked_cross_ld(x, u, w, ORDER, True, minus_log, 7)
    _, std = m.predict_with_error(alphas, block=7)
    for k, al in enumerate(alphas):
        t = np.array([LD(al - BETA0) ** i / math.factorial(i) for i in range(ORDER + 1)])
        want = np.einsum("i,ijcd,j->cd", t, V, t)
        tb = np.einsum("i,cidj,j->cd", np.abs(t), bnd, np.abs(t))
        assert (np.abs(cov.values[k] - want) <= TOL * tb.astype(np.float64) + TINY).all()
        # the diagonal is predict_with_error's variance (its V comes from the per-column kernel: both bounds)
        for c in range(3):
            assert abs(cov.values[k, c, c] - float(std.values[k, c]) ** 2) <= 3 * TOL * float(tb[c, c]) + TINY
    _, cov0 = m.predict_cov(alphas)
    assert not np.array_equal(cov0.values, cov.values)
    pred1, cov1 = m.predict_cov(0.3, order=2, block=7)
    assert np.array_equal(pred1.values, m.predict(0.3, order=2).values) and cov1.shape == (3, 3)


@pytest.mark.parametrize("block,N", [(7, 331), (5, 320), (1, 9)])
def test_cross_blocking_curve(txm, block, N):
    """Level l against derivs_cross_cov(block=block 2^l) and against the definition under the bound; the lengths and
    counts against engine.block_levels; the level coordinate as in blocking_curve; the diagonal against blocking_curve."""
    from thermoextrap_amd import engine

    x, u, w = make_data(N, seed=1, ncol=3)
    m = _model(txm, x, u, w, 2)
    V, lengths, counts = m.cross_blocking_curve(block)
    el, ec = engine.block_levels(N, block)
    assert np.array_equal(lengths, el) and np.array_equal(counts, ec) and counts[-1] >= 2
    nl = len(lengths)
    assert V.dims == ("level", "order", "order_2", "val", "val_2") and V.shape == (nl, 3, 3, 3, 3)
    D, dl, dc = m.blocking_curve(block)
    assert np.array_equal(dl, lengths) and np.array_equal(dc, counts)
    assert np.array_equal(np.asarray(V["level"].values), np.asarray(D["level"].values))
    assert np.array_equal(np.asarray(V["level"].values), lengths)
    for l in range(nl):
        ref, bnd = blocked_cross_ld(x, u, w, 2, True, False, int(lengths[l]))
        got = np.transpose(V.values[l], (2, 0, 3, 1))
        _compare("cross_blocking_curve", got, ref, bnd, (block, N, l))
        lim = 2 * TOL * bnd.astype(np.float64) + TINY
        if 2 * lengths[l] <= N:
            assert (np.abs(got - _cicj(m.derivs_cross_cov(block=int(lengths[l])))) <= lim).all(), l
        for c in range(3):
            assert (np.abs(got[c, :, c, :] - D.values[l, :, :, c]) <= lim[c, :, c, :]).all(), (l, c)
    assert np.array_equal(V.values[0], m.derivs_cross_cov(block=block).values)           # level 0: the same launches
    f = np.array([1.0, 1.0, 0.5])
    Vn, _, _ = m.cross_blocking_curve(block, norm=True)
    np.testing.assert_allclose(Vn.values, V.values * f[None, :, None, None, None] * f[None, None, :, None, None], rtol=1e-15)
    with pytest.raises(ValueError):
        m.cross_blocking_curve(N // 2 + 1)
    _report("cross_blocking_curve")


def test_a_blocked_call_leaves_the_default_path_alone(txm, data3):
    x, u, w = data3
    fresh = _model(txm, x, u, w, ORDER).derivs_cross_cov().values
    m = _model(txm, x, u, w, ORDER)
    before = m.derivs_cross_cov().values.copy()
    m.derivs_cross_cov(block=7)
    m.cross_blocking_curve(7)
    m.predict_cov(0.6, block=7)
    assert np.array_equal(m.derivs_cross_cov().values, before) and np.array_equal(before, fresh)
    m2 = _model(txm, x, u, w, ORDER)
    V7 = m2.derivs_cross_cov(block=7).values
    assert ("dxcov", ORDER, False) not in m2._cache and ("dcov", ORDER, False) not in m2._cache
    assert np.array_equal(m2.derivs_cross_cov().values, fresh)
    assert np.array_equal(m2.derivs_cross_cov(block=7).values, V7) and np.array_equal(m.derivs_cross_cov(block=7).values, V7)
    assert not np.array_equal(V7, fresh)


def test_block_validation_and_unsupported_kinds(txm, data3):
    x, u, w = data3
    m = _model(txm, x, u, w, 2)
    N = len(u)
    for bad in (7.0, "7", True, [7], np.float64(7)):
        with pytest.raises(TypeError):
            m.derivs_cross_cov(block=bad)
    with pytest.raises(TypeError):
        m.predict_cov(0.6, block=2.5)
    with pytest.raises(TypeError):
        m.cross_blocking_curve(2.5)
    for bad in (0, -3, N // 2 + 1, N):
        with pytest.raises(ValueError):
            m.derivs_cross_cov(block=bad)
        with pytest.raises(ValueError):
            m.predict_cov(0.6, block=bad)
    m.derivs_cross_cov(block=N // 2)                                # two blocks: the shortest curve
    m.derivs_cross_cov(block=np.int64(7))

    # every kind that raises NotImplementedError without a block raises it with one, before any launch
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
    for name, mm in models.items():
        with pytest.raises(NotImplementedError) as e1:
            mm.derivs_cross_cov(block=7)
        with pytest.raises(NotImplementedError):
            mm.predict_cov(0.6, block=7)
        with pytest.raises(NotImplementedError):
            mm.cross_blocking_curve(7)
        with pytest.raises(NotImplementedError) as e0:
            mm.derivs_cov(block=7)
        assert str(e1.value) == str(e0.value), name                                      # the same message


def test_more_than_255_columns_raise(txm, monkeypatch):
    from thermoextrap_amd import engine

    x, u, _ = make_data(40, seed=1, weighted=False, ncol=256)
    m = _model(txm, x, u, None, 1, True)
    monkeypatch.setattr(engine, "influence_block_cross_cov", lambda *a, **k: pytest.fail("a launch before the refusal"))
    with pytest.raises(ValueError, match="255"):
        m.derivs_cross_cov(block=4)
    with pytest.raises(ValueError, match="255"):
        m.predict_cov(0.6, block=4)
    with pytest.raises(ValueError, match="255"):
        m.cross_blocking_curve(4)
    assert m.derivs_cov(block=4).shape == (2, 2, 256)                                    # the per-column path has no such limit


# ---- a series with a known answer ----------------------------------------------------------------------------------------
def test_definition_on_correlated_ar1_columns(txm):
    """u and three independent e_k are AR(1) with rho = 0.9 and unit variance, x_0 = 0.7 u + e_0,
    x_1 = 0.5 u + 0.8 e_0 + 0.3 e_1, x_2 = -0.6 u + e_2, N = 2^20: the long-run covariance of the column means is
    19 Sigma / N with Sigma the population covariance (correlations 0.952 and -0.295).  At B = 1024 every entry of the
    blocked V[0, 0] lies within 0.25 * 19 sqrt(Sigma_cc Sigma_c'c') / N of it: five standard deviations sqrt(2 / 1023) of
    the estimator (an off-diagonal entry has sqrt((1 + r^2) / nb) <= sqrt(2 / nb) of that scale) plus the block bias.
    The iid V[0, 0, 0, 1] is 1 / 19 of the target within 5 %."""
    u, x = ar1_columns(0)
    m = _model(txm, x, u, None, 1)
    target, scale = ar1_scale()
    V = m.derivs_cross_cov(block=AR1_BLOCK).values[0, 0]
    dev = np.abs(V - target) / scale
    d = np.sqrt(np.diag(V))
    corr = V / np.outer(d, d)
    iid = float(m.derivs_cross_cov().values[0, 0, 0, 1]) / target[0, 1]
    print(f"AR(1) columns, N = 2^20, B = 1024: worst |V - 19 Sigma / N| / scale = {dev.max():.4f} (limit {AR1_LIMIT}); "
          f"blocked correlations {corr[0, 1]:.4f}, {corr[0, 2]:.4f}; iid V[0,0,0,1] / target = {iid:.4f}")
    assert (dev <= AR1_LIMIT).all()
    assert abs(iid - 1.0 / 19.0) <= 0.05 / 19.0
