"""Blocked delta-method error bars through the public interface: ExtrapModel.derivs_cov(block=...),
blocking_curve, predict_with_error(block=...), the state collections, gpr_input's method="delta" with a block and
timeseries.block_length -- against the definition restated in long double (tests/_influence_ref.py)

    V^B[i, j] = sum_b z_bi z_bj,   z_bk = sum_{n in block b} p_n psi_k(n)

within 1e-12 sum_b beta_bi beta_bj, beta_bk = sum_{n in b} p_n B_k(n) (the rounding bound of the block sums), against numpy
restatements of the models' variance formulas, and once against a series whose long-run variance is known."""

from __future__ import annotations

import math

import numpy as np
import pytest

from tests._influence_ref import bound_ld, cov_ld, ld_moments, make_data, psi_ld, series_for

pytestmark = pytest.mark.gpu

ORDER, BETA0 = 3, 0.5
CASES = [(c, m) for c in (True, False) for m in (False, True)]


def _model(txm, x, u, w, order, central=True, minus_log=False, beta=BETA0):
    DA = txm.DataArray
    xv = DA(x if x.ndim == 2 else x[:, None], ("rec", "val"))
    data = txm.DataCentralMomentsVals.from_vals(xv=xv, uv=DA(u, ("rec",)), order=order, central=central,
                                                weight=None if w is None else DA(w, ("rec",)))
    m = txm.beta.factory_extrapmodel(beta=beta, data=data)
    return m.new_like(minus_log=True) if minus_log else m


def _blocked_ld(x, u, w, order, central, minus_log, block):
    """(V [c][i, j], bound [c][i, j]) of the blocked estimator in long double, column by column."""
    from thermoextrap_amd import symbolic as S

    x2 = x if x.ndim == 2 else x[:, None]
    p, dx, du, mom = ld_moments(x2, u, w, order)
    a, b = S.influence_coefs(series_for(central), order, mom, minus_log=minus_log)
    starts = np.arange(0, len(u), block)
    V, bnd = [], []
    for c in range(x2.shape[1]):
        z = np.add.reduceat(p * psi_ld(a[c], b[c], dx[:, c], du), starts, axis=1)
        beta = np.add.reduceat(p * bound_ld(a[c], b[c], dx[:, c], du), starts, axis=1)
        V.append(z @ z.T)
        bnd.append(beta @ beta.T)
    return V, bnd


@pytest.fixture(scope="module")
def data2():
    return make_data(331, seed=0, ncol=2)           # two value columns, weighted, N no multiple of the blocks used


def test_block_one_is_the_iid_result(txm, data2):
    from thermoextrap_amd import symbolic as S

    x, u, w = data2
    m = _model(txm, x, u, w, ORDER)
    V1, V0 = m.derivs_cov(block=1), m.derivs_cov()
    assert V1.dims == V0.dims == ("order", "order_2", "val") and V1.shape == V0.shape == (ORDER + 1, ORDER + 1, 2)
    p, dx, du, mom = ld_moments(x, u, w, ORDER)
    a, b = S.influence_coefs(series_for(True), ORDER, mom)
    for c in range(2):
        bnd = cov_ld(bound_ld(a[c], b[c], dx[:, c], du), p)
        ratio = float((np.abs(V1.values[:, :, c] - V0.values[:, :, c]) / bnd).max())
        print(f"column {c}: worst |V(block=1) - V()| / sum p^2 B_i B_j = {ratio:.2e}")
        assert ratio <= 1e-12


@pytest.mark.parametrize("central,minus_log", CASES)
def test_derivs_cov_block_matches_long_double(txm, data2, central, minus_log):
    x, u, w = data2
    m = _model(txm, x, u, w, ORDER, central, minus_log)
    for block in (7, 64):
        V = m.derivs_cov(block=block)
        assert V.dims == ("order", "order_2", "val") and V.shape == (ORDER + 1, ORDER + 1, 2)
        ref, bnd = _blocked_ld(x, u, w, ORDER, central, minus_log, block)
        for c in range(2):
            ratio = float((np.abs(V.values[:, :, c] - ref[c]) / bnd[c]).max())
            print(f"central={central} minus_log={minus_log} block={block} column {c}: worst ratio to the bound {ratio:.2e}")
            assert ratio <= 1e-12
            assert np.array_equal(V.values[:, :, c], V.values[:, :, c].T)
    # norm=True carries 1 / (i! j!); a lower order; the unweighted call
    f = np.array([1.0 / math.factorial(i) for i in range(ORDER + 1)])
    np.testing.assert_allclose(m.derivs_cov(norm=True, block=7).values, m.derivs_cov(block=7).values * f[:, None, None] * f[None, :, None],
                               rtol=1e-15)
    mu = _model(txm, x, u, None, ORDER, central, minus_log)
    V2 = mu.derivs_cov(order=2, block=7)
    ref, bnd = _blocked_ld(x, u, None, 2, central, minus_log, 7)
    assert V2.shape == (3, 3, 2)
    for c in range(2):
        assert (np.abs(V2.values[:, :, c] - ref[c]) <= 1e-12 * bnd[c]).all()


def test_a_blocked_call_leaves_the_default_path_alone(txm, data2):
    x, u, w = data2
    fresh = _model(txm, x, u, w, ORDER).derivs_cov().values
    m = _model(txm, x, u, w, ORDER)
    m.derivs_cov(block=7)
    m.blocking_curve(7)
    m.predict_with_error(0.6, block=7)
    assert np.array_equal(m.derivs_cov().values, fresh)
    m2 = _model(txm, x, u, w, ORDER)
    V7 = m2.derivs_cov(block=7).values
    m2.derivs_cov()
    assert np.array_equal(m2.derivs_cov(block=7).values, V7) and np.array_equal(m.derivs_cov(block=7).values, V7)
    assert not np.array_equal(V7, fresh)


@pytest.mark.parametrize("block,N", [(7, 331), (5, 320), (1, 9)])
def test_blocking_curve(txm, block, N):
    """Level l against derivs_cov(block=block 2^l) under the bound; the lengths and counts, N no multiple of block 2^l."""
    x, u, w = make_data(N, seed=1, ncol=2)
    m = _model(txm, x, u, w, 2)
    V, lengths, counts = m.blocking_curve(block)
    nl = len(lengths)
    want = [block << l for l in range(64) if -(-N // (block << l)) >= 2]
    assert list(lengths) == want and list(counts) == [-(-N // b) for b in want] and counts[-1] >= 2
    assert V.dims == ("level", "order", "order_2", "val") and V.shape == (nl, 3, 3, 2)
    for l in range(nl):
        # (a last level of one full and one short block has two blocks, but 2 B 2^l > N: derivs_cov refuses that length,
        # so every level is also held against the definition itself)
        ref, bnd = _blocked_ld(x, u, w, 2, True, False, int(lengths[l]))
        Vl = m.derivs_cov(block=int(lengths[l])).values if 2 * lengths[l] <= N else None
        for c in range(2):
            assert (np.abs(V.values[l, :, :, c] - ref[c]) <= 1e-12 * bnd[c]).all(), (l, c)
            if Vl is not None:
                assert (np.abs(V.values[l, :, :, c] - Vl[:, :, c]) <= 1e-12 * bnd[c]).all(), (l, c)
    assert np.array_equal(V.values[0], m.derivs_cov(block=block).values)         # level 0: the same block sums
    f = np.array([1.0, 1.0, 0.5])
    Vn, _, _ = m.blocking_curve(block, norm=True)
    np.testing.assert_allclose(Vn.values, V.values * f[None, :, None, None] * f[None, None, :, None], rtol=1e-15)
    with pytest.raises(ValueError):
        m.blocking_curve(N // 2 + 1)


@pytest.mark.parametrize("minus_log", [False, True])
def test_predict_with_error_block(txm, data2, minus_log):
    x, u, w = data2
    m = _model(txm, x, u, w, ORDER, True, minus_log)
    alphas = np.array([0.3, 0.5, 0.62])
    pred, std = m.predict_with_error(alphas, block=7)
    ref = m.predict(alphas)
    assert pred.dims == ref.dims == std.dims and np.array_equal(pred.values, ref.values)
    V = np.asarray(m.derivs_cov(block=7).values, np.longdouble)
    for i, al in enumerate(alphas):
        t = np.array([np.longdouble(al - BETA0) ** k / math.factorial(k) for k in range(ORDER + 1)])
        for c in range(2):
            var = float(t @ V[:, :, c] @ t)
            bnd = float(np.abs(t) @ np.abs(V[:, :, c]) @ np.abs(t))
            assert abs(float(std.values[i, c]) ** 2 - var) <= 1e-12 * bnd
    _, std0 = m.predict_with_error(alphas)
    assert not np.array_equal(std0.values, std.values)


# ---- state collections ---------------------------------------------------------------------------------------------------
NS, BETAS = (300, 257, 411), (0.4, 0.5, 0.6)


def _states(txm, order=2):
    return [_model(txm, *make_data(n, seed=10 + s, ncol=2), order, beta=BETAS[s]) for s, n in enumerate(NS)]


def _hermite_g(alpha0, order, alphas):
    npoly = len(alpha0) * (order + 1)
    p = np.arange(npoly)
    rows = []
    for a0 in alpha0:
        for j in range(order + 1):
            fall = np.array([math.perm(int(q), j) if q >= j else 0 for q in p], dtype=float)
            rows.append(fall * np.where(p >= j, np.power(float(a0), np.maximum(p - j, 0)), 0.0))
    return (np.asarray(alphas, float)[:, None] ** p[None, :]) @ np.linalg.inv(np.array(rows))


def _V(st, order, block):
    return np.transpose(st.derivs_cov(order=order, block=block).values, (2, 0, 1))        # (val, i, j)


def _interp_std(states, blocks, order, alphas):
    g = _hermite_g([st.alpha0 for st in states], order, alphas).reshape(len(alphas), len(states), order + 1)
    Vs = [_V(st, order, blocks[s]) for s, st in enumerate(states)]
    var = sum(np.einsum("ai,cij,aj->ac", g[:, s], Vs[s], g[:, s]) for s in range(len(states)))
    bnd = sum(np.einsum("ai,cij,aj->ac", np.abs(g[:, s]), np.abs(Vs[s]), np.abs(g[:, s])) for s in range(len(states)))
    return np.sqrt(var), np.sqrt(bnd)


def _weighted_std(states, blocks, order, alpha):
    a0 = np.array([st.alpha0 for st in states])
    dm = np.abs(alpha - a0) ** 20
    w = 1.0 - dm / dm.sum()
    fact = np.array([math.factorial(k) for k in range(order + 1)], dtype=float)
    var = bnd = 0.0
    for i, st in enumerate(states):
        t = (w[i] / w.sum()) * (alpha - a0[i]) ** np.arange(order + 1) / fact
        Vi = _V(st, order, blocks[i])
        var = var + np.einsum("i,cij,j->c", t, Vi, t)
        bnd = bnd + np.einsum("i,cij,j->c", np.abs(t), np.abs(Vi), np.abs(t))
    return np.sqrt(var), np.sqrt(bnd)


def _between(n_states, a0, alpha):
    i = min(max(int(np.searchsorted(a0, alpha, side="right")) - 1, 0), n_states - 2)
    return [i, i + 1]


ALPHAS = [0.3, 0.43, 0.5, 0.58, 0.7]
BLOCKINGS = [7, (7, 5, 16)]                      # an int for all states; one entry per state


@pytest.mark.parametrize("block", BLOCKINGS)
def test_collection_derivs_cov_block(txm, monkeypatch, block):
    from thermoextrap_amd import engine

    blocks = [block] * 3 if isinstance(block, int) else list(block)
    ref = [st.derivs_cov(block=blocks[s]).values for s, st in enumerate(_states(txm))]
    coll = txm.StateCollection(_states(txm))
    monkeypatch.setattr(engine, "influence_cov_batched", lambda *a, **k: pytest.fail("the iid batched path ran"))
    got = coll.derivs_cov(block=block)
    assert got.dims == ("beta", "order", "order_2", "val") and got.shape == (3, 3, 3, 2)
    for s in range(3):
        assert np.array_equal(got.values[s], ref[s])
    monkeypatch.undo()
    # the default path afterwards: what a fresh collection gives
    assert np.array_equal(coll.derivs_cov().values, txm.StateCollection(_states(txm)).derivs_cov().values)
    with pytest.raises(ValueError):
        coll.derivs_cov(block=[7, 5])
    with pytest.raises(TypeError):
        coll.derivs_cov(block=[7, 5.0, 16])


@pytest.mark.parametrize("block", BLOCKINGS)
def test_interp_model_predict_with_error_block(txm, block):
    blocks = [block] * 3 if isinstance(block, int) else list(block)
    m = txm.InterpModel(_states(txm))
    for alpha in (ALPHAS, 0.47):
        pred, std = m.predict_with_error(alpha, block=block)
        assert np.array_equal(pred.values, m.predict(alpha).values) and pred.dims == std.dims and pred.shape == std.shape
        ref, bnd = _interp_std(list(m), blocks, 2, np.atleast_1d(alpha))
        assert (np.abs(std.values.reshape(ref.shape) - ref) <= 1e-12 * bnd).all()
        assert (std.values > 0).all()


@pytest.mark.parametrize("block", BLOCKINGS)
def test_piecewise_models_predict_with_error_block(txm, block):
    blocks = [block] * 3 if isinstance(block, int) else list(block)
    states = _states(txm)
    a0 = np.array([st.alpha0 for st in states])
    pw, wm = txm.InterpModelPiecewise(states), txm.ExtrapWeightedModel(states)
    for alpha in (ALPHAS, 0.47):
        seq = np.atleast_1d(alpha)
        pred, std = pw.predict_with_error(alpha, method="between", block=block)
        assert np.array_equal(pred.values, pw.predict(alpha, method="between").values) and pred.shape == std.shape
        predw, stdw = wm.predict_with_error(alpha, method="between", block=block)
        assert np.array_equal(predw.values, wm.predict(alpha, method="between").values) and predw.shape == stdw.shape
        for k, a in enumerate(seq):
            idx = _between(3, a0, a)
            pair, pb = [states[i] for i in idx], [blocks[i] for i in idx]
            ref, bnd = _interp_std(pair, pb, 2, [a])
            assert (np.abs(std.values.reshape(len(seq), -1)[k] - ref[0]) <= 1e-12 * bnd[0]).all(), a
            refw, bndw = _weighted_std(pair, pb, 2, a)
            assert (np.abs(stdw.values.reshape(len(seq), -1)[k] - refw) <= 1e-12 * bndw).all(), a


def test_gp_input_delta_block(txm, data2):
    from thermoextrap_amd import gpr_input as G

    x, u, w = data2
    m = _model(txm, x, u, w, ORDER)
    xd, yd, cd = G.input_GP_from_state(m, method="delta")
    xb, yb, cb = G.input_GP_from_state(m, method="delta", block=7)
    assert np.array_equal(xb, xd) and np.array_equal(yb, yd)
    assert np.array_equal(cb, np.transpose(m.derivs_cov(block=7).values, (2, 0, 1))) and not np.array_equal(cb, cd)
    with pytest.raises(ValueError):
        G.input_GP_from_state(m, block=7)                           # the bootstrap takes no block
    states = _states(txm)
    for block in BLOCKINGS:
        blocks = [block] * 3 if isinstance(block, int) else list(block)
        xs, ys, cs = G.input_GP_from_states(states, method="delta", block=block)
        x0, y0, _ = G.input_GP_from_states(_states(txm), method="delta")
        assert np.array_equal(xs, x0) and np.array_equal(ys, y0) and cs.shape == (2, 9, 9)
        for s, st in enumerate(states):
            assert np.array_equal(cs[:, 3 * s:3 * s + 3, 3 * s:3 * s + 3], _V(st, 2, blocks[s]))
        assert not cs[:, :3, 3:].any()


def test_block_validation_and_unsupported_kinds(txm, data2):
    x, u, w = data2
    m = _model(txm, x, u, w, 2)
    N = len(u)
    for bad in (7.0, "7", True, [7], np.float64(7)):
        with pytest.raises(TypeError):
            m.derivs_cov(block=bad)
    with pytest.raises(TypeError):
        m.predict_with_error(0.6, block=2.5)
    with pytest.raises(TypeError):
        m.blocking_curve(2.5)
    for bad in (0, -3, N // 2 + 1, N):
        with pytest.raises(ValueError):
            m.derivs_cov(block=bad)
        with pytest.raises(ValueError):
            m.predict_with_error(0.6, block=bad)
    m.derivs_cov(block=N // 2)                                      # two blocks: the shortest curve
    m.derivs_cov(block=np.int64(7))

    # every kind that raises NotImplementedError without a block raises it with one
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
        with pytest.raises(NotImplementedError):
            mm.derivs_cov(block=7)
        with pytest.raises(NotImplementedError):
            mm.predict_with_error(0.6, block=7)
        with pytest.raises(NotImplementedError):
            mm.blocking_curve(7)
    for cls in (txm.InterpModel, txm.InterpModelPiecewise, txm.ExtrapWeightedModel):
        with pytest.raises(NotImplementedError):
            cls([B(0.4, vals), models["reduced"].new_like(alpha0=0.6)]).predict_with_error(0.5, block=7)
    with pytest.raises(NotImplementedError):
        txm.MBARModel([B(0.4, vals), B(0.6, vals)]).derivs_cov(block=7)


# ---- a series with a known answer ----------------------------------------------------------------------------------------
def _ar1(rng, n, rho):
    """AR(1), unit marginal variance, started in the stationary distribution."""
    eps = rng.standard_normal(n) * math.sqrt(1.0 - rho * rho)
    out = eps.tolist()
    out[0] = float(rng.standard_normal())
    for i in range(1, n):
        out[i] += rho * out[i - 1]
    return np.asarray(out)


@pytest.fixture(scope="module")
def ar1_series():
    rng = np.random.default_rng(0)
    n = 1 << 20
    u, e = _ar1(rng, n, 0.9), _ar1(rng, n, 0.9)
    return u, 0.7 * u + e


def test_definition_on_an_ar1_series(txm, ar1_series):
    """u and an independent e are AR(1) with rho = 0.9 and unit marginal variance, x = 0.7 u + e, N = 2^20: the long-run
    variance of the mean of x is (1 + rho) / (1 - rho) var(x) / N = 19 var(x) / N.  At B = 1024 the blocked V[0, 0] over
    that figure is within 0.25 of 1: 5 standard deviations of the estimator (sqrt(2 / 1023) = 4.4 % each) plus the -1 %
    block bias; the iid V[0, 0] is below 0.1 of it (expected ratio 1 / 19).  In numpy, seeds 0 - 5: blocked 0.92 .. 1.06,
    iid 0.053."""
    u, x = ar1_series
    m = _model(txm, x, u, None, 1)
    target = 19.0 * x.var() / len(x)
    blocked = float(m.derivs_cov(block=1024).values[0, 0, 0]) / target
    iid = float(m.derivs_cov().values[0, 0, 0]) / target
    print(f"AR(1), N = 2^20, B = 1024: blocked V[0,0] / (19 var(x) / N) = {blocked:.4f}, iid = {iid:.4f}")
    assert abs(blocked - 1.0) <= 0.25
    assert iid < 0.1


def test_block_length_on_the_ar1_series(txm, ar1_series):
    """g = (1 + rho) / (1 - rho) = 19: ten times it lies between 100 and 400."""
    from thermoextrap_amd import timeseries as T

    u, x = ar1_series
    B = T.block_length(u, x[:, None])
    print("timeseries.block_length on the AR(1) series:", B)
    assert isinstance(B, int) and 100 <= B <= 400
    assert T.block_length(u, x[:, None], factor=1.0) < B
    with pytest.raises(ValueError):
        T.block_length(u, x[:, None], factor=0.0)
