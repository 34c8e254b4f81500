"""``PerturbModel.predict_with_error`` / ``effective_samples`` / ``free_energy`` / ``blocking_curve``: the
labelled layer over ``engine.perturb_cov``.  The kernels are checked in test_perturb_cov_gpu.py and the estimator in
test_perturb_cov_cpu.py; here: values bit for bit ``predict``'s, dims and coords, the std against the model's own
bootstrap, the free energy and n_eff against the float64 formulas, the curve's shapes, and the refusal of a resampled
model."""

import numpy as np
import pytest

from tests import _perturb_cov_ref as pcr

pytestmark = pytest.mark.gpu

BETA0, DA = 0.5, 0.3
N, C = 20000, 3


@pytest.fixture(scope="module")
def case(txm):
    from thermoextrap_amd.xrlite import DataArray

    rng = np.random.default_rng(2024)
    x, u = pcr.make_data(rng, N, C)
    pm = txm.beta.factory_perturbmodel(BETA0, uv=DataArray(u, "rec"), xv=DataArray(x, ("rec", "val")))
    return pm, x, u, pcr.perturb_cov(x, u, [DA, -0.2, 0.0])


def test_predict_with_error_is_predict_and_matches_the_reference(case):
    pm, x, u, ref = case
    betas = BETA0 + np.array([DA, -0.2, 0.0])
    val, std = pm.predict_with_error(betas)
    pred = pm.predict(betas)
    assert val.dims == std.dims == pred.dims == ("beta", "val")
    assert np.array_equal(val.values, pred.values) and np.array_equal(val.coords["beta"], betas)
    assert np.array_equal(std.coords["beta"], betas)
    bound = 1e-12 * (ref.var_bound[0] + 2.0 * ref.S * ref.zP[0])
    assert np.all(np.abs(std.values**2 - ref.var[0]) <= bound + 4e-16 * ref.var[0])     # (sqrt and square: 2 eps)
    # a scalar alpha drops the axis, as predict does
    v0, s0 = pm.predict_with_error(BETA0 + DA)
    assert v0.dims == s0.dims == pm.predict(BETA0 + DA).dims == ("val",)
    assert np.array_equal(v0.values, pred.values[0]) and np.array_equal(s0.values, std.values[0])
    # another alpha name
    v1, s1 = pm.predict_with_error(betas[:2], alpha_name="b")
    assert v1.dims == s1.dims == ("b", "val") and np.array_equal(s1.values, std.values[:2])
    # more alphas than one pass holds
    many = BETA0 + np.linspace(-0.3, 0.3, 11)
    vm, sm = pm.predict_with_error(many)
    assert np.array_equal(vm.values, pm.predict(many).values) and sm.shape == (11, C) and np.all(sm.values > 0)


def test_multi_dimensional_xv(txm):
    from thermoextrap_amd.xrlite import DataArray

    rng = np.random.default_rng(1)
    x, u = pcr.make_data(rng, 3001, 6)
    flat = txm.beta.factory_perturbmodel(BETA0, uv=DataArray(u, "rec"), xv=DataArray(x, ("rec", "val")))
    cube = txm.beta.factory_perturbmodel(BETA0, uv=DataArray(u, "rec"), xv=DataArray(x.reshape(3001, 2, 3), ("rec", "p", "q")))
    betas = [0.4, 0.8]
    v, s = cube.predict_with_error(betas)
    vf, sf = flat.predict_with_error(betas)
    assert v.dims == s.dims == cube.predict(betas).dims == ("beta", "p", "q") and s.shape == (2, 2, 3)
    assert np.array_equal(v.values, cube.predict(betas).values)
    assert np.array_equal(s.values.reshape(2, 6), sf.values) and np.array_equal(v.values.reshape(2, 6), vf.values)
    curve, lengths, counts = cube.blocking_curve(betas, 100)
    assert curve.dims == ("level", "beta", "p", "q") and curve.shape == (len(lengths), 2, 2, 3)
    # 1-D xv
    one = txm.beta.factory_perturbmodel(BETA0, uv=DataArray(u, "rec"), xv=DataArray(x[:, 0], "rec"))
    v1, s1 = one.predict_with_error(betas)
    assert v1.dims == s1.dims == ("beta",) and np.array_equal(v1.values, one.predict(betas).values)
    assert one.predict_with_error(0.8)[1].dims == ()


def test_std_against_the_models_own_bootstrap(case):
    """``resample(nrep=400)`` -> ``predict`` -> std over rep: the ratio of the two stds has relative standard error
    1 / sqrt(2 * 399); the bound is 5 of them."""
    pm, x, u, ref = case
    _, std = pm.predict_with_error(BETA0 + DA)
    boot = pm.resample(sampler={"nrep": 400, "seed": 0}).predict(BETA0 + DA)
    assert boot.dims == ("rep", "val")
    ratio = boot.values.std(axis=0, ddof=1) / std.values
    print(f"bootstrap(400) / delta std: {ratio}")
    assert np.all(np.abs(ratio - 1.0) <= 5.0 / np.sqrt(2.0 * 399.0)), ratio


def test_free_energy_and_effective_samples(case):
    pm, x, u, ref = case
    betas = BETA0 + np.array([DA, -0.2, 0.0])
    f, df = pm.free_energy(betas)
    neff = pm.effective_samples(betas)
    assert f.dims == df.dims == neff.dims == ("beta",) and np.array_equal(neff.coords["beta"], betas)
    want_f, want_neff = [], []
    for d in betas - BETA0:
        uref = u.min() if d >= 0 else u.max()
        w = np.exp(-d * (u - uref))
        want_f.append(-(np.log(w.mean()) - d * uref))
        want_neff.append(w.sum() ** 2 / (w * w).sum())
    np.testing.assert_allclose(f.values, want_f, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(neff.values, want_neff, rtol=1e-12)
    np.testing.assert_allclose(df.values[:2] ** 2, 1.0 / np.array(want_neff[:2]) - 1.0 / N, rtol=1e-11)
    assert f.values[2] == 0.0 and df.values[2] <= 1e-9 and neff.values[2] == N        # alpha0 itself
    assert np.all(np.abs(f.values + ref.lnq) <= 1e-12 * ref.kbar * (1 + np.abs(ref.lnq)))
    # scalar alpha; the blocked form
    f0, df0 = pm.free_energy(BETA0 + DA)
    assert f0.dims == df0.dims == () and float(f0.values) == f.values[0] and float(df0.values) == df.values[0]
    assert pm.effective_samples(BETA0 + DA).dims == ()
    fb, dfb = pm.free_energy(betas, block=100)
    refb = pcr.perturb_cov(x, u, betas - BETA0, block=100)
    np.testing.assert_allclose(fb.values, f.values, rtol=1e-12, atol=1e-12)
    assert np.all(np.abs(dfb.values**2 - refb.var_lnq[0]) <= 1e-12 * refb.var_lnq_bound[0] + 4e-16 * refb.var_lnq[0])


def test_blocking_curve(case):
    pm, x, u, ref = case
    betas = BETA0 + np.array([DA, -0.2])
    B = 64
    curve, lengths, counts = pm.blocking_curve(betas, B)
    nlev = len(lengths)
    assert np.array_equal(lengths, B * 2 ** np.arange(nlev)) and np.array_equal(counts, -(-N // lengths))
    assert counts[-1] >= 2 and -(-N // (2 * lengths[-1])) < 2
    assert curve.dims == ("level", "beta", "val") and curve.shape == (nlev, 2, C)
    assert np.array_equal(curve.coords["level"], lengths)
    _, std = pm.predict_with_error(betas, block=B)
    assert np.array_equal(np.sqrt(curve.values[0]), std.values)                      # the same block sums, the same bits
    for l in (1, nlev - 1):
        _, s = pm.predict_with_error(betas, block=int(lengths[l]))
        np.testing.assert_allclose(np.sqrt(curve.values[l]), s.values, rtol=1e-12)
    refc = pcr.perturb_cov(x, u, betas - BETA0, block=B, n_levels=nlev)
    assert np.all(np.abs(curve.values - refc.var) <= 1e-12 * (refc.var_bound + 2.0 * refc.S[None] * refc.zP))
    c0, _, _ = pm.blocking_curve(BETA0 + DA, B)
    assert c0.dims == ("level", "val")
    np.testing.assert_allclose(c0.values, curve.values[:, 0], rtol=1e-12)            # (another kernel instance: one alpha)
    with pytest.raises(TypeError):
        pm.blocking_curve(betas, 64.0)
    with pytest.raises(ValueError):
        pm.blocking_curve(betas, N)                                                   # fewer than two blocks
    with pytest.raises(TypeError):
        pm.predict_with_error(betas, block=2.5)


def test_a_resampled_model_is_refused(case):
    pm = case[0]
    rs = pm.resample(sampler={"nrep": 4, "seed": 1})
    for call in (lambda: rs.predict_with_error(0.6), lambda: rs.effective_samples(0.6), lambda: rs.free_energy(0.6),
                 lambda: rs.blocking_curve(0.6, 10)):
        with pytest.raises(NotImplementedError, match="PerturbModel it was resampled from"):
            call()
    assert rs.predict(0.6).dims == ("rep", "val")                                     # predict itself is untouched
