"""The public ``block=`` methods of MBARModel on the device against the self-contained long-double restatement
tests/_mbar_block_ref.py (its own weighted-MBAR solve, its own sums, its own coefficient vectors): K = 3 overlapping
Gaussian states of about 4000 correlated records.

Tolerance: every blocked variance and covariance to 1e-10 sqrt(V_ii V_jj).  What separates the two sides is (a) the
device solve, converged to 1e-12 of N_k in the gradient against 1e-17 in the restatement: a relative change of the
weights of about 1e-13; (b) the pseudo-inverse, float64 on both sides, whose error is eps times the condition of
I - sqrt(N) G_s sqrt(N) on its range (below 100 here); (c) float64 against long-double sums, measured by
``test_float64_restatement_against_long_double`` below (printed; 4.1e-15 here).  1e-10 leaves three digits over their sum
(worst deviation seen on the card: 1.0e-13, on the free energies).  The identities between the methods (diagonal of the covariance against the error bar, cross_alpha
blocks) hold to 1e-12: they are different summation orders of the same products.

The two statistical checks of tests/test_mbar_block_cpu.py run here through the device path.
"""

import numpy as np
import pytest

import _mbar_block_ref as br
from test_mbar_block_cpu import A0, AR1_SEED, IID_SEED, TARGETS

pytestmark = pytest.mark.gpu
LD = np.longdouble
NS = [4000, 3777, 4100]
BLOCK = 50
_cache = {}


def make_model(a0, us, xs):
    import thermoextrap_amd as xtrap

    return xtrap.MBARModel([xtrap.beta.factory_extrapmodel(beta=b, data=xtrap.factory_data_values(uv=u, xv=x, order=1, central=False))
                            for b, x, u in zip(a0, xs, us)])


@pytest.fixture(scope="module")
def prob(txm):
    us, xs = br.ar1_states(NS, A0, 0.5, seed=21, C=2)
    targets = TARGETS + [A0[1]]                               # the last target is a sampled state
    return dict(us=us, xs=xs, targets=targets, model=make_model(A0, us, xs), ref=br.model(us, xs, A0, targets))


def ref_gamma(prob, block, n_levels=1):
    key = (id(prob["ref"]), str(block), n_levels)
    if key not in _cache:
        m = prob["ref"]
        _cache[key] = br.gammas(m.t, m.kappa, NS, block, n_levels)
    return _cache[key]


def worst(got, want):
    """max |got - want| / sqrt(want_ii want_jj) of two covariance matrices (the entries with a zero scale must be equal)."""
    want = np.asarray(want, dtype=LD)
    sc = np.sqrt(np.outer(np.diag(want), np.diag(want)))
    d = np.abs(np.asarray(got, dtype=LD) - want)
    assert not np.any(d[sc == 0])
    return float(np.max(d[sc > 0] / sc[sc > 0])) if np.any(sc > 0) else 0.0


def test_float64_restatement_against_long_double(prob):
    """The restatement's own float64 / long-double disagreement on l^T Gamma l: what the 1e-10 of the device tests is a
    margin over."""
    m = prob["ref"]
    L = np.concatenate([m.L_mean, m.L_sampled, m.L_target])
    want = br.quad(ref_gamma(prob, BLOCK).gamma[0], L)
    t64 = np.asarray(m.t, dtype=np.float64)
    bounds = br.block_bounds(NS, BLOCK)
    T = np.add.reduceat(t64, [lo for _, lo, _ in bounds], axis=0)
    st = np.array([s for s, _, _ in bounds])
    ln = np.array([hi - lo for _, lo, hi in bounds], dtype=np.float64)
    for s in range(3):
        T[st == s] -= (ln[st == s] / NS[s])[:, None] * T[st == s].sum(axis=0)[None, :]
    L64 = np.asarray(L, dtype=np.float64)
    dev = worst(L64 @ (T.T @ T) @ L64.T, want)
    print(f"\nfloat64 restatement against long double: {dev:.2e} of sqrt(V_ii V_jj)")
    assert dev < 1e-11


def test_predict_with_error_and_covariance_against_the_restatement(prob):
    m, ref, targets = prob["model"], prob["ref"], prob["targets"]
    na, C = len(targets), 2
    V = br.quad(ref_gamma(prob, BLOCK).gamma[0], ref.L_mean)
    mean0 = m.predict(targets).values
    mean, err = m.predict_with_error(targets, block=BLOCK)
    assert np.array_equal(mean.values, mean0), "the means are not predict's bits"
    assert mean.dims == err.dims and err.values.shape == (na, C)
    var = err.values.reshape(-1) ** 2
    dev = float(np.max(np.abs(var.astype(LD) - np.diag(V)) / np.diag(V)))
    mean_c, cov = m.predict_with_covariance(targets, block=BLOCK)
    mean_x, full = m.predict_with_covariance(targets, cross_alpha=True, block=BLOCK)
    assert np.array_equal(mean_c.values, mean0) and np.array_equal(mean_x.values, mean0)
    assert cov.values.shape == (na, C, C) and full.values.shape == (na, C, na, C)
    F = full.values.reshape(na * C, na * C)
    dev_full = worst(F, V)
    print(f"\nblock = {BLOCK}: worst deviation from the restatement: variance {dev:.2e}, cross-target covariance {dev_full:.2e}")
    assert dev <= 1e-10 and dev_full <= 1e-10
    assert np.array_equal(F, F.T) and np.array_equal(cov.values, np.swapaxes(cov.values, -1, -2))
    # the diagonal is the error bar squared; the a = a' blocks of the cross form are the plain form
    diag = np.einsum("acc->ac", cov.values).reshape(-1)
    assert np.max(np.abs(diag - var) / var) <= 1e-12
    for a in range(na):
        blk = F[a * C:(a + 1) * C, a * C:(a + 1) * C]
        sc = np.sqrt(np.outer(np.diag(blk), np.diag(blk)))
        assert np.max(np.abs(blk - cov.values[a]) / sc) <= 1e-12


def test_free_energies_against_the_restatement(prob):
    m, ref, targets = prob["model"], prob["ref"], prob["targets"]
    g = ref_gamma(prob, BLOCK).gamma[0]
    Vs, Vt = br.quad(g, ref.L_sampled), br.quad(g, ref.L_target)
    f0, df0 = m.free_energy()
    f, df = m.free_energy(block=BLOCK)
    assert np.array_equal(f.values, f0.values) and df.values[0] == 0.0
    dev_s = float(np.max(np.abs((df.values[1:] ** 2).astype(LD) - np.diag(Vs)[1:]) / np.diag(Vs)[1:]))
    cov = m.free_energy_covariance(block=BLOCK)
    assert cov.shape == (3, 3) and not cov[0].any() and not cov[:, 0].any() and np.array_equal(cov, cov.T)
    dev_c = worst(cov[1:, 1:], Vs[1:, 1:])
    assert np.max(np.abs(np.diag(cov)[1:] - df.values[1:] ** 2) / np.diag(cov)[1:]) <= 1e-12
    ft0, _ = m.free_energy(targets)
    ft, dft = m.free_energy(targets, block=BLOCK)
    assert np.array_equal(ft.values, ft0.values), "f of the targets is not the unblocked call's bits"
    dev_t = float(np.max(np.abs((dft.values ** 2).astype(LD) - np.diag(Vt)) / np.diag(Vt)))
    print(f"\nfree energies, block = {BLOCK}: sampled {dev_s:.2e}, their covariance {dev_c:.2e}, targets {dev_t:.2e}")
    assert dev_s <= 1e-10 and dev_c <= 1e-10 and dev_t <= 1e-10
    # a target on a sampled alpha0 is that state
    assert abs(ft.values[-1] - f.values[1]) <= 1e-8 * max(1.0, abs(f.values[1]))
    assert abs(dft.values[-1] - df.values[1]) <= 1e-8 * df.values[1]


def test_blocking_curve_against_the_restatement(prob):
    m, ref, targets = prob["model"], prob["ref"], prob["targets"]
    var, lengths, counts = m.blocking_curve(targets, BLOCK)
    nl = var.values.shape[0]
    assert nl == 7 and var.dims[0] == "level" and var.values.shape == (nl, len(targets), 2)
    g = ref_gamma(prob, BLOCK, nl)
    assert np.array_equal(counts, g.nblocks) and list(counts[0]) == [80, 76, 82] and list(counts[-1]) == [2, 2, 2]
    assert np.array_equal(lengths, BLOCK * (2 ** np.arange(nl))[:, None] * np.ones(3, dtype=np.int64)[None, :])
    dev = 0.0
    for l in range(nl):
        want = np.diag(br.quad(g.gamma[l], ref.L_mean))
        dev = max(dev, float(np.max(np.abs(var.values[l].reshape(-1).astype(LD) - want) / want)))
    print(f"\nblocking curve, {nl} levels: worst deviation from the restatement {dev:.2e}")
    assert dev <= 1e-10
    _, err = m.predict_with_error(targets, block=BLOCK)
    assert np.max(np.abs(var.values[0] - err.values ** 2) / var.values[0]) <= 1e-12


def test_per_state_blocks_from_block_lengths_end_to_end(prob):
    from thermoextrap_amd import timeseries

    m, ref, targets = prob["model"], prob["ref"], prob["targets"]
    blocks = timeseries.block_lengths(prob["us"], prob["xs"])
    assert len(blocks) == 3 and all(isinstance(b, int) and b >= 1 for b in blocks)
    _, err = m.predict_with_error(targets, block=blocks)
    want = np.diag(br.quad(br.gammas(ref.t, ref.kappa, NS, blocks).gamma[0], ref.L_mean))
    dev = float(np.max(np.abs((err.values.reshape(-1) ** 2).astype(LD) - want) / want))
    print(f"\nblock = timeseries.block_lengths(...) = {blocks}: worst deviation {dev:.2e}")
    assert dev <= 1e-10
    _, one = m.predict_with_error(targets, block=[blocks[0]] * 3)
    _, same = m.predict_with_error(targets, block=blocks[0])
    assert np.array_equal(one.values, same.values)
    with pytest.raises(ValueError, match="one entry per state"):
        m.predict_with_error(targets, block=blocks[:2])
    with pytest.raises(TypeError):
        m.predict_with_error(targets, block=2.5)
    with pytest.raises(ValueError):
        m.predict_with_error(targets, block=0)


def test_more_than_eight_targets_go_in_slabs(prob):
    m = prob["model"]
    targets = list(np.linspace(0.95, 1.3, 11))
    ref = br.model(prob["us"], prob["xs"], A0, targets)
    want = np.diag(br.quad(br.gammas(ref.t, ref.kappa, NS, BLOCK).gamma[0], ref.L_mean))
    mean, err = m.predict_with_error(targets, block=BLOCK)
    assert np.array_equal(mean.values, m.predict(targets).values)
    assert float(np.max(np.abs((err.values.reshape(-1) ** 2).astype(LD) - want) / want)) <= 1e-10
    _, cov = m.predict_with_covariance(targets, block=BLOCK)
    assert cov.values.shape == (11, 2, 2)
    assert np.max(np.abs(np.einsum("acc->ac", cov.values) - err.values ** 2) / err.values ** 2) <= 1e-12
    f, df = m.free_energy(targets, block=BLOCK)
    wt = np.diag(br.quad(br.gammas(ref.t, ref.kappa, NS, BLOCK).gamma[0], ref.L_target))
    assert float(np.max(np.abs((df.values ** 2).astype(LD) - wt) / wt)) <= 1e-10
    with pytest.raises(ValueError, match="8"):
        m.predict_with_covariance(targets, cross_alpha=True, block=BLOCK)


def test_block_none_is_unchanged_in_bits(prob):
    """The default path is the code it was: the same engine calls in the same order give the same bits, before and after
    blocked calls on the same model."""
    from thermoextrap_amd import engine

    m, targets = prob["model"], prob["targets"]
    us, xs, _, cshape = m._samples()
    sol = m._solution()
    avals = np.asarray(targets, dtype=float)
    means = engine.mbar_predict(xs, us, m.alpha0, sol.f, sol.logD, avals, upiv=sol.upiv)
    _, _, yy, b = engine.mbar_cov_sums(xs, us, m.alpha0, sol, avals, means)
    var = engine.mbar_mean_variance(m._gram(), m._counts(), yy, b, pinv=m._reduced_pinv())
    mean, err = m.predict_with_error(targets)
    assert np.array_equal(mean.values, means.cpu().numpy()) and np.array_equal(err.values, np.sqrt(np.clip(var, 0.0, None)))
    gram, b2 = engine.mbar_cross_cov_sums(xs, us, m.alpha0, sol, avals, means)
    cov = engine.mbar_mean_covariance(m._gram(), m._counts(), gram, b2, pinv=m._reduced_pinv())
    assert np.array_equal(m.predict_with_covariance(targets)[1].values, cov)
    th = engine.mbar_theta(m._gram(), m._counts())
    assert np.array_equal(m.free_energy_covariance(), th)
    before = [m.free_energy()[1].values, m.free_energy(targets)[1].values, m.free_energy(targets)[0].values]
    m.predict_with_error(targets, block=7)
    m.free_energy(targets, block=7)
    m.free_energy_covariance(block=7)
    after = [m.free_energy()[1].values, m.free_energy(targets)[1].values, m.free_energy(targets)[0].values]
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    assert np.array_equal(m.predict_with_error(targets)[1].values, err.values)
    assert np.array_equal(m.predict_with_error(targets, block=None)[1].values, err.values)


def test_statistics_through_the_device_path(txm):
    ns = [4000, 4000, 4000]
    us, xs = br.ar1_states(ns, A0, 0.0, seed=IID_SEED, C=1)
    m = make_model(A0, us, xs)
    theta = m.predict_with_error(TARGETS)[1].values ** 2
    one = m.predict_with_error(TARGETS, block=1)[1].values ** 2
    print("\niid 3 x 4000 on the device: block = 1 / Theta form", (one / theta).reshape(-1))
    assert np.all(np.abs(one / theta - 1) < 0.05)
    us, xs = br.ar1_states(ns, A0, 0.8, seed=AR1_SEED, C=1)
    m = make_model(A0, us, xs)
    theta = m.predict_with_error(TARGETS)[1].values ** 2
    blocked = m.predict_with_error(TARGETS, block=50)[1].values ** 2
    print("AR(1) phi = 0.8, B = 50 on the device: blocked / Theta form", (blocked / theta).reshape(-1))
    assert np.all((blocked / theta > 5) & (blocked / theta < 11))


def test_a_state_with_one_block_adds_nothing(prob):
    m, targets = prob["model"], prob["targets"]
    _, err = m.predict_with_error(targets, block=[5000, 5000, 5000])
    assert not err.values.any()
    _, a = m.predict_with_error(targets, block=[BLOCK, 3777, BLOCK])
    _, b = m.predict_with_error(targets, block=[BLOCK, 4000, BLOCK])          # above n_s: the whole state, the same blocks
    assert np.array_equal(a.values, b.values) and a.values.all()
