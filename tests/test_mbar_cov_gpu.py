"""GPU tests of MBAR's asymptotic error bars: the kernel txm_mbar_cov (txm_mbar_cov.hip) through the C ABI against
long-double sums, the public methods of MBARModel against the dense restatement of tests/test_mbar_cov_cpu.py, and the
asymptotic error against the spread of MBARModel.bootstrap.

Kernel parity.  g comes from the test's CPU solve (ref_solve), logD from txm_mbar_eval at that g, mean from
txm_mbar_predict; every sum is held to |hip - ref| <= 1e-12 * sum_n |term_n| -- the first-order bound of its own sum, the
rule of tests/test_perturb_gpu.py -- with ref the long-double sum at the same g and the same mean.  A weight's relative
error is at most (|exponent| + c) eps with exponents of a few hundred at most here (< 1e-13), and the summation adds eps
times (terms per lane + tree depth).  Every case prints its worst ratio |hip - ref| / sum |term| (run with -s).
What these cases reach of the kernel's paths: NA templates 1 / 2 / 4 / 8 (n_alpha 1, 2, 3, 8), the register (K <= 8) and
LDS (K = 12, 16) forms of the evaluation pass that supplies logD, one row tile of states (K <= 16; at K = 16 a second tile
holds the row of ones alone), C of 1, 3, 17 and 33 (one to three column groups, the column of ones at index 1 or 3 of its
group), a row pitch above C, states of 1 sample, of less than a tile and of several workgroups with a ragged last tile.
They do not reach a state row in a second row tile (K >= 17), the ones at index 15 or alone behind full tiles, two row
tiles together with two column groups, a binding workgroup cap, or a g that is no solution; and logD and the centres come
from two other device kernels.  All of that is group E of tests/test_mbar_kernels_gpu.py, with host-made inputs against
oracle/mbar_oracle.py cov_sums.  The one API-level case above 16 states is
test_api_above_sixteen_states_against_the_dense_restatement below.
"""

import ctypes as ct

import numpy as np
import pytest
import torch

from test_mbar_cov_cpu import (LD, bound, dense_theta, gauss_problem, gram_theta, ref_columns, ref_solve, rel,
                               target_sums)

pytestmark = pytest.mark.gpu
TOL = 1e-12


@pytest.fixture(scope="module")
def eng(txm):
    from thermoextrap_amd import engine

    return engine


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).cuda()


def problem(a0, ns, C, seed, mu=50.0, sd=2.0):
    """Gaussian energies around mu (at alpha: N(mu - sd^2 alpha, sd^2)) and C columns of mixed scale and offset."""
    rng = np.random.default_rng(seed)
    us = [rng.normal(mu - sd * sd * a, sd, n) for a, n in zip(a0, ns)]
    off, slope = rng.normal(0.0, 3.0, C), rng.normal(0.05, 0.02, C)
    xs = [off[None, :] + slope[None, :] * (u[:, None] - mu) + rng.normal(0, 0.3, (len(u), C)) for u in us]
    return us, xs


def device_sums(eng, us, xs, a0, f, targets, pitch=None):
    """(out (n_alpha, 1 + K + C (1 + K)), lnw, mean (n_alpha, C), g, upiv) of txm_mbar_cov through the C ABI."""
    from thermoextrap_amd import _lib

    L = _lib.load()
    K, C = len(us), xs[0].shape[1]
    ud = [dev(u) for u in us]
    if pitch is None:
        xd = [dev(x) for x in xs]
    else:                                   # rows of `pitch` doubles, the first C are the observables
        xd = []
        for x in xs:
            wide = torch.full((len(x), pitch), float("nan"), dtype=torch.float64, device="cuda")
            wide[:, :C] = dev(x)
            xd.append(wide[:, :C])
    tab, keep, ns, C2 = eng._mbar_table(ud, xd)
    assert C2 == C and all(tab[s].ldx_s == (pitch or C) for s in range(K) if ns[s] > 1)
    upiv = eng.mbar_pivot(ud)
    a0 = np.ascontiguousarray(a0, dtype=np.float64)
    g = np.log(ns) + np.asarray(f, dtype=np.float64) - a0 * upiv
    g = np.ascontiguousarray(g - g.max())
    logD = torch.empty(int(ns.sum()), dtype=torch.float64, device="cuda")
    eng.mbar_eval(ud, a0, g, upiv, logD)
    al = np.ascontiguousarray(targets, dtype=np.float64)
    mean = eng.mbar_predict(xd, ud, a0, f, logD, al, upiv=upiv)
    na = len(al)
    width = 1 + K + C * (1 + K)
    out = torch.full((na, width), float("nan"), dtype=torch.float64, device="cuda")
    lnw = torch.full((na,), float("nan"), dtype=torch.float64, device="cuda")
    nbytes = L.txm_mbar_cov_ws_bytes(K, C, na)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    dp = ct.POINTER(ct.c_double)
    rc = L.txm_mbar_cov(tab, K, C, float(upiv), a0.ctypes.data_as(dp), g.ctypes.data_as(dp), eng._ptr(logD),
                        al.ctypes.data_as(dp), na, eng._ptr(mean), eng._ptr(out), eng._ptr(lnw), eng._ptr(ws), nbytes,
                        eng._stream())
    torch.cuda.synchronize()
    assert rc == 0, _lib.last_error()
    del keep
    return out.cpu().numpy(), lnw.cpu().numpy(), mean.cpu().numpy(), g, upiv


def reference_sums(us, xs, a0, g, upiv, targets, mean):
    """Long-double Q, B, yy, b at the log-weights g and the centres `mean`, each with sum_n |term_n|, and ln sum_n v_an."""
    ut = np.concatenate([np.asarray(u, dtype=LD) for u in us]) - LD(upiv)
    x = np.concatenate([np.asarray(v, dtype=LD) for v in xs])
    N = np.array([len(u) for u in us], dtype=LD)
    t = np.asarray(g, dtype=LD)[:, None] - np.asarray(a0, dtype=LD)[:, None] * ut[None, :]
    m = t.max(0)
    e = np.exp(t - m)
    Ws = (e / e.sum(0)).T / N[None, :]                       # (n, K)
    ld = m + np.log(e.sum(0))
    res = []
    for a, mu in zip(targets, mean):
        ex = -LD(a) * ut - ld
        v = np.exp(ex - ex.max())
        wa = v / v.sum()
        d = x - np.asarray(mu, dtype=LD)[None, :]
        Q = (wa * wa).sum()
        B = (Ws * wa[:, None]).sum(0)
        yy = (wa[:, None] ** 2 * d * d).sum(0)
        bt = Ws[:, None, :] * (wa[:, None] * d)[:, :, None]  # (n, C, K)
        res.append({"Q": (Q, Q), "B": (B, B), "yy": (yy, yy), "b": (bt.sum(0), np.abs(bt).sum(0)),
                    "lnw": ex.max() + np.log(v.sum())})
    return res


def unpack(row, K, C):
    rest = row[1 + K:].reshape(C, 1 + K)
    return {"Q": row[0], "B": row[1:1 + K], "yy": rest[:, 0], "b": rest[:, 1:]}


def worst_ratio(out, ref, K, C):
    worst = {}
    for a, r in enumerate(ref):
        got = unpack(out[a], K, C)
        for key in ("Q", "B", "yy", "b"):
            want, scale = r[key]
            assert np.all(np.isfinite(got[key])), (a, key)
            q = np.max(np.abs(np.asarray(got[key], dtype=LD) - want) / scale)
            worst[key] = max(worst.get(key, 0.0), float(q))
    return worst


def spread_targets(a0, n):
    """n targets: one equal to a sampled alpha0, one below and one above the sampled range, the rest inside it."""
    lo, hi = min(a0), max(a0)
    t = [a0[len(a0) // 2], lo - 0.15, hi + 0.15] + list(np.linspace(lo, hi, max(n - 3, 1) + 2)[1:-1])
    return t[:n] if n > 1 else [hi + 0.15]


CASES = [
    # name, alpha0, samples per state, C, n_alpha, row pitch, mean of u
    ("K1_C1_na1", [1.0], [1000], 1, 1, None, 50.0),
    ("K1_C1_na2", [1.0], [333], 1, 2, None, 50.0),
    ("K2_C3_na8", [1.0, 1.2], [1025, 63], 3, 8, None, 50.0),
    ("K3_C1_na3", [1.0, 1.1, 1.2], [1, 37, 1000], 1, 3, None, 50.0),
    ("K8_C17_na8_large_u", list(1.0 + 0.1 * np.arange(8)), [1, 37, 1000, 129, 64, 65, 255, 300], 17, 8, None, 4.0e4),
    ("K12_C33_pitch40_na8", list(1.0 + 0.08 * np.arange(12)), [200 + 37 * k for k in range(12)], 33, 8, 40, 50.0),
    ("K16_C3_na2", list(1.0 + 0.06 * np.arange(16)), [50 + 7 * k for k in range(16)], 3, 2, None, 50.0),
]


@pytest.fixture(scope="module")
def solved():
    """The CPU solve of every case, once."""
    out = {}
    for i, (name, a0, ns, C, na, pitch, mu) in enumerate(CASES):
        us, xs = problem(a0, ns, C, seed=100 + i, mu=mu)
        out[name] = (us, xs, np.asarray(ref_solve(us, a0), dtype=np.float64))
    return out


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_kernel_against_long_double_sums(eng, solved, case):
    name, a0, ns, C, na, pitch, mu = case
    us, xs, f = solved[name]
    K = len(a0)
    targets = spread_targets(a0, na)
    if mu > 1e3:                                                       # unshifted, e^{-alpha u} would overflow
        assert max(targets) * min(u.min() for u in us) > 745.0 * 10
    out, lnw, mean, g, upiv = device_sums(eng, us, xs, a0, f, targets, pitch)
    ref = reference_sums(us, xs, a0, g, upiv, targets, mean)
    worst = worst_ratio(out, ref, K, C)
    print(f"\n{name}: worst |hip - ref| / sum |term|: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for key, v in worst.items():
        assert v <= TOL, (key, v)
    lw = np.array([float(r["lnw"]) for r in ref])
    assert np.max(np.abs(lnw - lw)) <= 1e-12 * max(1.0, np.max(np.abs(lw)))
    # the structure the maths promises: sum_k N_k B_ak = 1 and sum_k N_k b_kac = sum_n W_na d_nc = 0 (mean is predict's)
    N = np.array(ns, dtype=np.float64)
    for a in range(na):
        got = unpack(out[a], K, C)
        assert abs(got["B"] @ N - 1.0) <= 1e-12
        assert np.all(np.abs(got["b"] @ N) <= 1e-12 * np.sqrt(got["yy"] / got["Q"]) + 1e-300)


def test_two_calls_give_the_same_bits(eng, solved):
    name, a0, ns, C, na, pitch, mu = CASES[4]
    us, xs, f = solved[name]
    targets = spread_targets(a0, na)
    a = device_sums(eng, us, xs, a0, f, targets, pitch)
    b = device_sums(eng, us, xs, a0, f, targets, pitch)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_engine_takes_nine_targets_in_two_passes(eng, solved):
    """engine.mbar_cov_sums on 9 targets (8 + 1) against the same long-double sums, at the solution of the engine's own
    solve; the free energy of a target from lnw."""
    name, a0, ns, C, na, pitch, mu = CASES[2]
    us, xs, _ = solved[name]
    K = len(a0)
    ud, xd = [dev(u) for u in us], [dev(x) for x in xs]
    sol = eng.mbar_solve(ud, a0)
    targets = np.linspace(0.9, 1.3, 9)
    means = eng.mbar_predict(xd, ud, a0, sol.f, sol.logD, targets, upiv=sol.upiv)
    Q, B, yy, b, lnw = eng.mbar_cov_sums(xd, ud, a0, sol, targets, means, with_lnw=True)
    assert Q.shape == (9,) and B.shape == (9, K) and yy.shape == (9, C) and b.shape == (9, C, K)
    four = eng.mbar_cov_sums(xd, ud, a0, sol, targets, means)
    assert len(four) == 4 and all(np.array_equal(p, q) for p, q in zip(four, (Q, B, yy, b)))
    g, c = eng.mbar_solution_g(np.array(ns, dtype=np.float64), a0, sol)
    ref = reference_sums(us, xs, a0, g, sol.upiv, targets, means.cpu().numpy())
    packed = np.concatenate([Q[:, None], B, np.concatenate([yy[:, :, None], b], axis=2).reshape(9, -1)], axis=1)
    worst = worst_ratio(packed, ref, K, C)
    print("\nnine targets through the engine: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert max(worst.values()) <= TOL
    # -lnw is the target's free energy in the gauge of sol.f: against the restatement at the CPU solve
    fref = ref_solve(us, a0)
    _, _, lw = ref_columns(us, a0, fref, targets)
    np.testing.assert_allclose(-lnw, -np.asarray(lw, dtype=np.float64), rtol=0, atol=1e-10)


# ---- the public methods -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(txm):
    import thermoextrap_amd as xtrap

    a0, ns = [1.0, 1.25, 1.5], [60, 57, 64]
    us, xs = gauss_problem(a0, ns, C=2, seed=5)
    model = xtrap.MBARModel([xtrap.beta.factory_extrapmodel(beta=b, data=xtrap.factory_data_values(uv=u, xv=x, order=1, central=False))
                             for b, x, u in zip(a0, xs, us)])
    f = ref_solve(us, a0)
    targets = [1.25, 1.1, 1.7, 0.9]
    Ws, Wt, lnw = ref_columns(us, a0, f, targets)
    return {"model": model, "a0": a0, "Ns": np.array(ns, dtype=np.float64), "f": f, "targets": targets, "Ws": Ws, "Wt": Wt,
            "lnw": lnw, "x": np.concatenate(xs).astype(LD)}


def test_api_against_the_dense_restatement(small):
    """predict_with_error, free_energy (both forms), free_energy_covariance, overlap and effective_samples on K = 3,
    about 60 samples per state, C = 2, under the tolerance rule of tests/test_mbar_cov_cpu.py (variances compared)."""
    m, Ws, Wt, Ns, x, targets = small["model"], small["Ws"], small["Wt"], small["Ns"], small["x"], small["targets"]
    K = 3
    dense = dense_theta(Ws, Ns)
    own = rel(gram_theta(Ws, Ns), dense)
    tol = bound(own)
    scale = np.abs(dense).max()
    # sampled states
    th = m.free_energy_covariance()
    print(f"\nrestatement's own {own:.2e}; Theta {rel(th, dense):.2e}")
    assert th.shape == (K, K) and rel(th, dense) <= tol
    f, df = m.free_energy()
    assert f.dims == df.dims == ("beta",) and df.values[0] == 0.0 and f.values[0] == 0.0
    np.testing.assert_array_equal(f.values, m._solution().f)
    np.testing.assert_allclose(f.values, np.asarray(small["f"], dtype=np.float64), rtol=0, atol=1e-10)
    want = np.diag(dense) + dense[0, 0] - 2.0 * dense[0]
    assert np.all(np.abs(df.values ** 2 - want) <= tol * scale)
    ov = m.overlap()
    O = np.asarray(Ws.T @ Ws, dtype=np.float64) * Ns[None, :]
    assert np.abs(ov.matrix - O).max() <= tol and np.abs(ov.matrix.sum(1) - 1.0).max() <= 1e-12
    ev = np.sort(np.linalg.eigvals(O).real)[::-1]
    assert np.abs(ov.eigenvalues - ev).max() <= 1e-10 and abs(ov.scalar - (1.0 - ev[1])) <= 1e-10
    # targets
    mean, err = m.predict_with_error(targets)
    plain = m.predict(targets)
    assert mean.dims == err.dims == plain.dims == ("beta", "val") and err.values.shape == (4, 2)
    assert np.array_equal(mean.values, plain.values)
    np.testing.assert_array_equal(err.coords["beta"], targets)
    ft, dft = m.free_energy(targets)
    neff = m.effective_samples(targets)
    worst = 0.0
    for t, a in enumerate(targets):
        wa = Wt[:, t]
        mu, Q, B, yy, b = target_sums(Ws, wa, x)
        assert abs(neff.values[t] * float(Q) - 1.0) <= tol
        assert abs(ft.values[t] + float(small["lnw"][t])) <= 1e-10
        W1 = np.concatenate([Ws, wa[:, None]], axis=1)
        d1 = dense_theta(W1, np.append(Ns, 0.0))
        o1 = rel(gram_theta(W1, np.append(Ns, 0.0)), d1)
        v1 = d1[K, K] + d1[0, 0] - 2.0 * d1[0, K]
        assert abs(dft.values[t] ** 2 - v1) <= bound(own, o1) * max(v1, np.abs(d1).max())
        for c in range(2):
            Wy = np.concatenate([Ws, (wa * (x[:, c] - mu[c]))[:, None]], axis=1)
            dy = dense_theta(Wy, np.append(Ns, 0.0))[K, K]
            oy = abs(gram_theta(Wy, np.append(Ns, 0.0))[K, K] - dy) / dy
            worst = max(worst, abs(err.values[t, c] ** 2 - dy) / dy)
            assert abs(err.values[t, c] ** 2 - dy) <= bound(own, oy) * dy, (a, c)
    print(f"variance of the averages: worst relative difference from the dense Theta_yy {worst:.2e}")
    # a target at alpha0_k is state k
    k = small["a0"].index(targets[0])
    assert abs(ft.values[0] - f.values[k]) <= 1e-10 and abs(dft.values[0] ** 2 - df.values[k] ** 2) <= tol * scale
    one = m.predict_with_error(1.1)
    assert one[0].values.shape == one[1].values.shape == (1, 2)
    named = m.free_energy([1.1], alpha_name="b")
    assert named[0].dims == named[1].dims == ("b",)


def test_api_above_sixteen_states_against_the_dense_restatement(txm):
    """K = 17 (alpha0 1.0 ... 2.6, 9 to 13 samples per state, 187 pooled: dense_theta takes 200), C = 2: the public methods
    with a state row in the kernel's second row tile.  The restatement's own error is about 4e-15 on this shape, so the bound is
    its 1e-10 floor.  Nothing is asserted on the overlap eigenvalues: the smallest is about 1e-17, numerically zero."""
    import thermoextrap_amd as xtrap

    K = 17
    a0, ns = [1.0 + 0.1 * k for k in range(K)], ([9, 10, 11, 12, 13] * 4)[:K - 2] + [11, 11]
    assert sum(ns) == 187 and min(ns) == 9 and max(ns) == 13
    us, xs = gauss_problem(a0, ns, C=2, seed=17)
    m = xtrap.MBARModel([xtrap.beta.factory_extrapmodel(beta=b, data=xtrap.factory_data_values(uv=u, xv=x, order=1, central=False))
                         for b, x, u in zip(a0, xs, us)])
    fref = ref_solve(us, a0)
    targets = [a0[8], 1.35, 0.9, 2.7]
    Ws, Wt, lnw = ref_columns(us, a0, fref, targets)
    Ns, x = np.array(ns, dtype=np.float64), np.concatenate(xs).astype(LD)
    dense = dense_theta(Ws, Ns)
    own = rel(gram_theta(Ws, Ns), dense)
    tol, scale = bound(own), np.abs(dense).max()
    th = m.free_energy_covariance()
    print(f"\nK = 17: restatement's own {own:.2e}; Theta {rel(th, dense):.2e}")
    assert th.shape == (K, K) and rel(th, dense) <= tol
    f, df = m.free_energy()
    assert df.values[0] == 0.0 and f.values[0] == 0.0
    np.testing.assert_allclose(f.values, np.asarray(fref, dtype=np.float64), rtol=0, atol=1e-10)
    want = np.diag(dense) + dense[0, 0] - 2.0 * dense[0]
    assert np.all(np.abs(df.values ** 2 - want) <= tol * scale)
    mean, err = m.predict_with_error(targets)
    assert np.array_equal(mean.values, m.predict(targets).values) and err.values.shape == (4, 2)
    ft, dft = m.free_energy(targets)
    worst = 0.0
    for t, a in enumerate(targets):
        wa = Wt[:, t]
        mu = target_sums(Ws, wa, x)[0]
        assert abs(ft.values[t] + float(lnw[t])) <= 1e-10
        W1 = np.concatenate([Ws, wa[:, None]], axis=1)
        d1 = dense_theta(W1, np.append(Ns, 0.0))
        o1 = rel(gram_theta(W1, np.append(Ns, 0.0)), d1)
        v1 = d1[K, K] + d1[0, 0] - 2.0 * d1[0, K]
        assert abs(dft.values[t] ** 2 - v1) <= bound(own, o1) * max(v1, np.abs(d1).max())
        for c in range(2):
            Wy = np.concatenate([Ws, (wa * (x[:, c] - mu[c]))[:, None]], axis=1)
            dy = dense_theta(Wy, np.append(Ns, 0.0))[K, K]
            oy = abs(gram_theta(Wy, np.append(Ns, 0.0))[K, K] - dy) / dy
            worst = max(worst, abs(err.values[t, c] ** 2 - dy) / dy)
            assert abs(err.values[t, c] ** 2 - dy) <= bound(own, oy) * dy, (a, c)
    print(f"variance of the averages: worst relative difference from the dense Theta_yy {worst:.2e}")
    assert abs(ft.values[0] - f.values[8]) <= 1e-10 and abs(dft.values[0] ** 2 - df.values[8] ** 2) <= tol * scale


def test_asymptotic_error_matches_the_bootstrap_spread(txm):
    """The one statistical test.  K = 3 overlapping Gaussian states (4000, 3500, 4500 samples), nrep = 400, fixed seed:
    err / std over replicates of MBARBootstrap.predict lies in 1 +- 6 / sqrt(2 * 399) = 1 +- 0.21, six standard errors of
    a standard deviation estimated from 400 Gaussian replicates.  On the CPU, the restated formula against a numpy
    multinomial bootstrap (400 replicates, default_rng(2024)) of the same inputs gave the ratios
    CPU_RATIOS below."""
    import thermoextrap_amd as xtrap

    a0, ns, targets = [1.0, 1.15, 1.3], [4000, 3500, 4500], [1.05, 1.25]
    us, xs = gauss_problem(a0, ns, C=2, seed=11)
    model = xtrap.MBARModel([xtrap.beta.factory_extrapmodel(beta=b, data=xtrap.factory_data_values(uv=u, xv=x, order=1, central=False))
                             for b, x, u in zip(a0, xs, us)])
    _, err = model.predict_with_error(targets)
    rep = model.bootstrap({"nrep": 400, "seed": 20240607}).predict(targets).values        # (2, 400, 2)
    ratio = err.values / rep.std(axis=1, ddof=1)
    print("\nerr / bootstrap std:", np.array2string(ratio, precision=3), " CPU:", CPU_RATIOS)
    half = 6.0 / np.sqrt(2.0 * 399.0)
    assert np.all(np.abs(ratio - 1.0) <= half), ratio


CPU_RATIOS = "[[0.986 0.962] [1.005 0.963]]"   # (target, column); the numpy bootstrap took 1.2 s
