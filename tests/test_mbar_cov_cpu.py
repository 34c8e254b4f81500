"""CPU checks of MBAR's asymptotic covariance (Shirts & Chodera 2008, eq. 8 and appendix D): the host algebra of
engine.mbar_theta / mbar_mean_variance / mbar_overlap against a restatement written here, and the boundary of the new
entry point txm_mbar_cov (header, binding, workspace sizing, argument validation).  pymbar is not available: the paper's
formulas are restated below and shared with tests/test_mbar_cov_gpu.py.

The restatement
    ref_solve      MBAR by self-consistent iteration in long double until max |df| <= 1e-15 (gauge f_0 = 0)
    ref_columns    the weight matrix W: W_nk = e^{f_k - alpha0_k u_n} / D_n of the sampled states, W_na = w_an / sum_n w_an
    dense_theta    the definition Theta = W^T (I_N - W N W^T)^+ W with the N x N pseudo-inverse (N <= 200)
    gram_theta     the same from G = W^T W alone (pymbar's "svd-ew" written on G) -- the form the engine uses
    two_column     pymbar's error of an average: A^2 (Theta_AA + Theta_aa - 2 Theta_aA) with the column W_nA = W_na x_n / A
                   (needs x > 0), which equals Theta_yy of y_n = W_na (x_n - A) because Theta is bilinear in the columns
                   that were not sampled.

Tolerance (relative): max(1e-10, 10 x the disagreement between dense_theta and gram_theta on the same input) -- the
reference's own accuracy, printed by every test (run with -s).  Seen here on Theta of the sampled states: K = 1 0 (Theta is
exactly 0), K = 3 3.9e-15, two states at one alpha0 1.4e-15; with a target column at most 1.7e-15; on the variance of an
average (Theta_yy by Gram and by the two-column form against the dense Theta_yy) 8.4e-13 / 2.2e-12 / 2.7e-13 -- the
two-column form cancels A^2-sized terms -- so the bound is 1e-10 throughout.
"""

import ctypes as ct
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
LD = np.longdouble
PINV_CUT = 1e-12     # the null direction sits at ~1e-16, the smallest true eigenvalue of the cases here above 1e-3


# ---- the restatement ---------------------------------------------------------------------------------------------------
def ref_solve(us, a0, tol=1e-15, max_iter=200000):
    """f (long double, f_0 = 0): f_j <- -ln sum_n e^{-alpha0_j u_n - logD_n(f)} until nothing moves by more than tol.
    Iterated on u - <u> (free energies of order 1 whatever the offset of u) and shifted back at the end."""
    u = np.concatenate([np.asarray(v, dtype=LD) for v in us])
    ubar = u.sum() / len(u)
    u = u - ubar
    N = np.array([len(v) for v in us], dtype=LD)
    a = np.asarray(a0, dtype=LD)
    f = np.zeros(len(us), dtype=LD)
    for _ in range(max_iter):
        t = np.log(N)[:, None] + f[:, None] - a[:, None] * u[None, :]
        m = t.max(0)
        logD = m + np.log(np.exp(t - m).sum(0))
        e = -a[:, None] * u[None, :] - logD[None, :]
        em = e.max(1)
        fn = -(em + np.log(np.exp(e - em[:, None]).sum(1)))
        fn = fn - fn[0]
        done = np.max(np.abs(fn - f)) <= tol
        f = fn
        if done:
            return f + (a - a[0]) * ubar
    raise AssertionError("the self-consistent iteration did not converge")


def ref_logD(us, a0, f):
    u = np.concatenate([np.asarray(v, dtype=LD) for v in us])
    N = np.array([len(v) for v in us], dtype=LD)
    t = np.log(N)[:, None] + np.asarray(f, dtype=LD)[:, None] - np.asarray(a0, dtype=LD)[:, None] * u[None, :]
    m = t.max(0)
    return u, m + np.log(np.exp(t - m).sum(0))


def ref_columns(us, a0, f, targets=()):
    """(Ws (N, K), Wt (N, T), ln sum_n w_an (T,)) in long double."""
    u, logD = ref_logD(us, a0, f)
    a = np.asarray(a0, dtype=LD)
    Ws = np.exp(np.asarray(f, dtype=LD)[None, :] - u[:, None] * a[None, :] - logD[:, None])
    tg = np.asarray(targets, dtype=LD).reshape(-1)
    e = -u[:, None] * tg[None, :] - logD[:, None]
    em = e.max(0) if len(tg) else np.zeros(0, dtype=LD)
    w = np.exp(e - em[None, :])
    return Ws, w / w.sum(0)[None, :], em + np.log(w.sum(0))


def _pinv_sym(A):
    lam, V = np.linalg.eigh(0.5 * (A + A.T))
    keep = lam > PINV_CUT * max(float(np.abs(lam).max()), 1.0)
    return (V[:, keep] / lam[keep]) @ V[:, keep].T


def dense_theta(W, Ncol):
    """Theta = W^T (I_N - W N W^T)^+ W, the N x N definition."""
    W = np.asarray(W, dtype=np.float64)
    assert W.shape[0] <= 200
    A = np.eye(W.shape[0]) - (W * np.asarray(Ncol, dtype=np.float64)[None, :]) @ W.T
    return W.T @ _pinv_sym(A) @ W


def gram_theta(W, Ncol):
    """The same from the Gram matrix: G = V L V^T, S = L^{1/2}, Theta = V S (I - S V^T N V S)^+ S V^T."""
    W = np.asarray(W, dtype=LD)
    G = np.asarray(W.T @ W, dtype=np.float64)
    lam, V = np.linalg.eigh(0.5 * (G + G.T))
    VS = V * np.sqrt(np.clip(lam, 0.0, None))
    A = np.eye(G.shape[0]) - VS.T @ (np.asarray(Ncol, dtype=np.float64)[:, None] * VS)
    return VS @ _pinv_sym(A) @ VS.T


def two_column(Ws, wa, x, Ns):
    """pymbar's variance of A = sum_n W_na x_n (x > 0): A^2 (Theta_AA + Theta_aa - 2 Theta_aA), dense."""
    assert np.all(x > 0)
    A = (wa * x).sum()
    W = np.concatenate([Ws, wa[:, None], (wa * x / A)[:, None]], axis=1)
    K = Ws.shape[1]
    th = dense_theta(W, np.append(Ns, [0.0, 0.0]))
    return float(A) ** 2 * (th[K + 1, K + 1] + th[K, K] - 2.0 * th[K, K + 1])


def target_sums(Ws, wa, x):
    """(mean (C,), Q, B (K,), yy (C,), b (C, K)) of one target in long double: what txm_mbar_cov sums."""
    mean = (wa[:, None] * x).sum(0)
    d = x - mean[None, :]
    return mean, (wa * wa).sum(), (Ws * wa[:, None]).sum(0), (wa[:, None] ** 2 * d * d).sum(0), \
        np.einsum("nk,n,nc->ck", Ws, wa, d)


def rel(a, b, scale=None):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    s = float(np.max(np.abs(b))) if scale is None else float(scale)
    return float(np.max(np.abs(a - b))) / s if s > 0 else float(np.max(np.abs(a - b)))


def gauss_problem(a0, ns, C=2, seed=0):
    """Gaussian energies (at alpha: N(mu - var alpha, var)) and C positive observables tied to them."""
    rng = np.random.default_rng(seed)
    mu, sd = 50.0, 2.0
    us = [rng.normal(mu - sd * sd * a, sd, n) for a, n in zip(a0, ns)]
    xs = [np.stack([5.0 + 0.05 * u + rng.normal(0, 0.1, len(u)), 30.0 + 0.01 * (u - 45.0) ** 2 + rng.normal(0, 0.5, len(u)),
                    2.0 + np.cos(u), 10.0 + rng.normal(0, 1.0, len(u))][:C], axis=1) for u in us]
    return us, xs


CASES = {
    "K1": ([1.0], [100], [1.0, 1.2, 0.7]),
    "K3": ([1.0, 1.25, 1.5], [30, 37, 33], [1.25, 1.1, 1.8]),
    "twin": ([1.0, 1.0, 1.3], [40, 25, 35], [1.0, 1.15, 0.8]),     # two states at one alpha0: G has a repeated column
}


@pytest.fixture(scope="module", params=list(CASES))
def case(request):
    a0, ns, targets = CASES[request.param]
    us, xs = gauss_problem(a0, ns, seed=len(ns) + ns[0])
    f = ref_solve(us, a0)
    Ws, Wt, lnw = ref_columns(us, a0, f, targets)
    Ns = np.array(ns, dtype=np.float64)
    x = np.concatenate(xs).astype(LD)
    own = rel(gram_theta(Ws, Ns), dense_theta(Ws, Ns)) if len(ns) > 1 else float(np.abs(gram_theta(Ws, Ns)).max())
    return {"name": request.param, "a0": a0, "ns": ns, "targets": targets, "Ns": Ns, "Ws": Ws, "Wt": Wt, "x": x, "own": own}


def bound(*own):
    return max(1e-10, 10.0 * max(own))


# ---- the engine's algebra ----------------------------------------------------------------------------------------------
def test_theta_of_the_sampled_states(case):
    """engine.mbar_theta on G_s against the dense definition; symmetric, Theta N 1 = 0; K = 1: Theta_ss = 0."""
    from thermoextrap_amd import engine

    Ws, Ns = case["Ws"], case["Ns"]
    Gs = np.asarray(Ws.T @ Ws, dtype=np.float64)
    got, want = engine.mbar_theta(Gs, Ns), dense_theta(Ws, Ns)
    tol = bound(case["own"])
    print(f"\n{case['name']}: dense vs Gram (the restatement's own) {case['own']:.2e}, engine vs dense "
          f"{rel(got, want) if len(Ns) > 1 else np.abs(got).max():.2e}, bound {tol:.1e}")
    if len(Ns) == 1:
        assert np.abs(want).max() <= 1e-13 / Ns[0] and np.abs(got).max() <= tol / Ns[0]    # Theta_ss = 0 (scale 1 / N)
        return
    scale = np.abs(want).max()
    assert rel(got, want) <= tol
    assert np.abs(got - got.T).max() <= tol * scale
    assert np.abs(got @ Ns).max() <= tol * scale * Ns.sum()


def test_theta_with_a_target_column(case):
    """The (K + 1) x (K + 1) Theta of the Gram blocks G_s, B_a, Q_a -- what free_energy(alpha) uses -- against the dense
    definition, and var(f_a - f_0) from it; a target at a sampled alpha0_k reproduces that state's row."""
    from thermoextrap_amd import engine

    Ws, Ns, K = case["Ws"], case["Ns"], len(case["ns"])
    for t, a in enumerate(case["targets"]):
        W = np.concatenate([Ws, case["Wt"][:, t:t + 1]], axis=1)
        Nc = np.append(Ns, 0.0)
        want = dense_theta(W, Nc)
        G = np.asarray(W.T @ W, dtype=np.float64)
        scale = max(np.abs(want).max(), np.abs(G).max())     # K = 1 with the target at alpha0: Theta is all zeros
        own = rel(gram_theta(W, Nc), want, scale)
        got = engine.mbar_theta(G, Nc)
        tol = bound(case["own"], own)
        print(f"\n{case['name']} target {a}: own {own:.2e}, engine vs dense {rel(got, want, scale):.2e}, bound {tol:.1e}")
        assert rel(got, want, scale) <= tol
        var = lambda th, i: th[i, i] + th[0, 0] - 2.0 * th[0, i]      # noqa: E731
        assert abs(var(got, K) - var(want, K)) <= tol * max(var(want, K), scale)
        if a in case["a0"]:
            k = case["a0"].index(a)
            assert abs(var(got, K) - var(got, k)) <= tol * scale


def test_mean_variance_is_the_dense_theta_yy_and_pymbars_two_column_form(case):
    """engine.mbar_mean_variance (K x K work) against Theta_yy of the dense definition and against pymbar's
    A^2 (Theta_AA + Theta_aa - 2 Theta_aA).  K = 1: G = 1 / N and b = 0 exactly, so the closed form N b^2 / (1 - N G) is 0 / 0
    -- the pseudo-inverse makes the term 0 and the variance is yy, the single-state perturbation (ratio estimator) error."""
    from thermoextrap_amd import engine

    Ws, Ns, x, K = case["Ws"], case["Ns"], case["x"], len(case["ns"])
    Gs = np.asarray(Ws.T @ Ws, dtype=np.float64)
    pinv = engine.mbar_reduced_pinv(Gs, Ns)
    worst = 0.0
    for t, a in enumerate(case["targets"]):
        wa = case["Wt"][:, t]
        mean, Q, B, yy, b = target_sums(Ws, wa, x)
        got = engine.mbar_mean_variance(Gs, Ns, np.asarray(yy, dtype=np.float64), np.asarray(b, dtype=np.float64))
        again = engine.mbar_mean_variance(Gs, Ns, np.asarray(yy, dtype=np.float64), np.asarray(b, dtype=np.float64), pinv=pinv)
        assert np.array_equal(got, again) and got.shape == (x.shape[1],)
        for c in range(x.shape[1]):
            y = wa * (x[:, c] - mean[c])
            W = np.concatenate([Ws, y[:, None]], axis=1)
            Nc = np.append(Ns, 0.0)
            dense = dense_theta(W, Nc)[K, K]
            own = abs(gram_theta(W, Nc)[K, K] - dense) / dense
            pym = two_column(Ws, wa, x[:, c], Ns)
            tol = bound(case["own"], own, abs(pym - dense) / dense)
            worst = max(worst, own, abs(pym - dense) / dense)
            assert abs(got[c] - dense) <= tol * dense, (a, c, got[c], dense)
            assert abs(got[c] - pym) <= tol * pym, (a, c, got[c], pym)
            if K == 1:
                assert np.abs(pinv).max() == 0.0 and abs(float(b[c, 0])) <= 1e-15 * float(np.abs(y).sum())
                assert got[c] == float(yy[c])
    print(f"\n{case['name']}: the restatement's own disagreement over targets and columns {worst:.2e}")


def test_overlap_rows_sum_to_one(case):
    from thermoextrap_amd import engine
    from thermoextrap_amd.models import MBARModel, MBAROverlap

    Ws, Ns = case["Ws"], case["Ns"]
    Gs = np.asarray(Ws.T @ Ws, dtype=np.float64)
    O, ev, scalar = engine.mbar_overlap(Gs, Ns)
    np.testing.assert_allclose(O.sum(1), 1.0, rtol=0, atol=1e-12)
    assert np.all(np.diff(ev) <= 0) and abs(ev[0] - 1.0) <= 1e-12 and np.all(ev >= -1e-12)
    assert scalar == (1.0 - ev[1] if len(Ns) > 1 else 1.0) and 0.0 <= scalar <= 1.0
    np.testing.assert_allclose(np.sort(np.linalg.eigvals(O).real)[::-1], ev, rtol=0, atol=1e-12)

    class Stub(MBARModel):           # the public method over the same Gram matrix, without a device
        def __init__(self):
            self._cache = {"mbar_gram": Gs}

        def _counts(self):
            return Ns

    res = Stub().overlap()
    assert isinstance(res, MBAROverlap) and np.array_equal(res.matrix, O) and res.scalar == scalar
    np.testing.assert_allclose(res.matrix.sum(1), 1.0, rtol=0, atol=1e-12)
    th = Stub().free_energy_covariance()
    assert np.array_equal(th, engine.mbar_theta(Gs, Ns))


# ---- the boundary ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from thermoextrap_amd import _build, _lib

    _build.build_library()
    return _lib.load()


def test_header_binding_and_integration_notes_agree():
    """The argument list of txm_mbar_cov is the same in include/txmom.h, in INTEGRATION.md and (by count and kind) in the
    ctypes binding."""
    from thermoextrap_amd import _lib

    def proto(text, name):
        m = re.search(rf"\b(?:int|size_t)\s+{name}\s*\((.*?)\)\s*;", text, re.S)
        assert m, name
        return [" ".join(a.split()) for a in m.group(1).split(",")]

    hdr = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "txmom.h").read_text(), flags=re.S)
    doc = (ROOT / "INTEGRATION.md").read_text()
    for name in ("txm_mbar_cov", "txm_mbar_cov_ws_bytes"):
        args = proto(hdr, name)
        assert proto(doc, name) == args, name
        res, argtypes = _lib.SIGNATURES[name]
        assert len(argtypes) == len(args)
        for a, t in zip(args, argtypes):
            if "*" in a or a.startswith("txm_stream "):
                assert t in (ct.c_void_p, ct.POINTER(ct.c_double), ct.POINTER(_lib.MbarState)), a
            else:
                kind = {"double": ct.c_double, "int32_t": ct.c_int32, "int64_t": ct.c_int64, "size_t": ct.c_size_t}
                assert t is kind[a.split()[0]], a


def test_ws_bytes_and_validation_without_a_device(lib):
    from thermoextrap_amd import _lib

    for bad in ((0, 1, 1), (65, 1, 1), (2, 0, 1), (2, 65536, 1), (2, 1, 0), (2, 1, 9)):
        assert lib.txm_mbar_cov_ws_bytes(*bad) == 0, bad
    # about num_cus * 8 workgroups of 8 * 17 * 16 partial sums each, whatever the shape
    for ok in ((1, 1, 1), (3, 1, 1), (3, 33, 8), (12, 17, 8), (64, 33, 8), (64, 65535, 8)):
        assert lib.txm_mbar_cov_ws_bytes(*ok) >= 8 * 17 * 16 * 8 * ok[0] * (ok[1] // 16 + 1) * (ok[0] // 16 + 1), ok

    def states(K, n=100, C=4):
        tab = (_lib.MbarState * max(K, 1))()
        for s in range(max(K, 1)):
            tab[s].x, tab[s].u, tab[s].n, tab[s].ldx_s = 0x10000, 0x20000, n, C     # never dereferenced: refused first
        return tab

    d = (ct.c_double * 65)()
    p = ct.c_void_p(0x30000)

    def cov(tab, K, C=4, na=1, ws_bytes=1 << 40, a0=d, mean=p):
        return lib.txm_mbar_cov(tab, K, C, 0.0, a0, d, p, d, na, mean, p, None, p, ws_bytes, None)

    def refused(rc, words, status=-1):
        assert rc == status, (rc, _lib.last_error())
        assert all(w in _lib.last_error() for w in words), _lib.last_error()

    refused(cov(None, 2), ["mbar_cov", "null state table"])
    refused(cov(states(1), 0), ["K = 0"])
    refused(cov(states(65), 65), ["K = 65"])
    tab = states(3)
    tab[1].n = 0
    refused(cov(tab, 3), ["state 1", "n = 0"])
    tab = states(2)
    tab[1].x = None
    refused(cov(tab, 2), ["state 1", "null u or x"])
    refused(cov(states(2), 2, C=5), ["ldx_s = 4 < C = 5"])
    refused(cov(states(2), 2, C=0), ["C = 0"])
    refused(cov(states(2), 2, na=0), ["n_alpha = 0"])
    refused(cov(states(2), 2, na=9), ["n_alpha = 9"])
    refused(cov(states(2), 2, a0=None), ["null pointer"])
    refused(cov(states(2), 2, mean=None), ["null pointer"])
    bad = (ct.c_double * 65)()
    bad[1] = float("nan")
    refused(cov(states(2), 2, a0=bad), ["state 1 not finite"])
    refused(cov(states(2), 2, ws_bytes=16), ["workspace too small"], status=-3)
