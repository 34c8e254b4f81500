"""symbolic.influence_coefs: the empirical influence functions psi_k of the beta derivatives of <x>, checked on
the CPU in long double against derivatives with respect to the sample weights of the independent oracle
(oracle/derivs_oracle.py), against each other (central / raw form) and against a numpy multinomial bootstrap."""

from __future__ import annotations

import math

import numpy as np
import pytest

from oracle import derivs_oracle as DO
from tests._influence_ref import LD, cov_ld, ld_moments, make_data, psi_ld, series_for

from thermoextrap_amd import symbolic as S

ORDER = 4
CASES = [(c, m) for c in (True, False) for m in (False, True)]


@pytest.fixture(scope="module")
def data200():
    x, u, w = make_data(200, seed=0)
    p, dx, du, mom = ld_moments(x, u, w, ORDER)
    return dict(x=x, u=u, w=w, p=p, dx=dx, du=du, mom=mom)


def _psi(d, central, minus_log, order=ORDER):
    a, b = S.influence_coefs(series_for(central), order, d["mom"], minus_log=minus_log)
    assert a.shape == b.shape == (order + 1, order + 1)
    return psi_ld(a, b, d["dx"], d["du"])


def _oracle_derivs(x, u, w, order, minus_log):
    ru, rxu = DO.raw_moments(x, u, order, w)
    j = DO.average_jet(rxu, ru, order)
    return DO.jet_minus_log(j) if minus_log else j     # long double throughout


@pytest.mark.parametrize("central,minus_log", CASES)
def test_zero_mean(data200, central, minus_log):
    psi, p = _psi(data200, central, minus_log), data200["p"]
    for k in range(ORDER + 1):
        assert abs((p * psi[k]).sum()) <= 1e-13 * (p * np.abs(psi[k])).sum(), k


@pytest.mark.parametrize("central,minus_log", CASES)
def test_psi_is_the_weight_derivative(data200, central, minus_log):
    """psi_k(n) = W d d_k / d w_n, the oracle's derivative by central differences in long double, step 1e-6 w_n."""
    d = data200
    psi = _psi(d, central, minus_log)
    x, u = np.asarray(d["x"], LD), np.asarray(d["u"], LD)
    w = np.asarray(d["w"], LD)
    W = w.sum()
    fd = np.empty_like(psi)
    for n in range(len(u)):
        h = LD(1e-6) * w[n]
        wp, wm = w.copy(), w.copy()
        wp[n] += h
        wm[n] -= h
        fd[:, n] = W * (_oracle_derivs(x, u, wp, ORDER, minus_log) - _oracle_derivs(x, u, wm, ORDER, minus_log)) / (2 * h)
    worst = max(float(np.abs(psi[k] - fd[k]).max() / np.abs(psi[k]).max()) for k in range(ORDER + 1))
    print(f"central={central} minus_log={minus_log}: worst |psi - W dd/dw| / max|psi| = {worst:.2e}")
    assert worst <= 1e-7


@pytest.mark.parametrize("minus_log", [False, True])
def test_central_and_raw_forms_agree(data200, minus_log):
    pc, pr = _psi(data200, True, minus_log), _psi(data200, False, minus_log)
    for k in range(ORDER + 1):
        assert np.abs(pc[k] - pr[k]).max() <= 1e-10 * np.abs(pc[k]).max(), k


@pytest.mark.parametrize("central", [True, False])
def test_order_zero_is_the_variance_of_the_mean(data200, central):
    """Order 0 without the log: psi_0 = dx exactly (a = 0, b = 1), so V_00 = sum p^2 dx^2 exactly as formed."""
    d = data200
    a, b = S.influence_coefs(series_for(central), 0, d["mom"])
    assert a[0, 0] == 0 and b[0, 0] == 1
    psi = psi_ld(a, b, d["dx"], d["du"])
    assert np.array_equal(psi[0], d["dx"])
    assert cov_ld(psi, d["p"])[0, 0] == cov_ld(d["dx"][None, :], d["p"])[0, 0]


def test_float64_moments_give_float64_coefficients():
    x, u, w = make_data(200, seed=0)
    p, dx, du, mom = ld_moments(x, u, w, ORDER)
    mom64 = S.influence_moments(float(mom["xmean"]), float(mom["umean"]), [float(v) for v in mom["du"]],
                                [float(v) for v in mom["dxdu"]])
    a, b = S.influence_coefs(series_for(True), ORDER, mom64)
    a_ld, b_ld = S.influence_coefs(series_for(True), ORDER, mom)
    assert a.dtype == np.float64 and a_ld.dtype == LD
    scale = np.abs(np.asarray(a_ld, float)).max()
    assert np.abs(a - np.asarray(a_ld, float)).max() <= 1e-13 * scale


def test_columns_broadcast():
    x, u, w = make_data(200, seed=3, ncol=3)
    p, dx, du, mom = ld_moments(x, u, w, 2)
    a, b = S.influence_coefs(series_for(True), 2, mom, minus_log=True)
    assert a.shape == (3, 3, 3)
    for c in range(3):
        _, _, _, m1 = ld_moments(x[:, c], u, w, 2)
        a1, b1 = S.influence_coefs(series_for(True), 2, m1, minus_log=True)
        # (the 2-D moment sums run in another order than the 1-D ones: long-double rounding apart)
        assert np.abs(a[c] - a1).max() <= 1e-16 * np.abs(a1).max() and np.abs(b[c] - b1).max() <= 1e-16 * np.abs(b1).max()


def test_unsupported_atoms_raise():
    from thermoextrap_amd import beta

    _, _, _, mom = ld_moments(*make_data(50, seed=1), 2)
    with pytest.raises(NotImplementedError, match="xalpha"):
        S.influence_coefs(beta.factory_derivatives(name="x_ave", central=True, xalpha=True).series, 2, mom)
    with pytest.raises(NotImplementedError, match="callables"):
        S.influence_coefs([lambda *a: 0.0] * 3, 2, mom)


def test_against_numpy_bootstrap():
    """N = 2e4, unweighted, order 2: V from psi against the sample covariance S of 2000 multinomial replicates of the
    oracle's derivatives; |V_ij - S_ij| <= 5 se_ij with se_ij = std_r[(d_i - m_i)(d_j - m_j)] / sqrt(R)."""
    N, R, order = 20000, 2000, 2
    x, u, _ = make_data(N, seed=0, weighted=False)
    p, dx, du, mom = ld_moments(x, u, None, order)
    a, b = S.influence_coefs(series_for(True), order, mom)
    V = np.asarray(cov_ld(psi_ld(a, b, dx, du), p), float)
    counts = np.random.default_rng(1).multinomial(N, np.full(N, 1.0 / N), size=R)
    d = np.stack([DO.derivs_x_ave(x, u, order, w=counts[r]) for r in range(R)])       # [R, order + 1]
    dev = d - d.mean(axis=0)
    prod = dev[:, :, None] * dev[:, None, :]
    Sm = prod.sum(axis=0) / (R - 1)
    se = prod.std(axis=0, ddof=1) / math.sqrt(R)
    ratio = np.abs(V - Sm) / se
    print("bootstrap check: |V - S| / se =\n", np.array2string(ratio, precision=2), "\n se / |S| =\n",
          np.array2string(se / np.abs(Sm), precision=3))
    assert (ratio <= 5.0).all()


def test_entry_point_validates_without_a_device():
    """txm_influence_cov: argument errors come back as TXM_ERR_INVALID before any HIP call; the workspace query is host logic."""
    import ctypes as ct

    from thermoextrap_amd import _lib

    lib = _lib.load()
    p = ct.c_void_p(256)   # never dereferenced: every call below fails validation first
    names = ("x", "ls", "lc", "u", "w", "N", "C", "nf", "nq", "cu", "cx", "a", "b", "cov", "mean", "ws", "wsb", "st")
    good = dict(x=p, ls=4, lc=1, u=p, w=None, N=10, C=4, nf=3, nq=3, cu=0.0, cx=p, a=p, b=p, cov=p, mean=p, ws=p, wsb=1 << 30, st=None)

    def call(**bad):
        return lib.txm_influence_cov(*[{**good, **bad}[n] for n in names])

    assert call(x=None) == -1 and b"null" in lib.txm_last_error()
    assert call(N=0) == -1
    assert call(C=70000) == -1
    assert call(nf=10) == -1 and b"n_f" in lib.txm_last_error()
    assert call(nq=0) == -1 and b"n_q" in lib.txm_last_error()
    assert call(ls=3, lc=2) == -1
    assert call(ls=3) == -1 and b"pitch" in lib.txm_last_error()
    assert call(cu=float("nan")) == -1
    assert call(wsb=8) == -3
    assert lib.txm_influence_cov_ws_bytes(10, 4, 10) == 0 and lib.txm_influence_cov_ws_bytes(0, 4, 3) == 0
    need = lib.txm_influence_cov_ws_bytes(10**8, 32, 5)
    assert 8 * 37 * 32 * 256 * 8 <= need <= 8 * 37 * 32 * 256 * 8 + 4096     # 37 sums per column, 8 workgroups per CU, 256 CUs
