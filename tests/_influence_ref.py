"""Shared reference code of the delta-method tests (test_influence_cpu.py, test_influence_gpu.py, test_derivs_cov_gpu.py):
the test data, its weighted moments and the influence functions psi evaluated in long double.  Not a test module."""

from __future__ import annotations

import numpy as np

LD = np.longdouble


def make_data(n, seed=0, weighted=True, ncol=1):
    """u ~ N(3, 1), x = 0.7 u + 0.3 u^2 + N(2, 1) (column c scaled by 1 + c / 2), weights U(0.5, 1.5)."""
    rng = np.random.default_rng(seed)
    u = rng.normal(3.0, 1.0, n)
    x = np.stack([(0.7 * u + 0.3 * u * u + rng.normal(2.0, 1.0, n)) * (1.0 + 0.5 * c) for c in range(ncol)], axis=1)
    w = rng.uniform(0.5, 1.5, n) if weighted else None
    return (x[:, 0] if ncol == 1 else x), u, w


def ld_moments(x, u, w, order):
    """(p, dx, du, moments) in long double: normalised weights, deviations from the weighted means (x: (N,) or (N, C)) and the
    dict symbolic.influence_coefs takes."""
    from thermoextrap_amd import symbolic as S

    x, u = np.asarray(x, LD), np.asarray(u, LD)
    w = np.ones_like(u) if w is None else np.asarray(w, LD)
    p = w / w.sum()
    pc = p if x.ndim == 1 else p[:, None]
    um, xm = (p * u).sum(), (pc * x).sum(axis=0)
    du, dx = u - um, x - xm
    duc = du if x.ndim == 1 else du[:, None]
    mu = [(p * du**j).sum() for j in range(order + 1)]
    cc = [(pc * dx * duc**j).sum(axis=0) for j in range(order + 1)]
    return p, dx, du, S.influence_moments(xm, um, mu, cc)


def series_for(central):
    from thermoextrap_amd import beta

    return beta.factory_derivatives(name="x_ave", central=central).series


def psi_ld(a, b, dx, du):
    """psi[k, n] = sum_q (a[k, q] + b[k, q] dx_n) du_n^q in long double (one column)."""
    a, b = np.asarray(a, LD), np.asarray(b, LD)
    pw = np.stack([du**q for q in range(a.shape[-1])])            # [q, n]
    return a @ pw + (b @ pw) * dx[None, :]


def bound_ld(a, b, dx, du):
    """B[k, n] = sum_q (|a[k, q]| + |b[k, q]| |dx_n|) |du_n|^q."""
    return psi_ld(np.abs(np.asarray(a, LD)), np.abs(np.asarray(b, LD)), np.abs(dx), np.abs(du))


def cov_ld(psi, p):
    """V[i, j] = sum_n p_n^2 psi_i psi_j."""
    return np.einsum("n,in,jn->ij", p * p, psi, psi)
