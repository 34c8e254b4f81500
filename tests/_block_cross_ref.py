"""Shared reference code of the blocked cross-column delta-method tests (test_influence_block_cross_cpu.py,
test_derivs_cross_cov_block_gpu.py): the AR(1) series with a known long-run covariance of its column means and the
definition of DESIGN 4.15 restated through symbolic.influence_coefs in long double.  Not a test module."""

from __future__ import annotations

import math

import numpy as np

from tests._influence_ref import bound_ld, ld_moments, psi_ld, series_for

AR1_N, AR1_RHO, AR1_BLOCK = 1 << 20, 0.9, 1024
# x_0 = 0.7 u + e_0,  x_1 = 0.5 u + 0.8 e_0 + 0.3 e_1,  x_2 = -0.6 u + e_2  with u, e_0, e_1, e_2 independent, unit variance
AR1_MIX = np.array([[0.7, 1.0, 0.0, 0.0], [0.5, 0.8, 0.3, 0.0], [-0.6, 0.0, 0.0, 1.0]])
AR1_SIGMA = AR1_MIX @ AR1_MIX.T                 # the population covariance: correlations 0.952 (0, 1) and -0.295 (0, 2)
AR1_G = (1.0 + AR1_RHO) / (1.0 - AR1_RHO)       # 19: long-run covariance of the means = 19 Sigma / N
AR1_LIMIT = 0.25                                # 5 sqrt(2 / 1023) + the block bias, of 19 sqrt(Sigma_cc Sigma_c'c') / N


def _ar1(rng, n, rho):
    """AR(1), unit marginal variance, started in the stationary distribution."""
    eps = rng.standard_normal(n) * math.sqrt(1.0 - rho * rho)
    out = eps.tolist()
    out[0] = float(rng.standard_normal())
    for i in range(1, n):
        out[i] += rho * out[i - 1]
    return np.asarray(out)


def ar1_columns(seed=0, n=AR1_N):
    """(u [n], x [n, 3]): u and three independent e_k AR(1) with rho = 0.9, x = AR1_MIX (u, e_0, e_1, e_2)."""
    rng = np.random.default_rng(seed)
    s = np.stack([_ar1(rng, n, AR1_RHO) for _ in range(4)])
    return s[0], np.ascontiguousarray((AR1_MIX @ s).T)


def ar1_scale(n=AR1_N):
    """(target [3, 3], scale [3, 3]): 19 Sigma / N and 19 sqrt(Sigma_cc Sigma_c'c') / N."""
    d = np.sqrt(np.diag(AR1_SIGMA))
    return AR1_G * AR1_SIGMA / n, AR1_G * np.outer(d, d) / n


def blocked_means_cov(x, block):
    """The definition at order 0 in numpy: V[c, c'] = sum_b z_b[c] z_b[c'], z_b = sum_{n in b} (x_n - mean) / N."""
    z = np.add.reduceat((x - x.mean(axis=0)) / len(x), np.arange(0, len(x), block), axis=0)
    return z.T @ z


def blocked_cross_ld(x, u, w, order, central, minus_log, block):
    """(V, bound) [c, i, c', j] of the blocked estimator in long double through symbolic.influence_coefs on long-double
    moments: V = sum_b z_b z_b', z_b = sum_{n in b} p_n psi(n); the bound the same with B for psi."""
    from thermoextrap_amd import symbolic as S

    p, dx, du, mom = ld_moments(x, u, w, order)
    a, b = S.influence_coefs(series_for(central), order, mom, minus_log=minus_log)
    C, N = x.shape[1], len(u)
    psi = np.stack([psi_ld(a[c], b[c], dx[:, c], du) for c in range(C)]).reshape(C * (order + 1), N)
    B = np.stack([bound_ld(a[c], b[c], dx[:, c], du) for c in range(C)]).reshape(C * (order + 1), N)
    starts = np.arange(0, N, block)
    z, beta = np.add.reduceat(psi * p, starts, axis=1), np.add.reduceat(B * p, starts, axis=1)
    shape = (C, order + 1, C, order + 1)
    return (z @ z.T).reshape(shape), (beta @ beta.T).reshape(shape)
