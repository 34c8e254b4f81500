"""Shared reference of the PerturbModel error-bar tests (test_perturb_cov_cpu.py, test_perturb_cov_gpu.py,
test_perturb_model_error_gpu.py): txm_perturb_cov restated in ``numpy.longdouble``, one column at a time, following
oracle/tail_oracle.perturb (the same weights: ``exp(e - max e)``, ``e = -da u``), returning every output plus the
first-order bound its tolerance is measured against.  Not a test module."""

from __future__ import annotations

from typing import NamedTuple

import numpy as np

LD = np.longdouble


def make_data(rng, N, C):
    """``make_data`` of test_perturb_gpu.py: ideal-gas-scale u (mean 33 sigma from zero) and columns of different offset
    and slope."""
    u = rng.normal(174.85, 5.31, N)
    x = rng.normal(0.0, 1.0, C)[None, :] + rng.normal(1e-3, 5e-4, C)[None, :] * u[:, None] + rng.normal(0, 0.05, (N, C))
    return x, u


def ar1_data(rng, N, nreal, phi=0.9):
    """``nreal`` realisations of ``u = 174.85 + 2 z`` with z a stationary unit-variance AR(1) series of coefficient phi
    (statistical inefficiency (1 + phi) / (1 - phi)) and ``x = 0.5 + 0.1 u + N(0, 0.05)``: (x, u), each (nreal, N)."""
    z = np.empty((N, nreal))
    z[0] = rng.normal(size=nreal)
    eps = rng.normal(size=(N, nreal)) * np.sqrt(1.0 - phi * phi)
    for n in range(1, N):
        z[n] = phi * z[n - 1] + eps[n]
    u = 174.85 + 2.0 * z.T
    x = 0.5 + 0.1 * u + rng.normal(0.0, 0.05, (nreal, N))
    return np.ascontiguousarray(x), np.ascontiguousarray(u)


class PerturbCovRef(NamedTuple):
    """float64 copies of the long-double results.  ``mean`` (na, C): the centre used (the caller's, or the reference's
    own reweighted mean); ``var`` (L, na, C), ``neff`` (na,), ``lnq`` (na,), ``var_lnq`` (L, na) as txm_perturb_cov
    defines them; ``var_bound`` = sum_j (sum_{n in j} p kappa |x - m|)^2, ``var_lnq_bound`` = sum_j (sum_{n in j} p kappa
    + n_j / N)^2, ``kbar`` = sum p kappa with kappa_n = 1 + |da (u_n - uref)|; ``zP`` (L, na, C) = sum_j |z_j| P_j, the
    sensitivity of var to the centre (d var / d m = -2 sum_j z_j P_j); ``S`` (na, C) = sum p |x|, tail_oracle.perturb's
    scale."""

    mean: np.ndarray
    var: np.ndarray
    neff: np.ndarray
    lnq: np.ndarray
    var_lnq: np.ndarray
    var_bound: np.ndarray
    var_lnq_bound: np.ndarray
    kbar: np.ndarray
    zP: np.ndarray
    S: np.ndarray


def level_starts(N, block, n_levels):
    """The first row of every block of every level: level l has blocks of ``block * 2**l`` rows, the last may be short."""
    out = []
    for l in range(n_levels):
        step = min(int(block) << l, N)
        out.append(np.arange(0, N, step, dtype=np.int64))
    return out


def perturb_cov(x, u, dalphas, mean=None, block=1, n_levels=1) -> PerturbCovRef:
    """txm_perturb_cov in long double.  x (N, C) or (N,) (read as one column), u (N,), ``mean`` (na, C) float64 or None
    for the reference's own long-double mean."""
    x = np.asarray(x, dtype=np.float64)
    x2 = x.reshape(x.shape[0], -1)
    N, C = x2.shape
    ul = np.asarray(u, dtype=LD).reshape(N)
    da = np.atleast_1d(np.asarray(dalphas, dtype=np.float64)).ravel()
    na = len(da)
    starts = level_starts(N, block, n_levels)
    nj = [np.diff(np.append(s, N)).astype(LD) / LD(N) for s in starts]
    L = n_levels
    out = PerturbCovRef(np.empty((na, C)), np.empty((L, na, C)), np.empty(na), np.empty(na), np.empty((L, na)),
                        np.empty((L, na, C)), np.empty((L, na)), np.empty(na), np.empty((L, na, C)), np.empty((na, C)))
    for a, d in enumerate(da):
        d = LD(d)
        uref = ul.min() if d >= 0 else ul.max()
        arg = -d * (ul - uref)                       # <= 0, the largest is 0
        w = np.exp(arg)
        W = w.sum()
        p = w / W
        kappa = LD(1) + np.abs(arg)
        pk = p * kappa
        out.neff[a] = W * W / (w * w).sum()
        out.lnq[a] = np.log(W / LD(N)) - d * uref
        out.kbar[a] = pk.sum()
        for l in range(L):
            P = np.add.reduceat(p, starts[l])
            out.var_lnq[l, a] = ((P - nj[l]) ** 2).sum()
            out.var_lnq_bound[l, a] = ((np.add.reduceat(pk, starts[l]) + nj[l]) ** 2).sum()
        for c in range(C):
            xc = np.asarray(x2[:, c], dtype=LD)
            m = (p * xc).sum() if mean is None else LD(np.asarray(mean, dtype=np.float64).reshape(na, C)[a, c])
            out.mean[a, c] = m
            out.S[a, c] = (p * np.abs(xc)).sum()
            t = p * (xc - m)
            tb = pk * np.abs(xc - m)
            for l in range(L):
                z = np.add.reduceat(t, starts[l])
                out.var[l, a, c] = (z * z).sum()
                out.var_bound[l, a, c] = (np.add.reduceat(tb, starts[l]) ** 2).sum()
                out.zP[l, a, c] = (np.abs(z) * np.add.reduceat(p, starts[l])).sum()
    return out
