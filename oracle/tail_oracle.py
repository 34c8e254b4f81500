"""
oracle/tail_oracle.py -- TEST INFRASTRUCTURE, NOT PRODUCT.

Plain restatements, in ``numpy.longdouble`` (x87 80-bit, eps = 1.08e-19), of the kernels that turn moments into
answers: the exponential reweighting of ``txm_perturb``, the covariance over replicates, the raw <-> central
conversions and the merge / block bootstrap of pre-reduced states.  Every function is written from the mathematics
(the binomial theorem and the definition of a weighted average); none of them goes through ``liboracle.so``, so they
are independent of cmomy_oracle.c, and tests/test_tail_oracle_cpu.py pins each of them to mpmath at 50 digits.

State layout (oracle.py): ``[..., 2, K]``.
  central form  [0,0] = weight, [0,1] = <u>, [1,0] = <x>, otherwise [a,b] = <(x-<x>)^a (u-<u>)^b>
  raw form      [0,0] = weight, otherwise [a,b] = <x^a u^b>
1-D form ``[..., M]``: [0] = weight, [1] = <u>, central [b] = <(u-<u>)^b> / raw [b] = <u^b>.

Besides its value, each conversion can return the first-order bound of its own sum, ``sum |binom * m * shift
powers|`` per element: the scale against which a rounding error of that element is measured (README "Tolerances").
"""

from __future__ import annotations

from math import comb

import numpy as np

LD = np.longdouble
EPS_LD = float(np.finfo(LD).eps)


def _ld(a):
    return np.asarray(a, dtype=LD)


# ---------------------------------------------------------------------------
# perturbation averages
# ---------------------------------------------------------------------------
def perturb(x, u, dalphas, freq=None):
    """out[a, c] = sum_i f_i w_ai x_ic / sum_i f_i w_ai,  w_ai = exp(e_ai - max_i e_ai),  e_ai = -da_a u_i, the maximum
    taken over the samples with f_i > 0 (what is left of the series after resampling).

    x (N, C) or (N,); u (N,); freq None, (N,) or (nrep, N) counts.  Returns ``(avg, S)`` as float64, shaped
    (n_alpha, C) -- (nrep, n_alpha, C) for a 2-D freq, the C axis dropped for 1-D x -- where
    ``S[a, c] = sum f w |x| / sum f w`` is the natural scale of the output."""
    x = np.asarray(x, dtype=np.float64)
    squeeze = x.ndim == 1
    x2 = x.reshape(x.shape[0], -1)
    N, C = x2.shape
    ul = _ld(u).reshape(N)
    da = np.atleast_1d(np.asarray(dalphas, dtype=np.float64)).ravel()
    if freq is None:
        fr = np.ones((1, N), dtype=np.int64)
    else:
        fr = np.atleast_2d(np.asarray(freq, dtype=np.int64))
    if fr.shape[1] != N:
        raise ValueError("freq must be (nrep, N)")
    nrep = fr.shape[0]
    avg = np.empty((nrep, len(da), C))
    S = np.empty((nrep, len(da), C))
    for r in range(nrep):                    # one replicate and one column at a time: the long-double copies stay small
        live = fr[r] > 0
        if not live.any():
            raise ValueError("replicate without samples")
        fl = _ld(fr[r])
        W = np.empty((len(da), N), dtype=LD)
        for a, d in enumerate(da):
            e = -LD(d) * ul
            W[a] = fl * np.exp(e - e[live].max())
        den = W.sum(axis=1)
        for c in range(C):
            xc = _ld(x2[:, c])
            avg[r, :, c] = ((W * xc).sum(axis=1) / den).astype(np.float64)
            S[r, :, c] = ((W * np.abs(xc)).sum(axis=1) / den).astype(np.float64)
    if squeeze:
        avg, S = avg[..., 0], S[..., 0]
    if freq is None or np.ndim(freq) == 1:
        avg, S = avg[0], S[0]
    return avg, S


# ---------------------------------------------------------------------------
# covariance over replicates
# ---------------------------------------------------------------------------
def cov_over_rep(vals):
    """vals (n_ord, nrep, nval) -> ``(cov, sigma)``: cov (nval, n_ord, n_ord) is numpy.cov(vals[:, :, v], ddof=1),
    sigma (nval, n_ord) its root diagonal; two passes in long double, returned as float64."""
    v = _ld(vals)
    n_ord, nrep, nval = v.shape
    if nrep < 2:
        raise ValueError("cov_over_rep needs nrep >= 2")
    d = v - v.mean(axis=1, keepdims=True)
    cov = np.empty((nval, n_ord, n_ord), dtype=LD)
    for a in range(n_ord):
        for b in range(a, n_ord):
            cov[:, a, b] = cov[:, b, a] = (d[a] * d[b]).sum(axis=0) / LD(nrep - 1)
    sigma = np.sqrt(np.stack([cov[:, a, a] for a in range(n_ord)], axis=1))
    return cov.astype(np.float64), sigma.astype(np.float64)


# ---------------------------------------------------------------------------
# raw <-> central
# ---------------------------------------------------------------------------
def _shift_cov(m, sx, su):
    """Binomial shift of comoments.  m (n, 2, K) long double with m[:,0,0] read as 1; sx, su (n,).
    out[a][b] = sum_{i<=a, j<=b} C(a,i) C(b,j) m[i][j] sx^(a-i) su^(b-j), and the sum of the absolute terms."""
    n, _, K = m.shape
    out = np.zeros_like(m)
    bound = np.zeros_like(m)
    pu = [np.ones(n, dtype=LD)]
    for _ in range(K):
        pu.append(pu[-1] * su)
    for a in range(2):
        for b in range(K):
            for i in range(a + 1):
                for j in range(b + 1):
                    mij = np.ones(n, dtype=LD) if i + j == 0 else m[:, i, j]
                    t = LD(comb(a, i) * comb(b, j)) * mij * (sx if a - i else LD(1)) * pu[b - j]
                    out[:, a, b] += t
                    bound[:, a, b] += np.abs(t)
    return out, bound


def _central_to_about(c, ox, ou):
    """central-form states -> moments about the point (ox, ou): <(x-ox)^a (u-ou)^b>."""
    K = c.shape[-1]
    m = c.copy()
    m[:, 1, 0] = 0
    ua = np.zeros(c.shape[0], dtype=LD)
    if K > 1:
        ua = c[:, 0, 1].copy()
        m[:, 0, 1] = 0
    out, bound = _shift_cov(m, c[:, 1, 0] - ox, ua - ou)
    out[:, 0, 0] = bound[:, 0, 0] = c[:, 0, 0]
    return out, bound


def _about_to_central(m, ox, ou):
    """moments about (ox, ou) -> central-form states."""
    K = m.shape[-1]
    dx = m[:, 1, 0]
    du = m[:, 0, 1] if K > 1 else np.zeros(m.shape[0], dtype=LD)
    out, bound = _shift_cov(m, -dx, -du)
    out[:, 0, 0] = bound[:, 0, 0] = m[:, 0, 0]
    out[:, 1, 0] = ox + dx
    bound[:, 1, 0] = np.abs(ox) + np.abs(dx)
    if K > 1:
        out[:, 0, 1] = ou + du
        bound[:, 0, 1] = np.abs(ou) + np.abs(du)
    return out, bound


def convert_cov(states, to_central: bool, return_bound: bool = False):
    """central <-> raw on (..., 2, K) states, the weight [0,0] carried."""
    s = np.asarray(states, dtype=np.float64)
    p = _ld(s).reshape(-1, 2, s.shape[-1])
    zero = np.zeros(p.shape[0], dtype=LD)
    out, bound = (_about_to_central if to_central else _central_to_about)(p, zero, zero)
    out = out.astype(np.float64).reshape(s.shape)
    return (out, bound.astype(np.float64).reshape(s.shape)) if return_bound else out


def convert_1d(states, to_central: bool, return_bound: bool = False):
    """central <-> raw on (..., M) moment vectors, the weight [0] carried."""
    s = np.asarray(states, dtype=np.float64)
    M = s.shape[-1]
    p = _ld(s).reshape(-1, M)
    n = p.shape[0]
    ua = p[:, 1] if M > 1 else np.zeros(n, dtype=LD)
    su = -ua if to_central else ua
    out = np.zeros_like(p)
    bound = np.zeros_like(p)
    for b in range(M):
        for j in range(b + 1):
            if j == 0:
                mj = np.ones(n, dtype=LD)
            elif j == 1 and not to_central:
                mj = np.zeros(n, dtype=LD)          # the first central moment is 0; the slot holds <u>
            else:
                mj = p[:, j]
            t = LD(comb(b, j)) * mj * su ** (b - j)
            out[:, b] += t
            bound[:, b] += np.abs(t)
    out[:, 0] = bound[:, 0] = p[:, 0]
    if M > 1 and to_central:
        out[:, 1] = p[:, 1]
        bound[:, 1] = np.abs(p[:, 1])
    out = out.astype(np.float64).reshape(s.shape)
    return (out, bound.astype(np.float64).reshape(s.shape)) if return_bound else out


# ---------------------------------------------------------------------------
# merge / block bootstrap of pre-reduced states
# ---------------------------------------------------------------------------
def resample_data(data, freq, order, origin=None, return_bound: bool = False):
    """data (nrec, C, 2, K) central-form records, freq (nrep, nrec) counts -> (nrep, C, 2, K).

    Every record is expanded to its weight-scaled raw sums ``W <x^a u^b>`` about ``origin`` (zero by default; (C, 2) =
    per column (ou, ox) to keep ideal-gas-scale data away from the cancellation of powers of a mean 33 sigma from zero),
    the sums are added with the counts, divided by the total weight and re-centralised.  A record of weight 0
    contributes nothing whatever its moments say; an output of total weight 0 is all zeros.
    With ``return_bound`` also the first-order bound of the re-centralisation sum of every element."""
    d = np.asarray(data, dtype=np.float64)
    nrec, C, two, K = d.shape
    if two != 2 or K != order + 1:
        raise ValueError("data must be (nrec, C, 2, order+1)")
    fr = np.atleast_2d(np.asarray(freq, dtype=np.int64))
    if fr.shape[1] != nrec:
        raise ValueError("freq must be (nrep, nrec)")
    nrep = fr.shape[0]
    org = np.zeros((C, 2), dtype=LD) if origin is None else _ld(origin).reshape(C, 2)
    p = _ld(d).reshape(nrec * C, 2, K)
    ou = np.tile(org[:, 0], nrec)
    ox = np.tile(org[:, 1], nrec)
    m, _ = _central_to_about(p, ox, ou)
    W = p[:, 0, 0].copy()
    m[:, 0, 0] = 1
    sums = (W[:, None, None] * m).reshape(nrec, C, 2, K)
    sums[(W == 0).reshape(nrec, C)] = 0
    tot = np.einsum("ri,icak->rcak", _ld(fr), sums).reshape(nrep * C, 2, K)
    Wt = tot[:, 0, 0].copy()
    live = Wt != 0
    mm = np.zeros_like(tot)
    mm[live] = tot[live] / Wt[live, None, None]
    mm[:, 0, 0] = Wt
    out, bound = _about_to_central(mm, np.tile(org[:, 1], nrep), np.tile(org[:, 0], nrep))
    out[~live] = 0
    bound[~live] = 0
    out = out.astype(np.float64).reshape(nrep, C, 2, K)
    return (out, bound.astype(np.float64).reshape(nrep, C, 2, K)) if return_bound else out


def reduce_data(data, order, origin=None, return_bound: bool = False):
    """Merge of all records: (nrec, C, 2, K) -> (C, 2, K)."""
    nrec = np.asarray(data).shape[0]
    r = resample_data(data, np.ones((1, nrec), dtype=np.int64), order, origin, return_bound)
    return (r[0][0], r[1][0]) if return_bound else r[0]
