"""
oracle/mbar_oracle.py -- TEST INFRASTRUCTURE, NOT PRODUCT.

Plain restatements, in ``numpy.longdouble`` (x87 80-bit, eps = 1.08e-19), of what the four MBAR entry points
(txm_mbar.hip, txm_mbar_boot.hip) and the covariance pass (txm_mbar_cov.hip) sum, from the same float64 inputs the kernels get: the energies ``us`` of the K states,
``alpha0``, the shifted log-weights ``g``, the pivot ``upiv`` and, for a bootstrap replicate, the integer count ``c_n`` of
every pooled sample.  ``ut = u - upiv`` and every exponent are formed in long double.

    p_kn   = softmax_k(g_k - alpha0_k ut_n)          logD_n = ln sum_k e^{g_k - alpha0_k ut_n}
    S_k    = sum_n c_n p_kn      H_jk = sum_n c_n p_jn p_kn      obj = sum_n c_n logD_n
    <x>(a) = sum_n c_n w_an x_n / sum_n c_n w_an,     w_an = e^{-a ut_n - logD_n}
    W_nk = p_kn / N_k     W_na = w_an / sum_n w_an     d_nc = x_nc - mean_ac
    Q_a = sum_n W_na^2    B_ak = sum_n W_nk W_na       yy_ac = sum_n W_na^2 d_nc^2     b_kac = sum_n W_nk W_na d_nc

Next to every sum comes that sum's own first-order bound  sum_n kappa_n |term_n|  (README "Tolerances"), with the
per-sample conditioning

    kappa_n = 1 + max_k(|g_k| + |alpha0_k ut_n|) / 64

(for predict the maximum also runs over the targets' |a ut_n| + |logD_n|): a float64 exponent g_k - alpha0_k ut_n carries
an absolute error of at most eps (|g_k| + 2 |alpha0_k ut_n|) -- one rounding in u - upiv, one in the fma -- which is a
relative error of the weight of at most 128 eps kappa_n.  tests/test_mbar_oracle_cpu.py pins every function to mpmath at
50 digits.
"""

from __future__ import annotations

from typing import NamedTuple

import numpy as np

LD = np.longdouble
EPS_LD = float(np.finfo(LD).eps)


def _ld(a):
    return np.asarray(a, dtype=LD)


def pooled_ut(us, upiv):
    """ut_n = u_n - upiv over the pooled samples (state after state), long double."""
    return np.concatenate([_ld(u).reshape(-1) for u in us]) - LD(upiv)


def exponents(alpha0, g, ut):
    """t_kn = g_k - alpha0_k ut_n, (K, N) long double."""
    return _ld(g).reshape(-1, 1) - _ld(alpha0).reshape(-1, 1) * ut[None, :]


def kappa(alpha0, g, ut, targets=None, logD=None):
    """kappa_n (float64, (N,)).  ``g`` may be None (the unweighted predict sees logD, not g); with ``targets`` and ``logD``
    the maximum also runs over |a ut_n| + |logD_n|."""
    au = np.abs(ut)
    big = np.zeros(ut.shape, dtype=LD)
    if g is not None:
        big = (np.abs(_ld(g)).reshape(-1, 1) + np.abs(_ld(alpha0)).reshape(-1, 1) * au[None, :]).max(axis=0)
    if targets is not None:
        amax = np.abs(_ld(targets)).max()
        big = np.maximum(big, amax * au + np.abs(_ld(logD)))
    return (1.0 + big / 64.0).astype(np.float64)


class EvalSums(NamedTuple):
    """Values and bounds are long double; ``p_min`` is the smallest p_kn (its underflow is what a float64 kernel flushes)."""

    S: np.ndarray          # (K,)
    S_bound: np.ndarray
    H: np.ndarray          # (K, K), full symmetric
    H_bound: np.ndarray
    obj: np.longdouble
    obj_bound: np.longdouble
    logD: np.ndarray       # (N,) pooled, state after state
    kappa: np.ndarray      # (N,) float64
    p_min: float


def eval_sums(us, alpha0, g, upiv, counts=None) -> EvalSums:
    """What txm_mbar_eval (counts None) and one replicate of txm_mbar_boot_eval (counts (N_total,) integers) sum."""
    ut = pooled_ut(us, upiv)
    t = exponents(alpha0, g, ut)
    m = t.max(axis=0)
    e = np.exp(t - m)
    den = e.sum(axis=0)
    p = e / den
    ld = m + np.log(den)
    kap = kappa(alpha0, g, ut)
    c = np.ones(ut.shape, dtype=LD) if counts is None else _ld(np.asarray(counts, dtype=np.int64).reshape(-1))
    if c.shape != ut.shape:
        raise ValueError("counts must hold one integer per pooled sample")
    ck = c * _ld(kap)
    live = c > 0                                  # a bootstrap replicate leaves e^-1 of the samples out
    pl = p[:, live]
    cp, ckp = pl * c[live], pl * ck[live]
    return EvalSums(S=cp.sum(axis=1), S_bound=ckp.sum(axis=1), H=cp @ pl.T, H_bound=ckp @ pl.T, obj=(c * ld).sum(),
                    obj_bound=(ck * np.abs(ld)).sum(), logD=ld, kappa=kap, p_min=float(p.min()))


class Averages(NamedTuple):
    avg: np.ndarray        # (n_alpha, C) float64: the quotient, rounded once
    scale: np.ndarray      # (n_alpha, C) float64: sum c w |x| / sum c w
    kappa: np.ndarray      # (n_alpha,) float64: the largest kappa_n over the samples with c w above 1e-30 of the largest
    kappa_n: np.ndarray    # (N,) float64


def predict(us, xs, alpha0, upiv, targets, *, logD=None, g=None, counts=None) -> Averages:
    """What txm_mbar_predict (``logD``: the float64 values the kernel reads) and one replicate of txm_mbar_boot_predict
    (``g``: that replicate's log-weights, logD formed here in long double; ``counts`` its integer counts) compute."""
    if (logD is None) == (g is None):
        raise ValueError("give exactly one of logD and g")
    ut = pooled_ut(us, upiv)
    if g is not None:
        t = exponents(alpha0, g, ut)
        m = t.max(axis=0)
        ld = m + np.log(np.exp(t - m).sum(axis=0))
    else:
        ld = _ld(logD).reshape(-1)
    x = np.concatenate([_ld(v).reshape(len(v), -1) for v in xs])
    if ld.shape != ut.shape or x.shape[0] != ut.shape[0]:
        raise ValueError("logD and x need one row per pooled sample")
    c = np.ones(ut.shape, dtype=LD) if counts is None else _ld(np.asarray(counts, dtype=np.int64).reshape(-1))
    live = c > 0
    al = np.atleast_1d(np.asarray(targets, dtype=np.float64)).ravel()
    kn = kappa(alpha0, g, ut, al, ld)
    ax = np.abs(x)
    avg, scale, kap = np.empty((len(al), x.shape[1])), np.empty((len(al), x.shape[1])), np.empty(len(al))
    for i, a in enumerate(al):
        ex = -LD(a) * ut - ld
        w = c * np.exp(ex - ex[live].max())
        den = w.sum()
        avg[i] = ((w @ x) / den).astype(np.float64)
        scale[i] = ((w @ ax) / den).astype(np.float64)
        kap[i] = kn[w > LD(1e-30) * w.max()].max()
    return Averages(avg, scale, kap, kn)


class CovSums(NamedTuple):
    """Values and bounds are long double, one leading index per target.  ``den`` and ``dabs`` are what an absolute floor
    for products a float64 kernel flushes is built from (tests/test_mbar_kernels_gpu.py, group E)."""

    Q: np.ndarray          # (n_alpha,)
    Q_bound: np.ndarray
    B: np.ndarray          # (n_alpha, K)
    B_bound: np.ndarray
    yy: np.ndarray         # (n_alpha, C)
    yy_bound: np.ndarray
    b: np.ndarray          # (n_alpha, C, K): the order of the kernel's output
    b_bound: np.ndarray
    lnw: np.ndarray        # (n_alpha,) ln sum_n v_an
    den: np.ndarray        # (n_alpha,) sum_n v_an / max_n v_an: the denominator as the kernel holds it (>= 1)
    dabs: np.ndarray       # (n_alpha, C) sum_n |d_nc|
    kappa_n: np.ndarray    # (N,) float64
    kappa: float           # the largest kappa_n
    p_min: float


def cov_sums(us, xs, alpha0, g, upiv, targets, means, logD) -> CovSums:
    """What txm_mbar_cov sums.  p_kn is the softmax at ``g`` formed here; ``logD`` (N,) and ``means`` (n_alpha, C) are the
    float64 arrays the kernel reads.  The contractions over the samples are matrix products, one target at a time."""
    ut = pooled_ut(us, upiv)
    t = exponents(alpha0, g, ut)
    e = np.exp(t - t.max(axis=0))
    p = e / e.sum(axis=0)
    Wk = p / _ld([len(u) for u in us]).reshape(-1, 1)                   # (K, N)
    ld = _ld(logD).reshape(-1)
    x = np.concatenate([_ld(v).reshape(len(v), -1) for v in xs])
    al = np.atleast_1d(np.asarray(targets, dtype=np.float64)).ravel()
    mu = _ld(means).reshape(len(al), -1)
    if ld.shape != ut.shape or x.shape[0] != ut.shape[0] or mu.shape[1] != x.shape[1]:
        raise ValueError("logD and x need one row per pooled sample, means one row per target")
    kn = kappa(alpha0, g, ut, al, ld)
    kl = _ld(kn)
    K, C, na = Wk.shape[0], x.shape[1], len(al)
    Q, Qb, lnw, den = (np.empty(na, dtype=LD) for _ in range(4))
    B, Bb = np.empty((na, K), dtype=LD), np.empty((na, K), dtype=LD)
    yy, yyb, dabs = (np.empty((na, C), dtype=LD) for _ in range(3))
    b, bb = np.empty((na, C, K), dtype=LD), np.empty((na, C, K), dtype=LD)
    for i, a in enumerate(al):
        ex = -LD(a) * ut - ld
        mx = ex.max()
        v = np.exp(ex - mx)
        den[i] = v.sum()
        lnw[i] = mx + np.log(den[i])
        wa = v / den[i]
        d = x - mu[i][None, :]
        wd = wa[:, None] * d                                            # (N, C)
        kwa = kl * wa
        Q[i], Qb[i] = wa @ wa, kwa @ wa
        B[i], Bb[i] = Wk @ wa, Wk @ kwa
        yy[i], yyb[i] = (wd * wd).sum(axis=0), kl @ (wd * wd)
        b[i], bb[i] = (Wk @ wd).T, (Wk @ (kl[:, None] * np.abs(wd))).T
        dabs[i] = np.abs(d).sum(axis=0)
    return CovSums(Q, Qb, B, Bb, yy, yyb, b, bb, lnw, den, dabs, kn, float(kn.max()), float(p.min()))
