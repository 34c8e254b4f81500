"""Restatements behind the tests of MBARModel.histogram (txm_mbar_hist, engine.mbar_hist_sums, mbar_hist_covariance).

hist_sums    What txm_mbar_hist sums, in long double from the float64 g, logD and u the kernel reads (the style of
             oracle/mbar_oracle.py cov_sums): with the class of a sample its bin index, or nbins when the index is outside
             [0, nbins),
                 T_kab = sum_n W_nk W_na 1_b(n)    H_ab = sum_n W_na 1_b(n)    S_ab = sum_n W_na^2 1_b(n)
             and next to every sum its first-order bound sum_n kappa_n |term_n| (kappa_n of the oracle: 1 + the largest
             exponent magnitude of the sample / 64, over the states and the targets).
             The row of v_a^2 takes the same kappa as the others.  A device exponent carries at most
             eps (|g_k| + 2 |alpha0_k ut_n|) of absolute error, a relative weight error of at most 128 eps kappa_n =
             2.8e-14 kappa_n (tests/test_mbar_kernels_gpu.py); a product of two weights -- p_kn v_an in the rows k < K, and
             v_an v_an in the row K + 1 alike -- carries twice that, 5.7e-14 kappa_n, still 17 times below the 1e-12 the
             bound allows.  Group E holds Q_a = sum_n W_na^2 to the same expression.
floors       A product below 2^-1022 is lost before the division: per sample at most 2^-1022, over N_k den_a (T), den_a (H,
             where v_an itself is what underflows) or den_a^2 (S); den_a = sum_n v_an / max_n v_an >= 1.
dense_cov    The covariance between the bins by the N x N definition: the indicator columns y_n,b = W_na (1_b(n) - p_b) next
             to the sampled columns, Theta = W^T (I_N - W N W^T)^+ W (tests/test_mbar_cov_cpu.py dense_theta, N <= 200), and
             gram_cov the same from the Gram matrix of those columns: their disagreement is the restatement's own error.
"""

from typing import NamedTuple

import numpy as np

from oracle import mbar_oracle as mo
from test_mbar_cov_cpu import dense_theta, gram_theta

LD = np.longdouble
TINY = LD(2.0 ** -1022)


class HistSums(NamedTuple):
    """Values and bounds in long double, laid out as the kernel's out: (n_alpha, K + 2, nbins + 1)."""

    out: np.ndarray
    bound: np.ndarray
    floor: np.ndarray
    lnw: np.ndarray        # (n_alpha,)
    kappa: float
    count: np.ndarray      # (nbins + 1,) samples per class


def classes(bins, nbins):
    b = np.concatenate([np.asarray(v, dtype=np.int64).reshape(-1) for v in bins])
    return np.where((b < 0) | (b >= nbins), nbins, b)


def hist_sums(us, bins, alpha0, g, upiv, targets, logD, nbins) -> HistSums:
    ut = mo.pooled_ut(us, upiv)
    t = mo.exponents(alpha0, g, ut)
    e = np.exp(t - t.max(axis=0))
    p = e / e.sum(axis=0)
    ns = mo._ld([len(u) for u in us])
    Wk = p / ns.reshape(-1, 1)                                             # (K, N)
    ld = mo._ld(logD).reshape(-1)
    al = np.atleast_1d(np.asarray(targets, dtype=np.float64)).ravel()
    cl = classes(bins, nbins)
    assert cl.shape == ut.shape == ld.shape
    kn = mo.kappa(alpha0, g, ut, al, ld)
    kl = mo._ld(kn)
    K, na, N = Wk.shape[0], len(al), LD(len(ut))
    order = np.argsort(cl, kind="stable")                                  # the samples class after class
    present, start = np.unique(cl[order], return_index=True)

    def per_class(rows):
        full = np.zeros((rows.shape[0], nbins + 1), dtype=LD)
        full[:, present] = np.add.reduceat(rows[:, order], start, axis=1)
        return full

    out, bound, floor = (np.empty((na, K + 2, nbins + 1), dtype=LD) for _ in range(3))
    lnw = np.empty(na, dtype=LD)
    for i, a in enumerate(al):
        ex = -LD(a) * ut - ld
        mx = ex.max()
        v = np.exp(ex - mx)
        den = v.sum()
        lnw[i] = mx + np.log(den)
        wa = v / den
        rows = np.concatenate([Wk * wa[None, :], wa[None, :], (wa * wa)[None, :]])      # (K + 2, N), all >= 0
        out[i] = per_class(rows)
        bound[i] = per_class(rows * kl[None, :])
        floor[i, :K] = (TINY * N / (ns * den))[:, None]
        floor[i, K] = TINY * N / den
        floor[i, K + 1] = TINY * N / (den * den)
    return HistSums(out, bound, floor, lnw, float(kn.max()), np.bincount(cl, minlength=nbins + 1))


def indicator_columns(Wt_a, cl, nbins):
    """Y (N, nbins) long double for one target: y_n,b = W_na (1_b(n) - p_b), p_b = sum_n W_na 1_b(n); and p."""
    hot = np.zeros((len(cl), nbins + 1), dtype=LD)
    hot[np.arange(len(cl)), cl] = 1
    p = (Wt_a[:, None] * hot).sum(0)
    return (Wt_a[:, None] * (hot - p[None, :]))[:, :nbins], p


def dense_cov(Ws, Ns, Y):
    K = Ws.shape[1]
    W = np.concatenate([Ws, Y], axis=1)
    return dense_theta(W, np.append(Ns, np.zeros(Y.shape[1])))[K:, K:]


def gram_cov(Ws, Ns, Y):
    K = Ws.shape[1]
    W = np.concatenate([Ws, Y], axis=1)
    return gram_theta(W, np.append(Ns, np.zeros(Y.shape[1])))[K:, K:]


def class_sums(Ws, Wt_a, cl, nbins):
    """(H (nbins + 1,), S, T (K, nbins + 1)) of one target rounded to float64: what engine.mbar_hist_sums returns."""
    hot = np.zeros((len(cl), nbins + 1), dtype=LD)
    hot[np.arange(len(cl)), cl] = 1
    f = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    return f(Wt_a @ hot), f((Wt_a * Wt_a) @ hot), f((Ws * Wt_a[:, None]).T @ hot)
