"""The host half of MBAR: everything between two device passes that is numpy alone.

The damped Newton solvers (one problem, or R bootstrap replicates at once) take their device evaluation as an argument;
the rest is the algebra of the asymptotic covariance (Shirts & Chodera 2008, eq. 8 and appendix D): Theta =
W^T (I_N - W N W^T)^+ W over the columns W_nk = p_kn / N_k of the sampled states and W_na of the targets needs only the
Gram matrix G = W^T W.  Nothing here loads the library or touches a tensor; engine.py imports every name.
"""

from __future__ import annotations

from typing import TYPE_CHECKING

import numpy as np

from . import _lib

if TYPE_CHECKING:
    from .engine import MbarSolution


_MBAR_MAX_STEP = 50.0   # cap (in units of f) on the part of a step along directions without curvature


def mbar_newton(evaluate, N, b, *, f0=None, tol: float = 1e-12, max_iter: int = 100):
    """Damped Newton on the convex MBAR objective  F(f) = sum_n logD_n(f) - sum_k N_k f_k  over the K - 1 free energies
    f_1.. (gauge f_0 = 0).  ``evaluate(g) -> (S, H, obj)`` is one pass over the pooled samples at the log-weights
    g = b + f + c (b_k = ln N_k - alpha0_k upiv; the constant c = -max_k(b + f) keeps them near 0): S_k = sum_n p_kn,
    H_jk = sum_n p_jn p_kn (full symmetric) and obj = sum_n logD_n + c N_tot.  The gradient is S - N and the Hessian
    diag(S) - H.

    The reduced Hessian is eigen-decomposed: directions with curvature above 1e-12 of the largest get the Newton step;
    the rest (states without overlap) get the gradient over that floor, capped at 50 units of f, so a singular Hessian
    still gives a finite step.  The step is halved until the objective decreases (Armijo), or -- once the change is
    below the objective's rounding -- until the gradient does.  Converged: max_k |S_k - N_k| / N_k <= tol.

    Returns (f, g, iterations, evaluations, gradient) with g the log-weights of the last evaluation (the returned f)."""
    N = np.asarray(N, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    K = len(N)
    Ntot = float(N.sum())
    f = np.zeros(K) if f0 is None else np.asarray(f0, dtype=np.float64) - float(f0[0])
    eps = np.finfo(np.float64).eps

    def point(f):
        g = b + f
        c = -float(g.max())
        g = g + c
        S, H, obj = evaluate(g)
        S, H = np.asarray(S, dtype=np.float64), np.asarray(H, dtype=np.float64)
        F = obj - c * Ntot - float(N @ f)
        rnd = 64 * eps * (abs(obj) + abs(c) * Ntot + float(N @ np.abs(f)) + Ntot)
        return S, H, F, rnd, g

    S, H, F, rnd, g = point(f)
    n_eval = 1
    for it in range(max_iter + 1):
        grad = S - N
        err = float(np.max(np.abs(grad) / N))
        if not np.isfinite(err):
            raise _lib.TxmError(f"MBAR solve: the gradient is not finite (max |S_k - N_k| / N_k = {err})")
        if err <= tol:
            return f, g, it, n_eval, err
        if it == max_iter:
            break
        Hr = (np.diag(S) - H)[1:, 1:]
        gr = grad[1:]
        lam, V = np.linalg.eigh(0.5 * (Hr + Hr.T))
        floor = 1e-12 * max(float(lam.max()), float(N.min()))
        good = lam > floor
        proj = V.T @ gr
        step = -(V[:, good] @ (proj[good] / lam[good]))
        if not good.all():
            flat = -(V[:, ~good] @ (proj[~good] / floor))
            big = float(np.max(np.abs(flat)))
            if big > _MBAR_MAX_STEP:
                flat *= _MBAR_MAX_STEP / big
            step = step + flat
        slope = float(gr @ step)
        t = 1.0
        while True:
            fn = f.copy()
            fn[1:] += t * step
            Sn, Hn, Fn, rn, gn = point(fn)
            n_eval += 1
            errn = float(np.max(np.abs(Sn - N) / N))
            if Fn <= F + 1e-4 * t * slope or (abs(Fn - F) <= max(rnd, rn) and errn < err):
                break
            t *= 0.5
            if t < 1e-10:
                raise _lib.TxmError(f"MBAR solve: the line search found no decrease at iteration {it}; "
                                    f"max |S_k - N_k| / N_k = {err:.3e}")
        f, S, H, F, rnd, g = fn, Sn, Hn, Fn, rn, gn
    raise _lib.TxmError(f"MBAR solve did not converge in {max_iter} Newton iterations: "
                        f"max |S_k - N_k| / N_k = {err:.3e} > tol {tol:.1e}")


def mbar_newton_batched(evaluate, N, b, f0, *, tol: float = 1e-12, max_iter: int = 100):
    """``mbar_newton`` for R replicates at once: the same damped Newton per replicate (eigen-floor, step halving,
    convergence max_k |S_k - N_k| / N_k <= tol), one batched evaluation per trial point.

    ``evaluate(g, active) -> (S, H, obj)``: ``g`` is the full (R, K) array of log-weights (row r = b + f_r + c_r, the
    constant c_r = -max_k keeps them near 0), ``active`` the int array of the rows wanted; S (A, K), H (A, K, K) full
    symmetric and obj (A,) are those rows' weighted sums (S_k = sum_n c_n p_kn, ...), in the order of ``active``.
    A converged replicate is frozen: its f never changes again and it is absent from every later ``active``.
    ``f0``: (R, K), one start per replicate (``np.tile(f, (R, 1))`` for a common one).

    Returns (f (R, K), g (R, K) -- each row's log-weights at its f --, iterations (R,), evaluations, gradient (R,));
    ``evaluations`` counts calls of ``evaluate``."""
    N = np.asarray(N, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    K = len(N)
    Ntot = float(N.sum())
    f = np.array(f0, dtype=np.float64)
    if f.ndim != 2 or f.shape[1] != K:
        raise ValueError(f"f0 must be (R, {K})")
    R = f.shape[0]
    f -= f[:, :1]
    eps = np.finfo(np.float64).eps
    g = np.zeros((R, K))          # what the device is shown (trial rows included)
    g_acc = np.zeros((R, K))      # each row's log-weights at its accepted f
    n_eval = 0

    def point(fa, rows):
        nonlocal n_eval
        ga = b[None, :] + fa
        c = -ga.max(axis=1)
        g[rows] = ga + c[:, None]
        S, H, obj = evaluate(g, rows.copy())
        n_eval += 1
        S, H, obj = np.asarray(S, dtype=np.float64), np.asarray(H, dtype=np.float64), np.asarray(obj, dtype=np.float64)
        F = obj - c * Ntot - fa @ N
        rnd = 64 * eps * (np.abs(obj) + np.abs(c) * Ntot + np.abs(fa) @ N + Ntot)
        return S, H, F, rnd

    rows = np.arange(R)
    S, H, F, rnd = point(f, rows)
    g_acc[:] = g
    err = np.max(np.abs(S - N) / N, axis=1)
    its = np.zeros(R, dtype=np.int64)
    done = np.zeros(R, dtype=bool)
    for it in range(max_iter + 1):
        if not np.all(np.isfinite(err)):
            r = int(np.flatnonzero(~np.isfinite(err))[0])
            raise _lib.TxmError(f"MBAR bootstrap solve: the gradient of replicate {r} is not finite")
        done |= err <= tol
        rows = np.flatnonzero(~done)
        if len(rows) == 0:
            return f, g_acc, its, n_eval, err
        if it == max_iter:
            break
        steps = np.zeros((R, K - 1))
        slopes = np.zeros(R)
        for r in rows:
            grad = S[r] - N
            Hr = (np.diag(S[r]) - H[r])[1:, 1:]
            gr = grad[1:]
            lam, V = np.linalg.eigh(0.5 * (Hr + Hr.T))
            floor = 1e-12 * max(float(lam.max()), float(N.min()))
            good = lam > floor
            proj = V.T @ gr
            step = -(V[:, good] @ (proj[good] / lam[good]))
            if not good.all():
                flat = -(V[:, ~good] @ (proj[~good] / floor))
                big = float(np.max(np.abs(flat)))
                if big > _MBAR_MAX_STEP:
                    flat *= _MBAR_MAX_STEP / big
                step = step + flat
            steps[r] = step
            slopes[r] = float(gr @ step)
        t = np.ones(R)
        pending = rows
        while len(pending):
            fn = f[pending].copy()
            fn[:, 1:] += t[pending, None] * steps[pending]
            Sn, Hn, Fn, rn = point(fn, pending)
            errn = np.max(np.abs(Sn - N) / N, axis=1)
            ok = (Fn <= F[pending] + 1e-4 * t[pending] * slopes[pending]) | \
                ((np.abs(Fn - F[pending]) <= np.maximum(rnd[pending], rn)) & (errn < err[pending]))
            acc = pending[ok]
            f[acc], S[acc], H[acc], F[acc], rnd[acc], err[acc] = fn[ok], Sn[ok], Hn[ok], Fn[ok], rn[ok], errn[ok]
            g_acc[acc] = g[acc]
            its[acc] += 1
            pending = pending[~ok]
            t[pending] *= 0.5
            if len(pending) and t[pending].min() < 1e-10:
                r = int(pending[np.argmin(t[pending])])
                raise _lib.TxmError(f"MBAR bootstrap solve: the line search of replicate {r} found no decrease at "
                                    f"iteration {it}; max |S_k - N_k| / N_k = {err[r]:.3e}")
    worst = int(rows[np.argmax(err[rows])])
    raise _lib.TxmError(f"MBAR bootstrap solve did not converge in {max_iter} Newton iterations: {len(rows)} of {R} "
                        f"replicates left, the worst is replicate {worst} with max |S_k - N_k| / N_k = "
                        f"{err[worst]:.3e} > tol {tol:.1e}")


def mbar_unpack_h(packed, K: int) -> np.ndarray:
    """The symmetric (..., K, K) Hessian term from the evaluation passes' packed upper triangle (..., K (K + 1) / 2),
    row-major: every entry is stored into both places, none is added to."""
    packed = np.asarray(packed, dtype=np.float64)
    iu = np.triu_indices(K)
    H = np.zeros((*packed.shape[:-1], K, K))
    H[..., iu[0], iu[1]] = packed
    H[..., iu[1], iu[0]] = packed
    return H


_MBAR_PINV_CUT = 1e-12   # eigenvalues of I - sqrt(N) G sqrt(N) below this fraction of the largest are its null space


def mbar_solution_g(ns, alpha0, sol: MbarSolution):
    """The shifted log-weights the solve's last evaluation ran at (``mbar_newton``'s g = b + f - max(b + f)) and the
    shift c = -max(b + f): ``sol.logD`` is ln sum_k N_k e^{f_k - alpha0_k u_n} + c."""
    a0 = np.asarray(alpha0, dtype=np.float64).reshape(-1)
    g = np.log(np.asarray(ns, dtype=np.float64)) - a0 * sol.upiv + np.asarray(sol.f, dtype=np.float64)
    c = -float(g.max())
    return g + c, c


def _sym_pinv(A: np.ndarray) -> np.ndarray:
    lam, V = np.linalg.eigh(0.5 * (A + A.T))
    keep = lam > _MBAR_PINV_CUT * max(float(np.max(np.abs(lam))), 1.0)
    return (V[:, keep] / lam[keep]) @ V[:, keep].T


def mbar_theta(G, N) -> np.ndarray:
    """Theta = W^T (I - W N W^T)^+ W from the Gram matrix G = W^T W = V L V^T alone: V S (I - S V^T N V S)^+ S V^T with
    S = L^{1/2} (negative eigenvalues of G, rounding, clipped to 0).  N: the sample count of every column, 0 for the
    columns that were not sampled (targets)."""
    G = np.asarray(G, dtype=np.float64)
    N = np.asarray(N, dtype=np.float64).reshape(-1)
    if G.shape != (len(N), len(N)):
        raise ValueError("G must be square with one row per entry of N")
    lam, V = np.linalg.eigh(0.5 * (G + G.T))
    S = np.sqrt(np.clip(lam, 0.0, None))
    VS = V * S
    A = np.eye(len(N)) - VS.T @ (N[:, None] * VS)
    return VS @ _sym_pinv(A) @ VS.T


def mbar_reduced_pinv(Gs, N) -> np.ndarray:
    """(I_K - sqrt(N) G_s sqrt(N))^+ of the sampled block: singular along sqrt(N) by construction (the rows of the
    overlap matrix sum to 1), hence a pseudo-inverse.  Taken once per model."""
    rn = np.sqrt(np.asarray(N, dtype=np.float64).reshape(-1))
    Gs = np.asarray(Gs, dtype=np.float64)
    return _sym_pinv(np.eye(len(rn)) - rn[:, None] * Gs * rn[None, :])


def mbar_mean_variance(Gs, N, yy, b, *, pinv=None) -> np.ndarray:
    """var of an MBAR average at a target from the K x K block alone: with y_n = W_na (x_n - <x>_a), the unsampled column
    y has Theta_yy = yy + (sqrt(N) b)^T (I_K - sqrt(N) G_s sqrt(N))^+ (sqrt(N) b), yy = sum_n y_n^2 and
    b_k = sum_n W_nk y_n.  ``yy`` (...,) and ``b`` (..., K) broadcast; ``pinv``: ``mbar_reduced_pinv(Gs, N)`` if the
    caller keeps it."""
    rn = np.sqrt(np.asarray(N, dtype=np.float64).reshape(-1))
    P = mbar_reduced_pinv(Gs, N) if pinv is None else pinv
    rb = np.asarray(b, dtype=np.float64) * rn
    return np.asarray(yy, dtype=np.float64) + np.einsum("...j,jk,...k->...", rb, P, rb)


def mbar_mean_covariance(Gs, N, gram, b, *, pinv=None) -> np.ndarray:
    """cov of MBAR averages from the K x K block alone: Theta is bilinear in the unsampled columns, so two of them,
    y_i and y_j, have Theta_ij = gram_ij + (sqrt(N) b_i)^T (I_K - sqrt(N) G_s sqrt(N))^+ (sqrt(N) b_j) with
    gram_ij = sum_n y_ni y_nj and b_ik = sum_n W_nk y_ni.  ``gram`` (..., M, M) and ``b`` (..., M, K): the leading axes
    broadcast; the diagonal is ``mbar_mean_variance``.  The second term is averaged with its transpose, so a symmetric
    ``gram`` gives an exactly symmetric result.  ``pinv``: ``mbar_reduced_pinv(Gs, N)`` if the caller keeps it."""
    rn = np.sqrt(np.asarray(N, dtype=np.float64).reshape(-1))
    P = mbar_reduced_pinv(Gs, N) if pinv is None else pinv
    rb = np.asarray(b, dtype=np.float64) * rn
    q = np.einsum("...ik,kl,...jl->...ij", rb, P, rb)
    return np.asarray(gram, dtype=np.float64) + 0.5 * (q + np.swapaxes(q, -1, -2))


def mbar_overlap(Gs, N):
    """The overlap matrix O = G_s diag(N) of the sampled states (rows sum to 1), its eigenvalues in descending order --
    those of the symmetric sqrt(N) G_s sqrt(N), which is similar to O -- and the scalar 1 - the second largest
    (1 for a single state)."""
    Gs = np.asarray(Gs, dtype=np.float64)
    N = np.asarray(N, dtype=np.float64).reshape(-1)
    rn = np.sqrt(N)
    ev = np.linalg.eigvalsh(rn[:, None] * (0.5 * (Gs + Gs.T)) * rn[None, :])[::-1].copy()
    return Gs * N[None, :], ev, (float(1.0 - ev[1]) if len(ev) > 1 else 1.0)


# ---- reweighted histograms (MBARModel.histogram; include/txmom.h txm_mbar_hist) -----------------------------------------
# For indicator columns 1_b every sum of the covariance is a weighted histogram over the classes (the nbins bins, then the
# class of the samples outside the range): H_b = sum_n W_na 1_b, S_b = sum_n W_na^2 1_b, T_kb = sum_n W_nk W_na 1_b.  Every
# complement below is a sum over the OTHER classes -- additions of non-negative numbers only, never 1 - p or Q - S_b -- so
# a bin that holds 99.9 % of the weight keeps full relative accuracy.

def _sum_of_others(v: np.ndarray) -> np.ndarray:
    """out[..., b] = sum_{b'' != b} v[..., b''] by additions alone (the entries before b, then the entries after it)."""
    v = np.asarray(v, dtype=np.float64)
    out = np.zeros_like(v)
    out[..., 1:] += np.cumsum(v, axis=-1)[..., :-1]
    out[..., :-1] += np.cumsum(v[..., ::-1], axis=-1)[..., ::-1][..., 1:]
    return out


def _sum_without_pairs(v: np.ndarray) -> np.ndarray:
    """out[b, b'] = sum_{b'' not in (b, b')} v[b''] for b < b' (0 elsewhere) by additions alone: the entries before b, the
    entries strictly between (a running sum along row b) and the entries after b'."""
    v = np.asarray(v, dtype=np.float64)
    m = len(v)
    before = np.concatenate([[0.0], np.cumsum(v)[:-1]])
    after = np.concatenate([np.cumsum(v[::-1])[::-1][1:], [0.0]])
    run = np.cumsum(np.triu(np.broadcast_to(v, (m, m)), 1), axis=1)      # run[b, j] = sum_{b < i <= j} v[i]
    between = np.zeros((m, m))
    between[:, 1:] = run[:, :-1]
    return np.triu(before[:, None] + between + after[None, :], 1)


def mbar_hist_terms(H, S, T):
    """The diagonal of the Gram matrix and the b vectors of the bins from the class sums of one or more targets:
    ``H``, ``S`` (..., nbins + 1) and ``T`` (..., K, nbins + 1), the last class the samples outside the range.  Returns
    (yy (..., nbins), b (..., nbins, K)):  yy_b = (1 - p_b)^2 S_b + p_b^2 (Q - S_b),
    b_k,b = (1 - p_b) T_kb - p_b (B_k - T_kb), every complement a sum over the other classes."""
    H, S, T = (np.asarray(a, dtype=np.float64) for a in (H, S, T))
    p, q, rest_s, rest_t = H[..., :-1], _sum_of_others(H)[..., :-1], _sum_of_others(S)[..., :-1], _sum_of_others(T)[..., :-1]
    yy = q * q * S[..., :-1] + p * p * rest_s
    b = q[..., None, :] * T[..., :-1] - p[..., None, :] * rest_t
    return yy, np.swapaxes(b, -1, -2)


def mbar_hist_variance(Gs, N, H, S, T, *, pinv=None) -> np.ndarray:
    """var of every bin of a reweighted histogram, (..., nbins): ``mbar_mean_variance`` of ``mbar_hist_terms``."""
    yy, b = mbar_hist_terms(H, S, T)
    return mbar_mean_variance(Gs, N, yy, b, pinv=pinv)


def mbar_hist_covariance(Gs, N, H, S, T, *, pinv=None) -> np.ndarray:
    """The asymptotic covariance between the bins of a reweighted histogram, (n_alpha, nbins, nbins), from the class sums
    of ``engine.mbar_hist_sums`` (``H``, ``S`` (n_alpha, nbins + 1), ``T`` (n_alpha, K, nbins + 1)) through
    ``mbar_mean_covariance``.  The Gram matrix of the indicator columns d_b = 1_b - p_b in closed form:
        gram_bb  = (1 - p_b)^2 S_b + p_b^2 (Q - S_b)
        gram_bb' = -p_b' (1 - p_b) S_b - p_b (1 - p_b') S_b' + p_b p_b' (Q - S_b - S_b')       (b != b')
    with 1 - p_b, Q - S_b and Q - S_b - S_b' sums over the other classes; the upper triangle is mirrored, so the result
    is exactly symmetric."""
    H, S, T = (np.asarray(a, dtype=np.float64) for a in (H, S, T))
    if H.ndim != 2 or S.shape != H.shape or T.ndim != 3 or T.shape[0] != H.shape[0] or T.shape[2] != H.shape[1]:
        raise ValueError("H and S must be (n_alpha, nbins + 1) and T (n_alpha, K, nbins + 1)")
    na, nb = H.shape[0], H.shape[1] - 1
    yy, b = mbar_hist_terms(H, S, T)
    q = _sum_of_others(H)[:, :-1]
    gram = np.empty((na, nb, nb))
    for a in range(na):
        p, s = H[a, :-1], S[a, :-1]
        rest = _sum_without_pairs(S[a])[:nb, :nb]
        ps = q[a] * s
        up = np.triu(-(ps[:, None] * p[None, :]) - (p[:, None] * ps[None, :]) + (p[:, None] * p[None, :]) * rest, 1)
        gram[a] = up + up.T + np.diag(yy[a])
    return mbar_mean_covariance(Gs, N, gram, b, pinv=pinv)


# ---- blocked (batch-means) error bars for correlated series kept whole (include/txmom.h txm_mbar_block_cov) -------------
# Give sample n the mass 1 + eps_n in every sum over samples (N_k in the denominators fixed).  To first order an MBAR
# estimate moves by sum_n eps_n phi_n, and every influence phi_n is linear in the row
#   t_n = (W_n1 .. W_nK, {W_na, y_n,(a,0) .. y_n,(a,C-1)} for each target a),      M = K + n_alpha (C + 1) columns:
#   average            phi_n(a, c)       = y_n,(a,c) + c_ac^T W_n.,   c_ac = sqrt(N) P sqrt(N) b_ac
#   sampled state      phi_n(f_i - f_0)  = -[R W_n.]_i + [R W_n.]_0,  R = N^{-1/2} P N^{1/2}
#   target             phi_n(f_a - f_0)  = -W_na - (sqrt(N) P sqrt(N) B_a)^T W_n. + [R W_n.]_0
# with P = (I_K - sqrt(N) G_s sqrt(N))^+ (mbar_reduced_pinv).  The builders below return the coefficient vectors l as rows
# of a matrix L over the M columns; with Gamma the Gram matrix of the per-state-centred block sums of t_n (one stationary
# series per state, independent states) the covariance of the estimates is L Gamma L^T.  No nb / (nb - 1) factor; a state
# with a single block contributes exactly zero.

def mbar_block_width(K: int, n_alpha: int, C: int) -> int:
    """Columns of the row t_n: the K sampled states, then per target its weight and its C centred products."""
    return int(K) + int(n_alpha) * (int(C) + 1)


def _block_pinv(Gs, N, pinv):
    N = np.asarray(N, dtype=np.float64).reshape(-1)
    return N, np.sqrt(N), (mbar_reduced_pinv(Gs, N) if pinv is None else np.asarray(pinv, dtype=np.float64))


def mbar_block_coef_mean(Gs, N, b, *, pinv=None) -> np.ndarray:
    """L (n_alpha * C, M) of the averages <x_c>(a), row a C + c: 1 at y_(a,c) and c_ac on the K sampled columns.
    ``b`` (n_alpha, C, K): ``engine.mbar_cov_sums``' b for the targets of the Gamma call, in its order."""
    N, rn, P = _block_pinv(Gs, N, pinv)
    b = np.asarray(b, dtype=np.float64)
    na, C, K = b.shape
    L = np.zeros((na, C, mbar_block_width(K, na, C)))
    L[:, :, :K] = ((b * rn) @ P) * rn
    for a in range(na):
        L[a, np.arange(C), K + a * (C + 1) + 1 + np.arange(C)] = 1.0
    return L.reshape(na * C, -1)


def mbar_block_coef_sampled(Gs, N, M: int | None = None, *, pinv=None) -> np.ndarray:
    """L (K, M) of the sampled states' f_i - f_0 (row 0 is zero): -R_i. + R_0. on the K sampled columns."""
    N, rn, P = _block_pinv(Gs, N, pinv)
    K = len(N)
    R = (P * rn[None, :]) / rn[:, None]
    L = np.zeros((K, K if M is None else int(M)))
    L[:, :K] = R[0][None, :] - R
    L[0] = 0.0
    return L


def mbar_block_coef_target(Gs, N, B, C: int, *, pinv=None) -> np.ndarray:
    """L (n_alpha, M) of the targets' f_a - f_0: -1 at W_na, -(sqrt(N) P sqrt(N) B_a) + R_0. on the K sampled columns.
    ``B`` (n_alpha, K): ``engine.mbar_cov_sums``' B for the targets of the Gamma call, in its order."""
    N, rn, P = _block_pinv(Gs, N, pinv)
    B = np.asarray(B, dtype=np.float64)
    na, K = B.shape
    R0 = (P[0] * rn) / rn[0]
    L = np.zeros((na, mbar_block_width(K, na, C)))
    L[:, :K] = R0[None, :] - ((B * rn) @ P) * rn
    L[np.arange(na), K + np.arange(na) * (int(C) + 1)] = -1.0
    return L


def _block_lg(gamma, L):
    gamma = np.asarray(gamma, dtype=np.float64)
    L = np.asarray(L, dtype=np.float64)
    if L.ndim != 2 or gamma.ndim < 2 or gamma.shape[-1] != L.shape[-1] or gamma.shape[-2] != L.shape[-1]:
        raise ValueError(f"gamma {gamma.shape} does not match L {L.shape}: need (..., M, M) and (R, M)")
    return np.matmul(L, gamma), L


def mbar_block_covariance(gamma, L) -> np.ndarray:
    """L Gamma L^T for ``gamma`` (..., M, M) and ``L`` (R, M): (..., R, R), symmetrised so that a symmetric Gamma gives
    an exactly symmetric result."""
    LG, L = _block_lg(gamma, L)
    c = np.matmul(LG, L.T)
    return 0.5 * (c + np.swapaxes(c, -1, -2))


def mbar_block_variance(gamma, L) -> np.ndarray:
    """The diagonal of ``mbar_block_covariance``: l_r^T Gamma l_r for every row of ``L``, (..., R)."""
    LG, L = _block_lg(gamma, L)
    return np.einsum("...ri,ri->...r", LG, L)
