"""Shared reference code of the cross-column delta-method tests (test_influence_cross_cpu.py, test_influence_cross_gpu.py):
the definition of DESIGN 4.14 restated in long double on top of tests/_influence_ref.py.  Not a test module."""

from __future__ import annotations

import numpy as np

from tests._influence_ref import LD, bound_ld, psi_ld


def cross_cov_ld(p, psi):
    """V[c, i, c', j] = sum_n p_n^2 psi[c, i, n] psi[c', j, n] in long double (psi: [C, n_f, N])."""
    C, nf, N = psi.shape
    flat = psi.reshape(C * nf, N)
    return ((flat * (p * p)[None, :]) @ flat.T).reshape(C, nf, C, nf)


def psi_and_bound(x, u, w, a, b, cu, cx, cols=None):
    """(p, psi [C', n_f, N], B [C', n_f, N]) of the kernel's operands in long double: centres (cu, cx) as given, rows of
    weight zero selected out, total weight zero -> p = 0.  ``cols``: only these columns (C' = len(cols))."""
    N, C = x.shape
    cols = range(C) if cols is None else cols
    wl = np.ones(N, LD) if w is None else np.asarray(w, LD)
    live = wl != 0
    tot = wl.sum()
    p = wl / tot if tot != 0 else wl
    du = np.where(live, np.asarray(u, LD) - LD(cu), LD(0))
    psi, B = [], []
    for c in cols:
        dx = np.where(live, np.asarray(x[:, c], LD) - LD(cx[c]), LD(0))
        psi.append(psi_ld(a[c], b[c], dx, du))
        B.append(bound_ld(a[c], b[c], dx, du))
    return p, np.stack(psi), np.stack(B)


def reference(x, u, w, a, b, cu, cx, cols=None):
    """(V, bound), both [C', n_f, C', n_f]: the definition and sum_n p_n^2 B_i(n, c) B_j(n, c')."""
    p, psi, B = psi_and_bound(x, u, w, a, b, cu, cx, cols)
    return cross_cov_ld(p, psi), cross_cov_ld(p, B)
