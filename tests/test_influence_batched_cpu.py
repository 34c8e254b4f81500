"""txm_influence_cov_batched without a device: the host struct against its ctypes mirror, the workspace query, the entry's
validation -- and the variance formulas of InterpModel / ExtrapWeightedModel.predict_with_error restated in numpy against a
brute-force g' blockdiag(V) g on synthetic per-state covariances."""

from __future__ import annotations

import ctypes as ct
import math
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def lib():
    from thermoextrap_amd import _build, _lib

    _build.build_library()
    return _lib.load()


def test_inf_state_layout_matches_the_header():
    from thermoextrap_amd import _lib

    text = (ROOT / "include" / "txmom.h").read_text()
    body = re.search(r"typedef struct txm_inf_state \{(.*?)\} txm_inf_state;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [m.group(1) for m in re.finditer(r"(\w+);", body)]
    assert fields == [f[0] for f in _lib.InfState._fields_] == ["x", "u", "w", "n"]
    S = _lib.InfState
    assert (S.x.offset, S.u.offset, S.w.offset, S.n.offset) == (0, 8, 16, 24) and ct.sizeof(S) == 32
    assert S.n.size == 8
    sig = _lib.SIGNATURES["txm_influence_cov_batched"]
    assert sig[1][0] == ct.POINTER(_lib.InfState) and len(sig[1]) == 15


def test_workspace_query_is_host_logic(lib):
    W = lib.txm_influence_cov_batched_ws_bytes
    w1, w3, w64 = W(1, 1000, 4, 4), W(3, 1000, 4, 4), W(64, 1000, 4, 4)
    assert 0 < w1 < w3 < w64
    assert W(64, 10**6, 4, 4) > w64 and W(64, 10**6, 4, 9) > W(64, 10**6, 4, 4)
    # a state never needs more partials than the single call's workspace holds
    assert W(1, 10**9, 4, 4) <= lib.txm_influence_cov_ws_bytes(10**9, 4, 4) + 512
    assert W(65535, 40, 4, 3) > 0
    for bad in ((0, 1000, 4, 4), (65536, 1000, 4, 4), (3, 0, 4, 4), (3, 1000, 0, 4), (3, 1000, 70000, 4), (3, 1000, 4, 0),
                (3, 1000, 4, 10), (-1, 1000, 4, 4)):
        assert W(*bad) == 0, bad


def test_entry_validates_without_a_device(lib):
    """Argument errors come back as TXM_ERR_INVALID (-1) / TXM_ERR_WORKSPACE (-3) before any HIP call."""
    from thermoextrap_amd import _lib

    p = ct.c_void_p(256)      # never dereferenced: every call below fails validation first
    names = ("tab", "S", "ls", "C", "nf", "nq", "cu", "cx", "a", "b", "cov", "mean", "ws", "wsb", "st")

    def table(ns=(10, 7, 12), w=(None, None, None), x=(256, 512, 768)):
        t = (_lib.InfState * len(ns))()
        for s, n in enumerate(ns):
            t[s].x, t[s].u, t[s].w, t[s].n = x[s], 1024, w[s], n
        return t

    good = dict(tab=table(), S=3, ls=4, C=4, nf=3, nq=3, cu=p, cx=p, a=p, b=p, cov=p, mean=p, ws=p, wsb=1 << 30, st=None)

    def call(**bad):
        return lib.txm_influence_cov_batched(*[{**good, **bad}[n] for n in names])

    assert call(tab=None) == -1 and b"null" in lib.txm_last_error()
    for k in ("cu", "cx", "a", "b", "cov", "mean", "ws"):
        assert call(**{k: None}) == -1 and b"null" in lib.txm_last_error(), k
    assert call(S=0) == -1 and call(S=65536) == -1
    assert call(C=0) == -1 and call(C=70000, ls=70000) == -1
    assert call(nf=10) == -1 and b"n_f" in lib.txm_last_error()
    assert call(nq=0) == -1 and b"n_q" in lib.txm_last_error()
    assert call(ls=3) == -1 and b"pitch" in lib.txm_last_error()
    assert call(tab=table(ns=(10, 0, 12))) == -1 and b"state 1" in lib.txm_last_error()
    assert call(tab=table(x=(256, None, 768))) == -1 and b"state 1" in lib.txm_last_error()
    assert call(tab=table(w=(2048, None, 2048))) == -1 and b"weights" in lib.txm_last_error()
    assert call(tab=table(w=(None, 2048, None))) == -1 and b"weights" in lib.txm_last_error()
    assert call(wsb=8) == -3 and b"workspace" in lib.txm_last_error()


# ---- the variance formulas of predict_with_error, in numpy -----------------------------------------------------------
def _spd(rng, n):
    m = rng.normal(size=(n, n))
    return m @ m.T + 0.1 * np.eye(n)


def _hermite_rows(alpha0, order):
    """The matrix InterpModel._hermite_inverse inverts: row (s, j) = d^j/da^j a^p at alpha0_s."""
    npoly = len(alpha0) * (order + 1)
    p = np.arange(npoly)
    rows = []
    for a0 in alpha0:
        for j in range(order + 1):
            fall = np.array([math.perm(int(q), j) if q >= j else 0 for q in p], dtype=float)
            rows.append(fall * np.where(p >= j, np.power(float(a0), np.maximum(p - j, 0)), 0.0))
    return np.array(rows)


def _blockdiag(Vs):
    n = sum(v.shape[0] for v in Vs)
    out, k = np.zeros((n, n)), 0
    for v in Vs:
        out[k:k + v.shape[0], k:k + v.shape[0]] = v
        k += v.shape[0]
    return out


@pytest.mark.parametrize("S,order", [(2, 2), (3, 1), (4, 3)])
def test_interp_variance_is_the_block_diagonal_quadratic_form(S, order):
    """var = sum_s g_s' V_s g_s with g = (alpha^p) . hermite_inverse equals g' blockdiag(V) g, and g' D is the polynomial
    through the stacked derivatives D -- so the form is the variance of predict for independent states."""
    rng = np.random.default_rng(S * 10 + order)
    alpha0 = np.sort(rng.uniform(0.2, 0.9, S))
    inv = np.linalg.inv(_hermite_rows(alpha0, order))
    Vs = [_spd(rng, order + 1) for _ in range(S)]
    D = rng.normal(size=S * (order + 1))
    for alpha in (0.1, 0.45, 1.2):
        g = (alpha ** np.arange(inv.shape[0])) @ inv
        gs = g.reshape(S, order + 1)
        var = sum(gs[s] @ Vs[s] @ gs[s] for s in range(S))
        brute = g @ _blockdiag(Vs) @ g
        assert abs(var - brute) <= 1e-12 * brute
        # predict = (alpha^p) . (inv . D) = g . D: the two orders of one product, apart by rounding only
        # (first-order bound of either: eps * n * |alpha^p| |inv| |D|, n = 16 terms at the most)
        pw = alpha ** np.arange(inv.shape[0])
        assert abs(g @ D - pw @ (inv @ D)) <= 1e-14 * (np.abs(pw) @ np.abs(inv) @ np.abs(D))


def test_weighted_variance_is_the_block_diagonal_quadratic_form():
    """var = sum_i (w_i / sum w)^2 t_i' V_i t_i equals h' blockdiag(V_0, V_1) h with h = [w_0 t_0, w_1 t_1] / sum w."""
    rng = np.random.default_rng(5)
    order, a0 = 3, np.array([0.4, 0.7])
    Vs = [_spd(rng, order + 1) for _ in range(2)]
    fact = np.array([math.factorial(k) for k in range(order + 1)], dtype=float)
    for alpha in (0.3, 0.4, 0.55, 0.69, 0.9):
        dm = np.abs(alpha - a0) ** 20
        w = 1.0 - dm / dm.sum()
        t = [(alpha - a0[i]) ** np.arange(order + 1) / fact for i in range(2)]
        var = sum((w[i] / w.sum()) ** 2 * t[i] @ Vs[i] @ t[i] for i in range(2))
        h = np.concatenate([w[0] * t[0], w[1] * t[1]]) / w.sum()
        brute = h @ _blockdiag(Vs) @ h
        assert abs(var - brute) <= 1e-12 * brute
    # at a state the other state's weight is zero: the variance is that state's V[0, 0]
    dm = np.abs(0.4 - a0) ** 20
    w = 1.0 - dm / dm.sum()
    assert w[0] == 1.0 and w[1] == 0.0


def test_collection_methods_exist():
    """The public names of the feature (they run on the GPU: tests/test_states_delta_gpu.py)."""
    from thermoextrap_amd import engine, models

    assert callable(engine.influence_cov_batched)
    assert callable(models.StateCollection.derivs_cov)
    for cls in (models.InterpModel, models.InterpModelPiecewise, models.ExtrapWeightedModel):
        assert callable(cls.predict_with_error)
