"""The host side of the cross-column delta-method covariance of state collections, without a device: the
workspace and grid queries of txm_influence_cross_cov_batched against the plan rule restated in Python, every refusal of
the entry point, its binding against the header, and the three predict_cov contractions (InterpModel,
InterpModelPiecewise, ExtrapWeightedModel) against a brute-force G' blockdiag(V) G on random symmetric V_s with the device
call stubbed."""

from __future__ import annotations

import ctypes as ct
import math
import re
from pathlib import Path

import numpy as np
import pytest

HEADER = Path(__file__).resolve().parents[1] / "include" / "txmom.h"


def _lib_and_cus():
    """The library and the compute units it plans with: one tile pair and one state may take 8 workgroups per CU."""
    from thermoextrap_amd import _lib

    lib = _lib.load()
    q = lib.txm_influence_cross_cov_batched_grid(1, 10**12, 1)
    assert q >= 8 and q % 8 == 0
    return lib, q // 8


def _pairs(C):
    T = (C + 1 + 15) // 16
    return T * (T + 1) // 2


def _grid(S, n, C, cus):
    """The plan rule of include/txmom.h (f-14) restated."""
    q = max(1, 8 * cus // (_pairs(C) * S))
    return min(-(-n // 256), q)


SHAPES = [(1, 1, 1), (1, 70000, 4), (3, 1537, 33), (4, 10**6, 255), (64, 10**6, 4), (70, 40, 4), (70, 100000, 4),
          (2048, 257, 1), (5000, 10**5, 15), (65535, 10**7, 255), (17, 256, 16), (17, 257, 16)]


def test_grid_query_is_the_plan_rule():
    lib, cus = _lib_and_cus()
    for S, n, C in SHAPES:
        assert lib.txm_influence_cross_cov_batched_grid(S, n, C) == _grid(S, n, C, cus), (S, n, C)
    # q never exceeds the single call's cap, and S = 1 IS the single plan
    for C in (1, 15, 16, 33, 255):
        cap = max(1, 8 * cus // _pairs(C))
        for S in (1, 2, 64, 4000):
            assert lib.txm_influence_cross_cov_batched_grid(S, 10**12, C) <= cap
        assert lib.txm_influence_cross_cov_batched_grid(1, 10**12, C) == cap
    for bad in [(0, 10, 4), (65536, 10, 4), (3, 0, 4), (3, 10, 0), (3, 10, 256), (-1, 10, 4)]:
        assert lib.txm_influence_cross_cov_batched_grid(*bad) == 0, bad


def test_workspace_query_is_host_logic():
    """S (grid + 1) pairs records of 8 (256 (2 n_q - 1) + 8) bytes, the 256-byte-aligned table of 48-byte state records
    and 256 bytes; 0 for each bad argument; nondecreasing in n_max; never below the records the plan writes."""
    lib, cus = _lib_and_cus()
    Q = lib.txm_influence_cross_cov_batched_ws_bytes
    for S, n, C in SHAPES:
        for nf, nq in ((1, 1), (4, 4), (3, 5), (9, 9)):
            rec = 8 * (256 * (2 * nq - 1) + 8)
            written = S * (_grid(S, n, C, cus) + 1) * _pairs(C) * rec
            got = Q(S, n, C, nf, nq)
            assert got >= written + 256 + S * 8 * 4, (S, n, C, nf, nq)
            assert got == written + -(-S * 48 // 256) * 256 + 256, (S, n, C, nf, nq)
    if cus == 256:
        assert 29 * 10**6 <= Q(64, 10**6, 4, 4, 4) <= 32 * 10**6                 # "about 30 MB" at 64 x 1e6 x 4, order 3
    for bad in [(0, 10, 4, 3, 3), (65536, 10, 4, 3, 3), (3, 0, 4, 3, 3), (3, -5, 4, 3, 3), (3, 10, 0, 3, 3), (3, 10, 256, 3, 3),
                (3, 10, 4, 0, 3), (3, 10, 4, 10, 3), (3, 10, 4, 3, 0), (3, 10, 4, 3, 10)]:
        assert Q(*bad) == 0, bad
    for S, C in ((1, 4), (3, 33), (64, 4), (70, 255)):
        sizes = [Q(S, n, C, 4, 4) for n in (1, 2, 255, 256, 257, 1000, 10**4, 10**5, 10**6, 10**9, 10**15)]
        assert all(s0 <= s1 for s0, s1 in zip(sizes, sizes[1:])), (S, C)
    # a ragged batch writes no more than the query at its longest state allows
    for S, C, ns in ((4, 255, (5000, 40, 256, 9000)), (70, 4, (40,) * 68 + (10**5, 10**5))):
        rec = 8 * (256 * 7 + 8)
        written = sum((_grid(S, n, C, cus) + 1) * _pairs(C) * rec for n in ns)
        assert written + -(-S * 48 // 256) * 256 <= Q(S, max(ns), C, 4, 4)


def test_entry_point_validates_without_a_device():
    """Every refusal comes back before any HIP call, one case each."""
    from thermoextrap_amd import _lib

    lib = _lib.load()
    p = 0x10000   # never dereferenced: every call below fails validation first

    def states(S=3, n=(10, 20, 30), w=(None, None, None), x=(p, p, p), u=(p, p, p)):
        tab = (_lib.InfState * max(S, 1))()
        for s in range(min(max(S, 1), len(n))):
            tab[s].x, tab[s].u, tab[s].w, tab[s].n = x[s], u[s], w[s], n[s]
        return tab

    names = ("tab", "S", "ls", "C", "nf", "nq", "cu", "cx", "a", "b", "cov", "ws", "wsb", "st")
    vp = ct.c_void_p(p)
    good = dict(tab=states(), S=3, ls=4, C=4, nf=3, nq=3, cu=vp, cx=vp, a=vp, b=vp, cov=vp, ws=vp, wsb=1 << 30, st=None)

    def call(**bad):
        return lib.txm_influence_cross_cov_batched(*[{**good, **bad}[n] for n in names])

    for ptr in ("tab", "cu", "cx", "a", "b", "cov", "ws"):
        assert call(**{ptr: None}) == -1 and b"null" in lib.txm_last_error(), ptr
    assert call(S=0) == -1 and b"S=" in lib.txm_last_error()
    assert call(S=65536) == -1 and b"S=" in lib.txm_last_error()
    assert call(C=0) == -1 and b"C=" in lib.txm_last_error()
    assert call(C=256, ls=256) == -1 and b"255" in lib.txm_last_error()
    assert call(nf=0) == -1 and call(nf=10) == -1 and b"n_f" in lib.txm_last_error()
    assert call(nq=0) == -1 and call(nq=10) == -1 and b"n_q" in lib.txm_last_error()
    assert call(ls=3) == -1 and b"pitch" in lib.txm_last_error()
    assert call(tab=states(n=(10, 0, 30))) == -1 and b"n=0" in lib.txm_last_error()
    assert call(tab=states(n=(10, 20, -1))) == -1
    assert call(tab=states(x=(p, None, p))) == -1 and b"null" in lib.txm_last_error()
    assert call(tab=states(u=(p, p, None))) == -1 and b"null" in lib.txm_last_error()
    assert call(tab=states(w=(p, None, p))) == -1 and b"weights" in lib.txm_last_error()
    assert call(tab=states(w=(None, p, None))) == -1 and b"weights" in lib.txm_last_error()
    for S, n, C, nf, nq in [(3, (10, 20, 30), 4, 3, 3), (3, (10, 10**6, 30), 33, 2, 9)]:
        need = lib.txm_influence_cross_cov_batched_ws_bytes(S, max(n), C, nf, nq)
        assert call(tab=states(n=n), C=C, ls=C, nf=nf, nq=nq, wsb=need - 1) == -3 and b"workspace" in lib.txm_last_error()


def test_symbols_bound_with_the_header_signature():
    from thermoextrap_amd import _lib

    text = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    ctype = {"int64_t": ct.c_int64, "int": ct.c_int, "double": ct.c_double, "size_t": ct.c_size_t, "txm_stream": ct.c_void_p}
    ret = {"size_t": ct.c_size_t, "int": ct.c_int}
    lib = _lib.load()
    for name in ("txm_influence_cross_cov_batched_ws_bytes", "txm_influence_cross_cov_batched_grid",
                 "txm_influence_cross_cov_batched"):
        m = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, name
        args = []
        for arg in m.group(2).split(","):
            arg = arg.strip()
            if "txm_inf_state" in arg:
                args.append(ct.POINTER(_lib.InfState))
            else:
                args.append(ct.c_void_p if "*" in arg else ctype[arg.replace("const ", "").split()[0]])
        res, bound = _lib.SIGNATURES[name]
        assert res is ret[m.group(1)] and list(bound) == args, name
        assert getattr(lib, name).argtypes == args
    assert lib.txm_abi_version() == 2 == _lib.ABI_VERSION
    section = HEADER.read_text().split("(f-14)")[1]
    assert "not stream-capturable" in section and "NOT checked" in section and "BIT FOR BIT" in section


# ---- the predict_cov contractions on a stubbed device result ---------------------------------------------------------------
ORDER, C = 2, 3
ALPHA0 = (0.4, 0.5, 0.6)
ALPHAS = [0.3, 0.43, 0.5, 0.58, 0.7]


class _StubState:
    """What the collections read of a state, and nothing that launches."""

    def __init__(self, alpha0):
        self.alpha0, self.order, self.minus_log, self.alpha_name = alpha0, ORDER, False, "beta"


def _stubbed(cls, nstates, monkeypatch):
    """(model, [V_s]): a collection whose per-state covariances are random symmetric positive matrices and whose
    ``predict`` is a sentinel."""
    from thermoextrap_amd import models

    rng = np.random.default_rng(nstates)
    M = C * (ORDER + 1)
    V = []
    for _ in range(nstates):
        g = rng.normal(size=(M, M))
        V.append((g @ g.T).reshape(C, ORDER + 1, C, ORDER + 1))
    src = models._HostSource(["val"], [C], {"val": (("val",), np.arange(C) + 0.5)}, None)
    m = cls([_StubState(a) for a in ALPHA0[:nstates]])
    monkeypatch.setattr(cls, "_state_cross_covs", lambda self, order=None, minus_log=None, block=None:
                        ([v.copy() for v in V], [src] * nstates, [ORDER] * nstates))
    monkeypatch.setattr(cls, "predict", lambda self, alpha, **kw: "prediction")
    return m, V


def _hermite_g(alpha0, order, alphas):
    npoly = len(alpha0) * (order + 1)
    p = np.arange(npoly)
    rows = []
    for a0 in alpha0:
        for j in range(order + 1):
            fall = np.array([math.perm(int(q), j) if q >= j else 0 for q in p], dtype=float)
            rows.append(fall * np.where(p >= j, np.power(float(a0), np.maximum(p - j, 0)), 0.0))
    return (np.asarray(alphas, float)[:, None] ** p[None, :]) @ np.linalg.inv(np.array(rows))


def _brute(G, Vs):
    """G' blockdiag(V) G: G [S (order + 1)] the weights of the stacked derivatives of ONE column, the same for every
    column; V as a (S C (order + 1))^2 block-diagonal matrix over the states."""
    S, n1 = len(Vs), ORDER + 1
    big = np.zeros((S * C * n1, S * C * n1))
    for s, v in enumerate(Vs):
        big[s * C * n1:(s + 1) * C * n1, s * C * n1:(s + 1) * C * n1] = v.reshape(C * n1, C * n1)
    out = np.zeros((C, C))
    for c in range(C):
        for d in range(C):
            gc, gd = np.zeros(S * C * n1), np.zeros(S * C * n1)
            for s in range(S):
                gc[s * C * n1 + c * n1:s * C * n1 + (c + 1) * n1] = G[s * n1:(s + 1) * n1]
                gd[s * C * n1 + d * n1:s * C * n1 + (d + 1) * n1] = G[s * n1:(s + 1) * n1]
            out[c, d] = gc @ big @ gd
    return out


def _close(got, want):
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-9 * np.abs(want).max())


def test_interp_model_contraction(monkeypatch):
    from thermoextrap_amd import models

    m, V = _stubbed(models.InterpModel, 3, monkeypatch)
    pred, cov = m.predict_cov(ALPHAS)
    assert pred == "prediction"
    assert cov.dims == ("beta", "val", "val_2") and cov.shape == (len(ALPHAS), C, C)
    G = _hermite_g(ALPHA0, ORDER, ALPHAS)
    for k in range(len(ALPHAS)):
        _close(cov.values[k], _brute(G[k], V))
        assert np.allclose(cov.values[k], cov.values[k].T, rtol=1e-12)
    assert np.array_equal(cov["beta"].values, ALPHAS) and np.array_equal(cov["val_2"].values, np.arange(C) + 0.5)
    _, one = m.predict_cov(0.47)
    assert one.dims == ("val", "val_2")
    _close(one.values, _brute(_hermite_g(ALPHA0, ORDER, [0.47])[0], V))
    with pytest.raises(ValueError):
        m._predict_cov_from(0.47, ORDER, "beta", V[:2], None)


@pytest.mark.parametrize("method", ["between", "nearest"])
def test_piecewise_contraction(monkeypatch, method):
    from thermoextrap_amd import models

    m, V = _stubbed(models.InterpModelPiecewise, 3, monkeypatch)
    a0 = np.array(ALPHA0)
    for alpha in (ALPHAS, 0.47):
        pred, cov = m.predict_cov(alpha, method=method)
        seq = np.atleast_1d(alpha)
        assert pred == "prediction" and cov.shape == (*np.shape(alpha), C, C)
        for k, a in enumerate(seq):
            if method == "nearest":
                idx = [int(i) for i in np.argsort(np.abs(a0 - a))[:2]]
            else:
                i = min(max(int(np.searchsorted(a0, a, side="right")) - 1, 0), 1)
                idx = [i, i + 1]
            G = _hermite_g(a0[idx], ORDER, [a])[0]
            _close(cov.values.reshape(len(seq), C, C)[k], _brute(G, [V[i] for i in idx]))
    pairs = [v for k, v in m._cache.items() if k[0] == "pair"]
    assert pairs and all(k[0] == "hermite" for pair in pairs for k in pair._cache)      # no covariance in a pair's cache
    with pytest.raises(ValueError):
        m.predict_cov(0.9, bounded=True)


@pytest.mark.parametrize("nstates", [2, 3])
def test_weighted_contraction(monkeypatch, nstates):
    from thermoextrap_amd import models

    m, V = _stubbed(models.ExtrapWeightedModel, nstates, monkeypatch)
    a0 = np.array(ALPHA0[:nstates])
    pred, cov = m.predict_cov(ALPHAS)
    assert pred == "prediction" and cov.dims == ("beta", "val", "val_2")
    fact = np.array([math.factorial(k) for k in range(ORDER + 1)], float)
    for k, a in enumerate(ALPHAS):
        i = min(max(int(np.searchsorted(a0, a, side="right")) - 1, 0), nstates - 2)
        idx = [i, i + 1]
        dm = np.abs(a - a0[idx]) ** 20
        w = 1.0 - dm / dm.sum()
        G = np.concatenate([(w[j] / w.sum()) * (a - a0[s]) ** np.arange(ORDER + 1) / fact for j, s in enumerate(idx)])
        _close(cov.values[k], _brute(G, [V[s] for s in idx]))
    with pytest.raises(ValueError):
        m.predict_cov(0.9, bounded=True)


def test_mbar_model_refuses_in_the_words_of_derivs_cov():
    from thermoextrap_amd import models

    m = object.__new__(models.MBARModel)
    with pytest.raises(NotImplementedError, match="pooled samples"):
        m.derivs_cross_cov()
    with pytest.raises(NotImplementedError, match="pooled samples"):
        m.predict_cov(0.5)
