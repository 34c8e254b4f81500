"""CPU checks of the MBAR boundary (include/txmom.h section (f-5)): the header declares the entry points, the ctypes
mirror of txm_mbar_state matches it, workspace sizing and argument validation are host logic, and the host Newton loop
of the solve (engine.mbar_newton) converges, steps on a singular Hessian and gives up loudly -- driven by a numpy
restatement of the device evaluation pass."""

import ctypes as ct
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


def _header():
    return re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "txmom.h").read_text(), flags=re.S)


def test_header_declares_the_mbar_entry_points():
    text = _header()
    for name in ("txm_mbar_ws_bytes", "txm_mbar_eval", "txm_mbar_predict"):
        assert re.search(rf"\b{name}\s*\(", text), name


def test_mbar_state_mirror_matches_the_header():
    from thermoextrap_amd import _lib

    body = re.search(r"typedef struct txm_mbar_state \{(.*?)\} txm_mbar_state;", _header(), re.S).group(1)
    assert [m.group(1) for m in re.finditer(r"(\w+);", body)] == [f[0] for f in _lib.MbarState._fields_] == ["x", "u", "n", "ldx_s"]
    assert ct.sizeof(_lib.MbarState) == 32
    assert (_lib.MbarState.x.offset, _lib.MbarState.u.offset, _lib.MbarState.n.offset, _lib.MbarState.ldx_s.offset) == (0, 8, 16, 24)


def test_ws_bytes_is_host_logic(lib):
    for bad in ((0, 1, 1), (65, 1, 1), (2, 0, 1), (2, 65536, 1), (2, 1, 0), (2, 1, 9)):
        assert lib.txm_mbar_ws_bytes(*bad) == 0, bad
    small, wide, many = lib.txm_mbar_ws_bytes(4, 1, 1), lib.txm_mbar_ws_bytes(4, 32, 8), lib.txm_mbar_ws_bytes(64, 1, 1)
    assert 0 < small < wide and small < many


def _states(K, n=100, C=4):
    from thermoextrap_amd import _lib

    tab = (_lib.MbarState * max(K, 1))()
    for s in range(max(K, 1)):
        tab[s].x, tab[s].u, tab[s].n, tab[s].ldx_s = 0x10000, 0x20000, n, C   # never dereferenced: every call is refused first
    return tab


def test_eval_and_predict_refuse_bad_arguments_without_a_device(lib):
    from thermoextrap_amd import _lib

    d = (ct.c_double * 65)()
    out, ws = ct.c_void_p(0x30000), ct.c_void_p(0x40000)
    big = 1 << 40

    def ev(tab, K, ws_bytes=big, a0=d, g=d):
        return lib.txm_mbar_eval(tab, K, a0, g, 0.0, out, None, ws, ws_bytes, None)

    def pr(tab, K, C=4, na=1, ws_bytes=big):
        return lib.txm_mbar_predict(tab, K, C, 0.0, ct.c_void_p(0x50000), d, na, out, ws, ws_bytes, None)

    def refused(rc, words, status=-1):
        assert rc == status, (rc, _lib.last_error())
        msg = _lib.last_error()
        assert all(w in msg for w in words), msg

    refused(ev(None, 2), ["mbar_eval", "null state table"])
    refused(ev(_states(1), 0), ["K = 0"])
    refused(ev(_states(65), 65), ["K = 65"])
    tab = _states(3)
    tab[1].n = 0
    refused(ev(tab, 3), ["state 1", "n = 0"])
    tab = _states(3)
    tab[2].u = None
    refused(ev(tab, 3), ["state 2", "null u"])
    refused(ev(_states(2), 2, a0=None), ["null pointer"])
    refused(ev(_states(2), 2, ws_bytes=16), ["workspace too small"], status=-3)
    refused(pr(None, 2), ["mbar_predict", "null state table"])
    refused(pr(_states(1), 0), ["K = 0"])
    refused(pr(_states(65), 65), ["K = 65"])
    tab = _states(2)
    tab[1].x = None
    refused(pr(tab, 2), ["state 1", "null x"])
    refused(pr(_states(2, C=4), 2, C=5), ["ldx_s = 4 < C = 5"])
    refused(pr(_states(2), 2, C=0), ["C = 0"])
    refused(pr(_states(2), 2, na=0), ["n_alpha = 0"])
    refused(pr(_states(2), 2, na=9), ["n_alpha = 9"])
    tab = _states(2)
    tab[0].n = -5
    refused(pr(tab, 2), ["state 0", "n = -5"])
    refused(pr(_states(2), 2, ws_bytes=16), ["workspace too small"], status=-3)


# ---- the host Newton loop --------------------------------------------------------------------------------------
def _evaluator(us, a0, upiv):
    """numpy restatement of txm_mbar_eval: (S, H, sum logD) at the log-weights g; records every g it is called with."""
    ut = np.concatenate(us) - upiv
    a0 = np.asarray(a0, dtype=float)
    calls = []

    def evaluate(g):
        calls.append(np.array(g, dtype=float))
        t = g[:, None] - a0[:, None] * ut[None, :]
        m = t.max(0)
        e = np.exp(t - m)
        s = e.sum(0)
        p = e / s
        return p.sum(1), p @ p.T, float((m + np.log(s)).sum())

    return evaluate, calls


def _problem(a0, ns, seed=0):
    """Gaussian energies: at alpha the distribution of u is N(mu - var * alpha, var)."""
    rng = np.random.default_rng(seed)
    mu, sd = 50.0, 3.0
    us = [rng.normal(mu - sd * sd * a, sd, n) for a, n in zip(a0, ns)]
    N = np.array(ns, dtype=float)
    upiv = float(np.concatenate(us).mean())
    return us, N, np.log(N) - np.asarray(a0) * upiv, upiv


def _no_overlap():
    """Two states whose energies are 100 standard deviations apart."""
    a0, ns = [1.0, 6.0], [400, 300]
    rng = np.random.default_rng(1)
    us = [rng.normal(100.0, 1.0, ns[0]), rng.normal(0.0, 1.0, ns[1])]
    N = np.array(ns, dtype=float)
    upiv = float(np.concatenate(us).mean())
    return a0, us, N, np.log(N) - np.asarray(a0) * upiv, upiv


def test_newton_converges_in_the_gauge_f0_zero():
    from thermoextrap_amd import engine

    a0, ns = [0.8, 1.0, 1.25, 1.4], [3000, 2000, 2500, 1000]
    us, N, b, upiv = _problem(a0, ns)
    ev, calls = _evaluator(us, a0, upiv)
    f, g, it, n_eval, err = engine.mbar_newton(ev, N, b, tol=1e-12)
    assert f[0] == 0.0 and err <= 1e-12 and 1 <= it < 30 and n_eval == len(calls)
    # self-consistency in long double: f_j = -ln sum_n e^{-alpha0_j u_n - logD_n}
    u = np.concatenate(us).astype(np.longdouble)
    a = np.asarray(a0, dtype=np.longdouble)
    t = np.log(N.astype(np.longdouble))[:, None] + f.astype(np.longdouble)[:, None] - a[:, None] * u[None, :]
    m = t.max(0)
    logD = m + np.log(np.exp(t - m).sum(0))
    e = -a[:, None] * u[None, :] - logD[None, :]
    em = e.max(1)
    fsc = -(em + np.log(np.exp(e - em[:, None]).sum(1)))
    np.testing.assert_allclose(np.asarray(fsc - fsc[0], dtype=float), f, rtol=0, atol=1e-10)
    # the same answer from the engine's start (thermodynamic integration)
    f2, *_ = engine.mbar_newton(ev, N, b, f0=engine.mbar_initial_f(us, a0), tol=1e-12)
    np.testing.assert_allclose(f2, f, rtol=0, atol=1e-10)


def test_newton_steps_on_a_singular_hessian():
    """Started where every sample belongs to state 0, p_1n underflows to 0: the reduced Hessian S_1 - sum_n p_1n^2 is
    exactly 0 while the gradient is -N_1.  The loop must still take a finite step (bounded along the flat direction)
    and walk into the valley where each state keeps its own samples."""
    from thermoextrap_amd import engine

    a0, us, N, b, upiv = _no_overlap()
    ev, calls = _evaluator(us, a0, upiv)
    f, g, it, n_eval, err = engine.mbar_newton(ev, N, b, f0=[0.0, -2000.0], tol=1e-12)
    S0, H0, _ = ev(calls[0])
    assert S0[1] == 0.0 and (np.diag(S0) - H0)[1, 1] == 0.0          # the start really is singular
    first = (calls[1][1] - calls[1][0]) - (calls[0][1] - calls[0][0])  # the change of f_1 - f_0 in the first trial
    assert np.isfinite(first) and 0.0 < first <= engine._MBAR_MAX_STEP + 1e-9
    assert err <= 1e-12 and np.all(np.isfinite(f)) and f[0] == 0.0


def test_newton_raises_after_max_iter_naming_the_gradient():
    from thermoextrap_amd import _lib, engine

    a0, us, N, b, upiv = _no_overlap()
    ev, _ = _evaluator(us, a0, upiv)
    with pytest.raises(_lib.TxmError, match=r"did not converge in 3 Newton iterations: max \|S_k - N_k\| / N_k = "):
        engine.mbar_newton(ev, N, b, f0=[0.0, -2000.0], max_iter=3)
