"""CPU checks of the MBAR bootstrap boundary (include/txmom.h section (f-6)): the header declares the entry points, the
ctypes mirror of txm_mbar_boot_state matches it, the workspace query never grows with nrep x N_total, argument
validation is host logic, and the batched host Newton loop (engine.mbar_newton_batched) equals the single loop per
replicate, freezes converged replicates, steps on a singular Hessian and gives up loudly -- driven by a numpy
restatement of the weighted device evaluation pass."""

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


def test_header_declares_the_bootstrap_entry_points():
    text = _header()
    for name in ("txm_mbar_boot_ws_bytes", "txm_mbar_boot_eval", "txm_mbar_boot_predict"):
        assert re.search(rf"\b{name}\s*\(", text), name
    assert re.search(r"#define TXM_ABI_VERSION 2\b", (ROOT / "include" / "txmom.h").read_text())


def test_boot_state_mirror_matches_the_header():
    from thermoextrap_amd import _lib

    body = re.search(r"typedef struct txm_mbar_boot_state \{(.*?)\} txm_mbar_boot_state;", _header(), re.S).group(1)
    assert [m.group(1) for m in re.finditer(r"(\w+);", body)] == [f[0] for f in _lib.MbarBootState._fields_] == ["spec", "counts"]
    assert ct.sizeof(_lib.SamplerSpec) == 40
    assert ct.sizeof(_lib.MbarBootState) == ct.sizeof(_lib.SamplerSpec) + ct.sizeof(ct.c_void_p) == 48
    assert (_lib.MbarBootState.spec.offset, _lib.MbarBootState.counts.offset) == (0, ct.sizeof(_lib.SamplerSpec))


def test_workspace_never_scales_with_nrep_times_samples(lib):
    q = lib.txm_mbar_boot_ws_bytes
    for bad in ((0, 1, 1, 100, 1), (65, 1, 1, 100, 1), (2, 0, 1, 100, 1), (2, 65536, 1, 100, 1), (2, 1, 0, 100, 1),
                (2, 1, 9, 100, 1), (2, 1, 1, 1, 1), (2, 1, 1, 100, 0)):
        assert q(*bad) == 0, bad
    big = q(4, 32, 8, 10**8, 1000)
    assert 0 < big < 8 * 2**30, big            # a byte per (replicate, sample) would be 1e11
    prev = 0
    for nrep in (1, 2, 7, 100, 128, 1000, 5000):
        cur = q(4, 32, 8, 10**8, nrep)
        assert cur >= prev > -1, nrep
        prev = cur
    prev = 0
    for K, C, na in ((4, 32, 8), (1, 1, 1), (12, 5, 3), (64, 1, 1)):
        prev = 0
        for ntot in (64, 1000, 1024, 1025, 5000, 10**5, 10**6, 10**7, 10**8, 10**9):
            cur = q(K, C, na, ntot, 100)
            assert cur >= prev and cur > 0, (K, ntot)
            prev = cur
    assert q(4, 1, 1, 10**6, 10) < q(4, 32, 8, 10**6, 10)


def _tables(K, n=100, C=4, nrep=3):
    from thermoextrap_amd import _lib

    tab = (_lib.MbarState * max(K, 1))()
    stab = (_lib.MbarBootState * max(K, 1))()
    for s in range(max(K, 1)):
        tab[s].x, tab[s].u, tab[s].n, tab[s].ldx_s = 0x10000, 0x20000, n, C   # never dereferenced: every call is refused first
        stab[s].spec = _lib.SamplerSpec(seed=1, nrep=nrep, ndat=n, nsamp=0, rep0=s * nrep)
        stab[s].counts = 0x60000
    return tab, stab


def test_eval_and_predict_refuse_bad_arguments_without_a_device(lib):
    from thermoextrap_amd import _lib

    d = (ct.c_double * 65)()
    out, ws, g = ct.c_void_p(0x30000), ct.c_void_p(0x40000), ct.c_void_p(0x50000)
    big = 1 << 40

    def ev(tabs, K, ws_bytes=big, a0=d, g=g, n_active=1, upiv=0.0):
        return lib.txm_mbar_boot_eval(tabs[0], tabs[1], K, a0, g, None, n_active, upiv, out, ws, ws_bytes, None)

    def pr(tabs, K, C=4, na=1, ws_bytes=big, gref=d):
        return lib.txm_mbar_boot_predict(tabs[0], tabs[1], K, C, 0.0, d, g, gref, d, na, out, ws, ws_bytes, None)

    def refused(rc, words, status=-1):
        assert rc == status, (rc, _lib.last_error())
        msg = _lib.last_error()
        assert all(w in msg for w in words), msg

    for call, name in ((ev, "mbar_boot_eval"), (pr, "mbar_boot_predict")):
        refused(call((None, _tables(2)[1]), 2), [name, "null state table"])
        refused(call((_tables(2)[0], None), 2), [name, "null sampler table"])
        refused(call(_tables(1), 0), ["K = 0"])
        refused(call(_tables(65), 65), ["K = 65"])
        t = _tables(3)
        t[0][1].n = 0
        refused(call(t, 3), ["state 1", "n = 0"])
        t = _tables(3)
        t[0][2].u = None
        refused(call(t, 3), ["state 2", "null u"])
        t = _tables(3)
        t[1][1].counts = None
        refused(call(t, 3), ["state 1", "null sampler counts"])
        t = _tables(3)
        t[1][2].spec.ndat = 99
        refused(call(t, 3), ["state 2", "ndat = 99", "n = 100"])
        t = _tables(3)
        t[1][1].spec.nsamp = 50
        refused(call(t, 3), ["state 1", "nsamp = 50"])
        t = _tables(3)
        t[1][2].spec.nrep = 4
        refused(call(t, 3), ["state 2", "nrep = 4"])
        t = _tables(2)
        t[1][0].spec.nrep = t[1][1].spec.nrep = 0
        refused(call(t, 2), ["nrep = 0"])
        t = _tables(2)
        t[1][1].spec.rep0 = -1
        refused(call(t, 2), ["state 1", "stream replicates"])
        t = _tables(2)
        t[1][1].spec.rep0 = 2**32 - 2
        refused(call(t, 2), ["state 1", "stream replicates"])
        refused(call(_tables(2), 2, ws_bytes=16), ["workspace too small"], status=-3)
    refused(ev(_tables(2), 2, a0=None), ["null pointer"])
    refused(ev(_tables(2), 2, g=None), ["null pointer"])
    refused(ev(_tables(2), 2, n_active=0), ["n_active = 0"])
    refused(ev(_tables(2), 2, n_active=4), ["n_active = 4", "nrep = 3"])
    refused(ev(_tables(2), 2, upiv=float("nan")), ["pivot not finite"])
    bad = (ct.c_double * 65)()
    bad[1] = float("inf")
    refused(ev(_tables(2), 2, a0=bad), ["alpha0 of state 1"])
    t = _tables(2)
    t[0][1].x = None
    refused(pr(t, 2), ["state 1", "null x"])
    refused(pr(_tables(2, C=4), 2, C=5), ["ldx_s = 4 < C = 5"])
    refused(pr(_tables(2), 2, C=0), ["C = 0"])
    refused(pr(_tables(2), 2, na=0), ["n_alpha = 0"])
    refused(pr(_tables(2), 2, na=9), ["n_alpha = 9"])
    refused(pr(_tables(2), 2, gref=None), ["null pointer"])
    refused(pr(_tables(2), 2, gref=bad), ["gref of state 1"])


# ---- the batched host Newton loop ------------------------------------------------------------------------------
def _weighted_evaluator(us, a0, upiv, counts):
    """numpy restatement of txm_mbar_boot_eval: counts (R, N_total); records (g copy, active copy) of every call."""
    ut = np.concatenate(us) - upiv
    a0 = np.asarray(a0, dtype=float)
    calls = []

    def one(g, c):
        t = g[:, None] - a0[:, None] * ut[None, :]
        m = t.max(0)
        e = np.exp(t - m)
        s = e.sum(0)
        p = e / s
        return (p * c).sum(1), (p * c) @ p.T, float((c * (m + np.log(s))).sum())

    def evaluate(g, active):
        calls.append((np.array(g, dtype=float), np.array(active)))
        res = [one(g[r], counts[r]) for r in active]
        return np.array([x[0] for x in res]), np.array([x[1] for x in res]), np.array([x[2] for x in res])

    return evaluate, calls, one


def _problem(a0, ns, seed=0):
    rng = np.random.default_rng(seed)
    mu, sd = 50.0, 3.0
    us = [rng.normal(mu - sd * sd * a, sd, n) for a, n in zip(a0, ns)]
    N = np.array(ns, dtype=float)
    upiv = float(np.concatenate(us).mean())
    return us, N, np.log(N) - np.asarray(a0) * upiv, upiv


def _multinomial_counts(ns, R, seed):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.multinomial(n, np.full(n, 1.0 / n), size=R) for n in ns], axis=1).astype(float)


def test_batched_newton_equals_the_single_loop_per_replicate_and_freezes():
    from thermoextrap_amd import engine

    a0, ns, R = [0.8, 1.0, 1.25, 1.4], [3000, 2000, 2500, 1000], 6
    us, N, b, upiv = _problem(a0, ns)
    counts = _multinomial_counts(ns, R, 5)
    counts[2] = 1.0                                   # one replicate IS the point problem: converged at the start
    ev, calls, one = _weighted_evaluator(us, a0, upiv, counts)
    f_point = engine.mbar_newton(lambda g: one(g, np.ones(sum(ns))), N, b, tol=1e-12)[0]
    f, g, its, n_eval, err = engine.mbar_newton_batched(ev, N, b, np.tile(f_point, (R, 1)), tol=1e-12)
    assert f.shape == (R, 4) and np.all(f[:, 0] == 0.0) and np.all(err <= 1e-12) and n_eval == len(calls)
    assert its[2] == 0 and np.array_equal(f[2], f_point) and 1 <= its.max() <= 6
    for r in range(R):
        fr = engine.mbar_newton(lambda gg: one(gg, counts[r]), N, b, f0=f_point, tol=1e-12)[0]
        np.testing.assert_allclose(f[r], fr, rtol=0, atol=1e-13)
        np.testing.assert_allclose(g[r], b + f[r] - (b + f[r]).max(), rtol=0, atol=1e-13)
    # frozen: once a replicate is missing from an active list it never returns and its row of g never changes again
    assert np.array_equal(calls[0][1], np.arange(R)) and 2 not in calls[1][1]
    gone = {}
    for gcall, active in calls[1:]:
        for r in range(R):
            if r in gone:
                assert r not in active and np.array_equal(gcall[r], gone[r]), r
            elif r not in active:
                gone[r] = gcall[r].copy()
    assert len(calls[-1][1]) < R


def test_batched_newton_steps_on_a_singular_hessian():
    from thermoextrap_amd import engine

    a0, ns = [1.0, 6.0], [400, 300]
    rng = np.random.default_rng(1)
    us = [rng.normal(100.0, 1.0, ns[0]), rng.normal(0.0, 1.0, ns[1])]
    N = np.array(ns, dtype=float)
    upiv = float(np.concatenate(us).mean())
    b = np.log(N) - np.asarray(a0) * upiv
    counts = _multinomial_counts(ns, 3, 2)
    ev, calls, one = _weighted_evaluator(us, a0, upiv, counts)
    f, g, its, n_eval, err = engine.mbar_newton_batched(ev, N, b, np.tile([0.0, -2000.0], (3, 1)), tol=1e-12)
    S0, H0, _ = one(calls[0][0][0], counts[0])
    assert S0[1] == 0.0 and (np.diag(S0) - H0)[1, 1] == 0.0          # the start really is singular
    first = (calls[1][0][:, 1] - calls[1][0][:, 0]) - (calls[0][0][:, 1] - calls[0][0][:, 0])
    assert np.all(np.isfinite(first)) and np.all(first > 0.0) and np.all(first <= engine._MBAR_MAX_STEP + 1e-9)
    assert np.all(err <= 1e-12) and np.all(np.isfinite(f)) and np.all(f[:, 0] == 0.0)


def test_batched_newton_raises_after_max_iter_naming_the_worst_replicate():
    from thermoextrap_amd import _lib, engine

    a0, ns = [1.0, 6.0], [400, 300]
    rng = np.random.default_rng(1)
    us = [rng.normal(100.0, 1.0, ns[0]), rng.normal(0.0, 1.0, ns[1])]
    N = np.array(ns, dtype=float)
    upiv = float(np.concatenate(us).mean())
    b = np.log(N) - np.asarray(a0) * upiv
    ev, _, _ = _weighted_evaluator(us, a0, upiv, _multinomial_counts(ns, 2, 3))
    with pytest.raises(_lib.TxmError, match=r"did not converge in 3 Newton iterations: 2 of 2 replicates left, the worst is "
                                            r"replicate \d with max \|S_k - N_k\| / N_k = "):
        engine.mbar_newton_batched(ev, N, b, np.tile([0.0, -2000.0], (2, 1)), max_iter=3)
    with pytest.raises(ValueError, match="f0 must be"):
        engine.mbar_newton_batched(ev, N, b, np.zeros(2))
