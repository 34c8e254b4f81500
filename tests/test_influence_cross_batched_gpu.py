"""txm_influence_cross_cov_batched through the engine (engine.influence_cross_cov_batched): for every state

    cov[s][c][i][c'][j] = sum_n p_n^2 psi_i(n, c) psi_j(n, c')

against the long-double definition of tests/_influence_cross_ref.py within the bound of DESIGN 4.14,

    |cov - ref| <= 1e-12 sum_n p_n^2 B_i(n, c) B_j(n, c') + 2^-1022,

and against the single call on the same tensors: equal bits wherever the plan rule of include/txmom.h (f-14) promises
them (ceil(n_s / 256) <= q), the rounding bound where a state's budget binds.  The printed worst ratios are kept as
profiles/r20_cross_cov_states_gpu_tests.txt."""

from __future__ import annotations

import numpy as np
import pytest

from tests._influence_cross_ref import reference

pytestmark = pytest.mark.gpu

TOL = 1e-12
TINY = 2.0**-1022
SHARE = 256
_worst: dict = {}


def _problem(N, C, nf, nq, weighted, seed):
    """One state's operands on the host; centres 3 sigma off the means."""
    rng = np.random.default_rng(seed)
    u = rng.normal(3.0, 1.0, N)
    x = np.stack([(0.7 * u + 0.3 * u * u + rng.normal(2.0, 1.0, N)) * (1.0 + 0.5 * (c % 5)) for c in range(C)], axis=1)
    w = rng.uniform(0.5, 1.5, N) if weighted else None
    a, b = rng.normal(size=(C, nf, nq)), rng.normal(size=(C, nf, nq))
    cu = 3.0 + 3.0 * 1.0
    cx = np.array([(7.1 - 3.0 * 2.73) * (1.0 + 0.5 * (c % 5)) for c in range(C)])
    return x, u, w, a, b, cu, cx


def _problems(ns, C, nf, nq, weighted, seed=0):
    return [_problem(n, C, nf, nq, weighted, seed + 17 * s) for s, n in enumerate(ns)]


def _dev(v):
    import torch

    return None if v is None else torch.from_numpy(np.ascontiguousarray(v)).cuda()


def _device_x(x, pitch=None, misalign=False):
    import torch

    N, C = x.shape
    if pitch is not None:
        buf = torch.full((N, pitch), float("nan"), dtype=torch.float64, device="cuda")    # the padding is never read
        buf[:, :C] = torch.from_numpy(x).cuda()
        return buf[:, :C]
    if misalign:
        buf = torch.empty(N * C + 1, dtype=torch.float64, device="cuda")
        xd = buf[1:].view(N, C)
        xd.copy_(torch.from_numpy(x))
        assert xd.data_ptr() % 16 == 8
        return xd
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _tensors(probs, pitch=None, misalign=()):
    xs = [_device_x(p[0], pitch, s in misalign) for s, p in enumerate(probs)]
    us = [_dev(p[1]) for p in probs]
    ws = None if probs[0][2] is None else [_dev(p[2]) for p in probs]
    a, b = _dev(np.stack([p[3] for p in probs])), _dev(np.stack([p[4] for p in probs]))
    cu = np.array([p[5] for p in probs])
    cx = _dev(np.stack([p[6] for p in probs]))
    return xs, us, ws, a, b, cu, cx


def _batch(t):
    from thermoextrap_amd import engine

    xs, us, ws, a, b, cu, cx = t
    return engine.influence_cross_cov_batched(xs, us, a, b, cu, cx, ws=ws).cpu().numpy()


def _single(t, s):
    from thermoextrap_amd import engine

    xs, us, ws, a, b, cu, cx = t
    return engine.influence_cross_cov(xs[s], us[s], a[s], b[s], float(cu[s]), cx[s], w=None if ws is None else ws[s]).cpu().numpy()


def _q(S, C):
    """(q, single cap) from the device's CU count, q checked against the library's grid query."""
    import torch

    from thermoextrap_amd import engine

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    T = (C + 1 + 15) // 16
    pairs = T * (T + 1) // 2
    q = max(1, 8 * cus // (pairs * S))
    assert engine._L().txm_influence_cross_cov_batched_grid(S, 10**12, C) == q
    return q, max(1, 8 * cus // pairs)


def _against_reference(group, cov, prob, cols=None):
    """One state within the bound; returns the bound (float64) on the checked entries."""
    C, nf = prob[3].shape[:2]
    flat = cov.reshape(C * nf, C * nf)
    assert np.array_equal(flat, flat.T)                                                    # bitwise symmetric, every state
    ref, bnd = reference(*prob, cols=cols)
    sub = cov if cols is None else cov[np.ix_(cols, range(nf), cols, range(nf))]
    ratio = float((np.abs(sub - ref) / (TOL * bnd + TINY)).max()) * TOL
    _worst[group] = max(_worst.get(group, 0.0), ratio)
    assert ratio <= TOL, (group, ratio)
    return bnd.astype(np.float64)


def _report(group):
    print(f"{group}: worst |cov - ref| / sum p^2 B_ci B_c'j = {_worst.get(group, 0.0):.2e}")


NS3 = (1, 511, 1537)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("C", [1, 4, 15, 16, 33])
def test_bits_where_the_rule_promises_them(txm, C, weighted):
    """S = 3, n = (1, 511, 1537), n_q = n_f in {1, 2, 5, 9}: no state is capped, so every state has the single call's bits."""
    q, _ = _q(3, C)
    assert all(-(-n // SHARE) <= q for n in NS3)
    for nq in (1, 2, 5, 9):
        probs = _problems(NS3, C, nq, nq, weighted, seed=C + nq)
        t = _tensors(probs)
        cov = _batch(t)
        assert cov.shape == (3, C, nq, C, nq)
        for s, p in enumerate(probs):
            assert np.array_equal(cov[s], _single(t, s)), (C, nq, weighted, s)
            _against_reference("bits", cov[s], p)
    _report("bits")


def test_bits_with_n_f_unlike_n_q(txm):
    for C, nf, nq, weighted in ((4, 3, 5, True), (17, 5, 2, False)):
        probs = _problems(NS3, C, nf, nq, weighted, seed=3)
        t = _tensors(probs)
        cov = _batch(t)
        assert cov.shape == (3, C, nf, C, nf)
        for s, p in enumerate(probs):
            assert np.array_equal(cov[s], _single(t, s))
            _against_reference("n_f != n_q", cov[s], p)
    _report("n_f != n_q")


def test_one_state_is_the_single_call(txm):
    """S = 1: q is the single call's cap, whatever n."""
    q, cap = _q(1, 4)
    assert q == cap
    probs = _problems((70000,), 4, 4, 4, True, seed=5)
    t = _tensors(probs)
    cov = _batch(t)
    assert np.array_equal(cov[0], _single(t, 0))
    _against_reference("S = 1", cov[0], probs[0])
    _report("S = 1")


def _check_budget(group, probs, ns, C, cols=None):
    S = len(ns)
    q, cap = _q(S, C)
    shares = [-(-n // SHARE) for n in ns]
    capped = [min(sh, cap) > q for sh in shares]           # the single plan gives the state more workgroups than q
    assert any(capped) and not all(capped), (q, cap, shares)
    t = _tensors(probs)
    cov = _batch(t)
    nf = probs[0][3].shape[1]
    for s, p in enumerate(probs):
        bnd = _against_reference(group, cov[s], p, cols)
        one = _single(t, s)
        if capped[s]:
            sel = (cov[s], one) if cols is None else tuple(v[np.ix_(cols, range(nf), cols, range(nf))] for v in (cov[s], one))
            assert (np.abs(sel[0] - sel[1]) <= 2 * TOL * bnd + TINY).all(), (group, s)
        else:
            assert np.array_equal(cov[s], one), (group, s)
    _report(group)
    return capped


def test_budget_binds_at_255_columns(txm):
    """C = 255 (136 tile pairs), S = 4: states 0 and 3 get fewer workgroups than alone, states 1 and 2 the same."""
    q, _ = _q(4, 255)
    ns = (SHARE * (q + 4) + 1, 40, SHARE * q, 2 * SHARE * q + 17)
    probs = _problems(ns, 255, 2, 2, True, seed=1)
    capped = _check_budget("budget C=255", probs, ns, 255, cols=[0, 15, 16, 127, 254])
    assert capped == [True, False, False, True]


def test_budget_binds_at_70_states(txm):
    """C = 4, S = 70: all of 40 samples except two of 256 q + 300."""
    q, _ = _q(70, 4)
    ns = [40] * 70
    ns[11] = ns[64] = SHARE * q + 300
    probs = _problems(ns, 4, 4, 4, False, seed=2)
    capped = _check_budget("budget S=70", probs, ns, 4)
    assert [s for s, c in enumerate(capped) if c] == [11, 64]


def test_seventy_small_states(txm):
    probs = _problems([40] * 70, 4, 4, 4, True, seed=4)
    t = _tensors(probs)
    cov = _batch(t)
    for s, p in enumerate(probs):
        _against_reference("70 states", cov[s], p)
        if s % 9 == 0:
            assert np.array_equal(cov[s], _single(t, s))
    _report("70 states")


def test_state_of_total_weight_zero_gives_zeros_there_only(txm):
    probs = _problems((300, 777, 300), 17, 3, 3, True, seed=6)
    x, u, w, a, b, cu, cx = probs[1]
    x = x.copy()
    x[::3] = np.nan
    probs[1] = (x, u, np.zeros_like(w), a, b, cu, cx)
    t = _tensors(probs)
    cov = _batch(t)
    assert not cov[1].any()
    for s in (0, 2):
        assert cov[s].any() and np.array_equal(cov[s], _single(t, s))
        _against_reference("dead state", cov[s], probs[s])
    _report("dead state")


def test_zero_weight_rows_may_hold_anything(txm):
    ns = (700, 333, 1100)
    probs = _problems(ns, 16, 5, 5, True, seed=7)
    wild = []
    for x, u, w, a, b, cu, cx in probs:
        dead = np.arange(3, len(u), 7)
        w[dead] = 0.0
        x2, u2 = x.copy(), u.copy()
        x2[dead] = np.where(np.arange(len(dead))[:, None] % 2 == 0, 1e150, np.nan)
        u2[dead] = np.where(np.arange(len(dead)) % 3 == 0, np.nan, -1e150)
        wild.append((x2, u2, w, a, b, cu, cx))
    ref, got = _batch(_tensors(probs)), _batch(_tensors(wild))
    assert np.isfinite(ref).all() and np.array_equal(ref, got)
    for s, p in enumerate(wild):
        _against_reference("zero weight", got[s], p)
    _report("zero weight")


@pytest.mark.parametrize("C", [1, 15, 33])
def test_pitch(txm, C):
    """Rows of C + 3 doubles with NaN behind the columns, every state."""
    for weighted in (False, True):
        probs = _problems(NS3, C, 5, 5, weighted, seed=C)
        t = _tensors(probs, pitch=C + 3)
        cov = _batch(t)
        tight = _batch(_tensors(probs))
        assert np.array_equal(cov, tight)
        for s, p in enumerate(probs):
            _against_reference("pitch", cov[s], p)
    _report("pitch")


def test_a_misaligned_state_stays_in_the_one_launch(txm, monkeypatch):
    from thermoextrap_amd import engine

    probs = _problems(NS3, 4, 5, 5, True, seed=8)
    t = _tensors(probs, misalign=(1,))
    want = [_single(t, s) for s in range(3)]
    L = engine._L()
    n = {"single": 0, "batched": 0}
    real = L.txm_influence_cross_cov_batched

    def batched(*a):
        n["batched"] += 1
        return real(*a)

    def single(*a, **k):
        n["single"] += 1
        raise AssertionError("the engine looped over the single call")

    monkeypatch.setattr(L, "txm_influence_cross_cov_batched", batched)
    monkeypatch.setattr(engine, "influence_cross_cov", single)
    cov = _batch(t)
    assert n == {"single": 0, "batched": 1}
    for s, p in enumerate(probs):
        assert np.array_equal(cov[s], want[s])
        _against_reference("misaligned", cov[s], p)
    _report("misaligned")


def test_unequal_pitches_loop_over_the_single_call(txm, monkeypatch):
    from thermoextrap_amd import engine

    probs = _problems(NS3, 4, 3, 3, False, seed=9)
    xs, us, ws, a, b, cu, cx = _tensors(probs)
    xs[2] = _device_x(probs[2][0], pitch=9)
    n = {"single": 0}
    real = engine.influence_cross_cov

    def single(*args, **k):
        n["single"] += 1
        return real(*args, **k)

    monkeypatch.setattr(engine, "influence_cross_cov", single)
    cov = _batch((xs, us, ws, a, b, cu, cx))
    assert n["single"] == 3 and cov.shape == (3, 4, 3, 4, 3)
    for s, p in enumerate(probs):
        _against_reference("loop", cov[s], p)
    with pytest.raises(ValueError, match="255"):
        wide = _problems((5, 6), 256, 1, 1, False)
        _batch(_tensors(wide))


@pytest.mark.parametrize("C,nq,weighted", [(4, 4, True), (33, 9, False), (255, 1, True)])
def test_two_calls_same_bits(txm, C, nq, weighted):
    t = _tensors(_problems((5003, 40, 1537), C, nq if C < 255 else 1, nq, weighted, seed=10))
    assert np.array_equal(_batch(t), _batch(t))


def _raw_args(probs, nf, nq, C):
    """The C call's operands: (state table, device tensors kept alive, n_max)."""
    from thermoextrap_amd import _lib

    xs, us, ws, a, b, cu, cx = _tensors(probs)
    tab = (_lib.InfState * len(probs))()
    for s in range(len(probs)):
        tab[s].x, tab[s].u, tab[s].n = xs[s].data_ptr(), us[s].data_ptr(), xs[s].shape[0]
        tab[s].w = ws[s].data_ptr() if ws is not None else None
    cud = _dev(cu)
    return tab, (xs, us, ws, a, b, cud, cx), max(x.shape[0] for x in xs)


@pytest.mark.parametrize("ns,C,nf,nq", [((65, 1, 300), 3, 5, 5), ((641, 40), 17, 3, 5), ((SHARE + 1,), 33, 2, 9),
                                       ((2000, 7000, 40, 512), 255, 1, 1)])
def test_bands_behind_workspace_and_cov_are_untouched(txm, ns, C, nf, nq):
    """The C call with a workspace of exactly the queried size: 4 KiB behind it and behind cov keep their pattern; one
    byte less is refused."""
    import torch

    from thermoextrap_amd import _lib, engine

    L = engine._L()
    probs = _problems(ns, C, nf, nq, True, seed=11)
    tab, keep, n_max = _raw_args(probs, nf, nq, C)
    xs, us, ws, a, b, cud, cx = keep
    S = len(ns)
    need = L.txm_influence_cross_cov_batched_ws_bytes(S, n_max, C, nf, nq)
    wsb = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    ncov = S * (C * nf) ** 2
    cov = torch.full((ncov + 512,), -7.25, dtype=torch.float64, device="cuda")
    args = (tab, S, C, C, nf, nq, cud.data_ptr(), cx.data_ptr(), a.data_ptr(), b.data_ptr(), cov.data_ptr(), wsb.data_ptr())
    _lib.check(L.txm_influence_cross_cov_batched(*args, need, None), "txm_influence_cross_cov_batched")
    torch.cuda.synchronize()
    assert bool((wsb[need:] == 0xA5).all()) and bool((cov[ncov:] == -7.25).all())
    assert np.array_equal(cov[:ncov].cpu().numpy().reshape(S, C, nf, C, nf), _batch((xs, us, ws, a, b, np.asarray(cud.cpu()), cx)))
    assert L.txm_influence_cross_cov_batched(*args, need - 1, None) == -3


def test_every_refusal_returns_its_code_and_leaves_cov_unwritten(txm):
    import torch

    from thermoextrap_amd import _lib, engine

    L = engine._L()
    ns, C, nf, nq = (100, 30, 257), 4, 3, 3
    probs = _problems(ns, C, nf, nq, True, seed=12)
    tab, keep, n_max = _raw_args(probs, nf, nq, C)
    xs, us, ws, a, b, cud, cx = keep
    S = len(ns)
    cov = torch.full((S * (C * nf) ** 2,), -7.25, dtype=torch.float64, device="cuda")
    need = L.txm_influence_cross_cov_batched_ws_bytes(S, n_max, C, nf, nq)
    wsb = torch.empty(need, dtype=torch.uint8, device="cuda")

    def table(s_bad, field, value):
        """The state table with one field of one state replaced."""
        t2 = (_lib.InfState * S)()
        for s in range(S):
            t2[s].x, t2[s].u, t2[s].w, t2[s].n = tab[s].x, tab[s].u, tab[s].w, tab[s].n
        setattr(t2[s_bad], field, value)
        return t2

    names = ("tab", "S", "ls", "C", "nf", "nq", "cu", "cx", "a", "b", "cov", "ws", "wsb", "st")
    good = dict(tab=tab, S=S, ls=C, C=C, nf=nf, nq=nq, cu=cud.data_ptr(), cx=cx.data_ptr(), a=a.data_ptr(), b=b.data_ptr(),
                cov=cov.data_ptr(), ws=wsb.data_ptr(), wsb=need, st=None)

    def call(**bad):
        return L.txm_influence_cross_cov_batched(*[{**good, **bad}[n] for n in names])

    for ptr in ("tab", "cu", "cx", "a", "b", "ws"):
        assert call(**{ptr: None}) == -1, ptr
    assert call(S=0) == -1 and call(S=65536) == -1
    assert call(ls=C - 1) == -1 and b"pitch" in L.txm_last_error()
    assert call(C=256, ls=256) == -1 and b"255" in L.txm_last_error()
    assert call(C=0) == -1 and call(nf=10) == -1 and call(nf=0) == -1 and call(nq=0) == -1 and call(nq=10) == -1
    assert call(tab=table(1, "n", 0)) == -1 and call(tab=table(2, "n", -5)) == -1
    assert call(tab=table(2, "x", None)) == -1 and call(tab=table(0, "u", None)) == -1
    assert call(tab=table(1, "w", None)) == -1 and b"weights" in L.txm_last_error()
    assert call(wsb=need - 1) == -3
    torch.cuda.synchronize()
    assert bool((cov == -7.25).all())
    assert call(cov=None) == -1
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((cov == -7.25).any())

