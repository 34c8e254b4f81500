"""txm_influence_cov_batched through the C ABI (engine.influence_cov_batched): every state of a batch against the long-double
sums of its own samples within the first-order bound of tests/test_influence_gpu.py

    |cov_ij - ref| <= 1e-12 sum_n p_n^2 B_i(n) B_j(n)     |mean_k - ref| <= 1e-12 sum_n p_n B_k(n)

AND bit for bit against the single call (engine.influence_cov) on the same tensors: ragged sample counts around a
workgroup's share, every column layout of the row-major kernel, n_q across the two-column limit, more states than a CU
count, a dead state between live ones, and the wrapper's loop for operands the one launch cannot take."""

from __future__ import annotations

import numpy as np
import pytest

from tests._influence_ref import LD, bound_ld, psi_ld

pytestmark = pytest.mark.gpu

TOL = 1e-12
_worst = {"cov": 0.0, "mean": 0.0}
RAGGED = (1, 511, 1537)      # C = 4: 128 rows per workgroup, a share of 512 -> 1, 1 and 4 workgroups of the 4 launched


def _states(ns, C, nf, nq, weighted, seed):
    """Per state (x, u, w, a, b, cu, cx) on the host; centres 3 sigma off the means as in test_influence_gpu."""
    out = []
    for s, n in enumerate(ns):
        rng = np.random.default_rng(1000 * seed + s)
        u = rng.normal(3.0, 1.0, n)
        x = np.stack([(0.7 * u + 0.3 * u * u + rng.normal(2.0, 1.0, n)) * (1.0 + 0.5 * (c % 5)) for c in range(C)], axis=1)
        w = rng.uniform(0.5, 1.5, n) if weighted else None
        a, b = rng.normal(size=(C, nf, nq)), rng.normal(size=(C, nf, nq))
        cu = 6.0 + 0.1 * s
        cx = np.array([(7.1 - 3.0 * 2.73 + 0.2 * s) * (1.0 + 0.5 * (c % 5)) for c in range(C)])
        out.append([x, u, w, a, b, cu, cx])
    return out


def _dev(v):
    import torch

    return None if v is None else torch.from_numpy(np.ascontiguousarray(v)).cuda()


def _device_x(x, pitch):
    """x on the device, rows `pitch` doubles apart (the padding holds NaN: it is never read)."""
    import torch

    n, C = x.shape
    if pitch == C:
        return torch.from_numpy(x).cuda()
    buf = torch.full((n, pitch), float("nan"), dtype=torch.float64, device="cuda")
    buf[:, :C] = torch.from_numpy(x).cuda()
    return buf[:, :C]


def _upload(states, pitch=None):
    C = states[0][0].shape[1]
    xs = [_device_x(st[0], pitch or C) for st in states]
    us = [_dev(st[1]) for st in states]
    ws = None if states[0][2] is None else [_dev(st[2]) for st in states]
    a, b = _dev(np.stack([st[3] for st in states])), _dev(np.stack([st[4] for st in states]))
    cu = np.array([st[5] for st in states])
    cx = _dev(np.stack([st[6] for st in states]))
    return xs, us, ws, a, b, cu, cx


def _singles(ops):
    from thermoextrap_amd import engine

    xs, us, ws, a, b, cu, cx = ops
    out = [engine.influence_cov(xs[s], us[s], a[s], b[s], float(cu[s]), cx[s], w=None if ws is None else ws[s])
           for s in range(len(xs))]
    return [(c.cpu().numpy(), m.cpu().numpy()) for c, m in out]


def _batched(ops):
    from thermoextrap_amd import engine

    xs, us, ws, a, b, cu, cx = ops
    cov, mean = engine.influence_cov_batched(xs, us, a, b, cu, cx, ws=ws)
    return cov.cpu().numpy(), mean.cpu().numpy()


def _check(txm, ns, C, nf, nq, weighted, seed=0, pitch=None):
    states = _states(ns, C, nf, nq, weighted, seed)
    ops = _upload(states, pitch)
    cov, mean = _batched(ops)
    assert cov.shape == (len(ns), C, nf, nf) and mean.shape == (len(ns), C, nf)
    single = _singles(ops)
    for s, (x, u, w, a, b, cu, cx) in enumerate(states):
        assert np.array_equal(cov[s], single[s][0]) and np.array_equal(mean[s], single[s][1]), (ns, C, nf, nq, weighted, s)
        wl = np.ones(len(u), LD) if w is None else np.asarray(w, LD)
        p = wl / wl.sum()
        du = np.asarray(u, LD) - LD(cu)
        for c in range(C):
            dx = np.asarray(x[:, c], LD) - LD(cx[c])
            psi, B = psi_ld(a[c], b[c], dx, du), bound_ld(a[c], b[c], dx, du)
            cref = np.einsum("n,in,jn->ij", p * p, psi, psi)
            cbnd = np.einsum("n,in,jn->ij", p * p, B, B)
            rc = float((np.abs(cov[s, c] - cref) / cbnd).max())
            rm = float((np.abs(mean[s, c] - psi @ p) / (B @ p)).max())
            _worst["cov"], _worst["mean"] = max(_worst["cov"], rc), max(_worst["mean"], rm)
            assert rc <= TOL and rm <= TOL, (ns, C, nf, nq, weighted, s, c, rc, rm)
            assert np.array_equal(cov[s, c], cov[s, c].T)
    return cov, mean


def _say(what):
    print(f"{what}: worst ratio to the bound so far: cov {_worst['cov']:.2e}, mean {_worst['mean']:.2e}")


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("nq", [1, 2, 5, 6, 7, 9])
def test_ragged_states_across_the_two_column_limit(txm, nq, weighted):
    """S = 3, C = 4, n = (1, 511, 1537): a state that leaves three of the four launched workgroups idle, one a row short
    of a share, one of several shares with a tail; n_q = 6 | 7 crosses from two columns per lane to one."""
    _check(txm, RAGGED, 4, nq, nq, weighted, seed=nq)
    _say(f"C=4 n_q={nq} weighted={weighted}")


@pytest.mark.parametrize("C", [1, 3, 32, 33])
def test_ragged_states_every_column_layout(txm, C):
    """The same shares with one column per lane (odd C; C = 1 is one contiguous series per state), a full 16-lane row
    (C = 32) and a second column chunk behind a padded pitch (C = 33, rows 36 doubles apart)."""
    for weighted in (False, True):
        _check(txm, RAGGED, C, 3, 3, weighted, seed=C, pitch=36 if C == 33 else None)
    _say(f"C={C}")


def test_nf_differs_from_nq(txm):
    _check(txm, RAGGED, 4, 3, 5, True, seed=11)
    _check(txm, RAGGED, 3, 7, 2, False, seed=12)
    _say("n_f != n_q")


def test_one_state_is_the_single_call(txm):
    _check(txm, (1537,), 4, 4, 4, True, seed=13)


def test_more_states_than_compute_units_take_at_once(txm):
    """S = 70 states of n = 40: the state axis of the grid, not the samples, carries the launch."""
    _check(txm, (40,) * 70, 4, 3, 3, True, seed=14)
    _say("S=70")


def test_dead_state_between_live_ones(txm):
    """Total weight zero in the middle state: zeros there, the neighbours' bits untouched."""
    states = _states((300, 257, 700), 4, 3, 3, True, 15)
    ref = _batched(_upload(states))
    states[1][2] = np.zeros_like(states[1][2])
    cov, mean = _batched(_upload(states))
    assert not cov[1].any() and not mean[1].any()
    for s in (0, 2):
        assert np.array_equal(cov[s], ref[0][s]) and np.array_equal(mean[s], ref[1][s])
        assert cov[s].any() and np.isfinite(cov[s]).all()


def test_zero_weight_rows_may_hold_anything(txm):
    """Rows of weight zero holding 1e150 and NaN leave every bit where ordinary values leave it."""
    states = _states(RAGGED[1:], 4, 5, 5, True, 16)
    dead = []
    for st in states:
        d = np.arange(3, len(st[1]), 7)
        st[2][d] = 0.0
        dead.append(d)
    ref = _batched(_upload(states))
    for st, d in zip(states, dead):
        st[0][d] = np.where(np.arange(len(d))[:, None] % 2 == 0, 1e150, np.nan)
        st[1][d] = np.where(np.arange(len(d)) % 3 == 0, np.nan, -1e150)
    got = _batched(_upload(states))
    assert np.isfinite(ref[0]).all() and np.isfinite(ref[1]).all()
    assert np.array_equal(ref[0], got[0]) and np.array_equal(ref[1], got[1])


def test_misaligned_state_takes_the_loop(txm, monkeypatch):
    """One x a view offset by one double: the single calls of the other states read two columns per lane, this one's
    cannot, so the wrapper loops over influence_cov -- the result still equals the single calls bit for bit."""
    import torch

    from thermoextrap_amd import engine

    states = _states((300, 257, 700), 4, 3, 3, True, 17)
    xs, us, ws, a, b, cu, cx = _upload(states)
    n = states[1][0].shape[0]
    buf = torch.empty(n * 4 + 1, dtype=torch.float64, device="cuda")
    buf[1:].view(n, 4).copy_(xs[1])
    xs[1] = buf[1:].view(n, 4)
    assert xs[1].data_ptr() % 16 == 8 and xs[0].data_ptr() % 16 == 0
    ops = (xs, us, ws, a, b, cu, cx)
    calls = []
    real = engine.influence_cov
    monkeypatch.setattr(engine, "influence_cov", lambda *a_, **k_: (calls.append(1), real(*a_, **k_))[1])
    cov, mean = _batched(ops)
    assert len(calls) == 3
    monkeypatch.undo()
    for s, (c1, m1) in enumerate(_singles(ops)):
        assert np.array_equal(cov[s], c1) and np.array_equal(mean[s], m1)
    # all states misaligned alike: one launch again (one column per lane for every state, as their single calls)
    n0 = states[0][0].shape[0]
    buf0 = torch.empty(n0 * 4 + 1, dtype=torch.float64, device="cuda")
    buf0[1:].view(n0, 4).copy_(xs[0])
    ops2 = ([buf0[1:].view(n0, 4), xs[1]], us[:2], ws[:2], a[:2], b[:2], cu[:2], cx[:2])
    monkeypatch.setattr(engine, "influence_cov", lambda *a_, **k_: pytest.fail("the loop ran"))
    cov2, mean2 = _batched(ops2)
    monkeypatch.undo()
    for s, (c1, m1) in enumerate(_singles(ops2)):
        assert np.array_equal(cov2[s], c1) and np.array_equal(mean2[s], m1)


def test_two_calls_same_bits(txm):
    ops = _upload(_states((5000, 1537, 3000), 32, 5, 5, True, 18))
    r1, r2 = _batched(ops), _batched(ops)
    assert np.array_equal(r1[0], r2[0]) and np.array_equal(r1[1], r2[1])


def test_wrapper_rejects_bad_arguments(txm):
    import torch

    from thermoextrap_amd import _lib, engine

    z = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")  # noqa: E731
    xs, us = [z(10, 2), z(7, 2)], [z(10), z(7)]
    ab, cx, cu = z(2, 2, 3, 3), z(2, 2), [0.0, 0.0]
    engine.influence_cov_batched(xs, us, ab, ab, cu, cx)                           # the good call
    with pytest.raises(ValueError):
        engine.influence_cov_batched([], [], ab, ab, cu, cx)                       # S = 0
    with pytest.raises(ValueError):
        engine.influence_cov_batched(xs, us[:1], ab, ab, cu, cx)
    with pytest.raises(ValueError):
        engine.influence_cov_batched(xs, [z(10), z(8)], ab, ab, cu, cx)            # u of another length than x
    with pytest.raises(ValueError):
        engine.influence_cov_batched([z(10, 2), z(7, 3)], us, ab, ab, cu, cx)      # columns differ
    with pytest.raises(ValueError):
        engine.influence_cov_batched(xs, us, ab, ab[:, :, :2], cu, cx)
    with pytest.raises(ValueError):
        engine.influence_cov_batched(xs, us, ab[:1], ab[:1], cu, cx)
    with pytest.raises(ValueError):
        engine.influence_cov_batched(xs, us, ab, ab, cu, cx[:1])
    with pytest.raises(ValueError):
        engine.influence_cov_batched(xs, us, ab, ab, [0.0], cx)
    with pytest.raises(ValueError):
        engine.influence_cov_batched(xs, us, ab, ab, cu, cx, ws=[z(10), None])     # mixed w
    with pytest.raises(TypeError):
        engine.influence_cov_batched([xs[0].float(), xs[1]], us, ab, ab, cu, cx)
    big = z(2, 2, 3, 10)
    with pytest.raises(_lib.TxmError):
        engine.influence_cov_batched(xs, us, big, big, cu, cx)
