"""txm_influence_cov through the C ABI (engine.influence_cov): cov and mean against the same sums taken in long double with
the same coefficient arrays, within the first-order bound of the sums' own evaluation

    |cov_ij - ref| <= 1e-12 sum_n p_n^2 B_i(n) B_j(n)     |mean_k - ref| <= 1e-12 sum_n p_n B_k(n)
    B_k(n) = sum_q (|a_kq| + |b_kq| |dx|) |du|^q

on the smallest shapes at which the kernels can go wrong: every kernel instantiation the launcher selects (n_q = 1 .. 9 x
{two columns per lane, one column per lane, series layout} x {weighted, unweighted}), N around one workgroup's share, columns
that do not fill a lane group, a row pitch larger than C, centres 3 sigma off the means."""

from __future__ import annotations

import numpy as np
import pytest

from tests._influence_ref import LD, bound_ld, psi_ld

pytestmark = pytest.mark.gpu

TOL = 1e-12
_worst = {"cov": 0.0, "mean": 0.0}


def _share(C, nq, layout):
    """Rows one workgroup takes before the grid grows by one (txm_influence.hip, influence_plan): 4 row slots."""
    if layout == "col" or C == 1:
        return 4 * 256
    vec = 2 if (C % 2 == 0 and layout != "row_odd_pitch" and nq <= 6) else 1
    lanes = -(-C // vec)
    l2 = 0
    while (1 << l2) < lanes and l2 < 8:
        l2 += 1
    return 4 * (256 >> l2)


def _problem(N, C, nf, nq, weighted, seed):
    rng = np.random.default_rng(seed)
    u = rng.normal(3.0, 1.0, N)
    x = np.stack([(0.7 * u + 0.3 * u * u + rng.normal(2.0, 1.0, N)) * (1.0 + 0.5 * (c % 5)) for c in range(C)], axis=1)
    w = rng.uniform(0.5, 1.5, N) if weighted else None
    a, b = rng.normal(size=(C, nf, nq)), rng.normal(size=(C, nf, nq))
    # centres 3 sigma off the true means (of the distribution: N = 1 has no spread of its own)
    cu = 3.0 + 3.0 * 1.0
    cx = np.array([(7.1 - 3.0 * 2.73) * (1.0 + 0.5 * (c % 5)) for c in range(C)])        # <x> = 7.1, sd 2.73 before scaling
    return x, u, w, a, b, cu, cx


def _device_x(x, layout):
    import torch

    N, C = x.shape
    if layout == "row":
        return torch.from_numpy(x).cuda()
    if layout in ("row_pitch", "row_odd_pitch"):
        pitch = C + (4 if layout == "row_pitch" else 3) + C % 2          # even / odd pitch
        buf = torch.full((N, pitch), float("nan"), dtype=torch.float64, device="cuda")   # the padding is never read
        buf[:, :C] = torch.from_numpy(x).cuda()
        return buf[:, :C]
    assert layout == "col"
    return torch.from_numpy(np.ascontiguousarray(x.T)).cuda().T


def _run(txm, x, u, w, a, b, cu, cx, layout):
    import torch

    from thermoextrap_amd import engine

    dev = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v)).cuda()  # noqa: E731
    cov, mean = engine.influence_cov(_device_x(x, layout), dev(u), dev(a), dev(b), cu, dev(cx), w=dev(w))
    return cov.cpu().numpy(), mean.cpu().numpy()


def _check(txm, N, C, nf, nq, weighted, layout, seed=0):
    x, u, w, a, b, cu, cx = _problem(N, C, nf, nq, weighted, seed)
    cov, mean = _run(txm, x, u, w, a, b, cu, cx, layout)
    assert cov.shape == (C, nf, nf) and mean.shape == (C, nf)
    wl = np.ones(N, LD) if w is None else np.asarray(w, LD)
    p = wl / wl.sum()
    du = np.asarray(u, LD) - LD(cu)
    for c in range(C):
        dx = np.asarray(x[:, c], LD) - LD(cx[c])
        psi, B = psi_ld(a[c], b[c], dx, du), bound_ld(a[c], b[c], dx, du)
        cref = np.einsum("n,in,jn->ij", p * p, psi, psi)
        cbnd = np.einsum("n,in,jn->ij", p * p, B, B)
        mref, mbnd = psi @ p, B @ p
        rc = float((np.abs(cov[c] - cref) / cbnd).max())
        rm = float((np.abs(mean[c] - mref) / mbnd).max())
        _worst["cov"], _worst["mean"] = max(_worst["cov"], rc), max(_worst["mean"], rm)
        assert rc <= TOL and rm <= TOL, (N, C, nf, nq, weighted, layout, c, rc, rm)
        assert np.array_equal(cov[c], cov[c].T)
    return cov, mean


@pytest.mark.parametrize("nq", [1, 2, 5, 9])
@pytest.mark.parametrize("C", [1, 3, 32, 33])
def test_shapes_around_a_workgroup_share(txm, C, nq):
    """N in {1, 63, one workgroup's share -+ 1, three shares + 17}, weighted and unweighted, contiguous rows."""
    s = _share(C, nq, "row")
    for i, N in enumerate([1, 63, s - 1, s + 1, 3 * s + 17]):
        for weighted in (False, True):
            _check(txm, N, C, nq, nq, weighted, "row", seed=i)
    print(f"C={C} n_f=n_q={nq}: worst ratio to the bound so far: cov {_worst['cov']:.2e}, mean {_worst['mean']:.2e}")


@pytest.mark.parametrize("nq", range(1, 10))
def test_every_instantiation(txm, nq):
    """n_q = 1 .. 9 x {two columns per lane (even C, even pitch, n_q <= 6), one column per lane (odd pitch / odd C), series
    layout, one contiguous series} x {weighted, unweighted}; more than one workgroup each; a row pitch larger than C."""
    for layout, C in (("row", 4), ("row_pitch", 6), ("row_odd_pitch", 4), ("row", 5), ("col", 3), ("col", 1)):
        N = _share(C, nq, layout) + 45
        for weighted in (False, True):
            _check(txm, N, C, nq, nq, weighted, layout, seed=nq)
    print(f"n_q={nq}: worst ratio to the bound so far: cov {_worst['cov']:.2e}, mean {_worst['mean']:.2e}")


def test_nf_differs_from_nq_and_column_chunks(txm):
    _check(txm, 300, 4, 3, 5, True, "row")
    _check(txm, 300, 3, 7, 2, False, "col")
    _check(txm, 40, 514, 2, 2, True, "row")       # more than 256 lanes' worth of columns: two column chunks
    _check(txm, 40, 259, 2, 7, False, "row")


@pytest.mark.parametrize("layout,C", [("row", 4), ("row_odd_pitch", 3), ("col", 3)])
def test_zero_weight_rows_may_hold_anything(txm, layout, C):
    """Rows of weight zero holding +-1e150 (in x and in u) leave every bit where ordinary values leave it."""
    N, nq = 700, 5
    x, u, w, a, b, cu, cx = _problem(N, C, nq, nq, True, 5)
    dead = np.arange(3, N, 7)
    w[dead] = 0.0
    ref = _run(txm, x, u, w, a, b, cu, cx, layout)
    x2, u2 = x.copy(), u.copy()
    x2[dead] = np.where(np.arange(len(dead))[:, None] % 2 == 0, 1e150, -1e150)
    u2[dead] = np.where(np.arange(len(dead)) % 3 == 0, -1e150, 1e150)
    got = _run(txm, x2, u2, w, a, b, cu, cx, layout)
    assert np.isfinite(ref[0]).all() and np.isfinite(ref[1]).all()
    assert np.array_equal(ref[0], got[0]) and np.array_equal(ref[1], got[1])


@pytest.mark.parametrize("layout,C", [("row", 4), ("col", 3)])
def test_total_weight_zero_gives_zeros(txm, layout, C):
    x, u, w, a, b, cu, cx = _problem(300, C, 3, 3, True, 6)
    cov, mean = _run(txm, x, u, np.zeros_like(w), a, b, cu, cx, layout)
    assert not cov.any() and not mean.any()


@pytest.mark.parametrize("layout,C", [("row", 32), ("col", 3)])
def test_two_calls_same_bits(txm, layout, C):
    x, u, w, a, b, cu, cx = _problem(5000, C, 5, 5, True, 7)
    r1 = _run(txm, x, u, w, a, b, cu, cx, layout)
    r2 = _run(txm, x, u, w, a, b, cu, cx, layout)
    assert np.array_equal(r1[0], r2[0]) and np.array_equal(r1[1], r2[1])


def test_wrapper_rejects_bad_shapes(txm):
    import torch

    from thermoextrap_amd import _lib, engine

    x = torch.zeros((10, 2), dtype=torch.float64, device="cuda")
    u = torch.zeros(10, dtype=torch.float64, device="cuda")
    ab = torch.zeros((2, 3, 3), dtype=torch.float64, device="cuda")
    cx = torch.zeros(2, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        engine.influence_cov(x, u, ab, ab[:, :2], 0.0, cx)
    with pytest.raises(ValueError):
        engine.influence_cov(x, u, ab, ab, 0.0, cx[:1])
    big = torch.zeros((2, 3, 10), dtype=torch.float64, device="cuda")
    with pytest.raises(_lib.TxmError):
        engine.influence_cov(x, u, big, big, 0.0, cx)
