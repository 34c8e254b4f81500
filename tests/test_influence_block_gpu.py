"""txm_influence_block_cov through the engine (engine.influence_block_cov): every level's cov and the mean against the
definition restated in long double with the same coefficient arrays,

    z_b[k] = sum_{n in block b} p_n psi_k(n)      cov[l][i][j] = sum_b z_b[i] z_b[j]      mean[k] = sum_n p_n psi_k(n)

within the first-order bound of the block sums' own evaluation

    |cov - ref|[i][j] <= 1e-12 sum_b beta_bi beta_bj     |mean_k - ref| <= 1e-12 sum_n p_n B_k(n)
    beta_bk = sum_{n in b} p_n B_k(n),   B_k(n) = sum_q (|a_kq| + |b_kq| |dx|) |du|^q

(a block sum carries a first-order error of a few eps beta_bk and |z_bk| <= beta_bk; 1e-12 is the project's constant for
such bounds) on the smallest shapes at which the kernels can go wrong: block lengths below, at and above a workgroup's row
slots, N = k block + r with short and full last blocks, columns that do not fill a lane group, both column widths per lane,
a padded pitch, centres 3 sigma off, dead rows, a dead block, levels up to a single block."""

from __future__ import annotations

import numpy as np
import pytest

from tests._influence_ref import LD, bound_ld, psi_ld

pytestmark = pytest.mark.gpu

TOL = 1e-12
BLOCKS = [1, 2, 7, 64, 256, 1000]
CS = [1, 3, 4, 33]
NQS = [1, 2, 5, 6, 7, 9]
_worst = {"cov": 0.0, "mean": 0.0}


def _problem(N, C, nf, nq, weighted, seed):
    rng = np.random.default_rng(seed)
    u = rng.normal(3.0, 1.0, N)
    x = np.stack([(0.7 * u + 0.3 * u * u + rng.normal(2.0, 1.0, N)) * (1.0 + 0.5 * (c % 5)) for c in range(C)], axis=1)
    w = rng.uniform(0.5, 1.5, N) if weighted else None
    a, b = rng.normal(size=(C, nf, nq)), rng.normal(size=(C, nf, nq))
    cu = 3.0 + 3.0 * 1.0                                                                  # centres 3 sigma off the means
    cx = np.array([(7.1 - 3.0 * 2.73) * (1.0 + 0.5 * (c % 5)) for c in range(C)])
    return x, u, w, a, b, cu, cx


def _n_levels_to_one_block(N, block):
    """Levels 0 .. the first with a single block."""
    n = 1
    while -(-N // (block << (n - 1))) > 1:
        n += 1
    return n


def _device_x(x, pitch):
    import torch

    N, C = x.shape
    if pitch is None:
        return torch.from_numpy(x).cuda()
    buf = torch.full((N, pitch), float("nan"), dtype=torch.float64, device="cuda")        # the padding is never read
    buf[:, :C] = torch.from_numpy(x).cuda()
    return buf[:, :C]


def _run(x, u, w, a, b, cu, cx, block, n_levels, pitch=None):
    import torch

    from thermoextrap_amd import engine

    dev = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v)).cuda()  # noqa: E731
    cov, mean = engine.influence_block_cov(_device_x(x, pitch), dev(u), dev(a), dev(b), cu, dev(cx), block,
                                           n_levels=n_levels, w=dev(w))
    return cov.cpu().numpy(), mean.cpu().numpy()


def _reference(x, u, w, a, b, cu, cx, block, n_levels):
    """(cov [l][c], bound [l][c], mean [c], mean bound [c]) in long double; rows of weight zero are selected out."""
    N, C = x.shape
    wl = np.ones(N, LD) if w is None else np.asarray(w, LD)
    live = wl != 0
    tot = wl.sum()
    p = wl / tot if tot != 0 else wl
    du = np.where(live, np.asarray(u, LD) - LD(cu), LD(0))
    cov, bnd, mean, mbnd = [], [], [], []
    for c in range(C):
        dx = np.where(live, np.asarray(x[:, c], LD) - LD(cx[c]), LD(0))
        ppsi, pB = p * psi_ld(a[c], b[c], dx, du), p * bound_ld(a[c], b[c], dx, du)
        mean.append(ppsi.sum(axis=1))
        mbnd.append(pB.sum(axis=1))
        cl, bl = [], []
        for l in range(n_levels):
            starts = np.arange(0, N, block << l)
            z, beta = np.add.reduceat(ppsi, starts, axis=1), np.add.reduceat(pB, starts, axis=1)
            cl.append(z @ z.T)
            bl.append(beta @ beta.T)
        cov.append(cl)
        bnd.append(bl)
    tr = lambda v: [[v[c][l] for c in range(C)] for l in range(n_levels)]  # noqa: E731
    return tr(cov), tr(bnd), mean, mbnd


def _check(N, C, nf, nq, weighted, block, n_levels=None, pitch=None, seed=0, edit=None):
    x, u, w, a, b, cu, cx = _problem(N, C, nf, nq, weighted, seed)
    if edit is not None:
        x, u, w = edit(x, u, w)
    if n_levels is None:
        n_levels = _n_levels_to_one_block(N, block)
    cov, mean = _run(x, u, w, a, b, cu, cx, block, n_levels, pitch)
    assert cov.shape == (n_levels, C, nf, nf) and mean.shape == (C, nf)
    cref, cbnd, mref, mbnd = _reference(x, u, w, a, b, cu, cx, block, n_levels)
    for c in range(C):
        rm = float((np.abs(mean[c] - mref[c]) / mbnd[c]).max())
        _worst["mean"] = max(_worst["mean"], rm)
        assert rm <= TOL, (N, C, nf, nq, weighted, block, c, rm)
        for l in range(n_levels):
            rc = float((np.abs(cov[l, c] - cref[l][c]) / cbnd[l][c]).max())
            _worst["cov"] = max(_worst["cov"], rc)
            assert rc <= TOL, (N, C, nf, nq, weighted, block, l, c, rc)
            assert np.array_equal(cov[l, c], cov[l, c].T)
    return (x, u, w, a, b, cu, cx), cov, mean, cbnd


@pytest.mark.parametrize("block", BLOCKS)
def test_block_lengths_and_tails(txm, block):
    """N = k block + r, k in {1, 2, 5}, r in {0, 1, block - 1}: full, one-row and one-short last blocks, every level up to
    a single block; C, n_q and the weights rotate through their sets (every pairing is in test_every_instantiation)."""
    i = BLOCKS.index(block)
    for k in (1, 2, 5):
        for r in sorted({0, 1, block - 1}):
            C, nq = CS[i % 4], NQS[i % 6]
            _check(k * block + r, C, nq, nq, i % 2 == 0, block, seed=i)
            i += 1
    print(f"block={block}: worst ratio to the bound so far: cov {_worst['cov']:.2e}, mean {_worst['mean']:.2e}")


@pytest.mark.parametrize("nq", NQS)
def test_every_instantiation(txm, nq):
    """n_q x C in {1, 3, 4, 33} x {weighted, unweighted}: two columns per lane (even C, n_q <= 6) and one, at a block
    shorter than a workgroup's row slots (several blocks per workgroup step) and a longer one."""
    for C in CS:
        for weighted in (False, True):
            _check(5 * 7 + 3, C, nq, nq, weighted, 7, seed=nq)
            _check(2 * 300 + 41, C, nq, nq, weighted, 300, seed=nq + 1)
    print(f"n_q={nq}: worst ratio to the bound so far: cov {_worst['cov']:.2e}, mean {_worst['mean']:.2e}")


def test_n_below_block_nf_differs_from_nq_and_column_chunks(txm):
    _check(45, 4, 3, 5, True, 64)                   # N < block: one short block at every level
    _check(300, 4, 3, 5, True, 7)                   # n_f != n_q
    _check(300, 3, 7, 2, False, 64)
    _check(80, 514, 2, 2, True, 7)                  # more than 256 lanes' worth of columns: two column chunks
    _check(80, 259, 2, 7, False, 64)
    _check(20000, 4, 5, 5, True, 2)                 # more workgroup steps than one workgroup takes: the grid stride


@pytest.mark.parametrize("C,pitch", [(4, 8), (4, 7), (3, 6), (33, 40)])
def test_padded_pitch(txm, C, pitch):
    """Rows of `pitch` doubles with NaN behind the C columns: even pitches (two columns per lane) and an odd one."""
    for block in (7, 256):
        _check(3 * block + 5, C, 5, 5, True, block, pitch=pitch)


@pytest.mark.parametrize("C", [3, 4])
def test_zero_weight_rows_may_hold_anything(txm, C):
    """Rows of weight zero holding 1e150 and NaN (in x and in u) leave every bit where ordinary values leave it."""
    N, nq, block = 700, 5, 64
    x, u, w, a, b, cu, cx = _problem(N, C, nq, nq, True, 5)
    dead = np.arange(3, N, 7)
    w[dead] = 0.0
    nl = _n_levels_to_one_block(N, block)
    ref = _run(x, u, w, a, b, cu, cx, block, nl)
    x2, u2 = x.copy(), u.copy()
    x2[dead] = np.where(np.arange(len(dead))[:, None] % 2 == 0, 1e150, np.nan)
    u2[dead] = np.where(np.arange(len(dead)) % 3 == 0, np.nan, -1e150)
    got = _run(x2, u2, w, a, b, cu, cx, block, nl)
    assert np.isfinite(ref[0]).all() and np.isfinite(ref[1]).all()
    assert np.array_equal(ref[0], got[0]) and np.array_equal(ref[1], got[1])


@pytest.mark.parametrize("block", [7, 64, 1000])
def test_a_whole_block_of_zero_weight(txm, block):
    """Block 1 of four is dead (weight zero, holding NaN) between live ones: it contributes zero at every level."""
    def edit(x, u, w):
        w[block:2 * block] = 0.0
        x[block:2 * block] = np.nan
        u[block:2 * block] = 1e150
        return x, u, w

    _check(3 * block + block // 2 + 1, 4, 5, 5, True, block, seed=3, edit=edit)


@pytest.mark.parametrize("block,N,C", [(7, 7 * 37 + 3, 4), (64, 64 * 9, 3), (2, 257, 1)])
def test_levels_equal_level_zero_of_the_longer_block(txm, block, N, C):
    """Level l of one call against level 0 of a call at block 2^l (the same estimator by definition), under the bound."""
    prob, cov, mean, cbnd = _check(N, C, 5, 5, True, block, seed=11)
    for l in range(cov.shape[0]):
        c0, _ = _run(*prob, block << l, 1)
        for c in range(C):
            assert (np.abs(cov[l, c] - c0[0, c]) <= TOL * cbnd[l][c].astype(np.float64)).all(), (block, l, c)


@pytest.mark.parametrize("block,C", [(1, 33), (7, 4), (1000, 32)])
def test_two_calls_same_bits(txm, block, C):
    x, u, w, a, b, cu, cx = _problem(5003, C, 5, 5, True, 7)
    nl = _n_levels_to_one_block(5003, block)
    r1 = _run(x, u, w, a, b, cu, cx, block, nl)
    r2 = _run(x, u, w, a, b, cu, cx, block, nl)
    assert np.array_equal(r1[0], r2[0]) and np.array_equal(r1[1], r2[1])


@pytest.mark.parametrize("block", [7, 64])
def test_total_weight_zero_gives_zeros(txm, block):
    x, u, w, a, b, cu, cx = _problem(300, 4, 3, 3, True, 6)
    cov, mean = _run(x, u, np.zeros_like(w), a, b, cu, cx, block, 4)
    assert not cov.any() and not mean.any()


@pytest.mark.parametrize("N,C,nf,nq,block", [(5 * 7 + 3, 3, 5, 5, 7), (641, 4, 3, 5, 300), (80, 259, 2, 7, 2), (45, 4, 5, 5, 64)])
def test_bands_behind_workspace_and_cov_are_untouched(txm, N, C, nf, nq, block):
    """The C call with a workspace of exactly the queried size: 4 KiB behind it and behind cov keep their pattern."""
    import torch

    from thermoextrap_amd import _lib, engine

    L = engine._L()
    x, u, w, a, b, cu, cx = _problem(N, C, nf, nq, True, 9)
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()  # noqa: E731
    xd, ud, wd, ad, bd, cxd = dev(x), dev(u), dev(w), dev(a), dev(b), dev(cx)
    nl = _n_levels_to_one_block(N, block)
    need = L.txm_influence_block_cov_ws_bytes(N, C, nf, nq, block)
    assert need == 8 * -(-N // block) * (C * nf + 1) + 256
    ws = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    ncov = nl * C * nf * nf
    cov = torch.full((ncov + 512,), -7.25, dtype=torch.float64, device="cuda")
    mean = torch.full((C * nf + 512,), -7.25, dtype=torch.float64, device="cuda")
    _lib.check(L.txm_influence_block_cov(xd.data_ptr(), C, ud.data_ptr(), wd.data_ptr(), N, C, nf, nq, cu, cxd.data_ptr(),
                                         ad.data_ptr(), bd.data_ptr(), block, nl, cov.data_ptr(), mean.data_ptr(),
                                         ws.data_ptr(), need, None), "txm_influence_block_cov")
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0xA5).all()) and bool((cov[ncov:] == -7.25).all()) and bool((mean[C * nf:] == -7.25).all())
    ref = _run(x, u, w, a, b, cu, cx, block, nl)
    assert np.array_equal(cov[:ncov].cpu().numpy().reshape(nl, C, nf, nf), ref[0])
    # one byte short: refused, nothing enqueued
    assert L.txm_influence_block_cov(xd.data_ptr(), C, ud.data_ptr(), wd.data_ptr(), N, C, nf, nq, cu, cxd.data_ptr(),
                                     ad.data_ptr(), bd.data_ptr(), block, nl, cov.data_ptr(), mean.data_ptr(),
                                     ws.data_ptr(), need - 1, None) != 0


def test_wrapper_rejects_bad_arguments(txm):
    import torch

    from thermoextrap_amd import _lib, engine

    x = torch.zeros((10, 2), dtype=torch.float64, device="cuda")
    u = torch.zeros(10, dtype=torch.float64, device="cuda")
    ab = torch.zeros((2, 3, 3), dtype=torch.float64, device="cuda")
    cx = torch.zeros(2, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        engine.influence_block_cov(x, u, ab, ab[:, :2], 0.0, cx, 2)
    with pytest.raises(ValueError):
        engine.influence_block_cov(x, u, ab, ab, 0.0, cx, 0)
    with pytest.raises(ValueError):
        engine.influence_block_cov(x, u, ab, ab, 0.0, cx, 2, n_levels=33)
    big = torch.zeros((2, 3, 10), dtype=torch.float64, device="cuda")
    with pytest.raises(_lib.TxmError):
        engine.influence_block_cov(x, u, big, big, 0.0, cx, 2)
