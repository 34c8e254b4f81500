"""txm_influence_block_cross_cov through the engine (engine.influence_block_cross_cov): every level's

    z_b[c][k] = sum_{n in block b} p_n psi_k(n, c)      cov[l][c][i][c'][j'] = sum_b z_b[c][i] z_b[c'][j']
    mean[c][k] = sum_n p_n psi_k(n, c)

against the definition restated in long double with the same coefficient arrays (tests/_influence_cross_ref.py:
psi_and_bound; block sums of p psi and p B are the whole reference), within the first-order bound

    |cov - ref| <= 1e-12 sum_b beta_b(c, i) beta_b(c', j')      |mean - ref| <= 1e-12 sum_n p_n B_k(n, c)
    beta_b(c, k) = sum_{n in b} p_n B_k(n, c),   B_k = sum_q (|a_kq| + |b_kq| |dx|) |du|^q

on the smallest shapes at which the kernels can go wrong: M = C n_f at every position of the 16-column tile and of the
4 x 4-tile macro tile, every position of the 4-block step, a workgroup's share of 256 blocks - 1 / + 0 / + 1, several
workgroups with a ragged tail, the workgroup cap binding, block lengths with full, one-row and one-short last blocks,
N < B, and every level down to a single block with odd block counts on the way.  The printed worst ratios are kept as
profiles/r19_block_cross_cov_gpu_tests.txt."""

from __future__ import annotations

import numpy as np
import pytest

from tests._influence_cross_ref import psi_and_bound

pytestmark = pytest.mark.gpu

TOL = 1e-12
SHARE = 256            # blocks a workgroup takes before the grid grows by one (txm_influence_block_cross.hip, BX_SHARE)
NQS = [1, 2, 5, 6, 7, 9]
# (C, n_f): M = 1, 15, 16, 17, 32, 33, 165; then the macro-tile edge (4 tiles = 64 columns) at T = 3, 4, 5 and 8, 9 tiles
TILE_SHAPES = [(1, 1), (3, 5), (4, 4), (17, 1), (16, 2), (11, 3), (33, 5), (16, 3), (16, 4), (13, 5), (32, 4), (43, 3)]
_worst: dict = {}


def _problem(N, C, nf, nq, weighted, seed):
    rng = np.random.default_rng(seed)
    u = rng.normal(3.0, 1.0, N)
    x = np.stack([(0.7 * u + 0.3 * u * u + rng.normal(2.0, 1.0, N)) * (1.0 + 0.5 * (c % 5)) for c in range(C)], axis=1)
    w = rng.uniform(0.5, 1.5, N) if weighted else None
    a, b = rng.normal(size=(C, nf, nq)), rng.normal(size=(C, nf, nq))
    cu = 3.0 + 3.0 * 1.0                                                                  # centres 3 sigma off the means
    cx = np.array([(7.1 - 3.0 * 2.73) * (1.0 + 0.5 * (c % 5)) for c in range(C)])
    return x, u, w, a, b, cu, cx


def _levels_to_one_block(N, block):
    """Levels 0 .. the first with a single block."""
    n = 1
    while -(-N // (block << (n - 1))) > 1:
        n += 1
    return n


def _dev(v):
    import torch

    return None if v is None else torch.from_numpy(np.ascontiguousarray(v)).cuda()


def _device_x(x, pitch=None, misalign=False):
    """x on the device: tight, in rows of `pitch` doubles with NaN behind the C columns, or tight at a pointer 8 bytes off
    16-byte alignment."""
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
    return torch.from_numpy(x).cuda()


def _run(x, u, w, a, b, cu, cx, block, n_levels, pitch=None, misalign=False):
    from thermoextrap_amd import engine

    cov, mean = engine.influence_block_cross_cov(_device_x(x, pitch, misalign), _dev(u), _dev(a), _dev(b), cu, _dev(cx), block,
                                                 n_levels=n_levels, w=_dev(w))
    return cov.cpu().numpy(), mean.cpu().numpy()


def _reference(x, u, w, a, b, cu, cx, block, n_levels, cols=None):
    """(cov [l][C', n_f, C', n_f], bound likewise, mean [C', n_f], mean bound) in long double."""
    p, psi, B = psi_and_bound(x, u, w, a, b, cu, cx, cols)
    Cc, nf, N = psi.shape
    ppsi, pB = (psi * p).reshape(Cc * nf, N), (B * p).reshape(Cc * nf, N)
    cov, bnd = [], []
    for l in range(n_levels):
        starts = np.arange(0, N, block << l)
        z, beta = np.add.reduceat(ppsi, starts, axis=1), np.add.reduceat(pB, starts, axis=1)
        cov.append((z @ z.T).reshape(Cc, nf, Cc, nf))
        bnd.append((beta @ beta.T).reshape(Cc, nf, Cc, nf))
    return cov, bnd, ppsi.sum(axis=1).reshape(Cc, nf), pB.sum(axis=1).reshape(Cc, nf)


def _ratio(group, key, err, bnd, what):
    r = float((np.abs(err) / bnd).max())
    _worst.setdefault(group, {"cov": 0.0, "mean": 0.0})
    _worst[group][key] = max(_worst[group][key], r)
    assert r <= TOL, (what, key, r)


def _check(group, N, C, nf, nq, weighted, block, n_levels=None, seed=0, pitch=None, misalign=False, edit=None, cols=None):
    prob = _problem(N, C, nf, nq, weighted, seed)
    if edit is not None:
        prob = edit(*prob)
    if n_levels is None:
        n_levels = _levels_to_one_block(N, block)
    cov, mean = _run(*prob, block, n_levels, pitch=pitch, misalign=misalign)
    assert cov.shape == (n_levels, C, nf, C, nf) and mean.shape == (C, nf)
    for l in range(n_levels):
        flat = cov[l].reshape(C * nf, C * nf)
        assert np.array_equal(flat, flat.T), (N, C, nf, nq, block, l)                    # exact symmetry, every level
    cref, cbnd, mref, mbnd = _reference(*prob, block, n_levels, cols=cols)
    sel = (lambda v: v) if cols is None else (lambda v: v[np.ix_(cols, range(nf), cols, range(nf))])
    what = (N, C, nf, nq, weighted, block, pitch, misalign)
    _ratio(group, "mean", (mean if cols is None else mean[cols]) - mref, mbnd, what)
    for l in range(n_levels):
        _ratio(group, "cov", sel(cov[l]) - cref[l], cbnd[l], (*what, l))
    return prob, cov, mean, cbnd


def _report(group):
    w = _worst.get(group, {"cov": 0.0, "mean": 0.0})
    print(f"{group}: worst ratio to the bound: cov {w['cov']:.2e}, mean {w['mean']:.2e}  (limit {TOL:.0e})")


@pytest.mark.parametrize("C,nf", TILE_SHAPES)
def test_tile_and_macro_tile_edges(txm, C, nf):
    """M = C n_f around the tile and the macro-tile edges x {weighted, unweighted}, n_q rotating through its set
    (n_f != n_q almost everywhere), 9 and 37 blocks of 3 rows with a one-short last block, every level."""
    i = TILE_SHAPES.index((C, nf))
    for weighted in (False, True):
        _check("tile edges", 9 * 3 - 1, C, nf, NQS[i % 6], weighted, 3, seed=i)
        _check("tile edges", 37 * 3 - 1, C, nf, NQS[(i + 1) % 6], weighted, 3, seed=i + 1)
        i += 2
    _report("tile edges")


def test_255_columns(txm):
    """C = 255 with n_f = 2 (M = 510: 32 tiles, 8 macro tiles a side, 36 macro pairs), the reference restated on the
    columns at the tile and macro-tile edges, the first and the last; the full matrix is checked for symmetry."""
    cols = [0, 7, 8, 31, 32, 127, 128, 223, 224, 254]
    _check("255 columns", 2 * 41 + 1, 255, 2, 5, True, 2, seed=1, cols=cols)
    _check("255 columns", 7 * 300, 255, 2, 2, False, 7, n_levels=3, seed=2, cols=cols)
    _report("255 columns")


def test_grid_at_its_cap_of_macro_pairs(txm):
    """C = 255 with n_f = 9: M = 2295, 144 tiles, 36 macro tiles a side, 666 macro pairs -- more than the workgroup cap, one
    block workgroup each; ten blocks, one level."""
    cols = [0, 1, 7, 14, 15, 113, 114, 247, 248, 254]
    _check("M = 2295", 10 * 2, 255, 9, 2, True, 2, n_levels=1, seed=3, cols=cols)
    _report("M = 2295")


@pytest.mark.parametrize("nb", [1, 2, 3, 4, 5, 7, 8, 9])
def test_positions_of_the_four_block_step(txm, nb):
    for C, nf, nq in ((3, 5, 5), (17, 2, 6), (13, 5, 7)):
        _check("4-block step", nb * 2, C, nf, nq, nb % 2 == 0, 2, seed=nb)
        _check("4-block step", nb, C, nf, nq, nb % 2 == 1, 1, seed=nb + 1)
    _report("4-block step")


@pytest.mark.parametrize("nb", [SHARE - 1, SHARE, SHARE + 1, 5 * SHARE + 37])
def test_around_a_workgroup_share_of_blocks(txm, nb):
    """One workgroup's share of blocks - 1 / + 0 / + 1 (the grid grows from one workgroup to two) and several workgroups
    with a ragged tail; the inner levels walk back down through the share."""
    _check("share", nb * 2 - 1, 3, 5, 5, True, 2, seed=nb)
    _check("share", nb, 17, 2, 2, False, 1, seed=nb + 1)
    _check("share", nb * 3, 13, 5, 9, True, 3, n_levels=3, seed=nb + 2)
    _report("share")


def test_workgroup_cap_binds_and_waves_stride(txm):
    """M = 165 (3 macro tiles a side, 6 macro pairs) caps the block workgroups at 4 per CU / 6: more than twice that many
    shares of blocks makes every wave take several strided steps, at level 0 and at level 1.  Reference on the columns at
    the tile edges."""
    import torch

    cap = max(torch.cuda.get_device_properties(0).multi_processor_count * 4 // 6, 1)
    nb = 2 * cap * SHARE + 77
    _check("cap", nb, 33, 5, 2, True, 1, n_levels=3, seed=1, cols=[0, 3, 12, 13, 25, 32])
    _report("cap")


@pytest.mark.parametrize("block", [1, 2, 7, 64, 256, 1000])
def test_block_lengths_and_tails(txm, block):
    """N = k block + r, k in {1, 2, 5}, r in {0, 1, block - 1}, every level down to a single block; N < block."""
    i = [1, 2, 7, 64, 256, 1000].index(block)
    shapes = [(3, 5), (4, 4), (17, 1), (11, 3)]
    for k in (1, 2, 5):
        for r in sorted({0, 1, block - 1}):
            C, nf = shapes[i % 4]
            _check("block lengths", k * block + r, C, nf, NQS[i % 6], i % 2 == 0, block, seed=i)
            i += 1
    if block > 1:
        _check("block lengths", block - 1, 4, 3, 5, True, block, n_levels=3, seed=i)     # N < block: one short block
    _report("block lengths")


@pytest.mark.parametrize("N,block", [(7 * 37 + 3, 7), (64 * 9, 64), (257, 2), (2 * 11, 2), (3 * 13 * 8 + 1, 3)])
def test_every_level_down_to_a_single_block_and_one_beyond(txm, N, block):
    """Odd block counts at inner levels (37 -> 19 -> 10 -> 5 -> 3 -> 2 -> 1, 129 -> 65 -> 33 -> 17 -> 9 -> 5 -> 3 -> 2 -> 1,
    ...): an unpaired last block stays.  One level more than needed: a single block again."""
    nl = _levels_to_one_block(N, block) + 1
    _check("levels", N, 13, 5, 5, True, block, n_levels=nl, seed=N)
    _check("levels", N, 3, 2, 7, False, block, n_levels=nl, seed=N + 1)
    _report("levels")


@pytest.mark.parametrize("nq", NQS)
def test_every_pass_one_instantiation(txm, nq):
    """n_q x {even C: two columns per lane up to n_q = 6; odd C} x {weighted, unweighted}, n_f != n_q."""
    nf = 3 if nq != 3 else 2
    for C in (4, 11):
        for weighted in (False, True):
            _check("n_q", 5 * 7 + 3, C, nf, nq, weighted, 7, seed=nq)
            _check("n_q", 2 * 300 + 41, C, nf, nq, weighted, 300, seed=nq + 1)
    _report("n_q")


@pytest.mark.parametrize("C,pitch", [(4, 8), (4, 7), (3, 6), (33, 40), (33, 35)])
def test_pitch_and_pointer_alignment(txm, C, pitch):
    """Rows of `pitch` doubles with NaN behind the C columns (even and odd pitches); a tight x 8 bytes off 16-byte
    alignment."""
    for block in (7, 256):
        _check("pitch", 3 * block + 5, C, 5, 5, True, block, pitch=pitch)
        _check("pitch", 3 * block + 5, C, 5, 5, False, block, misalign=True)
    _report("pitch")


@pytest.mark.parametrize("C", [3, 4, 33])
def test_zero_weight_rows_may_hold_anything(txm, C):
    """Rows of weight zero holding 1e150 and NaN (in x and in u) leave every bit where ordinary values leave it."""
    N, nq, block = 700, 5, 64
    x, u, w, a, b, cu, cx = _problem(N, C, nq, nq, True, 5)
    dead = np.arange(3, N, 7)
    w[dead] = 0.0
    nl = _levels_to_one_block(N, block)
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
    def edit(x, u, w, a, b, cu, cx):
        w[block:2 * block] = 0.0
        x[block:2 * block] = np.nan
        u[block:2 * block] = 1e150
        return x, u, w, a, b, cu, cx

    _check("dead block", 3 * block + block // 2 + 1, 17, 3, 5, True, block, seed=3, edit=edit)
    _report("dead block")


@pytest.mark.parametrize("block", [7, 64])
def test_total_weight_zero_gives_zeros(txm, block):
    x, u, w, a, b, cu, cx = _problem(300, 17, 3, 3, True, 6)
    x[::3] = np.nan
    cov, mean = _run(x, u, np.zeros_like(w), a, b, cu, cx, block, 4)
    assert cov.shape == (4, 17, 3, 17, 3) and not cov.any() and not mean.any()


@pytest.mark.parametrize("C,nf,weighted", [(1, 5, True), (4, 5, False), (17, 2, True), (33, 5, False)])
def test_block_one_is_the_iid_cross_covariance(txm, C, nf, weighted):
    """block = 1, level 0 against engine.influence_cross_cov on the same operands, within the sum of the two calls'
    bounds (at block = 1 the blocked bound IS the iid one: sum_n p_n^2 B B')."""
    from thermoextrap_amd import engine

    prob, cov, _, cbnd = _check("block = 1", 3 * SHARE + 11, C, nf, nf, weighted, 1, n_levels=1, seed=C)
    x, u, w, a, b, cu, cx = prob
    iid = engine.influence_cross_cov(_dev(x), _dev(u), _dev(a), _dev(b), cu, _dev(cx), w=_dev(w)).cpu().numpy()
    assert (np.abs(cov[0] - iid) <= 2 * TOL * cbnd[0].astype(np.float64)).all()
    _report("block = 1")


@pytest.mark.parametrize("C,nf,nq,block,weighted", [(1, 5, 5, 7, True), (4, 5, 5, 64, False), (17, 2, 7, 3, True),
                                                    (33, 5, 5, 300, True)])
def test_diagonal_blocks_against_influence_block_cov(txm, C, nf, nq, block, weighted):
    """cov[l][c][:, c][:] of every level against engine.influence_block_cov, within the sum of the two calls' bounds; the
    means too."""
    from thermoextrap_amd import engine

    N = 11 * block + block // 2 + 1
    prob, cov, mean, cbnd = _check("diagonal", N, C, nf, nq, weighted, block, seed=C)
    x, u, w, a, b, cu, cx = prob
    nl = cov.shape[0]
    col, cmean = engine.influence_block_cov(_dev(x), _dev(u), _dev(a), _dev(b), cu, _dev(cx), block, n_levels=nl, w=_dev(w))
    col, cmean = col.cpu().numpy(), cmean.cpu().numpy()
    _, _, _, mbnd = _reference(*prob, block, 1)
    assert (np.abs(mean - cmean) <= 2 * TOL * mbnd.astype(np.float64)).all()
    for l in range(nl):
        for c in range(C):
            assert (np.abs(cov[l, c, :, c, :] - col[l, c]) <= 2 * TOL * cbnd[l][c, :, c, :].astype(np.float64)).all(), (l, c)
    _report("diagonal")


@pytest.mark.parametrize("block,N,C", [(7, 7 * 37 + 3, 4), (64, 64 * 9, 17), (2, 257, 1)])
def test_levels_equal_level_zero_of_the_longer_block(txm, block, N, C):
    """Level l of one call against level 0 of a call at block 2^l (the same estimator by definition), under both bounds."""
    prob, cov, _, cbnd = _check("levels vs blocks", N, C, 5, 5, True, block, seed=11)
    for l in range(cov.shape[0]):
        c0, _ = _run(*prob, block << l, 1)
        assert (np.abs(cov[l] - c0[0]) <= 2 * TOL * cbnd[l].astype(np.float64)).all(), (block, l)
    _report("levels vs blocks")


@pytest.mark.parametrize("block,C,nf", [(1, 33, 5), (7, 4, 5), (1000, 32, 4), (2, 255, 2)])
def test_two_calls_same_bits(txm, block, C, nf):
    x, u, w, a, b, cu, cx = _problem(5003, C, nf, 5, True, 7)
    nl = _levels_to_one_block(5003, block)
    r1 = _run(x, u, w, a, b, cu, cx, block, nl)
    r2 = _run(x, u, w, a, b, cu, cx, block, nl)
    assert np.array_equal(r1[0], r2[0]) and np.array_equal(r1[1], r2[1])


@pytest.mark.parametrize("N,C,nf,nq,block", [(5 * 7 + 3, 3, 5, 5, 7), (641, 17, 3, 5, 300), (SHARE * 2 + 3, 13, 5, 7, 2),
                                             (45, 255, 2, 2, 64), (8, 255, 9, 1, 4)])
def test_bands_behind_workspace_and_cov_are_untouched(txm, N, C, nf, nq, block):
    """The C call with a workspace of exactly the queried size: 4 KiB behind it, behind cov and behind mean keep their
    pattern; one byte less is refused."""
    import torch

    from thermoextrap_amd import _lib, engine

    L = engine._L()
    x, u, w, a, b, cu, cx = _problem(N, C, nf, nq, True, 9)
    xd, ud, wd, ad, bd, cxd = _dev(x), _dev(u), _dev(w), _dev(a), _dev(b), _dev(cx)
    nl = _levels_to_one_block(N, block)
    need = L.txm_influence_block_cross_cov_ws_bytes(N, C, nf, nq, block, nl)
    assert need >= 8 * -(-N // block) * (C * nf + 1) + 256
    ws = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    ncov = nl * (C * nf) ** 2
    cov = torch.full((ncov + 512,), -7.25, dtype=torch.float64, device="cuda")
    mean = torch.full((C * nf + 512,), -7.25, dtype=torch.float64, device="cuda")
    args = (xd.data_ptr(), C, ud.data_ptr(), wd.data_ptr(), N, C, nf, nq, cu, cxd.data_ptr(), ad.data_ptr(), bd.data_ptr(),
            block, nl, cov.data_ptr(), mean.data_ptr(), ws.data_ptr())
    _lib.check(L.txm_influence_block_cross_cov(*args, need, None), "txm_influence_block_cross_cov")
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0xA5).all()) and bool((cov[ncov:] == -7.25).all()) and bool((mean[C * nf:] == -7.25).all())
    ref = _run(x, u, w, a, b, cu, cx, block, nl)
    assert np.array_equal(cov[:ncov].cpu().numpy().reshape(nl, C, nf, C, nf), ref[0])
    assert np.array_equal(mean[:C * nf].cpu().numpy().reshape(C, nf), ref[1])
    assert L.txm_influence_block_cross_cov(*args, need - 1, None) == -3


def test_every_refusal_returns_its_code_and_leaves_cov_unwritten(txm):
    import torch

    from thermoextrap_amd import engine

    L = engine._L()
    N, C, nf, nq, block, nl = 100, 4, 3, 3, 7, 3
    x, u, w, a, b, cu, cx = _problem(N, C, nf, nq, True, 2)
    t = dict(x=_dev(x), u=_dev(u), w=_dev(w), cx=_dev(cx), a=_dev(a), b=_dev(b))
    cov = torch.full((nl * (C * nf) ** 2,), -7.25, dtype=torch.float64, device="cuda")
    mean = torch.full((C * nf,), -7.25, dtype=torch.float64, device="cuda")
    need = L.txm_influence_block_cross_cov_ws_bytes(N, C, nf, nq, block, nl)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    names = ("x", "ls", "u", "w", "N", "C", "nf", "nq", "cu", "cx", "a", "b", "block", "nl", "cov", "mean", "ws", "wsb", "st")
    good = dict(x=t["x"].data_ptr(), ls=C, u=t["u"].data_ptr(), w=t["w"].data_ptr(), N=N, C=C, nf=nf, nq=nq, cu=cu,
                cx=t["cx"].data_ptr(), a=t["a"].data_ptr(), b=t["b"].data_ptr(), block=block, nl=nl, cov=cov.data_ptr(),
                mean=mean.data_ptr(), ws=ws.data_ptr(), wsb=need, st=None)

    def call(**bad):
        return L.txm_influence_block_cross_cov(*[{**good, **bad}[n] for n in names])

    for ptr in ("x", "u", "cx", "a", "b", "mean", "ws"):
        assert call(**{ptr: None}) == -1, ptr
    assert call(ls=C - 1) == -1 and b"pitch" in L.txm_last_error()
    assert call(cu=float("nan")) == -1 and b"NaN" in L.txm_last_error()
    assert call(wsb=need - 1) == -3
    assert call(C=256, ls=256) == -1 and b"255" in L.txm_last_error()
    assert call(N=0) == -1 and call(C=0) == -1 and call(nf=10) == -1 and call(nf=0) == -1 and call(nq=0) == -1 and call(nq=10) == -1
    assert call(block=0) == -1 and b"block" in L.txm_last_error()
    assert call(nl=0) == -1 and call(nl=33) == -1 and b"n_levels" in L.txm_last_error()
    torch.cuda.synchronize()
    assert bool((cov == -7.25).all()) and bool((mean == -7.25).all())
    assert call(cov=None) == -1
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((cov == -7.25).any()) and not bool((mean == -7.25).any())


def test_wrapper_rejects_bad_arguments(txm):
    import torch

    from thermoextrap_amd import _lib, engine

    x = torch.zeros((10, 2), dtype=torch.float64, device="cuda")
    u = torch.zeros(10, dtype=torch.float64, device="cuda")
    ab = torch.zeros((2, 3, 3), dtype=torch.float64, device="cuda")
    cx = torch.zeros(2, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        engine.influence_block_cross_cov(x, u, ab, ab[:, :2], 0.0, cx, 2)
    with pytest.raises(ValueError):
        engine.influence_block_cross_cov(x, u, ab, ab, 0.0, cx, 0)
    with pytest.raises(ValueError):
        engine.influence_block_cross_cov(x, u, ab, ab, 0.0, cx, 2, n_levels=33)
    big = torch.zeros((2, 3, 10), dtype=torch.float64, device="cuda")
    with pytest.raises(_lib.TxmError):
        engine.influence_block_cross_cov(x, u, big, big, 0.0, cx, 2)
    wide = torch.zeros((10, 256), dtype=torch.float64, device="cuda")
    abw = torch.zeros((256, 2, 2), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="255"):
        engine.influence_block_cross_cov(wide, u, abw, abw, 0.0, torch.zeros(256, dtype=torch.float64, device="cuda"), 2)
