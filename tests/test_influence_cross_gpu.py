"""txm_influence_cross_cov through the engine (engine.influence_cross_cov) and ExtrapModel.derivs_cross_cov / predict_cov
(DESIGN 4.14): every block of

    cov[c][i][c'][j] = sum_n p_n^2 psi_i(n, c) psi_j(n, c')

against the definition restated in long double with the same coefficient arrays (tests/_influence_cross_ref.py), within
the first-order bound of the sums' own evaluation

    |cov - ref|[c][i][c'][j] <= 1e-12 sum_n p_n^2 B_i(n, c) B_j(n, c') + 2^-1022,   B_k = sum_q (|a_kq| + |b_kq| |dx|) |du|^q

(1e-12 is the project's constant for this family; 2^-1022 where float64 flushes) on the smallest shapes at which the
kernels can go wrong: the tile edge at every position relative to the column of ones (which sits behind the C
observables), one to three tiles a side, N below and above a 4-sample step, one wave's and one workgroup's share, several
workgroups with a ragged tail, and a grid at its cap that strides.  The printed worst ratios are kept as
profiles/r18_cross_cov_gpu_tests.txt."""

from __future__ import annotations

import math

import numpy as np
import pytest

from tests._influence_cross_ref import reference
from tests._influence_ref import LD, bound_ld, ld_moments, make_data, psi_ld, series_for

pytestmark = pytest.mark.gpu

TOL = 1e-12
TINY = 2.0**-1022
SHARE = 256            # samples a workgroup takes before the grid grows by one (txm_influence_cross.hip, cx_plan)
CS = [1, 2, 15, 16, 17, 31, 32, 33]
NQS = [1, 2, 5, 9]
NS = [1, 3, 4, 5, 63, 64, 65]
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


def _run(x, u, w, a, b, cu, cx, pitch=None, misalign=False):
    from thermoextrap_amd import engine

    cov = engine.influence_cross_cov(_device_x(x, pitch, misalign), _dev(u), _dev(a), _dev(b), cu, _dev(cx), w=_dev(w))
    return cov.cpu().numpy()


def _compare(group, cov, ref, bnd, what):
    """Every entry within the bound; the worst ratio of the group is kept for the printed record."""
    ratio = float((np.abs(cov - ref) / (TOL * bnd + TINY)).max()) * TOL
    _worst[group] = max(_worst.get(group, 0.0), ratio)
    assert ratio <= TOL, (what, ratio)


def _check(group, N, C, nf, nq, weighted, seed=0, pitch=None, misalign=False, edit=None, cols=None):
    prob = _problem(N, C, nf, nq, weighted, seed)
    if edit is not None:
        prob = edit(*prob)
    cov = _run(*prob, pitch=pitch, misalign=misalign)
    assert cov.shape == (C, nf, C, nf)
    flat = cov.reshape(C * nf, C * nf)
    assert np.array_equal(flat, flat.T), (N, C, nf, nq, weighted)                        # exact symmetry, every call
    ref, bnd = reference(*prob, cols=cols)
    sub = cov if cols is None else cov[np.ix_(cols, range(nf), cols, range(nf))]
    _compare(group, sub, ref, bnd, (N, C, nf, nq, weighted, pitch, misalign))
    return prob, cov, bnd


def _report(group):
    print(f"{group}: worst |cov - ref| / sum p^2 B_ci B_c'j = {_worst.get(group, 0.0):.2e}")


@pytest.mark.parametrize("C", CS)
def test_tile_edges_orders_and_small_n(txm, C):
    """C around the tile edge x n_q = n_f in {1, 2, 5, 9} x {weighted, unweighted}; N walks through {1, 3, 4, 5, 63, 64, 65}."""
    i = CS.index(C)
    for nq in NQS:
        for weighted in (False, True):
            _check("tile edges", NS[i % len(NS)], C, nq, nq, weighted, seed=i)
            i += 1
    _report("tile edges")


@pytest.mark.parametrize("N", NS)
def test_every_small_n(txm, N):
    """Every N of the list at one, two and three tiles a side, order 4."""
    for C in (2, 17, 33):
        _check("small N", N, C, 5, 5, N % 2 == 0, seed=N)
    _report("small N")


@pytest.mark.parametrize("N", [SHARE - 1, SHARE, SHARE + 1, 5 * SHARE + 37])
def test_around_a_workgroup_share(txm, N):
    """One workgroup's share - 1 / + 0 / + 1 (the grid grows from one workgroup to two) and several workgroups with a
    ragged tail; n_f != n_q once."""
    _check("share", N, 3, 5, 5, True, seed=N)
    _check("share", N, 17, 2, 2, False, seed=N + 1)
    _check("share", N, 33, 3, 5, True, seed=N + 2)
    _report("share")


def test_grid_at_its_cap_strides(txm):
    """C = 255 (16 tiles a side, 136 tile pairs) caps the grid at 8 workgroups per CU / 136 along the samples: N above
    twice that many shares makes every wave take several strided steps.  The reference is restated on the columns at
    the tile edges, the first and the last (the full matrix is checked for symmetry)."""
    import torch

    cap = max(torch.cuda.get_device_properties(0).multi_processor_count * 8 // 136, 1)
    N = 2 * cap * SHARE + 77
    cols = [0, 15, 16, 127, 239, 240, 254]
    _check("cap", N, 255, 2, 2, True, seed=1, cols=cols)
    _check("cap", N, 255, 1, 1, False, seed=2, cols=cols)
    _report("cap")


@pytest.mark.parametrize("C", [1, 15, 16, 33])
def test_pitch_and_pointer_alignment(txm, C):
    """Rows of C + 3 doubles with NaN behind the columns; a tight x whose pointer is 8 bytes off 16-byte alignment."""
    for weighted in (False, True):
        _check("pitch", 300, C, 5, 5, weighted, seed=C, pitch=C + 3)
        _check("pitch", 300, C, 5, 5, weighted, seed=C, misalign=True)
    _report("pitch")


@pytest.mark.parametrize("C", [2, 16, 33])
def test_zero_weight_rows(txm, C):
    """Rows of weight zero holding 1e150 and NaN (in x and in u) leave every bit where ordinary values in the same rows
    leave it.  Against the call with those rows REMOVED the comparison is to tolerance (the sum of the two calls' bounds):
    the samples' assignment to waves, and so the order of the sums, depends on N."""
    N, nq = 700, 5
    x, u, w, a, b, cu, cx = _problem(N, C, nq, nq, True, 5)
    dead = np.arange(3, N, 7)
    w[dead] = 0.0
    ref = _run(x, u, w, a, b, cu, cx)
    x2, u2 = x.copy(), u.copy()
    x2[dead] = np.where(np.arange(len(dead))[:, None] % 2 == 0, 1e150, np.nan)
    u2[dead] = np.where(np.arange(len(dead)) % 3 == 0, np.nan, -1e150)
    got = _run(x2, u2, w, a, b, cu, cx)
    assert np.isfinite(ref).all() and np.array_equal(ref, got)
    keep = np.setdiff1d(np.arange(N), dead)
    short = _run(x[keep], u[keep], w[keep], a, b, cu, cx)
    _, bnd = reference(x[keep], u[keep], w[keep], a, b, cu, cx)
    assert (np.abs(got - short) <= 2 * TOL * bnd.astype(np.float64) + TINY).all()
    # and the long-double definition skips them too
    lref, lbnd = reference(x2, u2, w, a, b, cu, cx)
    _compare("zero weight", got, lref, lbnd, ("dead rows", C))
    _report("zero weight")


@pytest.mark.parametrize("C", [3, 17])
def test_total_weight_zero_gives_zeros(txm, C):
    x, u, w, a, b, cu, cx = _problem(300, C, 3, 3, True, 6)
    x[::3] = np.nan
    cov = _run(x, u, np.zeros_like(w), a, b, cu, cx)
    assert cov.shape == (C, 3, C, 3) and not cov.any()


@pytest.mark.parametrize("C,nq", [(2, 5), (16, 9), (33, 2)])
def test_two_calls_same_bits(txm, C, nq):
    prob = _problem(5003, C, nq, nq, True, 7)
    assert np.array_equal(_run(*prob), _run(*prob))


@pytest.mark.parametrize("N,C,nf,nq", [(65, 3, 5, 5), (641, 17, 3, 5), (SHARE + 1, 33, 2, 9), (2000, 255, 1, 1)])
def test_bands_behind_workspace_and_cov_are_untouched(txm, N, C, nf, nq):
    """The C call with a workspace of exactly the queried size: 4 KiB behind it and behind cov keep their pattern; one
    byte less is refused."""
    import torch

    from thermoextrap_amd import _lib, engine

    L = engine._L()
    x, u, w, a, b, cu, cx = _problem(N, C, nf, nq, True, 9)
    xd, ud, wd, ad, bd, cxd = _dev(x), _dev(u), _dev(w), _dev(a), _dev(b), _dev(cx)
    need = L.txm_influence_cross_cov_ws_bytes(N, C, nf, nq)
    ws = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    ncov = (C * nf) ** 2
    cov = torch.full((ncov + 512,), -7.25, dtype=torch.float64, device="cuda")
    args = (xd.data_ptr(), C, ud.data_ptr(), wd.data_ptr(), N, C, nf, nq, cu, cxd.data_ptr(), ad.data_ptr(), bd.data_ptr(),
            cov.data_ptr(), ws.data_ptr())
    _lib.check(L.txm_influence_cross_cov(*args, need, None), "txm_influence_cross_cov")
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0xA5).all()) and bool((cov[ncov:] == -7.25).all())
    assert np.array_equal(cov[:ncov].cpu().numpy().reshape(C, nf, C, nf), _run(x, u, w, a, b, cu, cx))
    assert L.txm_influence_cross_cov(*args, need - 1, None) == -3


def test_every_refusal_returns_its_code_and_leaves_cov_unwritten(txm):
    import torch

    from thermoextrap_amd import engine

    L = engine._L()
    N, C, nf, nq = 100, 4, 3, 3
    x, u, w, a, b, cu, cx = _problem(N, C, nf, nq, True, 2)
    t = dict(x=_dev(x), u=_dev(u), w=_dev(w), cx=_dev(cx), a=_dev(a), b=_dev(b))
    cov = torch.full(((C * nf) ** 2,), -7.25, dtype=torch.float64, device="cuda")
    need = L.txm_influence_cross_cov_ws_bytes(N, C, nf, nq)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    names = ("x", "ls", "u", "w", "N", "C", "nf", "nq", "cu", "cx", "a", "b", "cov", "ws", "wsb", "st")
    good = dict(x=t["x"].data_ptr(), ls=C, u=t["u"].data_ptr(), w=t["w"].data_ptr(), N=N, C=C, nf=nf, nq=nq, cu=cu,
                cx=t["cx"].data_ptr(), a=t["a"].data_ptr(), b=t["b"].data_ptr(), cov=cov.data_ptr(), ws=ws.data_ptr(), wsb=need,
                st=None)

    def call(**bad):
        return L.txm_influence_cross_cov(*[{**good, **bad}[n] for n in names])

    for ptr in ("x", "u", "cx", "a", "b", "ws"):
        assert call(**{ptr: None}) == -1, ptr
    assert call(ls=C - 1) == -1 and b"pitch" in L.txm_last_error()
    assert call(cu=float("nan")) == -1 and b"NaN" in L.txm_last_error()
    assert call(wsb=need - 1) == -3
    assert call(C=256, ls=256) == -1 and b"255" in L.txm_last_error()
    assert call(N=0) == -1 and call(nf=10) == -1 and call(nq=0) == -1
    torch.cuda.synchronize()
    assert bool((cov == -7.25).all())
    assert call(cov=None) == -1
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((cov == -7.25).any())


@pytest.mark.parametrize("C,nq,weighted", [(1, 5, True), (4, 5, False), (17, 2, True), (32, 9, True), (33, 5, False)])
def test_diagonal_blocks_against_influence_cov(txm, C, nq, weighted):
    """cov[c][:, c][:] against txm_influence_cov on the same operands, within the sum of the two calls' bounds."""
    from thermoextrap_amd import engine

    N = 3 * SHARE + 11
    prob, cov, bnd = _check("differential", N, C, nq, nq, weighted, seed=C)
    x, u, w, a, b, cu, cx = prob
    single, _ = engine.influence_cov(_dev(x), _dev(u), _dev(a), _dev(b), cu, _dev(cx), w=_dev(w))
    single = single.cpu().numpy()
    for c in range(C):
        lim = 2 * TOL * bnd[c, :, c, :].astype(np.float64) + TINY
        assert (np.abs(cov[c, :, c, :] - single[c]) <= lim).all(), c
    _report("differential")


# ---- the public interface ------------------------------------------------------------------------------------------------

ORDER, BETA0 = 4, 0.5


def _model(txm, x, u, w, order, central, minus_log=False):
    DA = txm.DataArray
    data = txm.DataCentralMomentsVals.from_vals(xv=DA(x, ("rec", "val")), uv=DA(u, ("rec",)), order=order, central=central,
                                                weight=None if w is None else DA(w, ("rec",)))
    m = txm.beta.factory_extrapmodel(beta=BETA0, data=data)
    return m.new_like(minus_log=True) if minus_log else m


def _api_reference(x, u, w, order, central, minus_log):
    """(V, bound) [c, i, c', j] in long double through symbolic.influence_coefs on long-double moments."""
    from tests._influence_cross_ref import cross_cov_ld
    from thermoextrap_amd import symbolic as S

    p, dx, du, mom = ld_moments(x, u, w, order)
    a, b = S.influence_coefs(series_for(central), order, mom, minus_log=minus_log)
    C = x.shape[1]
    psi = np.stack([psi_ld(a[c], b[c], dx[:, c], du) for c in range(C)])
    B = np.stack([bound_ld(a[c], b[c], dx[:, c], du) for c in range(C)])
    return cross_cov_ld(p, psi), cross_cov_ld(p, B)


@pytest.fixture(scope="module")
def data3():
    return make_data(200, seed=0, ncol=3)


@pytest.mark.parametrize("central", [True, False])
@pytest.mark.parametrize("minus_log", [False, True])
@pytest.mark.parametrize("weighted", [True, False])
def test_derivs_cross_cov_matches_long_double(txm, data3, central, minus_log, weighted):
    """N = 200, three columns, order 4: V within 1e-12 sum p^2 B_ci B_c'j of the long-double restatement; the blocks
    c == c' against derivs_cov() within the two bounds; norm=True carries 1 / (i! j!)."""
    x, u, w = data3
    w = w if weighted else None
    m = _model(txm, x, u, w, ORDER, central, minus_log)
    V = m.derivs_cross_cov()
    assert V.dims == ("order", "order_2", "val", "val_2") and V.shape == (ORDER + 1, ORDER + 1, 3, 3)
    ref, bnd = _api_reference(x, u, w, ORDER, central, minus_log)
    got = np.transpose(V.values, (2, 0, 3, 1))                                           # [c, i, c', j]
    _compare("derivs_cross_cov", got, ref, bnd, (central, minus_log, weighted))
    assert np.array_equal(got.reshape(15, 15), got.reshape(15, 15).T)
    D = m.derivs_cov().values                                                            # (order, order_2, val)
    for c in range(3):
        assert (np.abs(got[c, :, c, :] - D[:, :, c]) <= 2 * TOL * bnd[c, :, c, :].astype(np.float64) + TINY).all(), c
    f = np.array([1.0 / math.factorial(i) for i in range(ORDER + 1)])
    Vn = m.derivs_cross_cov(norm=True)
    np.testing.assert_allclose(Vn.values, V.values * f[:, None, None, None] * f[None, :, None, None], rtol=1e-15)
    V2 = m.derivs_cross_cov(order=2)
    assert V2.shape == (3, 3, 3, 3)
    _report("derivs_cross_cov")


def test_linearity_in_the_observable(txm):
    """A third column x_2 = x_0 + x_1, no minus_log: V[2,2] = V[0,0] + V[0,1] + V[1,0] + V[1,1] for every (i, j), within
    the bounds of the five blocks."""
    x, u, w = make_data(300, seed=3, ncol=2)
    x3 = np.concatenate([x, (x[:, 0] + x[:, 1])[:, None]], axis=1)
    for central in (True, False):
        V = np.transpose(_model(txm, x3, u, w, ORDER, central).derivs_cross_cov().values, (2, 0, 3, 1))
        _, bnd = _api_reference(x3, u, w, ORDER, central, False)
        total = V[0, :, 0, :] + V[0, :, 1, :] + V[1, :, 0, :] + V[1, :, 1, :]
        lim = TOL * (bnd[2, :, 2, :] + bnd[0, :, 0, :] + bnd[0, :, 1, :] + bnd[1, :, 0, :] + bnd[1, :, 1, :]).astype(np.float64)
        # (x_2 as stored is the ROUNDED sum: relative 2^-53 on dx, far inside the bound's 1e-12)
        assert (np.abs(V[2, :, 2, :] - total) <= lim + TINY).all(), central


@pytest.mark.parametrize("minus_log", [False, True])
def test_predict_cov(txm, data3, minus_log):
    x, u, w = data3
    m = _model(txm, x, u, w, ORDER, True, minus_log)
    alphas = np.array([0.3, 0.5, 0.62])
    pred, cov = m.predict_cov(alphas)
    ref = m.predict(alphas)
    assert pred.dims == ref.dims and np.array_equal(pred.values, ref.values)             # bit for bit
    assert cov.dims == (*ref.dims, "val_2") and cov.shape == (3, 3, 3)
    V = np.asarray(m.derivs_cross_cov().values, LD)                                      # (i, j, c, c')
    _, bnd = _api_reference(x, u, w, ORDER, True, minus_log)
    _, std = m.predict_with_error(alphas)
    for k, al in enumerate(alphas):
        t = np.array([LD(al - BETA0) ** i / math.factorial(i) for i in range(ORDER + 1)])
        want = np.einsum("i,ijcd,j->cd", t, V, t)
        tb = np.einsum("i,cidj,j->cd", np.abs(t), bnd, np.abs(t))
        assert (np.abs(cov.values[k] - want) <= TOL * tb.astype(np.float64) + TINY).all()
        # the diagonal is predict_with_error's variance (its V comes from the per-column kernel: both bounds)
        for c in range(3):
            assert abs(cov.values[k, c, c] - float(std.values[k, c]) ** 2) <= 3 * TOL * float(tb[c, c]) + TINY
    pred1, cov1 = m.predict_cov(0.3, order=2)
    assert np.array_equal(pred1.values, m.predict(0.3, order=2).values) and cov1.shape == (3, 3)


def test_caches_are_separate(txm, data3):
    x, u, w = data3
    m = _model(txm, x, u, w, ORDER, True)
    before = m.derivs_cov().values.copy()
    assert ("dxcov", ORDER, False) not in m._cache
    m.derivs_cross_cov()
    assert ("dxcov", ORDER, False) in m._cache
    assert np.array_equal(m.derivs_cov().values, before)
    fresh = _model(txm, x, u, w, ORDER, True)
    fresh.derivs_cross_cov()
    assert ("dcov", ORDER, False) not in fresh._cache
    assert np.array_equal(fresh.derivs_cov().values, before)


def test_against_device_bootstrap(txm):
    """N = 4000, two columns, order 2, 400 device-bootstrap replicates: |V - S| <= 5 se on every entry of the 6 x 6 matrix,
    the blocks between the columns included; se = std_r[(d - m)(d' - m')] / sqrt(R) from the replicates themselves.  (The
    seeds are fixed; the long-double restatement alone passes the same comparison, which is asserted first.)"""
    R, order = 400, 2
    x, u, _ = make_data(4000, seed=7, weighted=False, ncol=2)
    m = _model(txm, x, u, None, order, True)
    V = np.transpose(m.derivs_cross_cov().values, (2, 0, 3, 1)).reshape(6, 6)            # [(c, i), (c', j)]
    d = m.resample({"nrep": R, "seed": 1, "device": True}).derivs().transpose("rep", "val", "order").values.reshape(R, 6)
    dev = d - d.mean(axis=0)
    prod = dev[:, :, None] * dev[:, None, :]
    Sm = prod.sum(axis=0) / (R - 1)
    se = prod.std(axis=0, ddof=1) / math.sqrt(R)
    ld = np.asarray(_api_reference(x, u, None, order, True, False)[0], float).reshape(6, 6)
    assert (np.abs(ld - Sm) <= 5.0 * se).all()
    ratio = np.abs(V - Sm) / se
    print("device bootstrap: worst |V - S| / se =", float(ratio.max()), " over the cross blocks:", float(ratio[:3, 3:].max()))
    assert (ratio <= 5.0).all()


def test_unsupported_kinds_raise(txm):
    """Every model kind derivs_cov refuses (test_derivs_cov_gpu.py::test_unsupported_kinds_raise) is refused here too."""
    DA = txm.DataArray
    x, u, w = make_data(120, seed=8, ncol=2)
    xv, uv = DA(x, ("rec", "val")), DA(u, ("rec",))
    B = txm.beta.factory_extrapmodel
    models = {}
    xd = DA(np.stack([x, 0.1 * x, 0.01 * x], axis=1), ("rec", "deriv", "val"))
    models["xalpha"] = B(BETA0, txm.DataCentralMomentsVals.from_vals(xv=xd, uv=uv, order=2, central=True, deriv_dim="deriv"),
                         xalpha=True)
    models["x_is_u"] = B(BETA0, txm.DataCentralMomentsVals.from_vals(xv=None, uv=uv, order=2, central=True, x_is_u=True),
                         name="u_ave")
    models["reduced"] = B(BETA0, txm.DataCentralMoments.from_vals(xv=xv, uv=uv, order=2, central=True, dim="rec"))
    for central in (False, True):
        models[f"values{central}"] = B(BETA0, txm.factory_data_values(order=2, uv=uv, xv=xv, central=central))
    vals = txm.DataCentralMomentsVals.from_vals(xv=xv, uv=uv, order=2, central=True)
    models["resampled"] = B(BETA0, vals).resample({"nrep": 4, "seed": 0})
    models["volume"] = txm.volume.factory_extrapmodel(volume=5.0, uv=uv, xv=xv, dxdqv=xv, ndim=1)

    class Meta(txm.DataCallback):
        pass

    models["callback"] = B(BETA0, vals.new_like(meta=Meta()))
    funcs = [lambda *a: a[0], lambda *a: -a[2][1], lambda *a: a[2][2]]
    models["callables"] = txm.ExtrapModel(alpha0=BETA0, data=vals, derivatives=txm.Derivatives(funcs), order=2)
    for name, m in models.items():
        with pytest.raises(NotImplementedError) as e1:
            m.derivs_cross_cov()
        with pytest.raises(NotImplementedError):
            m.predict_cov(0.6)
        with pytest.raises(NotImplementedError) as e0:
            m.derivs_cov()
        assert str(e1.value) == str(e0.value), name                                      # the same message


def test_more_than_255_columns_raise(txm):
    x, u, _ = make_data(40, seed=1, weighted=False, ncol=256)
    m = _model(txm, x, u, None, 1, True)
    with pytest.raises(ValueError, match="255"):
        m.derivs_cross_cov()
    with pytest.raises(ValueError, match="255"):
        m.predict_cov(0.6)
    assert m.derivs_cov().shape == (2, 2, 256)                                           # the per-column path has no such limit
