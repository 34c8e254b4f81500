"""The estimator behind ``PerturbModel.predict_with_error`` / ``free_energy`` / ``blocking_curve`` checked on the host:
the long-double reference of txm_perturb_cov (tests/_perturb_cov_ref.py) against what it claims to estimate, and the
parts of the C ABI that need no device.

* iid: the delta-method std of the reweighted mean and of ``lnq`` against a numpy multinomial bootstrap (2000
  replicates; the ratio of two such stds has relative standard error 1 / sqrt(2 * 1999), the bound is 5 of them).
* batch means on AR(1) series (phi = 0.9, statistical inefficiency g = 19): the mean blocked variance over 300
  realisations against the empirical variance of the 300 estimates.  The blocked form is biased by about -g / (2 B)
  = -19 / 512 at B = 256 and the empirical variance of 300 estimates has relative standard error sqrt(2 / 299); the iid
  form must be far too small (about 1 / g).
* identities: ``var_lnq = 1 / neff - 1 / N`` at block 1, ``da = 0`` is the plain ``sum (x - xbar)^2 / N^2`` with
  ``neff = N``, level l of a curve equals level 0 at ``B * 2**l``.

Figures observed: bootstrap ratios 0.977-1.021 (columns) and 1.025 (lnq) at n_eff = 1671; AR(1) blocked 0.951 and
iid 0.074, lnq 0.941 and 0.057.
"""

import ctypes as ct

import numpy as np
import pytest

from tests import _perturb_cov_ref as pcr

TXM_ERR_INVALID, TXM_ERR_WORKSPACE = -1, -3


@pytest.fixture(scope="module")
def lib():
    from thermoextrap_amd import _build, _lib

    _build.build_library()
    return _lib.load()


def test_reference_against_numpy_bootstrap():
    N, C, da, nrep = 20000, 3, 0.3, 2000
    rng = np.random.default_rng(2024)
    x, u = pcr.make_data(rng, N, C)
    ref = pcr.perturb_cov(x, u, [da])
    std_delta = np.sqrt(ref.var[0, 0])
    w = np.exp(-da * (u - u.min()))
    est = np.empty((nrep, C))
    lnq = np.empty(nrep)
    for r0 in range(0, nrep, 100):
        f = rng.multinomial(N, np.full(N, 1.0 / N), size=100).astype(np.float64)
        den = f @ w
        est[r0:r0 + 100] = (f @ (w[:, None] * x)) / den[:, None]
        lnq[r0:r0 + 100] = np.log(den / N) - da * u.min()
    tol = 5.0 / np.sqrt(2.0 * (nrep - 1))
    ratio = est.std(axis=0, ddof=1) / std_delta
    ratio_q = lnq.std(ddof=1) / np.sqrt(ref.var_lnq[0, 0])
    print(f"bootstrap / delta: columns {ratio}, lnq {ratio_q:.4f}, n_eff {ref.neff[0]:.0f}, tol {tol:.4f}")
    assert 1000 < ref.neff[0] < N
    assert np.all(np.abs(ratio - 1.0) <= tol), ratio
    assert abs(ratio_q - 1.0) <= tol, ratio_q
    # the bootstrap scatters about the same mean and lnq
    assert np.all(np.abs(est.mean(axis=0) - ref.mean[0]) <= 5 * std_delta / np.sqrt(nrep) + 0.05 * std_delta)
    assert abs(lnq.mean() - ref.lnq[0]) <= 0.2 * np.sqrt(ref.var_lnq[0, 0])


def test_batch_means_on_ar1():
    N, B, da, nreal = 20000, 256, 0.3, 300
    rng = np.random.default_rng(7)
    x, u = pcr.ar1_data(rng, N, nreal)
    est, lnq = np.empty(nreal), np.empty(nreal)
    vb, vi, qb, qi = (np.empty(nreal) for _ in range(4))
    for r in range(nreal):
        ref = pcr.perturb_cov(x[r], u[r], [da], block=1, n_levels=9)        # level 8: blocks of 256
        est[r], lnq[r] = ref.mean[0, 0], ref.lnq[0]
        vi[r], vb[r] = ref.var[0, 0, 0], ref.var[8, 0, 0]
        qi[r], qb[r] = ref.var_lnq[0, 0], ref.var_lnq[8, 0]
    lo, hi = 1.0 - 19.0 / 512.0 - 5.0 * np.sqrt(2.0 / (nreal - 1)), 1.0 + 5.0 * np.sqrt(2.0 / (nreal - 1))
    rb, ri = vb.mean() / est.var(ddof=1), vi.mean() / est.var(ddof=1)
    sb, si = qb.mean() / lnq.var(ddof=1), qi.mean() / lnq.var(ddof=1)
    print(f"AR(1) blocked / empirical {rb:.3f} (iid {ri:.3f}); lnq {sb:.3f} (iid {si:.3f}); bounds [{lo:.3f}, {hi:.3f}]")
    assert lo <= rb <= hi and ri < 0.2
    assert lo <= sb <= hi and si < 0.2
    # level 8 of a curve from block 1 is level 0 at block 256
    ref = pcr.perturb_cov(x[0], u[0], [da], block=B, n_levels=1)
    assert ref.var[0, 0, 0] == vb[0] and ref.var_lnq[0, 0] == qb[0]


def test_identities():
    rng = np.random.default_rng(3)
    N, C = 4099, 3
    x, u = pcr.make_data(rng, N, C)
    da = [0.3, -0.2, 0.0, 1.1]
    ref = pcr.perturb_cov(x, u, da)
    # block 1: var_lnq = 1 / neff - 1 / N (a difference of two numbers of size 1 / neff: 1e-15 of that)
    np.testing.assert_allclose(ref.var_lnq[0], 1.0 / ref.neff - 1.0 / N, rtol=0, atol=4e-16 / ref.neff.min())
    # da = 0: the plain variance of the mean and neff = N
    plain = ((x - x.mean(axis=0)) ** 2).sum(axis=0) / N**2
    np.testing.assert_allclose(ref.var[0, 2], plain, rtol=1e-13)
    assert ref.neff[2] == N and abs(ref.lnq[2]) < 1e-18 and ref.var_lnq[0, 2] < 1e-30
    np.testing.assert_allclose(ref.mean[2], x.mean(axis=0), rtol=1e-14)
    # level l of a curve equals level 0 at B 2^l, a short last block included (4099 = 7 * 585 + 4)
    curve = pcr.perturb_cov(x, u, da, block=7, n_levels=11)
    for l in (0, 1, 3, 9, 10):
        one = pcr.perturb_cov(x, u, da, block=7 << l, n_levels=1)
        assert np.array_equal(one.var[0], curve.var[l]) and np.array_equal(one.var_lnq[0], curve.var_lnq[l]), l
    # a single block: z = sum p (x - m) = 0 and sum p - 1 = 0, to rounding
    assert np.all(curve.var[10] <= 1e-30 * curve.var[0]) and np.all(curve.var_lnq[10] <= 1e-30)
    # the bounds bound: kappa >= 1
    assert np.all(ref.var_bound >= ref.var) and np.all(ref.kbar >= 1.0)
    # a caller's mean: var about m' is var + 2 (m - m') sum z P + (m - m')^2 sum P^2 -- checked at first order
    shifted = ref.mean + 1e-9 * ref.S
    ref2 = pcr.perturb_cov(x, u, da, mean=shifted)
    assert np.all(np.abs(ref2.var - ref.var)[0] <= 2 * 1e-9 * ref.S * ref.zP[0] + (1e-9 * ref.S) ** 2 / ref.neff[:, None] * 1.001)


def test_workspace_query_is_host_logic(lib):
    W = lib.txm_perturb_cov_ws_bytes
    head = lambda N: 256 + -(-min(max(1, -(-N // 2048)), 2048) * 16 // 256) * 256  # noqa: E731  (256 CUs before txm_init)
    # iid: independent of N beyond the pre-pass head, grows with the padded columns and with n_alpha
    assert W(1000, 32, 8, 1, 1) > 0
    assert W(10**8, 32, 8, 1, 1) - head(10**8) == W(1000, 32, 8, 1, 1) - head(1000)
    assert W(1000, 32, 8, 1, 1) < W(1000, 33, 8, 1, 1) == W(1000, 64, 8, 1, 1) < W(1000, 514, 8, 1, 1)
    assert W(1000, 32, 4, 1, 1) < W(1000, 32, 8, 1, 1)
    # blocked: the documented 8 nb n_alpha (C + 1) term (+ 16 nb n_alpha for the weight sums), nb = ceil(N / block)
    for N, C, na, B in ((100_000, 32, 8, 1024), (100_001, 5, 3, 7), (50, 1, 1, 100), (4099, 514, 2, 1)):
        nb = -(-N // B)
        body = W(N, C, na, B, 3) - head(N) - 256
        assert 8 * nb * na * (C + 1) + 16 * nb * na <= body < 8 * nb * na * (C + 1) + 16 * nb * na + 256, (N, C, na, B)
        assert W(N, C, na, B, 3) == W(N, C, na, B, 32) == (W(N, C, na, B, 1) if B > 1 else W(N, C, na, B, 2))
    # block 1 with levels is the blocked path: nb = N
    assert W(4099, 3, 2, 1, 2) > 8 * 4099 * 2 * 4 > W(4099, 3, 2, 1, 1) - head(4099)
    # bad arguments: 0
    for args in ((0, 3, 1, 1, 1), (10, 0, 1, 1, 1), (10, 65536, 1, 1, 1), (10, 3, 0, 1, 1), (10, 3, 9, 1, 1), (10, 3, 1, 0, 1),
                 (10, 3, 1, 1, 0), (10, 3, 1, 1, 33), (-5, 3, 1, 1, 1), (10, 3, 1, -1, 1)):
        assert W(*args) == 0, args
    assert W(10, 65535, 8, 1, 1) > 0 and W(10, 3, 8, 2**40, 32) > 0


def test_refusals_need_no_device(lib):
    """Every refusal of txm_perturb_cov happens before anything is enqueued: it runs on a machine without a GPU.  The
    pointers are never dereferenced."""
    da = (ct.c_double * 8)(*([0.1] * 8))
    p = ct.c_void_p(4096)
    big = 1 << 30

    def call(x=p, ldx=3, u=p, N=10, C=3, dap=da, na=2, mean=p, block=1, levels=1, var=p, neff=p, lnq=p, vq=p, ws=p, wsb=big):
        return lib.txm_perturb_cov(x, ldx, u, N, C, dap, na, mean, block, levels, var, neff, lnq, vq, ws, wsb, None)

    for name in ("x", "u", "dap", "mean", "var", "neff", "lnq", "vq", "ws"):
        assert call(**{name: None}) == TXM_ERR_INVALID, name
        assert b"null" in lib.txm_last_error()
    for kw in ({"N": 0}, {"N": -1}, {"C": 0}, {"C": 65536, "ldx": 65536}, {"ldx": 2}, {"na": 0}, {"na": 9}, {"block": 0},
               {"block": -3}, {"levels": 0}, {"levels": 33}):
        assert call(**kw) == TXM_ERR_INVALID, kw
    for block, levels in ((1, 1), (1, 2), (4, 3), (100, 1)):
        need = lib.txm_perturb_cov_ws_bytes(10, 3, 2, block, levels)
        assert need > 0
        assert call(block=block, levels=levels, wsb=need - 1) == TXM_ERR_WORKSPACE
        assert b"workspace" in lib.txm_last_error()
        assert call(block=block, levels=levels, wsb=0) == TXM_ERR_WORKSPACE
