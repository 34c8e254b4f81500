"""txm_perturb_cov (txm_perturb_cov.hip) and ``engine.perturb_cov`` against the long-double reference
tests/_perturb_cov_ref.py, on every kernel variant the launcher can select.

Tolerance, in the header's words.  With ``kappa_n = 1 + |da (u_n - uref)|`` (the exponent's rounding is the weight's
relative error) and the caller's ``mean``, which the reference uses too:

    var      |hip - ref| <= 1e-12 * sum_j (sum_{n in j} p_n kappa_n |x_n - m|)^2
    var_lnq  |hip - ref| <= 1e-12 * sum_j (sum_{n in j} p_n kappa_n + n_j / N)^2
    neff     |hip - ref| <= 1e-12 * kbar * neff,          kbar = sum_n p_n kappa_n
    lnq      |hip - ref| <= 1e-12 * kbar * (1 + |lnq|)

Through ``engine.perturb_cov`` the mean is txm_perturb's, the reference's is its own: ``d var / d m = -2 sum_j z_j P_j``
and ``|dm| <= 1e-12 S`` (test_perturb_gpu.py's bound, S from tail_oracle.perturb), so ``2 * 1e-12 * S * sum_j |z_j| P_j``
is added to the ``var`` bound.  The 1e-12 is the project's written tolerance; it is not fitted to the figures below.

Worst ratio ``|hip - ref| / bound`` observed on an MI355X (every test prints its own; run with ``-s``), as
(var, var_lnq, neff, lnq):
    dispatch (all 144 iid variants) 1.3e-15 1.8e-15 1.7e-15 7.8e-17; share-path boundaries 5.5e-16 5.7e-16 4.0e-16 6.9e-17;
    sizes (N to 2e5) 3.4e-16 2.2e-15 2.2e-15 0, blocked 7.6e-16 4.4e-16 2.0e-15 0; blocked path (B = 1 ... N + 1, every level)
    4.1e-16 7.9e-16 2.0e-15 0; far outlier 4.1e-16 6.4e-16 4.7e-16 7.6e-17; constant u / da = 0 2.1e-16 1.8e-39 0 0; weights beyond
    the underflow 0 9.4e-17 0 0; through the engine 7.4e-16 1.3e-15 1.0e-15 8.2e-17; the iid var against txm_influence_cov fed the
    materialised weights 1.2e-16 of the sum of the two bounds.  (profiles/r22_perturb_cov_gpu_tests.txt is the printed record.)

The cases follow ``pb_plan`` / ``pc_block_plan``: the test restates the plan in Python (``plan_of``) and asserts from it
which kernel variant a case reaches and that the workspace covers it.
"""

import ctypes as ct

import numpy as np
import pytest
import torch

from tests import _perturb_cov_ref as pcr
from oracle import tail_oracle as tl

pytestmark = pytest.mark.gpu

TOL = 1e-12
PB_BLOCK = 256
DA8 = np.array([0.3, -0.2, 1.1, -1.7, 0.01, 2.0, -0.6, 0.9])     # |da| * range(u) <= ~90 on the data of make_data
TXM_ERR_INVALID, TXM_ERR_WORKSPACE = -1, -3
WORST = {}


@pytest.fixture(scope="module")
def eng(txm):
    from thermoextrap_amd import engine

    return engine


@pytest.fixture(scope="module")
def lib(txm):
    from thermoextrap_amd import _lib

    return _lib.load()


def dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def cdiv(a, b):
    return -(-a // b)


def align_up(a, b):
    return cdiv(a, b) * b


def pitch_of(x2):
    N, C = x2.shape
    assert x2.stride(1) == 1
    return max(x2.stride(0), C) if N > 1 else C


def plan_of(x2, ldx, n_alpha, block=1, n_levels=1):
    """pb_plan / pc_block_plan and the workspace layout of txm_perturb_cov, restated."""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    N, C = x2.shape
    vec = 2 if (C % 2 == 0 and ldx % 2 == 0 and x2.data_ptr() % 16 == 0) else 1
    lanes = cdiv(C, vec)
    l2 = 0
    while (1 << l2) < lanes and l2 < 8:
        l2 += 1
    lpr = 1 << l2
    cpc = lpr * vec
    chunks = cdiv(C, cpc)
    gmm = max(1, min(cdiv(N, PB_BLOCK * 8), ncu * 8))
    head = 256 + align_up(gmm * 16, 256)
    p = {"vec": vec, "l2": l2, "chunks": chunks, "cols_pad": chunks * cpc, "iid": block == 1 and n_levels == 1,
         "share": lpr >= n_alpha and lpr <= 64 and n_alpha > 1 and min(lpr, cdiv(C, vec)) >= n_alpha}
    if p["iid"]:
        p["gx"] = max(1, min(cdiv(N, (PB_BLOCK >> l2) * 4), ncu * 8))
        p["need"] = head + p["gx"] * p["cols_pad"] * n_alpha * 8 + p["gx"] * n_alpha * 16
    else:
        rows = PB_BLOCK >> l2
        p["nb"] = cdiv(N, block)
        p["Bs"], p["G"] = (block, rows // block) if block < rows else (rows, 1)
        p["gx"] = min(cdiv(p["nb"], p["G"]), ncu * 8)
        p["need"] = head + align_up(8 * p["nb"] * n_alpha * (C + 1), 256) + 16 * p["nb"] * n_alpha
    return p


class Out:
    def __init__(self, n_levels, na, C):
        nan = float("nan")
        self.var = torch.full((n_levels, na, C), nan, dtype=torch.float64, device="cuda")
        self.neff = torch.full((na,), nan, dtype=torch.float64, device="cuda")
        self.lnq = torch.full((na,), nan, dtype=torch.float64, device="cuda")
        self.var_lnq = torch.full((n_levels, na), nan, dtype=torch.float64, device="cuda")

    def tensors(self):
        return self.var, self.neff, self.lnq, self.var_lnq

    def equal(self, other):
        return all(torch.equal(a, b) for a, b in zip(self.tensors(), other.tensors()))


def abi_call(eng, lib, x2, ldx, ud, da, mean_d, block, n_levels, ws_bytes):
    """txm_perturb_cov through the C ABI with a workspace of exactly ``ws_bytes`` bytes: (status, Out)."""
    N, C = x2.shape
    da = np.ascontiguousarray(da, dtype=np.float64)
    out = Out(n_levels, len(da), C)
    ws = torch.empty(max(int(ws_bytes), 1), dtype=torch.uint8, device="cuda")
    rc = lib.txm_perturb_cov(eng._ptr(x2), ldx, eng._ptr(ud), N, C, da.ctypes.data_as(ct.POINTER(ct.c_double)), len(da),
                             eng._ptr(mean_d), block, n_levels, eng._ptr(out.var), eng._ptr(out.neff), eng._ptr(out.lnq),
                             eng._ptr(out.var_lnq), eng._ptr(ws), int(ws_bytes), eng._stream())
    torch.cuda.synchronize()
    return rc, out


def np_mean(x, u, da):
    """A caller's mean in plain float64 (the kernel and the reference centre on whatever they are given)."""
    x2 = x.reshape(x.shape[0], -1)
    out = np.empty((len(da), x2.shape[1]))
    for a, d in enumerate(da):
        w = np.exp(-d * (u - (u.min() if d >= 0 else u.max())))
        out[a] = (w @ x2) / w.sum()
    return out


def _ratio(got, ref, bound):
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.all(np.isfinite(ref)) and np.all(bound >= 0)
    if not np.all(np.isfinite(got)):
        return np.inf
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    return float(r.max())


def ratios(var, neff, lnq, var_lnq, ref, sl=slice(None), engine_mean=False):
    """The four worst ratios of one result against the reference's alphas ``sl``."""
    vb = ref.var_bound[:, sl]
    if engine_mean:
        vb = vb + 2.0 * ref.S[None, sl] * ref.zP[:, sl]
    return (_ratio(var, ref.var[:, sl], vb), _ratio(var_lnq, ref.var_lnq[:, sl], ref.var_lnq_bound[:, sl]),
            _ratio(neff, ref.neff[sl], ref.kbar[sl] * ref.neff[sl]),
            _ratio(lnq, ref.lnq[sl], ref.kbar[sl] * (1.0 + np.abs(ref.lnq[sl]))))


def record(what, detail, r):
    key = what.split(":")[0]
    WORST[key] = tuple(max(a, b) for a, b in zip(WORST.get(key, (0.0,) * 4), r))
    print(f"perturb_cov {what} {detail}: ratios var={r[0]:.2e} var_lnq={r[1]:.2e} neff={r[2]:.2e} lnq={r[3]:.2e}")


def run_abi(eng, lib, xd, ud, da, ref, mean, what, sl=slice(None), block=1, n_levels=1, contract=True, coverage=None):
    """One call through the ABI with the caller's ``mean`` (na, C) the reference ``ref`` was computed with: the workspace
    covers the restated plan, exactly ws_bytes succeeds, the four outputs are within tolerance and finite; with
    ``contract`` a second call gives the same bits and one byte less is refused."""
    da = np.atleast_1d(np.asarray(da, dtype=np.float64))
    x2 = xd.unsqueeze(1) if xd.dim() == 1 else xd
    ldx = pitch_of(x2)
    N, C = x2.shape
    p = plan_of(x2, ldx, len(da), block, n_levels)
    have = lib.txm_perturb_cov_ws_bytes(N, C, len(da), block, n_levels)
    assert have >= p["need"], f"{what}: workspace {have} < plan {p['need']} ({p})"
    if coverage is not None:
        coverage.add((p["vec"], p["l2"], p["chunks"] > 1, len(da), p["share"]))
    mean_d = dev(mean)
    rc, out = abi_call(eng, lib, x2, ldx, ud, da, mean_d, block, n_levels, have)
    assert rc == 0, f"{what}: status {rc} with exactly txm_perturb_cov_ws_bytes"
    got = [t.cpu().numpy() for t in out.tensors()]
    assert all(np.all(np.isfinite(g)) for g in got), f"{what}: non-finite output"
    r = ratios(got[0], got[1], got[2], got[3], ref, sl)
    record(what, f"N={N} C={C} na={len(da)} B={block} L={n_levels} plan={p}", r)
    assert max(r) <= TOL, f"{what}: ratios {r}"
    if contract:
        rc, again = abi_call(eng, lib, x2, ldx, ud, da, mean_d, block, n_levels, have)
        assert rc == 0 and out.equal(again), f"{what}: two calls on the same inputs differ"
        rc, _ = abi_call(eng, lib, x2, ldx, ud, da, mean_d, block, n_levels, have - 1)
        assert rc == TXM_ERR_WORKSPACE, f"{what}: status {rc} one byte below txm_perturb_cov_ws_bytes"
    return out, p


# ---------------------------------------------------------------------------
# every (VEC, LPR_LOG2) pair, both chunk counts, n_alpha 1..8, share path on and off
# ---------------------------------------------------------------------------
# aligned even C: VEC 2 with 1, 2, ... 256 lanes and two chunks (514); odd C: VEC 1 with 1, 4, 8, ... 256 lanes and two
# chunks (257); C = 2 with an odd pitch and C = 4 one column into a wider tensor (misaligned x): VEC 1 with 2 and 4 lanes
CS = [(2, "aligned"), (4, "aligned"), (8, "aligned"), (16, "aligned"), (32, "aligned"), (64, "aligned"), (128, "aligned"),
      (256, "aligned"), (512, "aligned"), (514, "aligned"), (1, "aligned"), (2, "odd pitch"), (4, "misaligned"),
      (3, "aligned"), (5, "aligned"), (9, "aligned"), (17, "aligned"), (33, "aligned"), (65, "aligned"), (129, "aligned"),
      (257, "aligned")]


def place(x, layout):
    N, C = x.shape
    if layout == "aligned":
        return dev(x)
    wide = np.full((N, C + (3 if layout == "odd pitch" else 2)), 1e300)   # what lies beyond the columns must not be read
    off = 0 if layout == "odd pitch" else 1
    wide[:, off:off + C] = x
    return dev(wide)[:, off:off + C]


def test_every_variant_of_the_iid_dispatch(eng, lib):
    cov = set()
    N = 1537
    for C, layout in CS:
        rng = np.random.default_rng(2000 + C)
        x, u = pcr.make_data(rng, N, C)
        mean = np_mean(x, u, DA8)
        ref = pcr.perturb_cov(x, u, DA8, mean=mean)
        xd, ud = place(x, layout), dev(u)
        for na in range(1, 9):
            _, p = run_abi(eng, lib, xd, ud, DA8[:na], ref, mean[:na], f"dispatch: {layout}", sl=slice(0, na),
                           contract=(na in (1, 8)), coverage=cov)
            assert p["iid"] and p["vec"] == (2 if (layout == "aligned" and C % 2 == 0) else 1), p
    for na in range(1, 9):
        pairs = {(v, l) for (v, l, _, n, _) in cov if n == na}
        assert pairs == {(v, l) for v in (1, 2) for l in range(9)}, (na, sorted(pairs))
        assert {(v, m) for (v, _, m, n, _) in cov if n == na} == {(1, False), (1, True), (2, False), (2, True)}, na
        if na > 1:
            assert {s for (_, _, _, n, s) in cov if n == na} == {False, True}, na


def test_share_path_boundaries(eng, lib):
    """Both sides of LPR >= NA, nvalid >= NA and LPR <= 64 (the lanes 0..NA-1 of a row evaluate one alpha each), iid and
    blocked."""
    rng = np.random.default_rng(77)
    N = 1537
    x, u = pcr.make_data(rng, N, 130)
    ud = dev(u)
    cases = [  # (columns, layout, n_alpha, vec, LPR, share)
        (5, "aligned", 5, 1, 8, True), (5, "aligned", 6, 1, 8, False),            # nvalid 5 of 8 lanes
        (10, "aligned", 5, 2, 8, True), (10, "aligned", 6, 2, 8, False),          # VEC 2: 5 valid lanes of 8
        (10, "misaligned", 6, 1, 16, True),                                       # 10 lanes of 16
        (8, "aligned", 8, 2, 4, False), (7, "aligned", 8, 1, 8, False),           # LPR < NA, nvalid < NA
        (15, "aligned", 8, 1, 16, True), (128, "aligned", 8, 2, 64, True), (130, "aligned", 8, 2, 128, False),
        (64, "aligned", 2, 2, 32, True), (63, "aligned", 7, 1, 64, True),
    ]
    for C, layout, na, vec, lpr, share in cases:
        cols = x[:, :C]
        mean = np_mean(cols, u, DA8[:na])
        for block, n_levels in ((1, 1), (7, 3)):
            ref = pcr.perturb_cov(cols, u, DA8[:na], mean=mean, block=block, n_levels=n_levels)
            _, p = run_abi(eng, lib, place(cols, layout), ud, DA8[:na], ref, mean, f"share: C={C} NA={na}", block=block,
                           n_levels=n_levels, contract=False)
            assert (p["vec"], 1 << p["l2"], p["share"]) == (vec, lpr, share), p


@pytest.mark.parametrize("N", [1, 255, 1025, 4099, 200_000])
@pytest.mark.parametrize("C", [1, 32])
def test_sizes(eng, lib, N, C):
    """Several row blocks per column, iid and blocked (B = 256 with every level up to the single block and one more)."""
    rng = np.random.default_rng(N + C)
    x, u = pcr.make_data(rng, N, C)
    da = DA8[[0, 3, 5]]
    mean = np_mean(x, u, da)
    xd, ud = dev(x), dev(u)
    ref = pcr.perturb_cov(x, u, da, mean=mean)
    _, p = run_abi(eng, lib, xd, ud, da, ref, mean, "sizes")
    assert p["gx"] > 1 or N < 4099
    nb = cdiv(N, 256)
    n_levels = max(1, int(np.ceil(np.log2(nb)))) + 2
    ref = pcr.perturb_cov(x, u, da, mean=mean, block=256, n_levels=n_levels)
    _, p = run_abi(eng, lib, xd, ud, da, ref, mean, "sizes blocked", block=256, n_levels=n_levels)
    assert not p["iid"] and p["nb"] == nb


# ---------------------------------------------------------------------------
# the blocked path
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("C,layout,na", [(5, "aligned", 3), (32, "aligned", 8), (6, "odd pitch", 2)])
def test_blocked_path(eng, lib, C, layout, na):
    """B in {1 with levels, 2, 7, 256, 1000, N, N + 1}: blocks packed several to a workgroup step (B < ROWS), one per
    step, a short last block (4099 = 7 * 585 + 4 = 256 * 16 + 3 = 1000 * 4 + 99), every level up to the single block and
    one beyond, a single block from the start."""
    N = 4099
    rng = np.random.default_rng(300 + C)
    x, u = pcr.make_data(rng, N, C)
    da = DA8[:na]
    mean = np_mean(x, u, da)
    xd, ud = place(x, layout), dev(u)
    level0 = {}
    for B in (1, 2, 7, 256, 1000, N, N + 1):
        nb = cdiv(N, B)
        n_levels = min(32, (int(np.ceil(np.log2(nb))) if nb > 1 else 0) + 2)
        ref = pcr.perturb_cov(x, u, da, mean=mean, block=B, n_levels=n_levels)
        out, p = run_abi(eng, lib, xd, ud, da, ref, mean, f"blocked: B={B}", block=B, n_levels=n_levels)
        assert not p["iid"] and p["nb"] == nb and p["Bs"] * p["G"] <= PB_BLOCK >> p["l2"]
        level0[B] = out
        if B == 7:
            assert p["G"] == (PB_BLOCK >> p["l2"]) // 7 or p["G"] == 1
    # B = 1 with levels: level 0 is the iid estimator (another kernel, another order of the same sums)
    ref = pcr.perturb_cov(x, u, da, mean=mean)
    iid, _ = run_abi(eng, lib, xd, ud, da, ref, mean, "blocked: iid twin", contract=False)
    r = ratios(level0[1].var[:1].cpu().numpy(), level0[1].neff.cpu().numpy(), level0[1].lnq.cpu().numpy(),
               level0[1].var_lnq[:1].cpu().numpy(), ref)
    assert max(r) <= TOL, r
    del iid
    # 32 levels: every level beyond the single block repeats it
    ref32 = pcr.perturb_cov(x, u, da, mean=mean, block=1000, n_levels=32)
    out, _ = run_abi(eng, lib, xd, ud, da, ref32, mean, "blocked: 32 levels", block=1000, n_levels=32, contract=False)
    assert torch.equal(out.var[3], out.var[31]) and torch.equal(out.var_lnq[3], out.var_lnq[31])
    # n_eff and lnq do not depend on the blocking beyond rounding
    for B, o in level0.items():
        np.testing.assert_allclose(o.neff.cpu().numpy(), ref.neff, rtol=1e-12 * ref.kbar.max())


def test_blocked_two_column_chunks(eng, lib):
    """C = 514 (VEC 2) and 257 (VEC 1): a row slot per workgroup, the block summed by one thread per column."""
    N = 300
    for C in (514, 257):
        rng = np.random.default_rng(C)
        x, u = pcr.make_data(rng, N, C)
        da = DA8[[0, 3]]
        mean = np_mean(x, u, da)
        ref = pcr.perturb_cov(x, u, da, mean=mean, block=16, n_levels=4)
        _, p = run_abi(eng, lib, dev(x), dev(u), da, ref, mean, "blocked: chunks", block=16, n_levels=4)
        assert p["chunks"] == 2 and p["Bs"] == 1 and p["G"] == 1


# ---------------------------------------------------------------------------
# values
# ---------------------------------------------------------------------------
def test_weights_underflow_beyond_745(eng, lib):
    """|da| * range(u) far beyond 745: all weights but the extreme sample's underflow -- neff = 1, var = 0 about that
    sample's row, var_lnq = (1 - 1/N)^2 + (N - 1) / N^2, everything finite."""
    N, C = 4099, 5
    rng = np.random.default_rng(N)
    x, u = pcr.make_data(rng, N, C)
    klo, khi = 2 * PB_BLOCK + 5, 2 * PB_BLOCK + 250
    u[klo] = u.min() - 10.0
    u[khi] = u.max() + 10.0
    da = np.array([100.0, -100.0, 80.0, -80.0])
    mean = x[[klo, khi, klo, khi]].copy()
    for block, n_levels in ((1, 1), (256, 3)):
        ref = pcr.perturb_cov(x, u, da, mean=mean, block=block, n_levels=n_levels)
        out, _ = run_abi(eng, lib, dev(x), dev(u), da, ref, mean, "underflow", block=block, n_levels=n_levels)
        assert np.array_equal(out.neff.cpu().numpy(), np.ones(4))
        assert np.array_equal(out.var.cpu().numpy(), np.zeros((n_levels, 4, C)))
        np.testing.assert_allclose(out.lnq.cpu().numpy(), -np.log(N) - da * u[[klo, khi, klo, khi]], rtol=1e-14)


@pytest.mark.parametrize("where", ["first", "last"])
def test_far_outlier(eng, lib, where):
    """One sample 300 / |da| beyond the rest, at the first and at the last row."""
    N, C = 4099, 5
    rng = np.random.default_rng(10)
    x, u = pcr.make_data(rng, N, C)
    k = 0 if where == "first" else N - 1
    for sign in (1.0, -1.0):
        uu = u.copy()
        uu[k] = u.min() - 300.0 if sign > 0 else u.max() + 300.0
        da = np.array([sign, -sign, 0.5 * sign])
        mean = np_mean(x, uu, da)
        for block, n_levels in ((1, 1), (7, 4)):
            ref = pcr.perturb_cov(x, uu, da, mean=mean, block=block, n_levels=n_levels)
            out, _ = run_abi(eng, lib, dev(x), dev(uu), da, ref, mean, "outlier", block=block, n_levels=n_levels)
            assert out.neff[0].item() == 1.0                        # every other weight is e^-300 or less


def test_constant_u_and_zero_dalpha(eng, lib):
    rng = np.random.default_rng(9)
    N, C = 5000, 7
    x, u = pcr.make_data(rng, N, C)
    plain = ((x - x.mean(axis=0)) ** 2).sum(axis=0) / N**2
    for uu, da in ((np.full(N, 174.85), DA8), (u, np.array([0.0, -0.0, 0.0]))):
        mean = np.broadcast_to(x.mean(axis=0), (len(da), C)).copy()
        for block, n_levels in ((1, 1), (100, 2)):
            ref = pcr.perturb_cov(x, uu, da, mean=mean, block=block, n_levels=n_levels)
            out, _ = run_abi(eng, lib, dev(x), dev(uu), da, ref, mean, "constant u / da = 0", block=block, n_levels=n_levels)
            assert np.array_equal(out.neff.cpu().numpy(), np.full(len(da), float(N)))
            np.testing.assert_allclose(out.lnq.cpu().numpy(), -da * uu[0] if uu[0] == uu[1] else 0.0, rtol=1e-14, atol=0)
            assert np.all(out.var_lnq.cpu().numpy() <= 1e-15 / N)
            if block == 1:
                np.testing.assert_allclose(out.var[0].cpu().numpy(), np.broadcast_to(plain, (len(da), C)), rtol=1e-13)


def test_refusals(eng, lib):
    x = torch.ones((10, 3), dtype=torch.float64, device="cuda")
    u = torch.ones(10, dtype=torch.float64, device="cuda")
    mean = torch.ones((2, 3), dtype=torch.float64, device="cuda")
    out = Out(1, 2, 3)
    ws = torch.empty(1 << 22, dtype=torch.uint8, device="cuda")
    da = (ct.c_double * 8)(*([0.1] * 8))
    P = eng._ptr

    def call(x_=P(x), ldx=3, u_=P(u), N=10, C=3, dap=da, na=2, mean_=P(mean), block=1, levels=1, var=P(out.var),
             neff=P(out.neff), lnq=P(out.lnq), vq=P(out.var_lnq), ws_=P(ws), wsb=ws.numel()):
        return lib.txm_perturb_cov(x_, ldx, u_, N, C, dap, na, mean_, block, levels, var, neff, lnq, vq, ws_, wsb, eng._stream())

    for name in ("x_", "u_", "dap", "mean_", "var", "neff", "lnq", "vq", "ws_"):
        assert call(**{name: None}) == TXM_ERR_INVALID, name
    for kw in ({"N": 0}, {"C": 0}, {"C": 65536, "ldx": 65536}, {"ldx": 2}, {"na": 0}, {"na": 9}, {"block": 0}, {"levels": 0},
               {"levels": 33}):
        assert call(**kw) == TXM_ERR_INVALID, kw
    assert call(wsb=lib.txm_perturb_cov_ws_bytes(10, 3, 2, 1, 1) - 1) == TXM_ERR_WORKSPACE
    assert call(block=2, levels=2, wsb=lib.txm_perturb_cov_ws_bytes(10, 3, 2, 2, 2) - 1) == TXM_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert torch.isnan(out.var).all() and torch.isnan(out.neff).all()      # nothing was enqueued
    # nothing above left the library in a bad state: constant u, x = 1 -> var 0, neff N
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.var.cpu().numpy(), np.zeros((1, 2, 3))) and np.array_equal(out.neff.cpu().numpy(), [10.0, 10.0])
    with pytest.raises(ValueError):
        eng.perturb_cov(x, u, [0.1], block=0)
    with pytest.raises(ValueError):
        eng.perturb_cov(x, u, [0.1], n_levels=33)
    with pytest.raises(ValueError):
        eng.perturb_cov(x, u[:9], [0.1])
    with pytest.raises(TypeError):
        eng.perturb_cov(x.float(), u, [0.1])


# ---------------------------------------------------------------------------
# differential: the parent's route to the iid variance
# ---------------------------------------------------------------------------
def test_iid_var_against_influence_cov_with_materialised_weights(eng, lib):
    """``txm_influence_cov`` (n_f = n_q = 1, a = 0, b = 1, centre = the mean) fed ``w = e^{-da (u - uref)}`` computes the
    same sum.  Its own bound is ``1e-12 * sum p^2 (x - m)^2`` (B = |dx|); the weights it is given differ from the
    kernel's by their exponent's rounding, which var_bound's kappa covers: the sum of the two bounds."""
    N, C = 20000, 32
    rng = np.random.default_rng(4)
    x, u = pcr.make_data(rng, N, C)
    da = DA8[[0, 3, 5]]
    mean = np_mean(x, u, da)
    ref = pcr.perturb_cov(x, u, da, mean=mean)
    xd, ud = dev(x), dev(u)
    out, _ = run_abi(eng, lib, xd, ud, da, ref, mean, "differential", contract=False)
    a = torch.zeros((C, 1, 1), dtype=torch.float64, device="cuda")
    b = torch.ones((C, 1, 1), dtype=torch.float64, device="cuda")
    for i, d in enumerate(da):
        w = torch.exp(-d * (ud - (ud.min() if d >= 0 else ud.max())))
        cov, _ = eng.influence_cov(xd, ud, a, b, 0.0, dev(mean[i]), w=w)
        diff = np.abs(cov[:, 0, 0].cpu().numpy() - out.var[0, i].cpu().numpy())
        r = float((diff / (ref.var_bound[0, i] + ref.var[0, i])).max())
        print(f"perturb_cov differential: da={d} |cov - influence_cov| / (sum of bounds) = {r:.2e}")
        assert r <= TOL


# ---------------------------------------------------------------------------
# engine.perturb_cov: txm_perturb's mean, more than eight alphas, 1-D x
# ---------------------------------------------------------------------------
def check_engine(eng, x, u, da, xd, ud, what, block=1, n_levels=1):
    ref = pcr.perturb_cov(x, u, da, block=block, n_levels=n_levels)
    avg, S = tl.perturb(x, u, da)
    np.testing.assert_allclose(S.reshape(ref.S.shape), ref.S, rtol=1e-15)
    del avg
    res = eng.perturb_cov(xd, ud, da, block=block, n_levels=n_levels)
    assert torch.equal(res.mean, eng.perturb(xd, ud, da)), f"{what}: mean is not engine.perturb's"
    sq = x.ndim == 1
    var = res.var.cpu().numpy()
    assert var.shape == ((n_levels, len(da)) if sq else (n_levels, len(da), x.shape[1])) and res.mean.shape == var.shape[1:]
    assert res.neff.shape == res.lnq.shape == (len(da),) and res.var_lnq.shape == (n_levels, len(da))
    r = ratios(var.reshape(ref.var.shape), res.neff.cpu().numpy(), res.lnq.cpu().numpy(), res.var_lnq.cpu().numpy(), ref,
               engine_mean=True)
    record(what, f"N={x.shape[0]} na={len(da)} B={block} L={n_levels}", r)
    assert max(r) <= TOL, r
    return res


@pytest.mark.parametrize("n_alpha", [3, 9, 17])
@pytest.mark.parametrize("C", [5, 32])
def test_engine_slices_more_than_eight_alphas(eng, n_alpha, C):
    rng = np.random.default_rng(n_alpha)
    x, u = pcr.make_data(rng, 3001, C)
    da = rng.uniform(-2.0, 2.0, n_alpha)
    check_engine(eng, x, u, da, dev(x), dev(u), "engine")
    check_engine(eng, x, u, da, dev(x), dev(u), "engine blocked", block=100, n_levels=3)


def test_engine_layouts(eng):
    rng = np.random.default_rng(5)
    N, C = 3001, 10
    x, u = pcr.make_data(rng, N, C)
    ud = dev(u)
    r1 = check_engine(eng, x[:, 0], u, DA8[:3], dev(x[:, 0]), ud, "engine: 1-D x")
    assert r1.var.shape == (1, 3)
    xt = dev(x.T.copy())
    r2 = check_engine(eng, x, u, DA8[:3], xt.t(), ud, "engine: x.t()")            # copied to row-major
    r3 = check_engine(eng, x, u, DA8[:3], place(x, "odd pitch"), ud, "engine: odd pitch", block=7, n_levels=2)
    del r2, r3
    r4 = check_engine(eng, x[:1], u[:1], DA8, dev(x[:1]), dev(u[:1]), "engine: N = 1")
    assert torch.equal(r4.var, torch.zeros_like(r4.var)) and torch.equal(r4.neff, torch.ones_like(r4.neff))


def test_print_worst():
    for k, v in sorted(WORST.items()):
        print(f"perturb_cov worst {k}: var={v[0]:.1e} var_lnq={v[1]:.1e} neff={v[2]:.1e} lnq={v[3]:.1e}")
