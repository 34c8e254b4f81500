"""``engine.perturb`` (txm_perturb.hip) against the long-double reference oracle/tail_oracle.perturb, at the shapes the
dispatch code distinguishes.

Tolerance.  ``|hip - ref| <= 1e-12 * S`` with ``S[a, c] = sum f w |x| / sum f w`` the natural scale of the output, and
every output finite.  1e-12 scale-relative is the project's moment tolerance (``RTOL`` of test_kernels_gpu.py, README
"Tolerances"); here it is also a bound: a weight's relative error is at most ``(|arg| + c) eps`` with |arg| < 745
before it underflows (<= 1.7e-13), and the summation adds ``eps * (terms per thread + tree depth)``.  The plain
float64 numpy restatement of the formula stays within 7.5e-14 * S of the oracle for N up to 1e6 and
``|da| * range(u)`` up to ~100, so the inputs below cannot fail on the reference's account.

Worst ratio ``|hip - ref| / S`` observed on an MI355X (every test prints its own; run with ``-s``):
    dispatch cross product 1.3e-15, share-path boundaries 1.2e-15, layouts 4.5e-16, grid sizes (N to 2e6) 9.2e-16,
    replicates 1.5e-15, replicate without the extreme sample (da * gap 50 / 600 / 800) 1.1e-15, far outlier 5.3e-16,
    da = 0 against the plain mean 2.2e-16, constant u 2.1e-16, weights beyond the underflow 0 (the extreme row itself).
    The 1e-12 is the project's written tolerance; it is not fitted to these figures.

The cases follow ``pb_plan`` / ``perturb_kernel``: the test restates the plan in Python (``plan_of``), asserts from it
which kernel variant a case reaches, and checks the workspace contract against it.  The ``da * gap = 800`` replicate
(a bootstrap row that does not hold the extreme sample) returned NaN while the kernel subtracted the global extreme
of ``u``: the extremes are now taken per replicate over the samples of positive count, and the case is a plain
assertion.
"""

import ctypes as ct

import numpy as np
import pytest
import torch

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


def dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def make_data(rng, N, C):
    """Ideal-gas-scale u (mean 33 sigma from zero) and columns of different offset and slope."""
    u = rng.normal(174.85, 5.31, N)
    x = rng.normal(0.0, 1.0, C)[None, :] + rng.normal(1e-3, 5e-4, C)[None, :] * u[:, None] + rng.normal(0, 0.05, (N, C))
    return x, u


def cdiv(a, b):
    return -(-a // b)


def align_up(a, b):
    return cdiv(a, b) * b


def operand(x):
    """The (N, C) tensor and row pitch engine.perturb hands to the library (it copies what is not row-major)."""
    x2 = x.unsqueeze(1) if x.dim() == 1 else x
    if x2.stride(1) != 1 or (x2.shape[0] > 1 and x2.stride(0) < x2.shape[1]):
        x2 = x2.contiguous()
    N, C = x2.shape
    return x2, (max(x2.stride(0), C) if N > 1 else C)


def plan_of(x2, ldx, nrep, n_alpha):
    """pb_plan, the pre-pass grid and the workspace layout of txm_perturb, restated."""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    N, C = x2.shape
    vec = 2 if (C % 2 == 0 and ldx % 2 == 0 and x2.data_ptr() % 16 == 0) else 1
    lanes = cdiv(C, vec)
    l2 = 0
    while (1 << l2) < lanes and l2 < 8:
        l2 += 1
    cpc = (1 << l2) * vec
    chunks = cdiv(C, cpc)
    gx = max(1, min(cdiv(N, (PB_BLOCK >> l2) * 4), max(1, ncu * 8 // min(nrep, 8))))
    gmm = max(1, min(cdiv(N, PB_BLOCK * 8), ncu * 8 // nrep))
    head = align_up(nrep * 16, 256) + align_up(nrep * gmm * 16, 256)
    lpr = 1 << l2
    nvalid_last = cdiv(C - (chunks - 1) * cpc, vec)
    return {"vec": vec, "l2": l2, "chunks": chunks, "cols_pad": chunks * cpc, "gx": gx, "gmm": gmm,
            "need": head + nrep * gx * chunks * cpc * n_alpha * 16,
            # block-uniform exp sharing (first chunk; with chunks > 1 LPR is 256 and nothing is shared)
            "share": lpr >= n_alpha and lpr <= 64 and n_alpha > 1 and min(lpr, cdiv(C, vec)) >= n_alpha,
            "nvalid_last": nvalid_last}


def abi_perturb(eng, x2, ldx, u, da, freq, ws_bytes):
    """txm_perturb through the C ABI with a workspace of exactly ``ws_bytes`` bytes: (status, out)."""
    from thermoextrap_amd import _lib

    L = _lib.load()
    N, C = x2.shape
    nrep = 1 if freq is None else freq.shape[0]
    da = np.ascontiguousarray(da, dtype=np.float64)
    out = torch.full((nrep, len(da), C), float("nan"), dtype=torch.float64, device="cuda")
    ws = torch.empty(max(int(ws_bytes), 1), dtype=torch.uint8, device="cuda")
    rc = L.txm_perturb(eng._ptr(x2), ldx, eng._ptr(u), N, C, da.ctypes.data_as(ct.POINTER(ct.c_double)), len(da),
                       eng._ptr(freq), nrep, eng._ptr(out), eng._ptr(ws), int(ws_bytes), eng._stream())
    torch.cuda.synchronize()
    return rc, out


def ratio(got, ref, S):
    got = np.asarray(got)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.all(np.isfinite(ref)) and np.all(S >= 0)
    if not np.all(np.isfinite(got)):
        return np.inf
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(S > 0, err / S, np.where(err == 0, 0.0, np.inf))
    return float(r.max())


def run_case(eng, xd, ud, da, ref, S, what, freq=None, coverage=None, abi=True, tol=TOL):
    """One shape through engine.perturb: workspace contract, bit-identical second call through the ABI, tolerance.
    ``ref``, ``S``: the oracle's (n_alpha, C) / (nrep, n_alpha, C) for the columns and alphas passed."""
    from thermoextrap_amd import _lib

    L = _lib.load()
    da = np.atleast_1d(np.asarray(da, dtype=np.float64))
    x2, ldx = operand(xd)
    N, C = x2.shape
    nrep = 1 if freq is None else freq.shape[0]
    plans = []
    for a0 in range(0, len(da), 8):                        # the engine's 8-wide slices
        na = len(da[a0:a0 + 8])
        p = plan_of(x2, ldx, nrep, na)
        have = L.txm_perturb_ws_bytes(N, C, na, nrep)
        assert have >= p["need"], f"{what}: workspace {have} < plan {p['need']} ({p})"
        plans.append((p, na, have))
        if coverage is not None:
            coverage.add((p["vec"], p["l2"], p["chunks"] > 1, na))
    got = eng.perturb(xd, ud, da, freq=freq)
    gn = got.cpu().numpy()
    r = ratio(gn.reshape(ref.shape), ref, S)
    WORST[what.split(":")[0]] = max(WORST.get(what.split(":")[0], 0.0), r)
    print(f"perturb {what}: N={N} C={C} n_alpha={len(da)} nrep={nrep} plan={plans[0][0]} ratio={r:.3e}")
    assert np.all(np.isfinite(gn)), f"{what}: non-finite output"
    assert r <= tol, f"{what}: |hip - ref| / S = {r:.3e}"
    if abi:                                                # (bounds were checked against the plan above)
        p, na, have = plans[0]
        rc, out = abi_perturb(eng, x2, ldx, ud.contiguous(), da[:8], freq, have)
        assert rc == 0, f"{what}: status {rc} with exactly txm_perturb_ws_bytes"
        first = got.reshape(nrep, len(da), C)[:, :na]
        assert torch.equal(out, first), f"{what}: two calls on the same inputs differ"
        rc, _ = abi_perturb(eng, x2, ldx, ud.contiguous(), da[:8], freq, have - 1)
        assert rc == TXM_ERR_WORKSPACE, f"{what}: status {rc} one byte below txm_perturb_ws_bytes"
    return gn, plans[0][0]


# ---------------------------------------------------------------------------
# every (VEC, LPR_LOG2) pair, both chunk counts, n_alpha 1..8 (+ the engine's 8-wide slicing)
# ---------------------------------------------------------------------------
CS = [1, 2, 3, 4, 5, 7, 8, 10, 16, 17, 31, 32, 33, 64, 100, 127, 128, 129, 255, 256, 257, 300, 512, 514, 600, 1026]


def test_every_variant_of_the_dispatch(eng):
    """C x n_alpha at N ~ 3000.  An even C runs twice: as an aligned tensor (VEC 2) and as columns 1..C of a wider one
    (odd base offset -> VEC 1), which is what reaches VEC 1 with 2, 4 and 9..16 lanes.  The restated plan must show all
    18 (VEC, LPR_LOG2) pairs and both chunk counts for every n_alpha in 1..8."""
    cov = set()
    N = 3001
    for C in CS:
        rng = np.random.default_rng(1000 + C)
        x, u = make_data(rng, N, C)
        ref, S = tl.perturb(x, u, DA8)
        ud = dev(u)
        layouts = [("aligned", dev(x))]
        if C % 2 == 0:
            wide = np.zeros((N, C + 2))
            wide[:, 1:C + 1] = x
            layouts.append(("offset", dev(wide)[:, 1:C + 1]))
        for name, xd in layouts:
            for na in range(1, 9):
                _, p = run_case(eng, xd, ud, DA8[:na], ref[:na], S[:na], f"dispatch: {name}", coverage=cov, abi=(na in (1, 5, 8)))
                assert p["vec"] == (2 if (name == "aligned" and C % 2 == 0) else 1)
    for na in range(1, 9):
        pairs = {(v, l) for (v, l, _, n) in cov if n == na}
        assert pairs == {(v, l) for v in (1, 2) for l in range(9)}, (na, sorted(pairs))
        assert {m for (_, _, m, n) in cov if n == na} == {False, True}, na
        assert {(v, m) for (v, _, m, n) in cov if n == na} == {(1, False), (1, True), (2, False), (2, True)}, na


@pytest.mark.parametrize("n_alpha", [9, 16, 17])
@pytest.mark.parametrize("C", [5, 32])
def test_more_than_eight_alphas_are_sliced(eng, n_alpha, C):
    rng = np.random.default_rng(n_alpha)
    x, u = make_data(rng, 3001, C)
    da = rng.uniform(-2.0, 2.0, n_alpha)
    ref, S = tl.perturb(x, u, da)
    run_case(eng, dev(x), dev(u), da, ref, S, "slicing")


# ---------------------------------------------------------------------------
# share path boundaries
# ---------------------------------------------------------------------------
def test_share_path_boundaries(eng):
    """Both sides of LPR >= NA, nvalid >= NA and LPR <= 64 (the lanes 0..NA-1 of a row evaluate one alpha each)."""
    rng = np.random.default_rng(77)
    N = 3001
    x, u = make_data(rng, N, 130)
    ud = dev(u)
    wide = np.zeros((N, 12))
    wide[:, 1:11] = x[:, :10]
    cases = [  # (tensor, columns, n_alpha, vec, LPR, share)
        (dev(x[:, :5]), x[:, :5], 5, 1, 8, True), (dev(x[:, :5]), x[:, :5], 6, 1, 8, False),        # nvalid 5 of 8 lanes
        (dev(x[:, :10]), x[:, :10], 5, 2, 8, True), (dev(x[:, :10]), x[:, :10], 6, 2, 8, False),    # VEC 2: 5 valid lanes of 8
        (dev(wide)[:, 1:11], x[:, :10], 5, 1, 16, True), (dev(wide)[:, 1:11], x[:, :10], 6, 1, 16, True),  # 10 lanes of 16
        (dev(x[:, :8]), x[:, :8], 8, 2, 4, False), (dev(x[:, :7]), x[:, :7], 8, 1, 8, False),       # LPR < NA, nvalid < NA
        (dev(x[:, :15]), x[:, :15], 8, 1, 16, True),
        (dev(x[:, :128]), x[:, :128], 8, 2, 64, True), (dev(x), x, 8, 2, 128, False),               # LPR 64 -> 128
        (dev(x[:, :64]), x[:, :64], 2, 2, 32, True), (dev(x[:, :63]), x[:, :63], 7, 1, 64, True),
    ]
    for xd, cols, na, vec, lpr, share in cases:
        ref, S = tl.perturb(cols, u, DA8[:na])
        _, p = run_case(eng, xd, ud, DA8[:na], ref, S, f"share: C={cols.shape[1]} NA={na}")
        assert (p["vec"], 1 << p["l2"], p["share"]) == (vec, lpr, share), p


# ---------------------------------------------------------------------------
# layout
# ---------------------------------------------------------------------------
def test_layouts(eng):
    rng = np.random.default_rng(5)
    N, C = 3001, 10
    x, u = make_data(rng, N, C)
    ud = dev(u)
    ref, S = tl.perturb(x, u, DA8[:3])
    wide = np.full((N, C + 4), 1e300)                       # what lies beyond the columns must not be read into a sum
    wide[:, :C] = x
    _, p = run_case(eng, dev(wide)[:, :C], ud, DA8[:3], ref, S, "layout: pitch > C")
    assert p["vec"] == 2
    wide = np.full((N, C + 3), 1e300)
    wide[:, :C] = x
    _, p = run_case(eng, dev(wide)[:, :C], ud, DA8[:3], ref, S, "layout: odd pitch, even C")
    assert p["vec"] == 1
    # 1-D x
    g, _ = run_case(eng, dev(x[:, 0]), ud, DA8[:3], ref[:, 0], S[:, 0], "layout: 1-D x")
    assert g.shape == (3,)
    # a transposed view: the engine copies it
    xt = dev(x.T.copy())
    assert not xt.t().is_contiguous()
    run_case(eng, xt.t(), ud, DA8[:3], ref, S, "layout: x.t()")
    # N = 1 and N = 2 (also as rows of a pitched tensor)
    for n in (1, 2):
        r, s = tl.perturb(x[:n], u[:n], DA8)
        run_case(eng, dev(x[:n]), dev(u[:n]), DA8, r, s, f"layout: N = {n}")
        run_case(eng, dev(wide)[:n, :C], dev(u[:n]), DA8, r, s, f"layout: N = {n} pitched")
        r, s = tl.perturb(x[:n, 0], u[:n], DA8)
        run_case(eng, dev(x[:n, 0]), dev(u[:n]), DA8, r, s, f"layout: N = {n} 1-D")


# ---------------------------------------------------------------------------
# grid: several row blocks per column (gx > 1), the partial layout, the pre-pass block cap
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N", [255, 1025, 4099, 200_000, 2_000_000])
@pytest.mark.parametrize("C", [1, 32])
def test_grid_sizes(eng, N, C):
    rng = np.random.default_rng(N + C)
    x, u = make_data(rng, N, C)
    da = DA8[[0, 3, 5]] if N <= 200_000 else DA8[[0, 3]] * 0.5
    ref, S = tl.perturb(x, u, da)
    _, p = run_case(eng, dev(x), dev(u), da, ref, S, "grid")
    if N >= 4099:
        assert p["gx"] > 1
    # the same rows with a column count that pads (cols_pad > C) so the partial stride differs from C
    if C == 32 and N <= 200_000:
        ref, S = tl.perturb(x[:, :27], u, da)
        _, p = run_case(eng, dev(x[:, :27]), dev(u), da, ref, S, "grid: C = 27")
        assert p["cols_pad"] == 32 and (p["gx"] > 1 or N < 1025)


def test_minmax_prepass_at_its_block_cap(eng):
    """N = 5e6: the extremes pre-pass would want 2442 blocks and is capped at 8 per CU; the extremes sit in the last
    block's stride and nowhere else matters for da * gap beyond the float64 range of exp."""
    N = 5_000_000
    rng = np.random.default_rng(50)
    x, u = make_data(rng, N, 1)
    ref, S = tl.perturb(x, u, [0.4, -0.4])
    _, p = run_case(eng, dev(x), dev(u), [0.4, -0.4], ref, S, "minmax cap")
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    assert p["gmm"] == ncu * 8 < cdiv(N, 2048)
    # put the two extremes into the last pre-pass block (thread 3 / 200 of block gmm - 1, second sweep)
    last = (p["gmm"] - 1) * PB_BLOCK + p["gmm"] * PB_BLOCK
    u[last + 3] = u.min() - 500.0
    u[last + 200] = u.max() + 500.0
    ref, S = tl.perturb(x, u, [2.0, -2.0])
    g, _ = run_case(eng, dev(x), dev(u), [2.0, -2.0], ref, S, "minmax cap: extremes in the last block")
    np.testing.assert_allclose(g[:, 0], [x[last + 3, 0], x[last + 200, 0]], rtol=1e-12)


# ---------------------------------------------------------------------------
# replicates
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nrep", [1, 3, 8, 9, 40])
@pytest.mark.parametrize("C", [1, 27, 32])
def test_replicates(eng, orc, nrep, C):
    """freq rows from DeviceSampler.freq() (about 37 % zeros), a row with its first half zeroed, a row of all ones
    (which must give the freq=None answer).  N = 50_000 at C = 32 wants 782 row blocks: above the cap for nrep >= 3,
    which changes at nrep > 8."""
    N = 50_000 if C > 1 else 300_000
    rng = np.random.default_rng(nrep * 100 + C)
    x, u = make_data(rng, N, C)
    xd, ud = dev(x), dev(u)
    s = eng.DeviceSampler(900 + nrep, nrep, N)
    fd = s.freq().clone()
    if nrep >= 3:
        fd[1, : N // 2] = 0
        fd[2] = 1
    freq = fd.cpu().numpy()
    da = DA8[[0, 3, 5]]
    ref, S = tl.perturb(x, u, da, freq)
    g, p = run_case(eng, xd, ud, da, ref, S, f"replicates: C={C}", freq=fd)
    assert g.shape == (nrep, 3, C) and p["gx"] > 1
    if nrep >= 3:
        plain = eng.perturb(xd, ud, da).cpu().numpy()
        r0, s0 = tl.perturb(x, u, da)
        assert ratio(plain, r0, s0) <= TOL and ratio(g[2], r0, s0) <= TOL
        assert ratio(g[2], plain, s0) <= TOL


# ---------------------------------------------------------------------------
# exponents
# ---------------------------------------------------------------------------
def test_zero_dalpha_is_the_plain_mean(eng):
    rng = np.random.default_rng(8)
    for N, C in ((3001, 5), (100_000, 32), (7, 1)):
        x, u = make_data(rng, N, C)
        mean = np.asarray(x, dtype=np.longdouble).mean(axis=0).astype(np.float64)
        S = np.abs(x).mean(axis=0)
        for da in ([0.0], [-0.0], [0.0, -0.0, 0.0]):
            g = eng.perturb(dev(x), dev(u), da).cpu().numpy()
            for row in g:
                r = ratio(row, mean, S)
                print(f"perturb da = 0: N={N} C={C} ratio={r:.3e}")
                assert r <= 1e-13
            ref, S2 = tl.perturb(x, u, da)
            run_case(eng, dev(x), dev(u), da, ref, S2, "da = 0")


def test_constant_u(eng):
    rng = np.random.default_rng(9)
    x, _ = make_data(rng, 5000, 7)
    u = np.full(5000, 174.85)
    ref, S = tl.perturb(x, u, DA8)
    g, _ = run_case(eng, dev(x), dev(u), DA8, ref, S, "constant u")
    assert ratio(g, np.broadcast_to(x.mean(0), g.shape), np.broadcast_to(np.abs(x).mean(0), g.shape)) <= 1e-13


@pytest.mark.parametrize("where", ["first", "last prepass block", "end"])
def test_far_outlier(eng, where):
    """One sample 300 / |da| beyond the rest: every other weight is e^-300 for the da of its sign; for the other sign
    the reference point is the opposite extreme and the outlier's own weight is e^-(300 + ...)."""
    N, C = 4099, 5
    rng = np.random.default_rng(10)
    x, u = make_data(rng, N, C)
    k = {"first": 0, "last prepass block": 2 * PB_BLOCK + 17, "end": N - 1}[where]   # cdiv(4099, 2048) = 3 blocks
    for sign in (1.0, -1.0):
        uu = u.copy()
        uu[k] = u.min() - 300.0 if sign > 0 else u.max() + 300.0
        da = [sign, -sign, 0.5 * sign]
        ref, S = tl.perturb(x, uu, da)
        g, _ = run_case(eng, dev(x), dev(uu), da, ref, S, "outlier")
        np.testing.assert_allclose(g[0], x[k], rtol=1e-12)


@pytest.mark.parametrize("N,C", [(4099, 5), (300_000, 2)])
def test_weights_underflow_beyond_745(eng, N, C):
    """|da| * range(u) far beyond 745: all weights but the extreme sample's underflow; the answer is that sample's row.
    The two extremes stand 1000 / |da| clear of the rest and sit in the last block of the extremes pre-pass."""
    rng = np.random.default_rng(N)
    x, u = make_data(rng, N, C)
    gmm = cdiv(N, 2048)
    klo, khi = (gmm - 1) * PB_BLOCK + 5, (gmm - 1) * PB_BLOCK + 250
    u[klo] = u.min() - 10.0
    u[khi] = u.max() + 10.0
    da = [100.0, -100.0, 30.0, -30.0]
    ref, S = tl.perturb(x, u, da)
    g, p = run_case(eng, dev(x), dev(u), da, ref, S, "underflow")
    assert p["gmm"] == gmm > 1
    np.testing.assert_allclose(g, x[[klo, khi, klo, khi]], rtol=1e-12)
    np.testing.assert_allclose(ref, x[[klo, khi, klo, khi]], rtol=1e-12)


# ---------------------------------------------------------------------------
# a replicate that does not hold the extreme sample
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dag", [50, 600, 800])
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_replicate_without_the_extreme_sample(eng, dag, sign):
    """The extreme of u lies ``dag / |da|`` beyond the rest and replicate 0 has count 0 there.  The reference
    renormalises per replicate and is finite at 50, 600 and 800.  Subtracting the GLOBAL extreme leaves replicate 0
    with weights <= e^-dag: at 800 they all underflow and the average was 0/0 = NaN (observed before the extremes were
    taken per replicate over the samples of positive count); at 600 they are denormal-free but tiny, which is fine."""
    N, C = 3001, 5
    rng = np.random.default_rng(dag)
    x, u = make_data(rng, N, C)
    k = int(np.argmin(u) if sign > 0 else np.argmax(u))
    u[k] = (u.min() - dag) if sign > 0 else (u.max() + dag)
    fd = eng.DeviceSampler(4242 + dag, 3, N).freq().clone()
    fd[0, k] = 0
    fd[1, k] = 2
    fd[2] = 1
    fd[2, k] = 0
    freq = fd.cpu().numpy()
    da = [sign, 0.25 * sign, -sign]
    ref, S = tl.perturb(x, u, da, freq)
    assert np.all(np.isfinite(ref))
    run_case(eng, dev(x), dev(u), da, ref, S, f"no extreme: da*g = {dag}", freq=fd)


# ---------------------------------------------------------------------------
# argument errors
# ---------------------------------------------------------------------------
def test_argument_errors(eng):
    from thermoextrap_amd import TxmError

    x = torch.ones((10, 3), dtype=torch.float64, device="cuda")
    u = torch.ones(10, dtype=torch.float64, device="cuda")
    for na in (0, 9):                                       # at the ABI: the engine never passes these
        rc, _ = abi_perturb(eng, x, 3, u, np.zeros(na), None, 1 << 24)
        assert rc == TXM_ERR_INVALID, (na, rc)
    from thermoextrap_amd import _lib

    assert _lib.load().txm_perturb_ws_bytes(10, 3, 0, 1) == 0 and _lib.load().txm_perturb_ws_bytes(10, 3, 9, 1) == 0
    with pytest.raises(ValueError):
        eng.perturb(x, u, [0.1], freq=torch.ones((2, 9), dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        eng.perturb(x, u[:9], [0.1])
    with pytest.raises(TxmError):
        eng.perturb(x[:4], u[:4], [0.1], freq=torch.ones((65536, 4), dtype=torch.int64, device="cuda"))
    with pytest.raises(TypeError):
        eng.perturb(x.float(), u, [0.1])
    # nothing above left the library in a bad state
    g = eng.perturb(x, u, [0.1]).cpu().numpy()
    assert np.array_equal(g, np.ones((1, 3)))
