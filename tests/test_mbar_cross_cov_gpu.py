"""GPU tests of MBAR's covariance across columns and targets: the kernel txm_mbar_cross_cov (txm_mbar_cross_cov.hip)
through the C ABI against long-double sums, its workspace behaviour (it declares no size query: it runs in the workspace of
the txm_mbar_cov call it follows and plans its launch from the bytes it is given), MBARModel.predict_with_covariance against
the dense restatement of tests/test_mbar_cov_cpu.py, a check that needs no reference, and one statistical test against
MBARModel.bootstrap.

Kernel parity.  logD (txm_mbar_eval), mean (txm_mbar_predict) and lnw (txm_mbar_cov) are read back from the device calls
and taken as given: the reference forms W_na = e^{-a ut_n - logD_n - lnw_a} and the sums in long double from those float64
values.  Every entry is held to

    |hip - ref| <= 1e-12 sum_n kappa'_n |term_n|,      kappa'_n = kappa_n + max_a |lnw_a| / 64,

kappa_n = 1 + max(|g_k| + |alpha0_k ut_n|, |a ut_n| + |logD_n|) / 64 from oracle.mbar_oracle.kappa: group E's rule
(tests/test_mbar_kernels_gpu.py) with one more term.  There a weight's exponent -a ut_n - logD_n - M_a carries an absolute
error of eps (|a ut_n| (rounding of u - upiv) + |a ut_n| + |logD_n| (the fma)) plus the last subtraction's, whose operand M_a
is itself one of the sample exponents; 128 eps kappa_n covers it.  Here the subtrahend is lnw_a, which no sample bounds: the
last subtraction rounds a number of size at most |a ut_n| + |logD_n| + |lnw_a|, an absolute error of the exponent -- a
relative error of the weight -- of eps |lnw_a| more.  Adding |lnw_a| / 64 to kappa_n adds 2 eps |lnw_a| to 128 eps kappa_n,
twice that.  A term holds two weights, so its relative error is at most 256 eps kappa'_n = 5.7e-14 kappa'_n before the ulps
of exp, the products and the summation (terms per lane + the waves + the records): 1e-12 leaves 17x for those, as in
group E.  No floor for underflow is needed: no weight of these cases is below 1e-60.

What the cases reach: T = 1, 2, 3 and 16 column tiles (1, 3, 6 and 136 pairs), the NA templates 1, 2, 4 and 8 (n_alpha
1, 2, 3, 8), states of 1 sample, of less than a tile and of several sample workgroups with a ragged last tile, a row
pitch above C, u of order 4e4, one full tile (C = 16) and C = 255.  Each case prints its worst ratio (run with -s).
"""

import ctypes as ct

import numpy as np
import pytest
import torch

from _bands import Banded
from oracle.mbar_oracle import kappa
from test_mbar_cov_cpu import LD, bound, dense_theta, gauss_problem, gram_theta, ref_columns, ref_solve
from test_mbar_cov_gpu import CASES as COV_CASES
from test_mbar_cov_gpu import problem, spread_targets

pytestmark = pytest.mark.gpu
TOL = 1e-12
HEAD = 64 * 32 + 2 * 64 * 8 + 256

_BY_NAME = {c[0]: c for c in COV_CASES}
CASES = [_BY_NAME[n] for n in ("K1_C1_na1", "K2_C3_na8", "K3_C1_na3", "K8_C17_na8_large_u", "K12_C33_pitch40_na8")] + [
    # name, alpha0, samples per state, C, n_alpha, row pitch, mean of u
    ("K3_C16_na2", [1.0, 1.1, 1.2], [70, 1, 300], 16, 2, None, 50.0),
    ("K2_C255_na1", [1.0, 1.2], [25, 15], 255, 1, None, 50.0),
]
# (tiles a side, NA template) of the same-alpha call, and the targets of the cross call (n_alpha 2, 3 or 8)
EXPECT = {"K1_C1_na1": (1, 1, 2), "K2_C3_na8": (1, 8, 8), "K3_C1_na3": (1, 4, 3), "K8_C17_na8_large_u": (2, 8, 8),
          "K12_C33_pitch40_na8": (3, 8, 8), "K3_C16_na2": (1, 2, 2), "K2_C255_na1": (16, 1, 2)}


@pytest.fixture(scope="module")
def eng(txm):
    from thermoextrap_amd import engine

    return engine


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).cuda()


class Inputs:
    """One case on the device: the state table, logD of txm_mbar_eval at the CPU solve, mean of txm_mbar_predict, and out
    (yy among it) and lnw of txm_mbar_cov -- everything txm_mbar_cross_cov takes, and its long-double reference."""

    def __init__(self, eng, case, na):
        from thermoextrap_amd import _lib

        name, a0, ns, C, _, pitch, mu = case
        self.L = L = _lib.load()
        self.eng, self.K, self.C, self.na, self.ns = eng, len(a0), C, na, ns
        i = [c[0] for c in COV_CASES].index(name) if name in _BY_NAME else 50 + C
        us, xs = problem(a0, ns, C, seed=100 + i, mu=mu)
        f = np.asarray(ref_solve(us, a0), dtype=np.float64)
        self.ud = [dev(u) for u in us]
        if pitch is None:
            self.xd = [dev(x) for x in xs]
        else:
            self.xd = []
            for x in xs:
                wide = torch.full((len(x), pitch), float("nan"), dtype=torch.float64, device="cuda")
                wide[:, :C] = dev(x)
                self.xd.append(wide[:, :C])
        self.tab, self.keep, nsf, C2 = eng._mbar_table(self.ud, self.xd)
        assert C2 == C and all(self.tab[s].ldx_s == (pitch or C) for s in range(self.K) if ns[s] > 1)
        self.upiv = eng.mbar_pivot(self.ud)
        self.a0 = np.ascontiguousarray(a0, dtype=np.float64)
        g = np.log(nsf) + f - self.a0 * self.upiv
        self.g = np.ascontiguousarray(g - g.max())
        self.logD = torch.empty(int(nsf.sum()), dtype=torch.float64, device="cuda")
        eng.mbar_eval(self.ud, self.a0, self.g, self.upiv, self.logD)
        self.al = np.ascontiguousarray(spread_targets(a0, na), dtype=np.float64)
        self.mean = eng.mbar_predict(self.xd, self.ud, self.a0, f, self.logD, self.al, upiv=self.upiv).contiguous()
        self.nbytes = L.txm_mbar_cov_ws_bytes(self.K, C, na)
        assert self.nbytes > 0
        K = self.K
        out = torch.full((na, 1 + K + C * (1 + K)), float("nan"), dtype=torch.float64, device="cuda")
        self.lnw = torch.full((na,), float("nan"), dtype=torch.float64, device="cuda")
        self.ws = torch.empty(self.nbytes, dtype=torch.uint8, device="cuda")
        dp = ct.POINTER(ct.c_double)
        rc = L.txm_mbar_cov(self.tab, K, C, float(self.upiv), self.a0.ctypes.data_as(dp), self.g.ctypes.data_as(dp),
                            eng._ptr(self.logD), self.al.ctypes.data_as(dp), na, eng._ptr(self.mean), eng._ptr(out),
                            eng._ptr(self.lnw), eng._ptr(self.ws), self.nbytes, eng._stream())
        torch.cuda.synchronize()
        assert rc == 0, _lib.last_error()
        self.yy = out.cpu().numpy()[:, 1 + K:].reshape(na, C, 1 + K)[:, :, 0]
        # the long-double reference from the float64 values the kernel reads
        ut = np.concatenate([np.asarray(u, dtype=LD) for u in us]) - LD(self.upiv)
        ld, lw = self.logD.cpu().numpy().astype(LD), self.lnw.cpu().numpy().astype(LD)
        x = np.concatenate([np.asarray(v, dtype=LD) for v in xs])
        mean = self.mean.cpu().numpy().astype(LD)
        W = np.exp(-np.asarray(self.al, dtype=LD)[None, :] * ut[:, None] - ld[:, None] - lw[None, :])     # (N, na)
        assert float(W[W > 0].min()) > 1e-60 and abs(float(W.sum(0).max()) - 1.0) < 1e-9
        Y = (W[:, :, None] * (x[:, None, :] - mean[None, :, :])).reshape(len(ut), na * C)
        kap = (kappa(self.a0, self.g, ut, self.al, ld).astype(LD) + np.abs(lw).max() / 64)
        self.ref = Y.T @ Y                                                                               # (na C, na C)
        self.ref_bound = (np.abs(Y) * kap[:, None]).T @ np.abs(Y)

    def plan(self, cross, ws_bytes=None):
        p = (ct.c_int64 * 4)()
        rc = self.L.txm_mbar_cross_cov_plan(self.K, self.C, self.na, cross, max(self.ns), self.nbytes if ws_bytes is None else ws_bytes, p)
        return rc, list(p)

    def call(self, cross, out_ptr, ws_ptr, ws_bytes):
        dp = ct.POINTER(ct.c_double)
        rc = self.L.txm_mbar_cross_cov(self.tab, self.K, self.C, float(self.upiv), self.eng._ptr(self.logD),
                                       self.al.ctypes.data_as(dp), self.na, self.eng._ptr(self.mean), self.eng._ptr(self.lnw),
                                       cross, out_ptr, ws_ptr, ws_bytes, self.eng._stream())
        torch.cuda.synchronize()
        return rc

    def run(self, cross):
        """out of the call in txm_mbar_cov's own workspace, as the engine makes it."""
        from thermoextrap_amd import _lib

        M = self.na * self.C
        out = torch.full((M, M) if cross else (self.na, self.C, self.C), float("nan"), dtype=torch.float64, device="cuda")
        rc = self.call(cross, self.eng._ptr(out), self.eng._ptr(self.ws), self.nbytes)
        assert rc == 0, _lib.last_error()
        return out.cpu().numpy()

    def worst(self, got, cross):
        """max |hip - ref| / bound over the entries; every entry finite."""
        assert np.all(np.isfinite(got))
        na, C = self.na, self.C
        if cross:
            return float(np.max(np.abs(got.astype(LD) - self.ref) / self.ref_bound))
        w = 0.0
        for a in range(na):
            s = slice(a * C, (a + 1) * C)
            w = max(w, float(np.max(np.abs(got[a].astype(LD) - self.ref[s, s]) / self.ref_bound[s, s])))
        return w


_inputs = {}


def inputs(eng, case, na):
    key = (case[0], na)
    if key not in _inputs:
        _inputs[key] = Inputs(eng, case, na)
    return _inputs[key]


def expected_plan(inp, cross, ws_bytes, cus8):
    T = -(-inp.C // 16)
    pairs = T * (T + 1) // 2
    per_gx, rec = pairs * (inp.na if cross else 1), inp.na * 256 * 8
    gx = max(1, min((ws_bytes - HEAD) // rec // per_gx, -(-max(inp.ns) // 256), max(1, cus8 // per_gx)))
    return [T, pairs, gx, HEAD + gx * per_gx * rec]


@pytest.fixture(scope="module")
def cus8(txm):
    """Eight workgroups per CU, read from the plan of a shape where nothing else binds."""
    from thermoextrap_amd import _lib

    L = _lib.load()
    p = (ct.c_int64 * 4)()
    assert L.txm_mbar_cross_cov_plan(1, 1, 1, 0, 10**9, L.txm_mbar_cov_ws_bytes(1, 1, 1), p) == 0
    assert p[2] % 8 == 0 and p[2] >= 8
    return int(p[2])


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_kernel_against_long_double_sums(eng, cus8, case):
    name, a0, ns, C, na, pitch, mu = case
    T, NA, na_cross = EXPECT[name]
    assert {1: 1, 2: 2, 3: 4, 4: 4}.get(na, 8) == NA and -(-C // 16) == T
    same = inputs(eng, case, na)
    if mu > 1e3:                                                       # unshifted, e^{-alpha u} would overflow
        assert max(same.al) * min(float(u.min()) for u in same.ud) > 745.0 * 10
    rc, p = same.plan(0)
    assert rc == 0 and p == expected_plan(same, 0, same.nbytes, cus8) and p[2] == -(-max(ns) // 256), p
    got = same.run(0)
    assert all(np.array_equal(got[a], got[a].T) for a in range(na))
    w_same = same.worst(got, 0)
    assert w_same <= TOL, w_same
    # the diagonal is txm_mbar_cov's yy, each within its own bound (the same expression: sum_n kappa_n W^2 d^2)
    diag = np.stack([np.diag(got[a]) for a in range(na)])
    dbound = np.stack([np.diag(same.ref_bound)[a * C:(a + 1) * C] for a in range(na)]).astype(np.float64)
    assert np.all(np.abs(diag - same.yy) <= 2 * TOL * dbound)
    # the cross form
    cr = inputs(eng, case, na_cross)
    rc, q = cr.plan(1)
    assert rc == 0 and q == expected_plan(cr, 1, cr.nbytes, cus8), q
    full = cr.run(1)
    assert np.array_equal(full, full.T)
    w_cross = cr.worst(full, 1)
    assert w_cross <= TOL, w_cross
    # its diagonal blocks are the same-alpha result of the same targets bit for bit (both plans cut the samples alike)
    rc, p2 = cr.plan(0)
    assert rc == 0 and p2[2] == q[2]
    again = got if na_cross == na else cr.run(0)
    for a in range(na_cross):
        assert np.array_equal(full[a * C:(a + 1) * C, a * C:(a + 1) * C], again[a])
    print(f"\n{name}: T {T}, pairs {p[1]}, sample workgroups {p[2]}; worst |hip - ref| / sum kappa |term|: "
          f"same-alpha (n_alpha {na}) {w_same:.2e}, cross (n_alpha {na_cross}) {w_cross:.2e}")


@pytest.mark.parametrize("cross", [0, 1], ids=["same_alpha", "cross_alpha"])
def test_workspace_at_the_smallest_plan_and_at_the_full_query(eng, cus8, cross):
    """The K8 case in guard-banded buffers of exactly the plan's minimum (one sample workgroup) and of the full query: both
    within the bound, the 64 KiB bands intact, equal bits on two calls; one byte short refuses and leaves out painted."""
    from thermoextrap_amd import _lib

    inp = inputs(eng, _BY_NAME["K8_C17_na8_large_u"], 8)
    rc, refused = inp.plan(cross, 0)
    assert rc == -3
    least = refused[3]
    assert least == expected_plan(inp, cross, least, cus8)[3] and least < inp.nbytes
    shape = (8 * 17, 8 * 17) if cross else (8, 17, 17)
    results = []
    for nbytes, gx in ((least, 1), (inp.nbytes, 4)):
        rc, p = inp.plan(cross, nbytes)
        assert rc == 0 and p[2] == gx and p[3] <= nbytes, p
        bits = []
        for _ in range(2):
            ws = Banded(nbytes, "nan")
            out = Banded(int(np.prod(shape)) * 8, "value")
            rc = inp.call(cross, ct.c_void_p(out.ptr), ct.c_void_p(ws.ptr), nbytes)
            assert rc == 0, _lib.last_error()
            assert ws.check() and out.check() and out.unwritten() == 0
            bits.append(out.view().cpu().numpy().reshape(shape).copy())
        assert np.array_equal(bits[0], bits[1])
        w = inp.worst(bits[0], cross)
        print(f"\n{'cross' if cross else 'same-alpha'}, {nbytes} bytes, {gx} sample workgroup(s): worst ratio {w:.2e}")
        assert w <= TOL
        results.append(bits[0])
    assert np.array_equal(results[1], inp.run(cross))                   # the full query: what a plain buffer gives
    ws = Banded(least - 1, "nan")
    out = Banded(int(np.prod(shape)) * 8, "value")
    rc = inp.call(cross, ct.c_void_p(out.ptr), ct.c_void_p(ws.ptr), least - 1)
    assert rc == -3 and "workspace too small" in _lib.last_error()
    assert out.unwritten() == int(np.prod(shape)) and ws.holds_fill() and ws.check() and out.check()


# ---- the public method ----------------------------------------------------------------------------------------------------
def make_model(a0, us, xs):
    import thermoextrap_amd as xtrap

    return xtrap.MBARModel([xtrap.beta.factory_extrapmodel(beta=b, data=xtrap.factory_data_values(uv=u, xv=x, order=1, central=False))
                            for b, x, u in zip(a0, xs, us)])


def dense_check(model, a0, ns, us, xs, targets, cross):
    """predict_with_covariance against the dense Theta of [Ws, y_i, y_j] (entry [K, K + 1]; the diagonal from [Ws, y_i]),
    under bound(own, own of the entry) relative to sqrt(Theta_ii Theta_jj).  Returns (mean, cov, worst relative)."""
    K, C, na = len(a0), xs[0].shape[1], len(targets)
    f = ref_solve(us, a0)
    Ws, Wt, _ = ref_columns(us, a0, f, targets)
    Ns, x = np.array(ns, dtype=np.float64), np.concatenate(xs).astype(LD)
    own = float(np.abs(gram_theta(Ws, Ns) - dense_theta(Ws, Ns)).max() / max(np.abs(dense_theta(Ws, Ns)).max(), 1e-300)) if K > 1 else 0.0
    mu = np.einsum("na,nc->ac", Wt, x)
    Y = (Wt[:, :, None] * (x[:, None, :] - mu[None, :, :])).reshape(len(x), na * C)
    mean, cov = model.predict_with_covariance(targets, cross_alpha=cross)
    got = cov.values.reshape(na * C, na * C) if cross else cov.values
    N1, N2 = np.append(Ns, 0.0), np.append(Ns, [0.0, 0.0])
    var = [dense_theta(np.concatenate([Ws, Y[:, [i]]], axis=1), N1)[K, K] for i in range(na * C)]
    worst = 0.0
    for i in range(na * C):
        for j in range(i, na * C):
            if not cross and i // C != j // C:
                continue
            g = got[i, j] if cross else got[i // C, i % C, j % C]
            scale = np.sqrt(var[i] * var[j])
            if i == j:
                want, o = var[i], 0.0
            else:
                W = np.concatenate([Ws, Y[:, [i, j]]], axis=1)
                d = dense_theta(W, N2)
                want, o = d[K, K + 1], abs(gram_theta(W, N2)[K, K + 1] - d[K, K + 1]) / scale
            worst = max(worst, abs(g - want) / scale)
            assert abs(g - want) <= bound(own, o) * scale, (i, j, g, want)
    return mean, cov, worst


@pytest.fixture(scope="module")
def small(txm):
    a0, ns = [1.0, 1.25, 1.5], [60, 57, 64]
    us, xs = gauss_problem(a0, ns, C=2, seed=5)
    return {"model": make_model(a0, us, xs), "a0": a0, "ns": ns, "us": us, "xs": xs, "targets": [1.25, 1.1, 1.7, 0.9]}


@pytest.mark.parametrize("cross", [False, True], ids=["same_alpha", "cross_alpha"])
def test_api_against_the_dense_restatement(small, cross):
    m, targets = small["model"], small["targets"]
    mean, cov, worst = dense_check(m, small["a0"], small["ns"], small["us"], small["xs"], targets, cross)
    print(f"\nK = 3, cross_alpha={cross}: worst difference from the dense Theta over sqrt(Theta_ii Theta_jj) {worst:.2e}")
    assert np.array_equal(mean.values, m.predict(targets).values) and mean.dims == ("beta", "val")
    _, err = m.predict_with_error(targets)
    if cross:
        assert cov.dims == ("beta", "val", "beta_2", "val_2") and cov.values.shape == (4, 2, 4, 2)
        np.testing.assert_array_equal(cov.coords["beta_2"], targets)
        diag = np.einsum("acac->ac", cov.values)
        flat = cov.values.reshape(8, 8)
        assert np.array_equal(flat, flat.T)
    else:
        assert cov.dims == ("beta", "val", "val_2") and cov.values.shape == (4, 2, 2)
        diag = np.einsum("acc->ac", cov.values)
    np.testing.assert_array_equal(cov.coords["beta"], targets)
    np.testing.assert_allclose(diag, err.values ** 2, rtol=1e-12, atol=0)
    one = m.predict_with_covariance(1.1, alpha_name="b", cross_alpha=cross)
    assert one[1].dims == (("b", "val", "b_2", "val_2") if cross else ("b", "val", "val_2")) and one[0].values.shape == (1, 2)


def test_api_carries_the_coordinates_of_the_value_dims(txm):
    """Labelled xv: cov has label_cov's coordinates -- those of the value dims and their copies under the _2 names."""
    import thermoextrap_amd as xtrap
    from thermoextrap_amd.xrlite import DataArray

    a0, ns = [1.0, 1.3], [40, 45]
    us, xs = gauss_problem(a0, ns, C=3, seed=3)
    states = [xtrap.beta.factory_extrapmodel(beta=b, data=xtrap.factory_data_values(
        uv=DataArray(u, ("rec",)), xv=DataArray(x, ("rec", "bin"), coords={"bin": [0.5, 1.5, 2.5]}), order=1, central=False))
        for b, x, u in zip(a0, xs, us)]
    m = xtrap.MBARModel(states)
    mean, cov = m.predict_with_covariance([1.1, 1.2])
    assert cov.dims == ("beta", "bin", "bin_2") and mean.dims == ("beta", "bin")
    np.testing.assert_array_equal(cov.coords["bin"], [0.5, 1.5, 2.5])
    np.testing.assert_array_equal(cov.coords["bin_2"], [0.5, 1.5, 2.5])
    _, full = m.predict_with_covariance([1.1, 1.2], cross_alpha=True)
    assert full.dims == ("beta", "bin", "beta_2", "bin_2")
    np.testing.assert_array_equal(full.coords["bin_2"], [0.5, 1.5, 2.5])
    np.testing.assert_array_equal(full.coords["beta_2"], [1.1, 1.2])
    for a in range(2):
        assert np.array_equal(full.values[a, :, a, :], cov.values[a])


def test_api_single_state_is_the_gram_matrix(txm):
    """K = 1: the pseudo-inverse term vanishes and cov = sum_n y y' -- the perturbation (ratio estimator) covariance.  The
    reference: long double from the weights e^{-(a - alpha0) u} and the means predict returned."""
    a0, ns, targets = [1.0], [150], [1.0, 1.15]
    us, xs = gauss_problem(a0, ns, C=3, seed=8)
    m = make_model(a0, us, xs)
    mean, cov = m.predict_with_covariance(targets, cross_alpha=True)
    u, x = np.asarray(us[0], dtype=LD), np.asarray(xs[0], dtype=LD)
    e = -(np.asarray(targets, dtype=LD)[None, :] - LD(1.0)) * (u - u.mean())[:, None]
    W = np.exp(e - e.max(0))
    W = W / W.sum(0)
    Y = (W[:, :, None] * (x[:, None, :] - mean.values.astype(LD)[None, :, :])).reshape(len(u), 6)
    want = np.asarray(Y.T @ Y, dtype=np.float64)
    sd = np.sqrt(np.diag(want))
    assert np.all(np.abs(cov.values.reshape(6, 6) - want) <= 1e-10 * np.outer(sd, sd))


def test_api_above_sixteen_states_against_the_dense_restatement(txm):
    """K = 17, 187 pooled samples, C = 2 (the shape of tests/test_mbar_cov_gpu.py): two targets, the cross form."""
    K = 17
    a0, ns = [1.0 + 0.1 * k for k in range(K)], ([9, 10, 11, 12, 13] * 4)[:K - 2] + [11, 11]
    us, xs = gauss_problem(a0, ns, C=2, seed=17)
    m = make_model(a0, us, xs)
    _, _, worst = dense_check(m, a0, ns, us, xs, [1.35, 2.7], True)
    print(f"\nK = 17: worst difference from the dense Theta over sqrt(Theta_ii Theta_jj) {worst:.2e}")


def test_a_linear_combination_is_the_error_bar_of_the_combined_column(txm):
    """Needs no reference: q' cov q over C = 5 columns is predict_with_error()^2 of a second model whose observable is the
    single column x q -- the same kernels on either side of the same solve.  1e-10 relative; the cross form: the variance
    of a difference between two targets is non-negative and below (err_1 + err_2)^2."""
    a0, ns, targets = [1.0, 1.2, 1.4], [700, 333, 450], [1.1, 1.3, 0.9]
    us, xs = problem(a0, ns, 5, seed=77)
    q = np.random.default_rng(7).normal(size=5)
    wide, narrow = make_model(a0, us, xs), make_model(a0, us, [x @ q for x in xs])
    _, cov = wide.predict_with_covariance(targets)
    _, err = narrow.predict_with_error(targets)
    var = np.einsum("c,acd,d->a", q, cov.values, q)
    want = err.values.reshape(3) ** 2
    worst = float(np.max(np.abs(var - want) / want))
    print(f"\nq' cov q against the combined column's err^2: worst relative difference {worst:.2e}")
    assert worst <= 1e-10
    _, full = wide.predict_with_covariance(targets, cross_alpha=True)
    _, e5 = wide.predict_with_error(targets)
    for a in range(3):
        for b in range(a + 1, 3):
            for c in range(5):
                d = full.values[a, c, a, c] + full.values[b, c, b, c] - 2.0 * full.values[a, c, b, c]
                assert 0.0 <= d < (e5.values[a, c] + e5.values[b, c]) ** 2, (a, b, c, d)


def test_asymptotic_correlations_match_the_bootstrap(txm):
    """The one statistical test.  K = 3 overlapping Gaussian states (4000, 3500, 4500 samples), C = 3, targets 1.05 and 1.25,
    nrep = 400, fixed seed: every off-diagonal correlation of the 6 x 6 matrix (index a C + c) lies within 6 / sqrt(nrep - 3)
    = 0.301 of the bootstrap's in Fisher's z -- six standard errors --, every standard deviation within 1 +- 6 / sqrt(2 * 399)
    of the bootstrap's spread."""
    a0, ns, targets = [1.0, 1.15, 1.3], [4000, 3500, 4500], [1.05, 1.25]
    us, xs = gauss_problem(a0, ns, C=3, seed=11)
    m = make_model(a0, us, xs)
    _, cov = m.predict_with_covariance(targets, cross_alpha=True)
    rep = m.bootstrap({"nrep": 400, "seed": 20240607}).predict(targets).values             # (2, 400, 3)
    boot = np.cov(np.moveaxis(rep, 1, 0).reshape(400, 6), rowvar=False, ddof=1)
    asym = cov.values.reshape(6, 6)
    sa, sb = np.sqrt(np.diag(asym)), np.sqrt(np.diag(boot))
    ratio = sa / sb
    iu = np.triu_indices(6, 1)
    z = np.abs(np.arctanh((asym / np.outer(sa, sa))[iu]) - np.arctanh((boot / np.outer(sb, sb))[iu])) * np.sqrt(400 - 3)
    print("\nstd ratio:", np.array2string(ratio, precision=3), " worst |dz| in standard errors:", f"{z.max():.2f}",
          " same column at the two targets r =", np.array2string(np.array([asym[c, 3 + c] / (sa[c] * sa[3 + c]) for c in range(3)]), precision=3),
          " CPU:", CPU_Z)
    assert np.all(np.abs(ratio - 1.0) <= 6.0 / np.sqrt(2.0 * 399.0)), ratio
    assert np.all(z <= 6.0), z


CPU_Z = "below 2.2 standard errors"   # the restated formula against a numpy multinomial bootstrap of the same inputs (400 replicates)


def test_refusals(small):
    import thermoextrap_amd as xtrap

    m = small["model"]
    with pytest.raises(ValueError, match="8"):
        m.predict_with_covariance(np.linspace(0.9, 1.7, 9), cross_alpha=True)
    assert m.predict_with_covariance(np.linspace(0.9, 1.7, 9))[1].values.shape == (9, 2, 2)       # 8 + 1 targets, two passes
    with pytest.raises(NotImplementedError, match="pooled samples"):
        m.predict_cov(0.5)
    rng = np.random.default_rng(1)
    u = rng.normal(50.0, 2.0, 20)
    wide = xtrap.MBARModel([xtrap.beta.factory_extrapmodel(beta=1.0, data=xtrap.factory_data_values(
        uv=u, xv=rng.normal(size=(20, 256)), order=1, central=False))])
    with pytest.raises(ValueError, match="255"):
        wide.predict_with_covariance(1.1)
