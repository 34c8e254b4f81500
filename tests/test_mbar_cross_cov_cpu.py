"""CPU checks of MBAR's covariance across columns and targets (MBARModel.predict_with_covariance): the host algebra
engine.mbar_mean_covariance against the dense restatement of tests/test_mbar_cov_cpu.py, and the boundary of the entry
points txm_mbar_cross_cov / txm_mbar_cross_cov_plan (header, binding, the launch plan as host logic, refusals).

Theta is bilinear in the columns that were not sampled, so the covariance of two averages is the off-diagonal entry
[K, K + 1] of the dense Theta of [Ws, y_1, y_2] (N = 0 for both), y_n,(a,c) = W_na (x_nc - mean_ac).  Tolerance: that file's
``bound(own)`` rule -- max(1e-10, 10 x the disagreement of dense_theta and gram_theta on the same input) -- relative to
sqrt(Theta_11 Theta_22), the scale of an off-diagonal entry (a covariance may be near zero).

The plan.  txm_mbar_cross_cov declares no size query: it runs in the workspace of the txm_mbar_cov call it follows and plans
its launch from the bytes it is given.  That the query of txm_mbar_cov always holds the smallest plan is what
test_the_plan_fits_the_workspace_of_the_call_it_follows holds, over K, C, n_alpha and both modes.
"""

import ctypes as ct
import re

import numpy as np
import pytest

from test_mbar_cov_cpu import CASES, LD, ROOT, bound, dense_theta, gauss_problem, gram_theta, ref_columns, ref_solve, rel

HEAD = 64 * 32 + 2 * 64 * 8 + 256          # the workspace head of the MBAR entry points (state table, g, alpha0, M)


@pytest.fixture(scope="module", params=["K1", "K3", "twin"])
def case(request):
    a0, ns, targets = CASES[request.param]
    us, xs = gauss_problem(a0, ns, seed=len(ns) + ns[0])
    f = ref_solve(us, a0)
    Ws, Wt, _ = ref_columns(us, a0, f, targets[:2])
    Ns = np.array(ns, dtype=np.float64)
    x = np.concatenate(xs).astype(LD)
    own = rel(gram_theta(Ws, Ns), dense_theta(Ws, Ns)) if len(ns) > 1 else float(np.abs(gram_theta(Ws, Ns)).max())
    mean = np.einsum("na,nc->ac", Wt, x)                                     # (2 targets, 2 columns)
    Y = (Wt[:, :, None] * (x[:, None, :] - mean[None, :, :])).reshape(len(x), 4)   # column a * 2 + c
    return {"name": request.param, "K": len(ns), "Ns": Ns, "Ws": Ws, "Y": Y, "own": own}


def test_mean_covariance_is_the_dense_theta_of_two_unsampled_columns(case):
    from thermoextrap_amd import engine

    Ws, Ns, Y, K = case["Ws"], case["Ns"], case["Y"], case["K"]
    Gs = np.asarray(Ws.T @ Ws, dtype=np.float64)
    gram = np.asarray(Y.T @ Y, dtype=np.float64)                             # (4, 4): the cross form
    b = np.asarray(Y.T @ Ws, dtype=np.float64)                               # (4, K)
    pinv = engine.mbar_reduced_pinv(Gs, Ns)
    got = engine.mbar_mean_covariance(Gs, Ns, gram, b)
    assert got.shape == (4, 4) and np.array_equal(got, engine.mbar_mean_covariance(Gs, Ns, gram, b, pinv=pinv))
    Nc = np.append(Ns, [0.0, 0.0])
    worst = 0.0
    for i in range(4):
        for j in range(i + 1, 4):
            W = np.concatenate([Ws, Y[:, [i, j]]], axis=1)
            dense = dense_theta(W, Nc)
            scale = np.sqrt(dense[K, K] * dense[K + 1, K + 1])
            own = abs(gram_theta(W, Nc)[K, K + 1] - dense[K, K + 1]) / scale
            worst = max(worst, own)
            assert abs(got[i, j] - dense[K, K + 1]) <= bound(case["own"], own) * scale, (i, j)
    print(f"\n{case['name']}: the restatement's own disagreement on the off-diagonal entries {worst:.2e}")
    # the diagonal is mbar_mean_variance; symmetric; K = 1: the pseudo-inverse term vanishes
    var = engine.mbar_mean_variance(Gs, Ns, np.diag(gram), b, pinv=pinv)
    assert np.all(np.abs(np.diag(got) - var) <= 1e-14 * var)
    sym = 0.5 * (gram + gram.T)
    full = engine.mbar_mean_covariance(Gs, Ns, sym, b, pinv=pinv)
    assert np.array_equal(full, full.T) and np.abs(got - got.T).max() <= 1e-14 * np.abs(got).max()
    if K == 1:
        assert np.array_equal(got, gram)
    # the same-alpha form: leading axes broadcast, each target's block of the cross form
    same = engine.mbar_mean_covariance(Gs, Ns, np.stack([gram[:2, :2], gram[2:, 2:]]), b.reshape(2, 2, K), pinv=pinv)
    assert same.shape == (2, 2, 2)
    scale = np.abs(got).max()
    assert np.abs(same[0] - got[:2, :2]).max() <= 1e-14 * scale and np.abs(same[1] - got[2:, 2:]).max() <= 1e-14 * scale


# ---- the boundary ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from thermoextrap_amd import _build, _lib

    _build.build_library()
    return _lib.load()


def test_header_binding_and_integration_notes_agree():
    from thermoextrap_amd import _lib

    def proto(text, name):
        m = re.search(rf"\bint\s+{name}\s*\((.*?)\)\s*;", text, re.S)
        assert m, name
        return [" ".join(a.split()) for a in m.group(1).split(",")]

    hdr = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "txmom.h").read_text(), flags=re.S)
    doc = (ROOT / "INTEGRATION.md").read_text()
    kind = {"double": ct.c_double, "int32_t": ct.c_int32, "int64_t": ct.c_int64, "size_t": ct.c_size_t}
    for name in ("txm_mbar_cross_cov_plan", "txm_mbar_cross_cov"):
        args = proto(hdr, name)
        assert proto(doc, name) == args, name
        res, argtypes = _lib.SIGNATURES[name]
        assert res is ct.c_int and len(argtypes) == len(args)
        for a, t in zip(args, argtypes):
            if "*" in a or a.startswith("txm_stream "):
                assert t in (ct.c_void_p, ct.POINTER(ct.c_double), ct.POINTER(ct.c_int64), ct.POINTER(_lib.MbarState)), a
            else:
                assert t is kind[a.split()[0]], a
    # no size query of its own (tests/test_workspace_table_cpu.py holds every one the header declares to a contract row)
    assert not re.search(r"^size_t\s+txm_mbar_cross\w*\(", hdr, flags=re.M)


def plan(lib, K, C, na, cross, n_max, ws_bytes):
    p = (ct.c_int64 * 4)(-1, -1, -1, -1)
    rc = lib.txm_mbar_cross_cov_plan(K, C, na, cross, n_max, ws_bytes, p)
    return rc, list(p)


def records(C, na, cross):
    T = -(-C // 16)
    return T, T * (T + 1) // 2, (T * (T + 1) // 2) * (na if cross else 1), na * 256 * 8


@pytest.mark.parametrize("cross", [0, 1], ids=["same_alpha", "cross_alpha"])
def test_the_plan_fits_the_workspace_of_the_call_it_follows(lib, cross):
    """For every K, C and n_alpha of the list: with the bytes txm_mbar_cov asks for the plan succeeds, has at least one
    sample workgroup and uses no more than it was given; it is what the shapes say (tiles, pairs, the three caps)."""
    cus8 = None
    for K in (1, 2, 3, 5, 7, 13, 16, 17, 64):
        for C in (1, 15, 16, 17, 32, 33, 255):
            for na in range(1, 9):
                ws = lib.txm_mbar_cov_ws_bytes(K, C, na)
                assert ws > 0
                T, pairs, per_gx, rec = records(C, na, cross)
                for n_max in (1, 256, 257, 10**9):
                    rc, p = plan(lib, K, C, na, cross, n_max, ws)
                    assert rc == 0, (K, C, na, n_max, p)
                    assert p[0] == T and p[1] == pairs and p[2] >= 1, (K, C, na, n_max, p)
                    assert p[3] == HEAD + p[2] * per_gx * rec <= ws, (K, C, na, n_max, p)
                    assert p[2] <= -(-n_max // 256)
                if cus8 is None:                                   # K = 1, C = 1, one target: only the workgroup cap binds
                    cus8 = p[2]
                    assert cus8 % 8 == 0 and cus8 >= 8
                fit = (ws - HEAD) // rec // per_gx
                assert p[2] == max(1, min(fit, cus8 // per_gx, -(-10**9 // 256))), (K, C, na, p)
    # the widest cross form: one sample workgroup, 136 pairs x 8 row targets
    rc, p = plan(lib, 1, 255, 8, 1, 10**8, lib.txm_mbar_cov_ws_bytes(1, 255, 8))
    assert rc == 0 and p[:2] == [16, 136] and p[2] == max(1, cus8 // 1088)


def test_the_plan_is_monotone_in_the_bytes_and_refuses_below_its_minimum(lib):
    for K, C, na, cross, n_max in ((8, 17, 8, 0, 1000), (8, 17, 8, 1, 1000), (3, 33, 3, 1, 5000), (1, 255, 1, 0, 4000),
                                   (64, 255, 8, 1, 10**6), (2, 1, 1, 0, 10**7)):
        T, pairs, per_gx, rec = records(C, na, cross)
        least = HEAD + per_gx * rec
        rc, p = plan(lib, K, C, na, cross, n_max, least)
        assert rc == 0 and p[2] == 1 and p[3] == least
        rc, p = plan(lib, K, C, na, cross, n_max, least - 1)
        assert rc == -3 and p[2] == 0 and p[3] == least            # refused: the smallest workspace the call takes
        rc, p = plan(lib, K, C, na, cross, n_max, 0)
        assert rc == -3 and p[3] == least
        full = lib.txm_mbar_cov_ws_bytes(K, C, na)
        last, top = 1, None
        for ws in np.unique(np.concatenate([np.linspace(least, 4 * full, 97).astype(np.int64),
                                            least + per_gx * rec * np.arange(1, 6) - 1, least + per_gx * rec * np.arange(1, 6)])):
            rc, p = plan(lib, K, C, na, cross, n_max, int(ws))
            assert rc == 0 and p[2] >= last and p[3] <= ws, (K, C, na, cross, ws, p)
            last = p[2]
        rc, top = plan(lib, K, C, na, cross, n_max, 1 << 50)
        assert rc == 0 and top[2] >= last and top[2] <= -(-n_max // 256)
    for bad in ((0, 4, 1, 0, 10), (65, 4, 1, 0, 10), (2, 0, 1, 0, 10), (2, 256, 1, 0, 10), (2, 4, 0, 0, 10), (2, 4, 9, 1, 10),
                (2, 4, 1, 2, 10), (2, 4, 1, 0, 0)):
        rc, _ = plan(lib, *bad, 1 << 40)
        assert rc == -1, bad
    assert lib.txm_mbar_cross_cov_plan(2, 4, 1, 0, 10, 1 << 40, None) == -1


def test_refusals_without_a_device(lib):
    from thermoextrap_amd import _lib

    def states(K, n=100, C=4):
        tab = (_lib.MbarState * max(K, 1))()
        for s in range(max(K, 1)):
            tab[s].x, tab[s].u, tab[s].n, tab[s].ldx_s = 0x10000, 0x20000, n, C     # never dereferenced: refused first
        return tab

    d = (ct.c_double * 9)()
    p = ct.c_void_p(0x30000)

    def call(tab, K, C=4, na=1, cross=0, ws_bytes=1 << 40, logD=p, al=d, mean=p, lnw=p, out=p, ws=p):
        return lib.txm_mbar_cross_cov(tab, K, C, 0.0, logD, al, na, mean, lnw, cross, out, ws, ws_bytes, None)

    def refused(rc, words, status=-1):
        assert rc == status, (rc, _lib.last_error())
        assert all(w in _lib.last_error() for w in words), _lib.last_error()

    refused(call(states(2), 2, C=0), ["mbar_cross_cov", "C = 0"])
    refused(call(states(2, C=256), 2, C=256), ["C = 256", "255"])
    refused(call(states(2), 2, na=0), ["n_alpha = 0"])
    refused(call(states(2), 2, na=9), ["n_alpha = 9"])
    refused(call(states(1), 0), ["K = 0"])
    refused(call(states(65), 65), ["K = 65"])
    refused(call(states(2), 2, cross=2), ["cross_alpha = 2"])
    refused(call(None, 2), ["null state table"])
    tab = states(3)
    tab[1].n = 0
    refused(call(tab, 3), ["state 1", "n = 0"])
    tab = states(2)
    tab[1].x = None
    refused(call(tab, 2), ["state 1", "null u or x"])
    refused(call(states(2), 2, C=5), ["ldx_s = 4 < C = 5"])
    for name in ("logD", "al", "mean", "lnw", "out", "ws"):
        refused(call(states(2), 2, **{name: None}), ["null pointer"])
    bad = (ct.c_double * 9)()
    bad[1] = float("inf")
    refused(call(states(2), 2, na=2, al=bad), ["target 1 not finite"])
    # a short workspace: one byte below the smallest plan, in both modes
    for cross in (0, 1):
        least = HEAD + (3 if cross else 1) * 3 * 256 * 8
        refused(call(states(2), 2, na=3, cross=cross, ws_bytes=least - 1), ["workspace too small"], status=-3)
    refused(call(states(2), 2, ws_bytes=16), ["workspace too small"], status=-3)
