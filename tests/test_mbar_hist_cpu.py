"""CPU checks of MBARModel.histogram's host half: engine.bin_index against numpy.histogram, the closed-form covariance
_mbar_host.mbar_hist_covariance against the dense restatement (tests/_mbar_hist_ref.py), and the boundary of the entry
points txm_mbar_hist / txm_mbar_hist_plan (header, binding, the launch plan as host logic, refusals without a device).

Tolerance of the covariance: the rule of tests/test_mbar_cov_cpu.py -- max(1e-10, 10 x the disagreement of the dense and
Gram forms of the restatement itself), relative to sqrt(Theta_ii Theta_jj); both sides are CPU restatements.  The
multinomial case (K = 1, alpha = alpha0: W_n = 1 / N exactly) is held to 1e-12 / N: the closed form is a handful of
roundings of numbers of size p / N.
"""

import ctypes as ct
import re

import numpy as np
import pytest
import torch

import _mbar_hist_ref as hr
from test_mbar_cov_cpu import CASES, LD, ROOT, bound, gauss_problem, ref_columns, ref_solve

HEAD = 64 * 32 + 2 * 64 * 8 + 256 + 64 * 8     # the MBAR workspace head (state table, g, alpha0, M), then the bin pointers
SIZE_MAX = ct.c_size_t(-1).value


# ---- bin_index ----------------------------------------------------------------------------------------------------------
def numpy_assignment(v, edges):
    """The bin numpy.histogram puts every value into (-1: none), found by asking it one value at a time."""
    out = np.full(len(v), -1, dtype=np.int64)
    for i, x in enumerate(v):
        if np.isnan(x):
            continue
        h = np.histogram([x], edges)[0]
        if h.sum():
            out[i] = int(np.argmax(h))
    return out


@pytest.mark.parametrize("kind", ["uniform", "ragged"])
def test_bin_index_is_numpy_histograms_assignment(kind):
    from thermoextrap_amd import engine

    rng = np.random.default_rng(3)
    if kind == "uniform":
        edges = np.histogram_bin_edges(np.empty(0), bins=13, range=(-1.3, 2.9))
    else:
        edges = np.cumsum(np.concatenate([[-2.0], rng.uniform(0.01, 0.7, 17)]))
    inner = rng.uniform(edges[0], edges[-1], 300)
    near = np.concatenate([np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf)])
    v = np.concatenate([inner, edges, near, [edges[0] - 1.0, edges[-1] + 1.0, np.nan, -np.inf, np.inf]])
    got = engine.bin_index(torch.as_tensor(v), edges)
    assert got.dtype == torch.int32 and got.shape == (len(v),)
    got = got.numpy()
    want = numpy_assignment(v, edges)
    assert np.array_equal(got, want)
    nb = len(edges) - 1
    assert got[len(inner)] == 0 and got[len(inner) + nb] == nb - 1            # the first edge, the right end
    assert np.all(got[-5:] == -1) and got[len(inner) + len(edges)] == -1      # below, above, NaN, the infinities
    finite = v[np.isfinite(v)]
    idx = engine.bin_index(finite, edges).numpy()                             # (a numpy array is taken too)
    assert np.array_equal(np.histogram(finite, edges)[0], np.bincount(idx[idx >= 0], minlength=nb))
    with pytest.raises(ValueError):
        engine.bin_index(v, edges[::-1])


# ---- mbar_hist_covariance -----------------------------------------------------------------------------------------------
def class_pattern(name, u, nbins):
    """The class (bin index, nbins = outside) of every pooled sample."""
    if name == "spread":                      # quantile bins of u, a few samples outside
        q = np.quantile(u, np.linspace(0.03, 0.97, nbins + 1))
        cl = np.searchsorted(q, u, side="right") - 1
        return np.where((cl < 0) | (cl >= nbins), nbins, cl)
    if name == "heavy":                       # one bin with all but the lowest-weight samples
        cl = np.full(len(u), 1)
        cl[np.argsort(u)[-3:]] = [0, 2, nbins]
        return cl
    if name == "empty":                       # bin 2 holds nothing
        cl = np.arange(len(u)) % nbins
        return np.where(cl == 2, 3, cl)
    raise KeyError(name)


@pytest.fixture(scope="module", params=["K1", "K3", "twin"])
def solved(request):
    a0, ns, targets = CASES[request.param]
    us, _ = gauss_problem(a0, ns, seed=len(ns) + ns[0])
    f = ref_solve(us, a0)
    Ws, Wt, _ = ref_columns(us, a0, f, targets)
    Ns = np.array(ns, dtype=np.float64)
    return {"name": request.param, "u": np.concatenate(us), "Ws": Ws, "Wt": Wt, "Ns": Ns}


@pytest.mark.parametrize("pattern", ["spread", "heavy", "empty"])
def test_hist_covariance_against_the_dense_restatement(solved, pattern):
    from thermoextrap_amd import engine

    Ws, Wt, Ns, nbins = solved["Ws"], solved["Wt"], solved["Ns"], 5
    cl = class_pattern(pattern, solved["u"], nbins)
    Gs = np.asarray(Ws.T @ Ws, dtype=np.float64)
    sums = [hr.class_sums(Ws, Wt[:, a], cl, nbins) for a in range(Wt.shape[1])]
    H, S, T = (np.stack([s[i] for s in sums]) for i in range(3))
    got = engine.mbar_hist_covariance(Gs, Ns, H, S, T)
    assert got.shape == (Wt.shape[1], nbins, nbins)
    assert np.array_equal(got, engine.mbar_hist_covariance(Gs, Ns, H, S, T, pinv=engine.mbar_reduced_pinv(Gs, Ns)))
    var = engine.mbar_hist_variance(Gs, Ns, H, S, T)
    worst = 0.0
    for a in range(Wt.shape[1]):
        assert np.array_equal(got[a], got[a].T)                                   # exactly symmetric
        Y, p = hr.indicator_columns(Wt[:, a], cl, nbins)
        dense, gram = hr.dense_cov(Ws, Ns, Y), hr.gram_cov(Ws, Ns, Y)
        sd = np.sqrt(np.clip(np.diag(dense), 0.0, None))
        scale = np.outer(sd, sd)
        live = scale > 0
        own = float(np.max(np.abs(gram - dense)[live] / scale[live]))
        err = float(np.max(np.abs(got[a] - dense)[live] / scale[live]))
        worst = max(worst, err)
        print(f"\n{solved['name']} {pattern} target {a}: restatement's own {own:.2e}, closed form vs dense {err:.2e}")
        assert err <= bound(own)
        assert np.all(np.abs(var[a] - np.diag(dense)) <= bound(own) * np.diag(scale))
        if pattern == "heavy":
            assert p[1] > 0.9
        if pattern == "empty":                                                    # an empty bin: zero row and column, exactly
            assert H[a, 2] == 0.0 and not got[a][2].any() and not got[a][:, 2].any() and var[a][2] == 0.0


def test_heavy_bin_keeps_relative_accuracy():
    """A bin with 99.9 % of the weight: its variance is that of the 0.1 % outside it.  The closed form, fed float64 sums,
    matches the long-double Gram diagonal sum_n W^2 (1_b - p_b)^2 to a few ulps; (1 - p) formed by subtraction would lose
    three digits before squaring."""
    from thermoextrap_amd import _mbar_host

    rng = np.random.default_rng(11)
    N, nbins = 20000, 3
    w = rng.uniform(0.5, 1.5, N).astype(LD)
    w /= w.sum()
    cl = np.full(N, 1)
    cl[:20] = rng.choice([0, 2, nbins], 20)
    H, S, T = hr.class_sums((w * 0 + LD(1) / N)[:, None], w, cl, nbins)
    assert H[1] > 0.998
    yy, _ = _mbar_host.mbar_hist_terms(H, S, T)
    Y, _ = hr.indicator_columns(w, cl, nbins)
    want = (Y * Y).sum(0)
    assert np.all(np.abs(yy.astype(LD) - want) <= 16 * np.finfo(np.float64).eps * want)


def test_one_state_at_its_own_alpha_is_the_multinomial():
    from thermoextrap_amd import engine

    rng = np.random.default_rng(5)
    N, nbins = 1000, 6
    cnt = rng.multinomial(N, [0.3, 0.2, 0.0, 0.25, 0.05, 0.15, 0.05]).astype(np.float64)     # bin 2 empty, 5 % outside
    H, S, T = (cnt / N)[None], (cnt / N**2)[None], (cnt / N**2)[None, None]
    got = engine.mbar_hist_covariance(np.array([[1.0 / N]]), np.array([float(N)]), H, S, T)[0]
    p = cnt[:nbins] / N
    want = (np.diag(p) - np.outer(p, p)) / N
    assert np.max(np.abs(got - want)) <= 1e-12 / N and np.array_equal(got, got.T)
    with pytest.raises(ValueError):
        engine.mbar_hist_covariance(np.array([[1.0 / N]]), np.array([float(N)]), H, S[:, :-1], T)


# ---- the boundary -------------------------------------------------------------------------------------------------------
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
    for name in ("txm_mbar_hist_plan", "txm_mbar_hist"):
        args = proto(hdr, name)
        assert proto(doc, name) == args, name
        res, argtypes = _lib.SIGNATURES[name]
        assert res is ct.c_int and len(argtypes) == len(args)
        for a, t in zip(args, argtypes):
            if "*" in a or a.startswith("txm_stream "):
                assert t in (ct.c_void_p, ct.POINTER(ct.c_double), ct.POINTER(ct.c_int64), ct.POINTER(ct.c_void_p),
                             ct.POINTER(_lib.MbarState)), a
            else:
                assert t is kind[a.split()[0]], a
    assert not re.search(r"^size_t\s+txm_mbar_hist\w*\(", hdr, flags=re.M)        # no size query: planned from ws_bytes
    assert "txm_mbar_hist.hip" in __import__("thermoextrap_amd._build", fromlist=["SOURCES"]).SOURCES


def plan(lib, K, nbins, na, n_max, ws_bytes):
    p = (ct.c_int64 * 4)(-1, -1, -1, -1)
    rc = lib.txm_mbar_hist_plan(K, nbins, na, n_max, ws_bytes, p)
    return rc, list(p)


def shape(K, nbins, na):
    """(bin tiles per workgroup, groups, row tiles, bytes of one sample workgroup's records): 32 accumulator tiles per wave
    split between the targets (1, 2, 4 or 8) and the bin tiles."""
    NT = nbins // 16 + 1
    bt = min(NT, 32 // (1 if na == 1 else 2 if na == 2 else 4 if na <= 4 else 8))
    G, RT = -(-NT // bt), -(-(K + 2) // 16)
    return bt, G, RT, G * RT * na * bt * 256 * 8


def test_the_smallest_and_the_full_plan(lib):
    cus4 = None
    for K in (1, 14, 15, 64):
        for nbins in (1, 15, 16, 17, 1023):
            for na in (1, 2, 3, 8):
                bt, G, RT, rec = shape(K, nbins, na)
                assert RT == {1: 1, 14: 1, 15: 2, 64: 5}[K]
                least = HEAD + rec
                for n_max in (1, 256, 257, 10**9):
                    rc, p = plan(lib, K, nbins, na, n_max, least)
                    assert rc == 0 and p == [bt, G, 1, least], (K, nbins, na, n_max, p)
                    rc, p = plan(lib, K, nbins, na, n_max, least - 1)
                    assert rc == -3 and p == [bt, G, 0, least], (K, nbins, na, n_max, p)       # refused: the size it takes
                    rc, full = plan(lib, K, nbins, na, n_max, SIZE_MAX)
                    assert rc == 0 and full[:2] == [bt, G] and full[3] == HEAD + full[2] * rec
                    assert 1 <= full[2] <= -(-n_max // 256)
                    if cus4 is None and n_max == 10**9:        # K = 1, one bin, one target: only the workgroup cap binds
                        cus4 = full[2]
                        assert cus4 % 4 == 0 and cus4 >= 4
                    if cus4 is not None:
                        assert full[2] == max(1, min(-(-n_max // 256), cus4 // (G * RT))), (K, nbins, na, n_max, full)
                    rc, again = plan(lib, K, nbins, na, n_max, full[3])                        # the engine's two steps
                    assert rc == 0 and again == full
                    if full[2] > 1:
                        rc, less = plan(lib, K, nbins, na, n_max, full[3] - 1)
                        assert rc == 0 and less[2] == full[2] - 1 and less[3] == full[3] - rec
    rc, p = plan(lib, 8, 1023, 8, 10**6, 0)
    assert rc == -3 and p[2] == 0 and p[3] == HEAD + shape(8, 1023, 8)[3]
    for bad in ((0, 4, 1, 10), (65, 4, 1, 10), (2, 0, 1, 10), (2, 1024, 1, 10), (2, 4, 0, 10), (2, 4, 9, 10), (2, 4, 1, 0)):
        rc, _ = plan(lib, *bad, 1 << 40)
        assert rc == -1, bad
    assert lib.txm_mbar_hist_plan(2, 4, 1, 10, 1 << 40, None) == -1


def test_refusals_without_a_device(lib):
    from thermoextrap_amd import _lib

    def states(K, n=100):
        tab = (_lib.MbarState * max(K, 1))()
        for s in range(max(K, 1)):
            tab[s].x, tab[s].u, tab[s].n, tab[s].ldx_s = None, 0x20000, n, 0       # never dereferenced: refused first
        return tab

    def bins(K):
        return (ct.c_void_p * max(K, 1))(*([0x40000] * max(K, 1)))

    d = (ct.c_double * 65)()
    p = ct.c_void_p(0x30000)
    unset = object()

    def call(tab, K, nbins=4, na=1, ws_bytes=1 << 40, bin_tab=unset, a0=d, g=d, logD=p, al=d, out=p, lnw=p, ws=p):
        bt = bins(K) if bin_tab is unset else bin_tab
        return lib.txm_mbar_hist(tab, bt, K, nbins, 0.0, a0, g, logD, al, na, out, lnw, ws, ws_bytes, None)

    def refused(rc, words, status=-1):
        assert rc == status, (rc, _lib.last_error())
        assert all(w in _lib.last_error() for w in words), _lib.last_error()

    refused(call(states(1), 0), ["mbar_hist", "K = 0"])
    refused(call(states(65), 65), ["K = 65"])
    refused(call(states(2), 2, nbins=0), ["nbins = 0"])
    refused(call(states(2), 2, nbins=1024), ["nbins = 1024", "1023"])
    refused(call(states(2), 2, na=0), ["n_alpha = 0"])
    refused(call(states(2), 2, na=9), ["n_alpha = 9"])
    refused(call(None, 2), ["null state table"])
    refused(call(states(2), 2, bin_tab=None), ["null table of bin indices"])
    tab = states(3)
    tab[1].n = 0
    refused(call(tab, 3), ["state 1", "n = 0"])
    tab = states(2)
    tab[1].u = None
    refused(call(tab, 2), ["state 1", "null u"])
    bt = bins(2)
    bt[1] = None
    refused(call(states(2), 2, bin_tab=bt), ["state 1", "null bin indices"])
    for name in ("a0", "g", "logD", "al", "out", "ws"):
        refused(call(states(2), 2, **{name: None}), ["null pointer"])
    bad = (ct.c_double * 65)()
    bad[1] = float("inf")
    refused(call(states(2), 2, na=2, al=bad), ["target 1 not finite"])
    refused(call(states(2), 2, g=bad), ["state 1 not finite"])
    least = HEAD + shape(2, 4, 3)[3]
    refused(call(states(2), 2, na=3, ws_bytes=least - 1), ["workspace too small", str(least)], status=-3)
    refused(call(states(2), 2, ws_bytes=16), ["workspace too small"], status=-3)
