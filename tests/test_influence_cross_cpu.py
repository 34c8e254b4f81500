"""The host side of the cross-column delta-method covariance, without a device: the workspace query and the
argument validation of txm_influence_cross_cov, its binding, the definition V[c,i,c',j] = sum p^2 psi_ci psi_c'j in long
double against a numpy bootstrap of two correlated columns, and the label logic of ExtrapModel.derivs_cross_cov /
predict_cov on a stubbed device result."""

from __future__ import annotations

import ctypes as ct
import math
import re
from pathlib import Path

import numpy as np

from oracle import derivs_oracle as DO
from tests._influence_cross_ref import cross_cov_ld
from tests._influence_ref import ld_moments, make_data, psi_ld, series_for

from thermoextrap_amd import symbolic as S

HEADER = Path(__file__).resolve().parents[1] / "include" / "txmom.h"


def _records(N, C, cus=256):
    """The plan of txm_influence_cross.hip restated: T tiles a side, upper-triangle pairs, one workgroup per 256 samples
    and pair up to 8 workgroups per CU in all; (records of partials the query allows for, records the launch writes)."""
    T = (C + 1 + 15) // 16
    pairs = T * (T + 1) // 2
    shares = -(-N // 256)
    grid_x = min(shares, max(cus * 8 // pairs, 1))
    allowed = min(shares * pairs, max(cus * 8, pairs))
    return allowed + pairs, grid_x * pairs + pairs


def test_workspace_query_is_host_logic():
    """8 (256 (2 n_q - 1) + 8) doubles per record; partial records for every (workgroup, tile pair) and one summed record
    per pair; 0 for each bad argument; nondecreasing in C; never less than what the launch writes."""
    from thermoextrap_amd import _lib

    Q = _lib.load().txm_influence_cross_cov_ws_bytes
    for N, C, nf, nq in [(1, 1, 1, 1), (255, 15, 5, 5), (256, 16, 5, 5), (257, 33, 2, 9), (10**8, 32, 5, 5), (10**8, 255, 9, 9),
                         (4000, 255, 1, 1), (10**6, 4, 3, 5)]:
        allowed, written = _records(N, C)
        assert Q(N, C, nf, nq) == allowed * (256 * (2 * nq - 1) + 8) * 8 + 256, (N, C, nf, nq)
        assert written <= allowed
    assert Q(10**8, 255, 9, 9) <= 80 * 10**6                                # 76 MB at the widest call the entry takes
    for bad in [(0, 3, 5, 5), (-4, 3, 5, 5), (1000, 0, 5, 5), (1000, 256, 5, 5), (1000, 3, 0, 5), (1000, 3, 10, 5),
                (1000, 3, 5, 0), (1000, 3, 5, 10)]:
        assert Q(*bad) == 0, bad
    for N in (1, 300, 5000, 10**5, 10**8):
        sizes = [Q(N, C, 5, 5) for C in range(1, 256)]
        assert all(s0 <= s1 for s0, s1 in zip(sizes, sizes[1:])), N
        for C in range(1, 256):
            allowed, written = _records(N, C)
            assert written <= allowed, (N, C)


def test_entry_point_validates_without_a_device():
    """txm_influence_cross_cov: every refusal comes back before any HIP call, one case each; the launcher asks for exactly
    what the query returns (one byte less is TXM_ERR_WORKSPACE)."""
    from thermoextrap_amd import _lib

    lib = _lib.load()
    p = ct.c_void_p(256)   # never dereferenced: every call below fails validation first
    names = ("x", "ls", "u", "w", "N", "C", "nf", "nq", "cu", "cx", "a", "b", "cov", "ws", "wsb", "st")
    good = dict(x=p, ls=4, u=p, w=None, N=10, C=4, nf=3, nq=3, cu=0.0, cx=p, a=p, b=p, cov=p, ws=p, wsb=1 << 30, st=None)

    def call(**bad):
        return lib.txm_influence_cross_cov(*[{**good, **bad}[n] for n in names])

    for ptr in ("x", "u", "cx", "a", "b", "cov", "ws"):
        assert call(**{ptr: None}) == -1 and b"null" in lib.txm_last_error(), ptr
    assert call(N=0) == -1
    assert call(C=0) == -1
    assert call(C=256, ls=256) == -1 and b"255" in lib.txm_last_error()
    assert call(nf=10) == -1 and b"n_f" in lib.txm_last_error()
    assert call(nf=0) == -1 and b"n_f" in lib.txm_last_error()
    assert call(nq=0) == -1 and b"n_q" in lib.txm_last_error()
    assert call(nq=10) == -1 and b"n_q" in lib.txm_last_error()
    assert call(ls=3) == -1 and b"pitch" in lib.txm_last_error()
    assert call(cu=float("nan")) == -1 and b"NaN" in lib.txm_last_error()
    for N, C, nf, nq in [(10, 4, 3, 3), (10**6, 33, 2, 9)]:
        need = lib.txm_influence_cross_cov_ws_bytes(N, C, nf, nq)
        assert call(N=N, C=C, ls=C, nf=nf, nq=nq, wsb=need - 1) == -3 and b"workspace" in lib.txm_last_error()


def test_symbols_bound_with_the_header_signature():
    """Both symbols are in the binding's table with the argument list include/txmom.h declares, and resolve in the
    library; the ABI version did not move."""
    from thermoextrap_amd import _lib

    text = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    ctype = {"int64_t": ct.c_int64, "int": ct.c_int, "double": ct.c_double, "size_t": ct.c_size_t, "txm_stream": ct.c_void_p}
    ret = {"size_t": ct.c_size_t, "int": ct.c_int}
    lib = _lib.load()
    for name in ("txm_influence_cross_cov_ws_bytes", "txm_influence_cross_cov"):
        m = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, name
        args = []
        for arg in m.group(2).split(","):
            arg = arg.strip()
            args.append(ct.c_void_p if "*" in arg else ctype[arg.replace("const ", "").split()[0]])
        res, bound = _lib.SIGNATURES[name]
        assert res is ret[m.group(1)] and list(bound) == args, name
        assert getattr(lib, name).argtypes == args
    assert lib.txm_abi_version() == 2 == _lib.ABI_VERSION


def test_against_numpy_bootstrap_two_correlated_columns():
    """N = 2e4, unweighted, order 1, two columns that share u: every entry of V = sum p^2 psi_ci psi_c'j -- the blocks
    between the columns included -- against the covariance of 2000 multinomial replicates of the oracle's derivatives;
    |V - S| <= 5 se with se = std_r[(d - m)(d' - m')] / sqrt(R)."""
    N, R, order = 20000, 2000, 1
    x, u, _ = make_data(N, seed=0, weighted=False, ncol=2)
    p, dx, du, mom = ld_moments(x, u, None, order)
    a, b = S.influence_coefs(series_for(True), order, mom)
    psi = np.stack([psi_ld(a[c], b[c], dx[:, c], du) for c in range(2)])
    V = np.asarray(cross_cov_ld(p, psi), float).reshape(2 * (order + 1), 2 * (order + 1))
    counts = np.random.default_rng(1).multinomial(N, np.full(N, 1.0 / N), size=R)
    d = np.stack([np.concatenate([DO.derivs_x_ave(x[:, c], u, order, w=counts[r]) for c in range(2)]) for r in range(R)])
    dev = np.asarray(d - d.mean(axis=0), float)                                        # [R, (c, i)]
    prod = dev[:, :, None] * dev[:, None, :]
    Sm = prod.sum(axis=0) / (R - 1)
    se = prod.std(axis=0, ddof=1) / math.sqrt(R)
    ratio = np.abs(V - Sm) / se
    corr = V[0, order + 1] / math.sqrt(V[0, 0] * V[order + 1, order + 1])
    print("bootstrap check: |V - S| / se =\n", np.array2string(ratio, precision=2), f"\n correlation of the two means: {corr:.3f}")
    assert (ratio <= 5.0).all()
    assert abs(corr) > 0.3                                                             # the off-diagonal blocks are not small


def _stub_model(order, out_dims, out_shape, coords):
    """An ExtrapModel whose device result is already in its cache: the label logic alone runs."""
    import torch

    from thermoextrap_amd import models

    C = int(np.prod(out_shape))
    rng = np.random.default_rng(3)
    g = rng.normal(size=(C * (order + 1), C * (order + 1)))
    cov = (g @ g.T).reshape(C, order + 1, C, order + 1)
    m = object.__new__(models.ExtrapModel)
    m.alpha0, m.order, m.minus_log, m.alpha_name = 0.5, order, False, "beta"
    m.data = None
    src = models._HostSource(out_dims, out_shape, coords, None)
    m._cache = {("dxcov", order, False): (torch.from_numpy(cov.copy()), src)}
    return m, cov


def test_label_logic_on_a_stubbed_engine_call():
    from thermoextrap_amd.xrlite import DataArray

    order = 2
    coords = {"r": (("r",), np.array([0.5, 1.5, 2.5]))}
    m, cov = _stub_model(order, ["r", "comp"], [3, 2], coords)
    V = m.derivs_cross_cov()
    assert V.dims == ("order", "order_2", "r", "comp", "r_2", "comp_2") and V.shape == (3, 3, 3, 2, 3, 2)
    c4 = cov.reshape(3, 2, order + 1, 3, 2, order + 1)                               # (r, comp, i, r', comp', j)
    assert np.array_equal(V.values, np.transpose(c4, (2, 5, 0, 1, 3, 4)))
    assert np.array_equal(V["r"].values, coords["r"][1]) and np.array_equal(V["r_2"].values, coords["r"][1])
    Vn = m.derivs_cross_cov(norm=True)
    f = np.array([1.0, 1.0, 0.5])
    np.testing.assert_allclose(Vn.values, V.values * f[:, None, None, None, None, None] * f[None, :, None, None, None, None],
                               rtol=1e-15)
    assert ("dcov", order, False) not in m._cache and list(m._cache) == [("dxcov", order, False)]

    sentinel = object()
    m.predict = lambda alpha, **kw: sentinel
    alphas = np.array([0.3, 0.5, 0.62, 0.7])
    pred, pc = m.predict_cov(alphas)
    assert pred is sentinel
    assert pc.dims == ("beta", "r", "comp", "r_2", "comp_2") and pc.shape == (4, 3, 2, 3, 2)
    for k, al in enumerate(alphas):
        t = np.array([(al - 0.5) ** i / math.factorial(i) for i in range(order + 1)])
        ref = np.einsum("i,cidj,j->cd", t, cov, t).reshape(3, 2, 3, 2)
        np.testing.assert_allclose(pc.values[k], ref, rtol=1e-13, atol=1e-13 * np.abs(ref).max())
    assert np.array_equal(pc["beta"].values, alphas) and np.array_equal(pc["r_2"].values, coords["r"][1])
    assert isinstance(pc, DataArray)
    # alpha0 itself: t = (1, 0, 0), the covariance of the means
    assert np.array_equal(pc.values[1].reshape(6, 6), cov[:, 0, :, 0])
