"""The host side of the blocked cross-column delta-method covariance, without a device: the workspace query
and the argument validation of txm_influence_block_cross_cov, its binding, the level and label logic of
ExtrapModel.derivs_cross_cov(block=...) / cross_blocking_curve / predict_cov(block=...) on a stubbed device result, and the
definition in numpy on three correlated AR(1) columns whose long-run covariance is known."""

from __future__ import annotations

import ctypes as ct
import math
import re
from pathlib import Path

import numpy as np

from tests._block_cross_ref import AR1_BLOCK, AR1_LIMIT, ar1_columns, ar1_scale, blocked_means_cov

HEADER = Path(__file__).resolve().parents[1] / "include" / "txmom.h"


def _written(N, C, nf, block, cus=256):
    """The plan of txm_influence_block_cross.hip restated -- doubles the launches write: pass 1's block sums and weights,
    the column-sum partials, W, one record of 16 tiles per (block workgroup, macro pair) and the summed records."""
    M, nb = C * nf, -(-N // block)
    TM = -(-(-(-M // 16)) // 4)
    pairs = TM * (TM + 1) // 2
    gy = min(-(-nb // 256), max(cus * 4 // pairs, 1))
    parts = min(-(-nb // 64), 256)
    return nb * (M + 1) + parts * (M + 1) + 1 + (gy + 1) * pairs * 4096


def test_workspace_query_is_host_logic():
    """0 for every bad argument; nondecreasing in n_levels; never below pass 1's own workspace nor below what the launches
    write; 45 MB of records at the widest call."""
    from thermoextrap_amd import _lib

    lib = _lib.load()
    Q = lib.txm_influence_block_cross_cov_ws_bytes
    shapes = [(1000, 3, 5, 5, 7), (1000, 3, 5, 5, 1000), (1000, 3, 5, 5, 4096), (1, 1, 1, 1, 1), (10**8, 32, 5, 5, 1024),
              (10**8, 32, 5, 5, 16), (10**6, 255, 9, 2, 1000), (1001, 255, 9, 9, 1000), (70000, 13, 5, 7, 1), (4000, 255, 2, 2, 3)]
    for N, C, nf, nq, block in shapes:
        sizes = [Q(N, C, nf, nq, block, nl) for nl in range(1, 33)]
        assert all(s0 <= s1 for s0, s1 in zip(sizes, sizes[1:])), (N, C, nf, nq, block)
        pass1 = 8 * -(-N // block) * (C * nf + 1) + 256
        assert pass1 == lib.txm_influence_block_cov_ws_bytes(N, C, nf, nq, block)
        assert sizes[0] >= pass1 and sizes[0] >= 8 * _written(N, C, nf, block), (N, C, nf, nq, block)
    assert Q(20, 255, 9, 2, 2, 1) <= 45 * 10**6
    # next to the 25.6 GB of samples: pass 1's 126 MB and 36 MB of records
    assert Q(10**8, 32, 5, 5, 1024, 17) <= 8 * 97657 * 161 + 40 * 10**6
    for bad in [(0, 3, 5, 5, 7, 1), (-5, 3, 5, 5, 7, 1), (1000, 0, 5, 5, 7, 1), (1000, 256, 5, 5, 7, 1), (1000, 3, 0, 5, 7, 1),
                (1000, 3, 10, 5, 7, 1), (1000, 3, 5, 0, 7, 1), (1000, 3, 5, 10, 7, 1), (1000, 3, 5, 5, 0, 1),
                (1000, 3, 5, 5, -1, 1), (1000, 3, 5, 5, 7, 0), (1000, 3, 5, 5, 7, 33), (1000, 3, 5, 5, 7, -2)]:
        assert Q(*bad) == 0, bad


def test_entry_point_validates_without_a_device():
    """txm_influence_block_cross_cov: every refusal comes back before any HIP call, one case each."""
    from thermoextrap_amd import _lib

    lib = _lib.load()
    p = ct.c_void_p(256)   # never dereferenced: every call below fails validation first
    names = ("x", "ls", "u", "w", "N", "C", "nf", "nq", "cu", "cx", "a", "b", "block", "nl", "cov", "mean", "ws", "wsb", "st")
    good = dict(x=p, ls=4, u=p, w=None, N=10, C=4, nf=3, nq=3, cu=0.0, cx=p, a=p, b=p, block=2, nl=3, cov=p, mean=p, ws=p,
                wsb=1 << 30, st=None)

    def call(**bad):
        return lib.txm_influence_block_cross_cov(*[{**good, **bad}[n] for n in names])

    for ptr in ("x", "u", "cx", "a", "b", "cov", "mean", "ws"):
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
    assert call(block=0) == -1 and b"block" in lib.txm_last_error()
    assert call(block=-4) == -1 and b"block" in lib.txm_last_error()
    assert call(nl=0) == -1 and b"n_levels" in lib.txm_last_error()
    assert call(nl=33) == -1 and b"n_levels" in lib.txm_last_error()
    for N, C, nf, nq, block in [(10, 4, 3, 3, 2), (10**6, 33, 2, 9, 16)]:
        need = lib.txm_influence_block_cross_cov_ws_bytes(N, C, nf, nq, block, 3)
        assert call(N=N, C=C, ls=C, nf=nf, nq=nq, block=block, wsb=need - 1) == -3 and b"workspace" in lib.txm_last_error()


def test_symbols_bound_with_the_header_signature():
    """Both symbols are in the binding's table with the argument list include/txmom.h declares, and resolve in the
    library; the ABI version did not move."""
    from thermoextrap_amd import _lib

    text = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    ctype = {"int64_t": ct.c_int64, "int": ct.c_int, "double": ct.c_double, "size_t": ct.c_size_t, "txm_stream": ct.c_void_p}
    ret = {"size_t": ct.c_size_t, "int": ct.c_int}
    lib = _lib.load()
    for name in ("txm_influence_block_cross_cov_ws_bytes", "txm_influence_block_cross_cov"):
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


def _stub_model(order, out_dims, out_shape, coords, block, n, with_iid=False):
    """An ExtrapModel whose blocked device results are already in its cache: the level and label logic alone runs."""
    import torch

    from thermoextrap_amd import engine, models

    C = int(np.prod(out_shape))
    lengths, counts = engine.block_levels(n, block)
    rng = np.random.default_rng(3)
    g = rng.normal(size=(len(lengths), C * (order + 1), C * (order + 1)))
    cov = (g @ np.transpose(g, (0, 2, 1))).reshape(len(lengths), C, order + 1, C, order + 1)
    m = object.__new__(models.ExtrapModel)
    m.alpha0, m.order, m.minus_log, m.alpha_name = 0.5, order, False, "beta"
    m.data = None
    src = models._HostSource(out_dims, out_shape, coords, None)
    m._cache = {("dxcov_block", order, False, block, True): (torch.from_numpy(cov.copy()), src, lengths, counts),
                ("dxcov_block", order, False, block, False): (torch.from_numpy(cov[0].copy()), src, lengths, counts)}
    return m, cov, lengths, counts


def test_level_and_label_logic_on_a_stubbed_engine_call():
    from thermoextrap_amd.xrlite import DataArray

    order, block, n = 2, 7, 331
    coords = {"r": (("r",), np.array([0.5, 1.5, 2.5]))}
    m, cov, lengths, counts = _stub_model(order, ["r", "comp"], [3, 2], coords, block, n)
    keys = list(m._cache)
    nl = len(lengths)
    assert nl == 6 and list(lengths) == [7, 14, 28, 56, 112, 224] and list(counts) == [48, 24, 12, 6, 3, 2]

    V = m.derivs_cross_cov(block=block)
    assert V.dims == ("order", "order_2", "r", "comp", "r_2", "comp_2") and V.shape == (3, 3, 3, 2, 3, 2)
    c0 = cov[0].reshape(3, 2, order + 1, 3, 2, order + 1)                            # (r, comp, i, r', comp', j)
    assert np.array_equal(V.values, np.transpose(c0, (2, 5, 0, 1, 3, 4)))
    assert np.array_equal(V["r"].values, coords["r"][1]) and np.array_equal(V["r_2"].values, coords["r"][1])
    f = np.array([1.0, 1.0, 0.5])
    Vn = m.derivs_cross_cov(norm=True, block=block)
    np.testing.assert_allclose(Vn.values, V.values * f[:, None, None, None, None, None] * f[None, :, None, None, None, None],
                               rtol=1e-15)

    W, bl, nbk = m.cross_blocking_curve(block)
    assert W.dims == ("level", "order", "order_2", "r", "comp", "r_2", "comp_2") and W.shape == (nl, 3, 3, 3, 2, 3, 2)
    assert np.array_equal(bl, lengths) and np.array_equal(nbk, counts) and bl is not lengths and nbk is not counts
    assert np.array_equal(W["level"].values, lengths)
    assert np.array_equal(W["r"].values, coords["r"][1]) and np.array_equal(W["r_2"].values, coords["r"][1])
    for l in range(nl):
        cl = cov[l].reshape(3, 2, order + 1, 3, 2, order + 1)
        assert np.array_equal(W.values[l], np.transpose(cl, (2, 5, 0, 1, 3, 4))), l
    Wn, _, _ = m.cross_blocking_curve(block, norm=True)
    np.testing.assert_allclose(Wn.values, W.values * f[None, :, None, None, None, None, None]
                               * f[None, None, :, None, None, None, None], rtol=1e-15)

    sentinel = object()
    m.predict = lambda alpha, **kw: sentinel
    alphas = np.array([0.3, 0.5, 0.62, 0.7])
    pred, pc = m.predict_cov(alphas, block=block)
    assert pred is sentinel and isinstance(pc, DataArray)
    assert pc.dims == ("beta", "r", "comp", "r_2", "comp_2") and pc.shape == (4, 3, 2, 3, 2)
    for k, al in enumerate(alphas):
        t = np.array([(al - 0.5) ** i / math.factorial(i) for i in range(order + 1)])
        ref = np.einsum("i,cidj,j->cd", t, cov[0], t).reshape(3, 2, 3, 2)
        np.testing.assert_allclose(pc.values[k], ref, rtol=1e-13, atol=1e-13 * np.abs(ref).max())
    assert np.array_equal(pc.values[1].reshape(6, 6), cov[0][:, 0, :, 0])            # alpha0 itself: the covariance of the means
    # the blocked path neither reads nor writes the iid entries
    assert list(m._cache) == keys and not any(k[0] in ("dxcov", "dcov", "dcov_block") for k in m._cache)


def test_block_argument_is_checked_before_anything_else():
    """TypeError for a non-integer block comes from _check_block_type, before the operands are looked at."""
    import pytest

    from thermoextrap_amd import models

    m = object.__new__(models.ExtrapModel)
    m.alpha0, m.order, m.minus_log, m.alpha_name, m.data, m._cache = 0.5, 2, False, "beta", None, {}
    for bad in (7.0, "7", True, [7], np.float64(7)):
        with pytest.raises(TypeError):
            m.derivs_cross_cov(block=bad)
        with pytest.raises(TypeError):
            m.cross_blocking_curve(bad)
        with pytest.raises(TypeError):
            m.predict_cov(0.6, block=bad)


def test_definition_on_correlated_ar1_columns_in_numpy():
    """The numpy restatement of the definition at order 0 on the AR(1) columns of tests/_block_cross_ref.py, seed 0,
    N = 2^20, B = 1024: every entry of V within 0.25 * 19 sqrt(Sigma_cc Sigma_c'c') / N of 19 Sigma / N; the iid entry
    (block = 1) of columns 0, 1 is 1 / 19 of the target within 5 %."""
    u, x = ar1_columns(0)
    target, scale = ar1_scale()
    V = blocked_means_cov(x, AR1_BLOCK)
    dev = np.abs(V - target) / scale
    d = np.sqrt(np.diag(V))
    corr = V / np.outer(d, d)
    iid = blocked_means_cov(x, 1)[0, 1] / target[0, 1]
    print(f"numpy, seed 0: worst |V - 19 Sigma / N| / scale = {dev.max():.4f}; blocked correlations {corr[0, 1]:.4f}, "
          f"{corr[0, 2]:.4f}; iid / target = {iid:.4f}")
    assert (dev <= AR1_LIMIT).all()
    assert abs(iid - 1.0 / 19.0) <= 0.05 / 19.0
