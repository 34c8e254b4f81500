"""Writes tests/golden/mbar_parent.npz: inputs and outputs of every MBAR pass over the pooled samples -- the engine's
mbar_eval, mbar_predict, mbar_gram, mbar_cov_sums, mbar_cross_cov_sums, mbar_block_gamma, mbar_hist_sums, mbar_boot_eval
and mbar_bootstrap_predict at a PINNED solution (f and the pivot are inputs, nothing is re-solved), and MBARModel /
MBARBootstrap through their public methods -- on the smallest shapes that reach each kernel and each host path.  Run once
on an MI355X with the build BEFORE the target passes were folded onto one host path and the entry points onto one
preamble (`python tests/golden/make_mbar_golden.py`); tests/test_mbar_golden_gpu.py holds every later build to these
bits, dims and coordinate values -- neither the kernels, their launch plans, the bytes handed to a call nor the order of
the host arithmetic are to change.  The plans depend on the device's CU count: record and check on the same kind of
device.  Do not regenerate it to make that test pass.

`--check-inputs` (no device): the assertions that the inputs are what this text says they are.  `--drop a,b,...`: model-
level entries (never engine-level ones, never dims or coordinates) that the recording build itself does not reproduce bit
for bit in a second process are left out of the file; the test then does not compare their values."""

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
WIDE = 19                                       # columns of the stored x: C = 17 is a slice of it, row pitch 19 > 17
NS = {"k3": [1, 50, 700],                       # one sample; less than a 64-sample tile; several tiles, a ragged last one
      "k9": [40, 300, 64, 129, 65, 77, 130, 41, 113],
      "k17": [40, 300, 64, 129, 65, 77, 41, 113, 50, 63, 90, 45, 70, 128, 55, 100, 48]}
TARGETS = {1: [1.13], 2: [0.97, 1.21], 3: [1.02, 1.1, 1.33], 5: [0.95, 1.0, 1.08, 1.2, 1.4],
           11: [0.9, 0.95, 1.0, 1.05, 1.1, 1.15, 1.2, 1.25, 1.3, 1.35, 1.4]}
NBINS = (1, 16, 40)
BLOCKS_K3 = [1000, 16, 5]                       # per state: longer than its state (1), shorter, shorter
NREP = 5
# (collection, C, number of targets, blocks of mbar_block_gamma): every n_alpha class {1, 2, 4, 8} of every kernel, a
# second 8-target pass of 3 (11 = 8 + 3), the register (K = 3) and the LDS kernels (K = 9, 17), one and two row tiles
CASES = [("k3", 1, 11, (1, 7, BLOCKS_K3)), ("k3", 17, 2, (7, BLOCKS_K3)), ("k3", 1, 1, (7,)),
         ("k9", 17, 3, (7,)), ("k9", 1, 5, (1, 7)),
         ("k17", 1, 2, (1, 7)), ("k17", 17, 1, (7,)), ("k17", 17, 5, ())]
BOOT_CASES = [("k9", 1, 5), ("k17", 17, 11)]    # (collection, C, number of targets)
N_LEVELS = 3


def alpha0_of(K):
    return 0.9 + 0.5 * np.arange(K) / max(K - 1, 1)


def host_solve(us, a0, iters=400):
    """MBAR free energies by the self-consistent iteration in numpy (gauge f_0 = 0): close to the solution, which is all
    the pinned engine-level calls need -- they take any f."""
    u = np.concatenate(us)
    lnN = np.log([len(v) for v in us])
    f = np.zeros(len(us))
    for _ in range(iters):
        t = lnN[None, :] + f[None, :] - u[:, None] * a0[None, :]
        m = t.max(axis=1)
        logD = m + np.log(np.exp(t - m[:, None]).sum(axis=1))
        e = -u[:, None] * a0[None, :] - logD[:, None]
        mm = e.max(axis=0)
        f = -(mm + np.log(np.exp(e - mm[None, :]).sum(axis=0)))
        f = f - f[0]
    return f


def make_inputs():
    rng = np.random.default_rng(20261021)
    d = {}
    for name, ns in NS.items():
        a0 = alpha0_of(len(ns))
        us = []
        for k, n in enumerate(ns):
            # (multiples of 2^-10: the stored inputs compress, the arithmetic on them is no different)
            u = np.round(rng.normal(10.0 - 2.25 * a0[k], 1.5, n) * 1024) / 1024
            x = np.round((np.linspace(1.0, 2.0, WIDE)[None, :] + 0.05 * u[:, None] + rng.normal(0, 0.1, (n, WIDE))) * 1024) / 1024
            d[f"in_u_{name}_{k}"], d[f"in_x_{name}_{k}"] = u, x
            us.append(u)
        d[f"in_f_{name}"] = host_solve(us, a0)
        d[f"in_upiv_{name}"] = np.float64(np.concatenate(us).sum() / sum(ns))
    # integer order parameter of the K = 3 states for histogram(values=[...], bins=5, range=None): -1 and 5 are outside
    for k, n in enumerate(NS["k3"]):
        d[f"in_cls_k3_{k}"] = rng.integers(-1, 6, n).astype(np.int64)
    return d


def check_inputs(d):
    """What the header says of the shapes, asserted on the host: no kernel runs."""
    tile, tile16 = 64, 16
    assert NS["k3"] == [1, 50, 700] and 50 < tile and 700 > 2 * tile and 700 % tile != 0
    for name, K in (("k9", 9), ("k17", 17)):
        assert len(NS[name]) == K and min(NS[name]) >= 40 and max(NS[name]) <= 300
    assert 3 <= 8 < 9 <= 16 < 17 <= 32                       # register kernel; LDS kernels of 16 and of 32 states
    assert 9 // 16 + 1 == 1 and 17 // 16 + 1 == 2            # row tiles of txm_mbar_cov
    assert (9 + 2 + 15) // 16 == 1 and (17 + 2 + 15) // 16 == 2   # row tiles of txm_mbar_hist
    assert 17 // tile16 + 1 == 2 and 17 % 2 == 1 and (17 + 15) // 16 == 2 and WIDE > 17   # column groups / tiles, odd, pitch
    for name, ns in NS.items():
        for k, n in enumerate(ns):
            x, u = d[f"in_x_{name}_{k}"], d[f"in_u_{name}_{k}"]
            assert x.shape == (n, WIDE) and u.shape == (n,) and x.dtype == u.dtype == np.float64
            s = x[:, :17]
            assert s.shape == (n, 17) and s.strides[0] == WIDE * 8 and (n == 1 or not s.flags["C_CONTIGUOUS"])
        assert d[f"in_f_{name}"].shape == (len(ns),) and d[f"in_f_{name}"][0] == 0.0 and np.isfinite(d[f"in_f_{name}"]).all()
        assert np.isfinite(d[f"in_upiv_{name}"])
    cls = lambda n: 1 if n <= 1 else 2 if n <= 2 else 4 if n <= 4 else 8   # noqa: E731
    assert sorted(TARGETS) == [1, 2, 3, 5, 11] and all(len(v) == n for n, v in TARGETS.items())
    for kernel_cases in ([c for c in CASES], [c for c in CASES if c[3]], [c for c in CASES if c[2] <= 8]):
        seen = set()
        for _, _, na, _ in kernel_cases:
            seen |= {cls(min(8, na - i0)) for i0 in range(0, na, 8)}
        assert seen == {1, 2, 4, 8}, seen                    # cov / hist / predict; block; cross_alpha
    assert any(na == 11 for _, _, na, _ in CASES) and 11 - 8 == 3
    assert {(c[0], c[1]) for c in CASES} == {(k, C) for k in NS for C in (1, 17)}
    assert NBINS == (1, 16, 40) and [nb // 16 + 1 for nb in NBINS] == [1, 2, 3]
    assert any(b > n for b, n in zip(BLOCKS_K3, NS["k3"])) and any(b < n for b, n in zip(BLOCKS_K3, NS["k3"]))
    blocks = {repr(b) for c in CASES for b in c[3]}
    assert blocks == {"1", "7", repr(BLOCKS_K3)} and all(c[0] == "k3" for c in CASES if BLOCKS_K3 in c[3])
    assert N_LEVELS == 3 and NREP == 5
    for k, n in enumerate(NS["k3"]):
        c = d[f"in_cls_k3_{k}"]
        assert c.shape == (n,) and c.dtype == np.int64 and c.min() >= -1 and c.max() <= 5
    return True


def _put(out, name, res):
    """A labelled result as values + dims + one entry per coordinate; arrays and tuples of them by position."""
    if isinstance(res, (tuple, list)):
        for i, r in enumerate(res):
            _put(out, f"{name}.{i}", r)
    elif hasattr(res, "dims") and hasattr(res, "_coords"):
        out["out_" + name] = np.asarray(res.values)
        out["dims_" + name] = np.array([str(k) for k in res.dims])
        for k, (cd, cv) in res._coords.items():
            out[f"coord_{name}__{k}"] = np.asarray(cv)
            out[f"cdims_{name}__{k}"] = np.array([str(c) for c in cd], dtype=str)
    else:
        out["out_" + name] = np.asarray(res)


def _collection(d, name):
    K = len(NS[name])
    return [np.array(d[f"in_u_{name}_{k}"]) for k in range(K)], [np.array(d[f"in_x_{name}_{k}"]) for k in range(K)]


def compute_engine(d):
    """out_e_*: every array the engine's MBAR calls return at the pinned solution."""
    import torch

    from thermoextrap_amd import engine

    out = {}
    dev = {}
    for name in NS:
        us, xs = _collection(d, name)
        K = len(us)
        a0 = alpha0_of(K)
        ud = [torch.as_tensor(u).cuda() for u in us]
        xw = [torch.as_tensor(x).cuda() for x in xs]
        ns = np.array([len(u) for u in us], dtype=np.float64)
        f, upiv = np.array(d[f"in_f_{name}"]), float(d[f"in_upiv_{name}"])
        logD = torch.empty(int(ns.sum()), dtype=torch.float64, device="cuda")
        stub = engine.MbarSolution(f, logD, upiv, 0, 0, 0.0)
        g, _ = engine.mbar_solution_g(ns, a0, stub)
        _put(out, f"e_eval_{name}", engine.mbar_eval(ud, a0, g, upiv, logD))
        out[f"out_e_logD_{name}"] = logD.cpu().numpy()
        _put(out, f"e_eval_nolog_{name}", engine.mbar_eval(ud, a0, g, upiv))
        _put(out, f"e_gram_{name}", engine.mbar_gram(ud, a0, stub))
        dev[name] = (ud, xw, a0, stub)
    for name, C, na, blocks in CASES:
        ud, xw, a0, sol = dev[name]
        xs = [x[:, 0].contiguous() for x in xw] if C == 1 else [x[:, :C] for x in xw]     # C = 17: pitch WIDE
        al = TARGETS[na]
        tag = f"{name}_c{C}_a{na}"
        means = engine.mbar_predict(xs, ud, a0, sol.f, sol.logD, al, upiv=sol.upiv)
        out[f"out_e_predict_{tag}"] = means.cpu().numpy()
        _put(out, f"e_cov_{tag}", engine.mbar_cov_sums(xs, ud, a0, sol, al, means))
        _put(out, f"e_cov_lnw_{tag}", engine.mbar_cov_sums(xs, ud, a0, sol, al, means, with_lnw=True))
        _put(out, f"e_xcov_{tag}", engine.mbar_cross_cov_sums(xs, ud, a0, sol, al, means))
        if na <= 8:
            _put(out, f"e_xcov_cross_{tag}", engine.mbar_cross_cov_sums(xs, ud, a0, sol, al, means, cross_alpha=True))
        for b, block in enumerate(blocks):
            res = engine.mbar_block_gamma(xs, ud, a0, sol, al, means, block, n_levels=N_LEVELS)
            _put(out, f"e_block{b}_{tag}", [*res.gamma, res.nblocks, res.b, res.B, res.lnw])
        for nb in NBINS:
            idx = [((u - float(u.min())) * (nb + 1.5) / 9.0).floor().to(torch.int32) - 1 for u in ud]    # some outside
            _put(out, f"e_hist{nb}_{tag}", engine.mbar_hist_sums(idx, ud, a0, sol, al, nb))
    for name, C, na in BOOT_CASES:
        ud, xw, a0, sol = dev[name]
        K = len(ud)
        xs = [x[:, 0].contiguous() for x in xw] if C == 1 else [x[:, :C] for x in xw]
        samplers = [engine.DeviceSampler(1234, NREP, int(u.shape[0]), rep0=s * NREP) for s, u in enumerate(ud)]
        ns = np.array([u.shape[0] for u in ud], dtype=np.float64)
        g0, _ = engine.mbar_solution_g(ns, a0, sol)
        shift = 0.01 * np.arange(NREP)[:, None] * np.arange(K)[None, :] / K
        _put(out, f"e_boot_eval_{name}", engine.mbar_boot_eval(ud, a0, samplers, g0[None, :] + shift, sol.upiv))
        _put(out, f"e_boot_eval_active_{name}", engine.mbar_boot_eval(ud, a0, samplers, g0[None, :] + shift, sol.upiv,
                                                                      active=[3, 0]))
        res = engine.mbar_bootstrap_predict(xs, ud, a0, samplers, np.asarray(sol.f)[None, :] + shift, sol, TARGETS[na])
        out[f"out_e_boot_predict_{name}_c{C}_a{na}"] = res.cpu().numpy()
    return out


def _model(txm, d, name, C):
    from thermoextrap_amd.data import xrwrap_uv, xrwrap_xv

    us, xs = _collection(d, name)
    a0 = alpha0_of(len(us))
    states = []
    for k, (u, x) in enumerate(zip(us, xs)):
        xv = xrwrap_xv(np.ascontiguousarray(x[:, 0] if C == 1 else x[:, :C]))
        data = txm.DataCentralMomentsVals.from_vals(xv=xv, uv=xrwrap_uv(u), order=1, central=True) if k % 2 == 1 else \
            txm.factory_data_values(uv=xrwrap_uv(u), xv=xv, order=1, central=False)
        states.append(txm.beta.factory_extrapmodel(beta=a0[k], data=data))
    return txm.MBARModel(states)


def _put_hist(out, name, h):
    _put(out, name, [h.p, h.std, h.outside, h.n_eff])
    out[f"out_{name}.edges"] = np.asarray(h.edges)
    if h.cov is not None:
        _put(out, name + ".cov", h.cov)


def compute_model(txm, d):
    """out_m_*: MBARModel and MBARBootstrap through their public methods (these solve for themselves)."""
    out = {}
    m3, m9, m17 = _model(txm, d, "k3", 17), _model(txm, d, "k9", 1), _model(txm, d, "k17", 17)
    A = TARGETS
    _put(out, "m_predict_k9", m9.predict(A[11]))
    _put(out, "m_predict_scalar_k3", m3.predict(1.07))
    _put(out, "m_with_error_k3", m3.predict_with_error(A[3]))
    _put(out, "m_with_error_block7_k3", m3.predict_with_error(A[3], block=7))
    _put(out, "m_with_error_blocks_k3", m3.predict_with_error(A[3], block=BLOCKS_K3))
    _put(out, "m_with_error_k17", m17.predict_with_error(A[5]))
    _put(out, "m_with_error_block7_k9", m9.predict_with_error(A[11], block=7))
    _put(out, "m_curve_k3", m3.blocking_curve(A[2], 7))
    _put(out, "m_curve_k9", m9.blocking_curve(A[11], [3] * 9, alpha_name="b"))
    _put(out, "m_with_cov_k3", m3.predict_with_covariance(A[2]))
    _put(out, "m_with_cov_cross_k3", m3.predict_with_covariance(A[2], cross_alpha=True))
    _put(out, "m_with_cov_block7_k3", m3.predict_with_covariance(A[2], block=7))
    _put(out, "m_with_cov_cross_block7_k9", m9.predict_with_covariance(A[3], cross_alpha=True, block=7))
    _put_hist(out, "m_hist_u_k3", m3.histogram(A[2], 16, values="u"))
    _put_hist(out, "m_hist_col_k3", m3.histogram(A[3], 40, values=3, cov=False))
    _put_hist(out, "m_hist_int_k3", m3.histogram(A[1], 5, values=[np.array(d[f"in_cls_k3_{k}"]) for k in range(3)]))
    h = m9.histogram(A[11], np.linspace(2.0, 12.0, 17), values="u")
    _put_hist(out, "m_hist_edges_k9", h)
    _put(out, "m_hist_free_energy_k9", h.free_energy(reference="max"))
    _put(out, "m_free_energy_k3", m3.free_energy())
    _put(out, "m_free_energy_targets_k3", m3.free_energy(A[3]))
    _put(out, "m_free_energy_targets_block7_k3", m3.free_energy(A[3], block=7))
    _put(out, "m_free_energy_block7_k3", m3.free_energy(block=7))
    _put(out, "m_free_energy_targets_k9", m9.free_energy(A[11], alpha_name="b"))
    _put(out, "m_free_energy_targets_blocks_k9", m9.free_energy(A[11], block=7))
    _put(out, "m_fe_cov_k3", m3.free_energy_covariance())
    _put(out, "m_fe_cov_block7_k3", m3.free_energy_covariance(block=7))
    _put(out, "m_fe_cov_k17", m17.free_energy_covariance())
    ov = m3.overlap()
    _put(out, "m_overlap_k3", [ov.matrix, ov.eigenvalues, np.float64(ov.scalar)])
    ov = m17.overlap()
    _put(out, "m_overlap_k17", [ov.matrix, ov.eigenvalues, np.float64(ov.scalar)])
    _put(out, "m_n_eff_k3", m3.effective_samples(A[3]))
    _put(out, "m_n_eff_k9", m9.effective_samples(A[11]))
    boot = m9.bootstrap({"nrep": NREP, "seed": 11})
    out["out_m_boot_f_k9"] = np.asarray(boot.f)
    _put(out, "m_boot_predict_k9", boot.predict(A[2]))
    _put(out, "m_boot_predict_k17", m17.bootstrap({"nrep": NREP, "seed": 5, "rep_dim": "r"}).predict(1.1))
    return out


def compute(txm, d):
    return {**compute_engine(d), **compute_model(txm, d)}


if __name__ == "__main__":
    sys.path.insert(0, str(HERE.parent.parent))
    args = [a for a in sys.argv[1:]]
    d = make_inputs()
    assert check_inputs(d)
    if "--check-inputs" in args:
        print("inputs ok:", len(d), "arrays,", sum(v.nbytes for v in d.values()), "bytes")
        sys.exit(0)
    drop = []
    if "--drop" in args:
        drop = [k for k in args[args.index("--drop") + 1].split(",") if k]
        del args[args.index("--drop"):args.index("--drop") + 2]
    import thermoextrap_amd as txa

    txa.require_gpu()
    res = compute(txa, d)
    bad = [k for k, v in res.items() if v.dtype.kind == "f" and not np.isfinite(v).all() and "hist_free_energy" not in k]
    assert not bad, bad
    assert all(k.startswith("out_m_") for k in drop) and all(k in res for k in drop), drop
    assert 5 * len(drop) <= sum(k.startswith("out_m_") for k in res), "at most a fifth of the model-level values may be dropped"
    for k in drop:
        del res[k]
    dest = Path(args[0]) if args else HERE / "mbar_parent.npz"
    np.savez_compressed(dest, **d, **res)
    print("wrote", dest, len(res), "entries,", dest.stat().st_size, "bytes")
