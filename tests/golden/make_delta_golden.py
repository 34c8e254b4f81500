"""Writes tests/golden/delta_parent.npz: inputs and outputs of the delta-method error bars through the PUBLIC model API --
derivs_cov, derivs_cross_cov, their block= forms and blocking curves, predict_with_error / predict_cov of ExtrapModel,
ExtrapWeightedModel, InterpModel and InterpModelPiecewise, StateCollection on its batched and loop paths, gpr_input with
method="delta" -- on the smallest shapes that reach each kernel and each host path.  Run once on an MI355X with the build
BEFORE the host code of these forms was folded onto shared helpers (`python tests/golden/make_delta_golden.py`);
tests/test_delta_golden_gpu.py holds every later build to these bits, dims and coordinate values -- neither the kernels,
their launch plans nor the order of the host arithmetic are to change.  The plans depend on the device's CU count: record
and check on the same kind of device.  Do not regenerate it to make that test pass."""

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
BETAS = (0.4, 0.5, 0.6)
ALPHAS3 = [0.45, 0.5, 0.56]                    # ExtrapModel.predict_*
ALPHAS_IN = [0.43, 0.58]                       # inside the first and the second interval of BETAS


def make_inputs():
    rng = np.random.default_rng(20261020)

    def gas(name, N, C, weighted=False):
        u = rng.normal(174.85, 5.31, N)
        x = rng.uniform(1.0, 2.0, C)[None, :] + rng.normal(1e-3, 5e-4, C)[None, :] * u[:, None] + rng.normal(0, 0.05, (N, C))
        d["in_x_" + name], d["in_u_" + name] = x, u
        if weighted:
            w = rng.uniform(0.5, 1.5, N)
            w[rng.random(N) < 0.1] = 0.0
            d["in_w_" + name] = w

    d = {}
    gas("c1", 301, 1)                  # the series kernel
    gas("c3", 517, 3)                  # row-major, one column per lane; block=4: a short last block, several levels
    gas("c4w", 1100, 4, True)          # two columns per lane, several workgroups, some zero weights
    gas("c3t", 301, 3)                 # handed over as (val, rec): the column-major kernel
    gas("c17w", 600, 17, True)         # cross: two tiles a side, three tile pairs
    gas("c5", 517, 5)                  # cross, norm / blocked / predictions
    for s, n in enumerate((301, 517, 1000)):
        gas(f"s{s}", n, 4)             # three ragged states
    return d


def _model(txm, d, name, beta=0.5, order=3, model_order=None, minus_log=False, transposed=False):
    DA = txm.DataArray
    x, u, w = d["in_x_" + name], d["in_u_" + name], d.get("in_w_" + name)
    if x.shape[1] == 1:
        xv = DA(np.ascontiguousarray(x[:, 0]), ("rec",))
    elif transposed:
        xv = DA(np.ascontiguousarray(x.T), ("val", "rec"), coords={"val": 0.5 * np.arange(x.shape[1])})
    else:
        xv = DA(np.array(x), ("rec", "val"), coords={"val": 0.5 * np.arange(x.shape[1])})
    data = txm.DataCentralMomentsVals.from_vals(xv=xv, uv=DA(np.array(u), ("rec",)), order=order, central=True,
                                                weight=None if w is None else DA(np.array(w), ("rec",)))
    m = txm.beta.factory_extrapmodel(beta=beta, data=data, order=model_order)
    return m.new_like(minus_log=True) if minus_log else m


def _states(txm, d, model_orders=(None, None, None)):
    """Fresh states: nothing cached, so every case takes the path its name says."""
    return [_model(txm, d, f"s{s}", beta=BETAS[s], order=2 if model_orders[s] is None else 3, model_order=model_orders[s])
            for s in range(3)]


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


def compute(txm, d):
    from thermoextrap_amd import gpr_input as G

    out = {}
    M = lambda name, **kw: _model(txm, d, name, **kw)  # noqa: E731
    # ---- ExtrapModel.derivs_cov: the four per-column kernels
    _put(out, "dcov_c1", M("c1").derivs_cov())
    _put(out, "dcov_c3", M("c3").derivs_cov(order=2))
    _put(out, "dcov_c4w_norm_mlog", M("c4w", minus_log=True).derivs_cov(norm=True))
    _put(out, "dcov_c3t", M("c3t", transposed=True).derivs_cov())
    # ---- blocked
    m = M("c3")
    _put(out, "dcov_c3_block4", m.derivs_cov(block=4))
    _put(out, "curve_c3_block4", m.blocking_curve(4))
    # ---- across columns
    _put(out, "dxcov_c17w", M("c17w").derivs_cross_cov())
    _put(out, "dxcov_c5_norm", M("c5").derivs_cross_cov(order=2, norm=True))
    m = M("c5", order=2)
    _put(out, "dxcov_c5_block4", m.derivs_cross_cov(block=4))
    _put(out, "xcurve_c5_block4", m.cross_blocking_curve(4))
    # ---- ExtrapModel predictions
    m = M("c5")
    _put(out, "extrap_with_error", m.predict_with_error(ALPHAS3))
    _put(out, "extrap_cov", m.predict_cov(ALPHAS3))
    # ---- collections: batched, blocked loop, ineligible loop
    _put(out, "states_dcov", txm.StateCollection(_states(txm, d)).derivs_cov())
    _put(out, "states_dxcov", txm.StateCollection(_states(txm, d)).derivs_cross_cov())
    _put(out, "states_dcov_blocks", txm.StateCollection(_states(txm, d)).derivs_cov(block=[2, 4, 8]))
    odd = (3, 2, 3)
    assert txm.StateCollection(_states(txm, d, odd))._delta_batch_eligible() is None
    _put(out, "loop_dcov", txm.StateCollection(_states(txm, d, odd)).derivs_cov(order=2))
    _put(out, "loop_dxcov", txm.StateCollection(_states(txm, d, odd)).derivs_cross_cov(order=2))
    # ---- the multi-state models, iid and blocked
    for tag, block in (("", None), ("_block4", 4)):
        wm = txm.ExtrapWeightedModel(_states(txm, d))
        _put(out, "weighted_with_error" + tag, wm.predict_with_error(ALPHAS_IN, block=block))
        _put(out, "weighted_cov" + tag, wm.predict_cov(ALPHAS_IN, block=block))
        im = txm.InterpModel(_states(txm, d))
        _put(out, "interp_with_error" + tag, im.predict_with_error(ALPHAS_IN, block=block))
        _put(out, "interp_cov" + tag, im.predict_cov(ALPHAS_IN, block=block))
        pw = txm.InterpModelPiecewise(_states(txm, d))
        _put(out, "piecewise_with_error_scalar" + tag, pw.predict_with_error(0.47, block=block))
        _put(out, "piecewise_with_error" + tag, pw.predict_with_error(ALPHAS_IN, block=block))
        _put(out, "piecewise_cov_scalar" + tag, pw.predict_cov(0.47, block=block))
        _put(out, "piecewise_cov" + tag, pw.predict_cov(ALPHAS_IN, block=block))
    # ---- gpr_input
    _put(out, "gp_state", G.input_GP_from_state(M("c3"), method="delta"))
    _put(out, "gp_states", G.input_GP_from_states(txm.StateCollection(_states(txm, d)), method="delta"))
    return out


if __name__ == "__main__":
    sys.path.insert(0, str(HERE.parent.parent))
    import thermoextrap_amd as txa

    txa.require_gpu()
    d = make_inputs()
    res = compute(txa, d)
    bad = [k for k, v in res.items() if v.dtype.kind == "f" and not np.isfinite(v).all()]
    assert not bad, bad
    dest = Path(sys.argv[1]) if len(sys.argv) > 1 else HERE / "delta_parent.npz"
    np.savez_compressed(dest, **d, **res)
    print("wrote", dest, len(res), "entries")
