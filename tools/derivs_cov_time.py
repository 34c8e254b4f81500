"""Delta-method error bars on the device, timed next to what they stand beside:

  (a) txm_influence_cov (engine.influence_cov) and txm_reduce_vals (engine.reduce_vals) on the same operands -- both read
      the sample matrix once: 8 N (C + 1) bytes (+ 8 N with weights);
  (b) gpr_input.input_GP_from_state(state, method="delta") and the same call with method="bootstrap", n_rep replicates on
      the device sampler, on one ExtrapModel over DataCentralMomentsVals.

    python tools/derivs_cov_time.py                       # N = 1e8, C = 32, order 4, n_rep = 100
    python tools/derivs_cov_time.py --n 1e6 --reps 3      # a quick look

One JSON line per measurement.  Times are host clocks around work that ends in a device synchronise; the arms of a comparison
alternate inside one process, after one warm-up call each; median and minimum over --reps rounds.  Bytes are what the
algorithm needs, computed from the shapes.  The data is bench.py's synthetic state point.
"""

from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def _alternate(arms: dict, reps: int) -> dict:
    """{name: [ms, ...]}: one warm-up call of every arm, then `reps` rounds, each running every arm once."""
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    out = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out[k].append((time.perf_counter() - t0) * 1e3)
    return out


def _stats(ts):
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e8)
    ap.add_argument("--c", type=int, default=32)
    ap.add_argument("--order", type=int, default=4)
    ap.add_argument("--nrep", type=int, default=100)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-api", action="store_true", help="only (a), the two kernels")
    args = ap.parse_args()

    import bench
    import thermoextrap_amd as txa
    from thermoextrap_amd import _build, engine, gpr_input
    from thermoextrap_amd.moments import DeviceDataArray

    txa.require_gpu()
    N, C, order = int(args.n), args.c, args.order
    x, u = bench.make_data(N, C, seed=1000, torch=torch)
    g = torch.Generator(device="cuda").manual_seed(7)
    w = torch.empty(N, dtype=torch.float64, device="cuda").uniform_(0.5, 1.5, generator=g)
    base = {"N": N, "C": C, "order": order, "csrc_sha": _build.csrc_sha(), "device": torch.cuda.get_device_name()}

    # ---- (a) the two kernels on the same operands ------------------------------------------------------------------------
    st = engine.reduce_vals(x, u, order)
    cu, cx = float(st[0, 0, 1]), st[:, 1, 0].contiguous()
    gen = torch.Generator(device="cuda").manual_seed(11)
    a = torch.randn((C, order + 1, order + 1), dtype=torch.float64, device="cuda", generator=gen)
    b = torch.randn((C, order + 1, order + 1), dtype=torch.float64, device="cuda", generator=gen)
    for weights, tag in ((None, "unweighted"), (w, "weighted")):
        ts = _alternate({"reduce_vals": lambda: engine.reduce_vals(x, u, order, w=weights),
                         "influence_cov": lambda: engine.influence_cov(x, u, a, b, cu, cx, w=weights)}, args.reps)
        nbytes = 8 * N * (C + 1 + (weights is not None))
        rec = {**base, "what": "kernels", "weights": tag, "bytes": nbytes}
        for k, v in ts.items():
            s = _stats(v)
            rec[k] = {**s, "TBs_at_median": round(nbytes / s["median_ms"] * 1e-9, 3)}
        rec["influence_over_reduce_median"] = round(rec["influence_cov"]["median_ms"] / rec["reduce_vals"]["median_ms"], 3)
        print(json.dumps(rec), flush=True)

    # ---- (b) the GP input of one state: delta method next to the bootstrap -------------------------------------------------
    if not args.skip_api:
        data = txa.DataCentralMomentsVals.from_vals(xv=DeviceDataArray(x, ("rec", "val")), uv=DeviceDataArray(u, ("rec",)),
                                                    order=order, central=True)
        seeds = iter(range(1, 1 << 30))

        def fresh():   # a model without cached derivatives or covariance, as a caller's first call sees it
            return txa.beta.factory_extrapmodel(5.6, data)

        ts = _alternate({
            "bootstrap": lambda: gpr_input.input_GP_from_state(fresh(), sampler={"nrep": args.nrep, "device": True,
                                                                                   "seed": next(seeds)}),
            "delta": lambda: gpr_input.input_GP_from_state(fresh(), method="delta"),
        }, max(3, args.reps // 2))
        rec = {**base, "what": "input_GP_from_state", "n_rep": args.nrep}
        for k, v in ts.items():
            rec[k] = _stats(v)
        rec["bootstrap_over_delta_median"] = round(rec["bootstrap"]["median_ms"] / rec["delta"]["median_ms"], 2)
        xb, yb, cb = gpr_input.input_GP_from_state(fresh(), sampler={"nrep": args.nrep, "device": True, "seed": 1})
        xd, yd, cd = gpr_input.input_GP_from_state(fresh(), method="delta")
        import numpy as np

        sd_b, sd_d = np.sqrt(np.einsum("kii->ki", cb)), np.sqrt(np.einsum("kii->ki", cd))
        rec["std_bootstrap_over_delta_by_order_median_over_columns"] = [round(float(v), 3) for v in np.median(sd_b / sd_d, axis=0)]
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
