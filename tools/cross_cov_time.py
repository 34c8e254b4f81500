"""The cross-column delta-method covariance on the device, timed next to what it stands beside, on the
same operands -- one ExtrapModel over DataCentralMomentsVals, its own influence coefficients:

  cross_cov      txm_influence_cross_cov (engine.influence_cross_cov): every block of the (C n_f)^2 matrix;
  influence_cov  txm_influence_cov (engine.influence_cov): the C diagonal blocks alone;
  bootstrap      the route to the same matrix without it: resample(nrep) on the device sampler -> derivs() -> covariance
                 over the replicates on the host.

    python tools/cross_cov_time.py                                  # N = 1e8, C = 32, order 4, nrep = 1000, unweighted
    python tools/cross_cov_time.py --weighted                       # the same with weights
    python tools/cross_cov_time.py --n 1e6 --c 4 31 32 33           # what the padding to tiles of 16 costs
    python tools/cross_cov_time.py --skip-bootstrap --reps 3        # a quick look

One JSON line per (C, weights).  Times are host clocks around work that ends in a device synchronise; the arms alternate
inside one process, after one warm-up call each; median and minimum over --reps rounds.  Bytes are what the algorithm
needs, computed from the shapes; the FMA count is the matrix pipe's, padding included: tile pairs * (2 n_q - 1) * 256 per
sample.  The data is bench.py's synthetic state point.
"""

from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
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
    ap.add_argument("--c", type=int, nargs="+", default=[32])
    ap.add_argument("--order", type=int, default=4)
    ap.add_argument("--nrep", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--weighted", action="store_true")
    ap.add_argument("--skip-bootstrap", action="store_true")
    args = ap.parse_args()

    import bench
    import thermoextrap_amd as txa
    from thermoextrap_amd import _build, engine
    from thermoextrap_amd.moments import DeviceDataArray

    txa.require_gpu()
    N, order = int(args.n), args.order
    nq = order + 1
    for C in args.c:
        x, u = bench.make_data(N, C, seed=1000, torch=torch)
        w = None
        if args.weighted:
            g = torch.Generator(device="cuda").manual_seed(7)
            w = torch.empty(N, dtype=torch.float64, device="cuda").uniform_(0.5, 1.5, generator=g)
        data = txa.DataCentralMomentsVals.from_vals(xv=DeviceDataArray(x, ("rec", "val")), uv=DeviceDataArray(u, ("rec",)),
                                                    order=order, central=True,
                                                    weight=None if w is None else DeviceDataArray(w, ("rec",)))
        model = txa.beta.factory_extrapmodel(5.6, data)
        x2, ut, wt, st, _ = model._delta_operands()
        a, b, um, xm = model._delta_coefs(st, order, False)
        a, b, xm = engine.to_device(a), engine.to_device(b), engine.to_device(xm)
        seeds = iter(range(1, 1 << 30))
        keep = {}

        def cross():
            keep["cross"] = engine.influence_cross_cov(x2, ut, a, b, um, xm, w=wt)

        def single():
            keep["single"] = engine.influence_cov(x2, ut, a, b, um, xm, w=wt)[0]

        def bootstrap():
            m = txa.beta.factory_extrapmodel(5.6, data)
            d = m.resample({"nrep": args.nrep, "device": True, "seed": next(seeds)}).derivs()
            v = d.transpose("rep", "val", "order").values.reshape(args.nrep, -1)
            keep["boot"] = np.cov(v, rowvar=False)

        arms = {"cross_cov": cross, "influence_cov": single}
        if not args.skip_bootstrap:
            arms["bootstrap"] = bootstrap
        ts = _alternate(arms, args.reps)
        T = (C + 1 + 15) // 16
        pairs = T * (T + 1) // 2
        nbytes = 8 * N * (C + 1 + (w is not None))
        fma = N * pairs * (2 * nq - 1) * 256
        rec = {"N": N, "C": C, "order": order, "weights": "weighted" if args.weighted else "unweighted", "reps": args.reps,
               "csrc_sha": _build.csrc_sha(), "device": torch.cuda.get_device_name(), "bytes": nbytes, "tiles_a_side": T,
               "tile_pairs": pairs, "matrix_fma": fma}
        for k, v in ts.items():
            rec[k] = _stats(v)
        s = rec["cross_cov"]["median_ms"]
        rec["cross_cov"]["TFLOPs_at_median"] = round(2 * fma / s * 1e-9, 2)
        rec["cross_cov"]["TBs_at_median"] = round(nbytes / s * 1e-9, 3)
        rec["influence_cov"]["TBs_at_median"] = round(nbytes / rec["influence_cov"]["median_ms"] * 1e-9, 3)
        rec["cross_over_single_median"] = round(s / rec["influence_cov"]["median_ms"], 2)
        V = keep["cross"].cpu().numpy().reshape(C * nq, C * nq)
        if "boot" in keep:
            rec["nrep"] = args.nrep
            rec["bootstrap_over_cross_median"] = round(rec["bootstrap"]["median_ms"] / s, 1)
            sd_v, sd_b = np.sqrt(np.diag(V)), np.sqrt(np.diag(keep["boot"]))
            rec["std_bootstrap_over_delta_median"] = round(float(np.median(sd_b / sd_v)), 3)
            cv, cb = V / np.outer(sd_v, sd_v), keep["boot"] / np.outer(sd_b, sd_b)
            rec["correlation_max_abs_difference"] = round(float(np.abs(cv - cb).max()), 3)
        print(json.dumps(rec), flush=True)
        del x, u, w, data, model, x2, ut, wt, keep


if __name__ == "__main__":
    main()
