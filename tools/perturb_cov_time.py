"""PerturbModel error bars on the device, timed next to what they stand beside:

  (a) --part kernels: on the same operands (N = 1e8, C = 32, 8 alphas by default)
        txm_perturb_cov, iid (block 1) and blocked (--block, default 1024, one level), the mean given;
        txm_perturb (engine.perturb), which reads the same 8 N (C + 1) bytes;
        the route there was before txm_perturb_cov: per alpha, torch ``exp`` into an N-vector of weights, then
        txm_influence_cov (n_f = n_q = 1, a = 0, b = 1, centre = the reweighted mean) with those weights -- one pass over
        x and one N-vector written and read PER ALPHA;
  (b) --part api: PerturbModel.predict_with_error next to resample(nrep) -> predict -> std over rep (N = 1e6 by default).

    python tools/perturb_cov_time.py --part kernels
    python tools/perturb_cov_time.py --part api --n 1e6

One JSON line per measurement.  Times are host clocks around work that ends in a device synchronise; the arms of a
comparison alternate inside one process, after one warm-up call each; median, minimum and the run-to-run spread (max - min,
standard deviation) over --reps rounds.  Bytes are what the algorithm needs, computed from the shapes.  The data is bench.py's
synthetic state point.  Run each part as a step of its own under a time limit.
"""

from __future__ import annotations

import argparse
import ctypes as ct
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

DA8 = [0.01, -0.01, 0.02, -0.02, 0.03, -0.03, 0.04, -0.04]   # |da| sigma_u <= 0.2: n_eff stays a large share of N


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
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4),
            "spread_ms": round(max(ts) - min(ts), 4), "stdev_ms": round(statistics.stdev(ts), 4) if len(ts) > 1 else 0.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("kernels", "api"), required=True)
    ap.add_argument("--n", type=float, default=None, help="default 1e8 (kernels) / 1e6 (api)")
    ap.add_argument("--c", type=int, default=32)
    ap.add_argument("--alphas", type=int, default=8)
    ap.add_argument("--block", type=int, default=1024)
    ap.add_argument("--nrep", type=int, default=100)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()

    import bench
    import thermoextrap_amd as txa
    from thermoextrap_amd import _build, _lib, engine
    from thermoextrap_amd.moments import DeviceDataArray

    txa.require_gpu()
    N = int(args.n if args.n is not None else (1e8 if args.part == "kernels" else 1e6))
    C = args.c
    da = np.ascontiguousarray((DA8 * ((args.alphas + 7) // 8))[:args.alphas], dtype=np.float64)
    x, u = bench.make_data(N, C, seed=1000, torch=torch)
    base = {"N": N, "C": C, "n_alpha": len(da), "csrc_sha": _build.csrc_sha(), "device": torch.cuda.get_device_name()}

    if args.part == "kernels":
        if len(da) > 8:
            raise SystemExit("--part kernels times single calls: at most 8 alphas")
        L = _lib.load()
        mean = engine.perturb(x, u, da)
        outs = {}

        def cov_call(block, n_levels=1):
            var = torch.empty((n_levels, len(da), C), dtype=torch.float64, device="cuda")
            small = torch.empty((2 + n_levels, len(da)), dtype=torch.float64, device="cuda")
            ws = engine.workspace(L.txm_perturb_cov_ws_bytes(N, C, len(da), block, n_levels))
            _lib.check(L.txm_perturb_cov(engine._ptr(x), C, engine._ptr(u), N, C, da.ctypes.data_as(ct.POINTER(ct.c_double)),
                                         len(da), engine._ptr(mean), block, n_levels, engine._ptr(var), engine._ptr(small[0]),
                                         engine._ptr(small[1]), engine._ptr(small[2:]), engine._ptr(ws), ws.numel(),
                                         engine._stream()), "txm_perturb_cov")
            outs[block] = var

        a0 = torch.zeros((C, 1, 1), dtype=torch.float64, device="cuda")
        b1 = torch.ones((C, 1, 1), dtype=torch.float64, device="cuda")
        lo, hi = float(u.min()), float(u.max())

        def influence_route():
            res = []
            for i, d in enumerate(da):
                w = torch.exp(-float(d) * (u - (lo if d >= 0 else hi)))
                res.append(engine.influence_cov(x, u, a0, b1, 0.0, mean[i].contiguous(), w=w)[0][:, 0, 0])
            outs["route"] = torch.stack(res)

        ts = _alternate({"perturb_cov_iid": lambda: cov_call(1), "perturb_cov_blocked": lambda: cov_call(args.block),
                         "perturb": lambda: engine.perturb(x, u, da), "exp_influence_cov_per_alpha": influence_route},
                        args.reps)
        nbytes = 8 * N * (C + 1)
        rec = {**base, "what": "kernels", "block": args.block, "bytes_one_pass": nbytes,
               "bytes_route": len(da) * (nbytes + 8 * N + 3 * 8 * N)}      # exp: read u, write w; the kernel reads w and u again
        for k, v in ts.items():
            s = _stats(v)
            rec[k] = {**s, "TBs_one_pass_at_median": round(nbytes / s["median_ms"] * 1e-9, 3)}
        route, iid = rec["exp_influence_cov_per_alpha"], rec["perturb_cov_iid"]
        rec["route_over_iid_median"] = round(route["median_ms"] / iid["median_ms"], 2)
        rec["route_minus_iid_over_route_spread"] = round((route["median_ms"] - iid["median_ms"]) / max(route["spread_ms"], 1e-9), 1)
        rec["iid_over_perturb_median"] = round(iid["median_ms"] / rec["perturb"]["median_ms"], 3)
        rec["blocked_over_iid_median"] = round(rec["perturb_cov_blocked"]["median_ms"] / iid["median_ms"], 3)
        rec["max_rel_diff_iid_vs_route"] = float(((outs[1][0] - outs["route"]).abs() / outs["route"]).max())
        print(json.dumps(rec), flush=True)
        return

    data = txa.DataValues.from_vals(xv=DeviceDataArray(x, ("rec", "val")), uv=DeviceDataArray(u, ("rec",)), order=0)
    pm = txa.PerturbModel(alpha0=5.6, data=data, alpha_name="beta")
    alphas = 5.6 + da
    seeds = iter(range(1, 1 << 30))
    ts = _alternate({
        "bootstrap": lambda: pm.resample(sampler={"nrep": args.nrep, "device": True, "seed": next(seeds)}).predict(alphas).std("rep"),
        "delta": lambda: pm.predict_with_error(alphas),
    }, args.reps)
    rec = {**base, "what": "PerturbModel", "n_rep": args.nrep}
    for k, v in ts.items():
        rec[k] = _stats(v)
    rec["bootstrap_over_delta_median"] = round(rec["bootstrap"]["median_ms"] / rec["delta"]["median_ms"], 2)
    sb = pm.resample(sampler={"nrep": args.nrep, "device": True, "seed": 1}).predict(alphas).std("rep").values * np.sqrt(
        args.nrep / (args.nrep - 1.0))
    sd = pm.predict_with_error(alphas)[1].values
    rec["std_bootstrap_over_delta_median_over_columns"] = [round(float(v), 3) for v in np.median(sb / sd, axis=1)]
    rec["n_eff"] = [round(float(v), 1) for v in pm.effective_samples(alphas).values]
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
