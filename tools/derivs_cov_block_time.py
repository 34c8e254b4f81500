"""Blocked delta-method error bars on the device, timed next to what they stand beside:

  (a) txm_influence_block_cov (engine.influence_block_cov, one level and the whole blocking curve), txm_influence_cov
      (engine.influence_cov) and txm_reduce_vals (engine.reduce_vals) on the same operands -- all read the sample matrix
      once: 8 N (C + 1) bytes (+ 8 N with weights); the blocked call also writes and re-reads its block sums,
      8 ceil(N / block) (C n_f + 1) bytes;
  (b) the two routes to an error bar from ONE correlated series (a moving average over --corr records of white noise,
      g ~ --corr): timeseries.decorrelate -> from_vals -> derivs_cov() against from_vals on the full series ->
      derivs_cov(block=...), the block length given.  timeseries.block_length on the same series is timed on its own.

    python tools/derivs_cov_block_time.py                                   # N = 1e8, C = 32, order 4, block 1024
    python tools/derivs_cov_block_time.py --n 1e6 --n-series 1e6 --reps 3   # a quick look

One JSON line per measurement.  Times are host clocks around work that ends in a device synchronise; the arms of a comparison
alternate inside one process, after one warm-up call each; median, minimum and spread (max - min) over --reps rounds.  Bytes
are what the algorithm needs, computed from the shapes.  The data of (a) is bench.py's synthetic state point.
"""

from __future__ import annotations

import argparse
import json
import math
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
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "spread_ms": round(max(ts) - min(ts), 4)}


def correlated_series(N, C, corr, seed):
    """u (N,), x (N, C) on the device: moving averages over `corr` records of independent white noise (g ~ corr),
    x_c = 0.7 u + its own average."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    cols = []
    for _ in range(1 + C):                          # column by column: one (N + corr,) cumulative sum alive at a time
        cs = torch.randn(N + corr, dtype=torch.float64, device="cuda", generator=g).cumsum(0)
        cols.append((cs[corr:] - cs[:-corr]) / math.sqrt(corr))
    u = 3.0 + cols[0]
    x = torch.stack([0.7 * u + c for c in cols[1:]], dim=1).contiguous()
    return x, u


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e8)
    ap.add_argument("--c", type=int, default=32)
    ap.add_argument("--order", type=int, default=4)
    ap.add_argument("--block", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--n-series", type=float, default=1e7, help="records of the correlated series of (b)")
    ap.add_argument("--corr", type=int, default=20, help="records the moving average of (b) spans")
    ap.add_argument("--skip-api", action="store_true", help="only (a), the kernels")
    args = ap.parse_args()

    import bench
    import thermoextrap_amd as txa
    from thermoextrap_amd import _build, engine, timeseries
    from thermoextrap_amd.moments import DeviceDataArray

    txa.require_gpu()
    N, C, order, block = int(args.n), args.c, args.order, args.block
    base = {"C": C, "order": order, "block": block, "csrc_sha": _build.csrc_sha(), "device": torch.cuda.get_device_name()}

    # ---- (a) the kernels on the same operands ----------------------------------------------------------------------------
    x, u = bench.make_data(N, C, seed=1000, torch=torch)
    g = torch.Generator(device="cuda").manual_seed(7)
    w = torch.empty(N, dtype=torch.float64, device="cuda").uniform_(0.5, 1.5, generator=g)
    st = engine.reduce_vals(x, u, order)
    cu, cx = float(st[0, 0, 1]), st[:, 1, 0].contiguous()
    gen = torch.Generator(device="cuda").manual_seed(11)
    a = torch.randn((C, order + 1, order + 1), dtype=torch.float64, device="cuda", generator=gen)
    b = torch.randn((C, order + 1, order + 1), dtype=torch.float64, device="cuda", generator=gen)
    n_levels = len(engine.block_levels(N, block)[0])
    for weights, tag in ((None, "unweighted"), (w, "weighted")):
        ts = _alternate({
            "reduce_vals": lambda: engine.reduce_vals(x, u, order, w=weights),
            "influence_cov": lambda: engine.influence_cov(x, u, a, b, cu, cx, w=weights),
            "influence_block_cov": lambda: engine.influence_block_cov(x, u, a, b, cu, cx, block, w=weights),
            "influence_block_cov_curve": lambda: engine.influence_block_cov(x, u, a, b, cu, cx, block, n_levels=n_levels,
                                                                            w=weights),
        }, args.reps)
        nbytes = 8 * N * (C + 1 + (weights is not None))
        rec = {**base, "N": N, "what": "kernels", "weights": tag, "bytes": nbytes, "curve_levels": n_levels,
               "block_sum_bytes": 8 * -(-N // block) * (C * (order + 1) + 1)}
        for k, v in ts.items():
            s = _stats(v)
            rec[k] = {**s, "TBs_at_median": round(nbytes / s["median_ms"] * 1e-9, 3)}
        rec["block_over_influence_median"] = round(rec["influence_block_cov"]["median_ms"] / rec["influence_cov"]["median_ms"], 3)
        rec["block_over_reduce_median"] = round(rec["influence_block_cov"]["median_ms"] / rec["reduce_vals"]["median_ms"], 3)
        print(json.dumps(rec), flush=True)
    del x, u, w

    # ---- (b) one correlated series: subsample and take the iid error bar, or keep it whole and block --------------------------
    if not args.skip_api:
        import numpy as np

        Ns = int(args.n_series)
        xs, us = correlated_series(Ns, C, args.corr, seed=5)
        xv, uv = DeviceDataArray(xs, ("rec", "val")), DeviceDataArray(us, ("rec",))
        kept = {}

        def route_decorrelate():
            ud, xd, _, info = timeseries.decorrelate(uv, xv)
            data = txa.DataCentralMomentsVals.from_vals(xv=xd, uv=ud, order=order, central=True)
            kept["n"], kept["g"] = info["n"], info["g"]
            return txa.beta.factory_extrapmodel(5.6, data).derivs_cov()

        def route_block():
            data = txa.DataCentralMomentsVals.from_vals(xv=xv, uv=uv, order=order, central=True)
            return txa.beta.factory_extrapmodel(5.6, data).derivs_cov(block=block)

        ts = _alternate({"decorrelate_then_iid": route_decorrelate, "full_series_blocked": route_block,
                         "block_length": lambda: timeseries.block_length(uv, xv)}, max(3, args.reps // 2))
        rec = {**base, "N": Ns, "what": "routes", "corr": args.corr, "g_max": round(kept["g"], 3), "n_kept": kept["n"]}
        for k, v in ts.items():
            rec[k] = _stats(v)
        rec["decorrelate_over_blocked_median"] = round(rec["decorrelate_then_iid"]["median_ms"] / rec["full_series_blocked"]["median_ms"], 2)
        sd_d = np.sqrt(np.einsum("iic->ic", route_decorrelate().values))
        sd_b = np.sqrt(np.einsum("iic->ic", route_block().values))
        rec["block_length"]["value"] = timeseries.block_length(uv, xv)
        rec["std_decorrelated_over_blocked_by_order_median_over_columns"] = [round(float(v), 3) for v in np.median(sd_d / sd_b, axis=1)]
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
