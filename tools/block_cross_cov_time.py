"""The blocked cross-column delta-method covariance on the device, timed next to what it stands beside:

  (a) txm_influence_block_cross_cov (engine.influence_block_cross_cov) at every --block, with txm_influence_block_cov
      (the same pass 1, the C diagonal blocks alone), txm_influence_cross_cov (the iid cross form) and txm_reduce_vals on
      the same operands.  All read the sample matrix once: 8 N (C + 1) bytes (+ 8 N with weights); the blocked calls also
      write and re-read their block sums, 8 nb (C n_f + 1) bytes, nb = ceil(N / block);
  (b) the whole cross blocking curve: engine.influence_block_cross_cov with every level of engine.block_levels, and
      ExtrapModel.cross_blocking_curve (the host copy and the labels included), at the first --block;
  (c) the two routes to a cross covariance from ONE correlated series (a moving average over --corr records of white noise,
      g ~ --corr): timeseries.decorrelate -> from_vals -> derivs_cross_cov() against from_vals on the full series ->
      derivs_cross_cov(block=...).

    python tools/block_cross_cov_time.py                                     # N = 1e8, C = 32, order 4, blocks 1024 and 16
    python tools/block_cross_cov_time.py --n 1e6 --n-series 1e6 --reps 3     # a quick look

One JSON line per measurement.  Times are host clocks around work that ends in a device synchronise; the arms of a comparison
alternate inside one process, after one warm-up call each; median, minimum and spread (max - min) over --reps rounds.  Bytes
are what the algorithm needs, computed from the shapes; the FMA count is the matrix pipe's at level 0, padding included:
tiles computed * 256 per block.  The data of (a) and (b) is bench.py's synthetic state point.
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


def tiles_computed(M):
    """Tiles of 16 x 16 the Gram pass computes for M logical columns: the upper triangle, tile by tile (the macro tiles of
    4 x 4 only group them)."""
    T = -(-M // 16)
    return T * (T + 1) // 2


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
    ap.add_argument("--block", type=int, nargs="+", default=[1024, 16])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--n-series", type=float, default=1e7, help="records of the correlated series of (c)")
    ap.add_argument("--corr", type=int, default=20, help="records the moving average of (c) spans")
    ap.add_argument("--skip-api", action="store_true", help="only (a), the kernels")
    args = ap.parse_args()

    import bench
    import thermoextrap_amd as txa
    from thermoextrap_amd import _build, engine, timeseries
    from thermoextrap_amd.moments import DeviceDataArray

    txa.require_gpu()
    N, C, order = int(args.n), args.c, args.order
    nf = order + 1
    base = {"C": C, "order": order, "csrc_sha": _build.csrc_sha(), "device": torch.cuda.get_device_name()}

    # ---- (a) the kernels on the same operands ----------------------------------------------------------------------------
    x, u = bench.make_data(N, C, seed=1000, torch=torch)
    g = torch.Generator(device="cuda").manual_seed(7)
    w = torch.empty(N, dtype=torch.float64, device="cuda").uniform_(0.5, 1.5, generator=g)
    st = engine.reduce_vals(x, u, order)
    cu, cx = float(st[0, 0, 1]), st[:, 1, 0].contiguous()
    gen = torch.Generator(device="cuda").manual_seed(11)
    a = torch.randn((C, nf, nf), dtype=torch.float64, device="cuda", generator=gen)
    b = torch.randn((C, nf, nf), dtype=torch.float64, device="cuda", generator=gen)
    for block in args.block:
        for weights, tag in ((None, "unweighted"), (w, "weighted")):
            ts = _alternate({
                "reduce_vals": lambda: engine.reduce_vals(x, u, order, w=weights),
                "influence_cross_cov": lambda: engine.influence_cross_cov(x, u, a, b, cu, cx, w=weights),
                "influence_block_cov": lambda: engine.influence_block_cov(x, u, a, b, cu, cx, block, w=weights),
                "influence_block_cross_cov": lambda: engine.influence_block_cross_cov(x, u, a, b, cu, cx, block, w=weights),
            }, args.reps)
            nb = -(-N // block)
            nbytes = 8 * N * (C + 1 + (weights is not None))
            fma = nb * tiles_computed(C * nf) * 256
            rec = {**base, "N": N, "what": "kernels", "block": block, "weights": tag, "bytes": nbytes, "blocks": nb,
                   "block_sum_bytes": 8 * nb * (C * nf + 1), "tiles_computed": tiles_computed(C * nf), "matrix_fma": fma}
            for k, v in ts.items():
                s = _stats(v)
                rec[k] = {**s, "TBs_at_median": round(nbytes / s["median_ms"] * 1e-9, 3)}
            extra = rec["influence_block_cross_cov"]["median_ms"] - rec["influence_block_cov"]["median_ms"]
            rec["cross_minus_block_median_ms"] = round(extra, 4)
            rec["matrix_TFLOPs_over_the_difference"] = round(2 * fma / extra * 1e-9, 2) if extra > 0 else None
            rec["block_cross_over_block_median"] = round(rec["influence_block_cross_cov"]["median_ms"]
                                                         / rec["influence_block_cov"]["median_ms"], 3)
            rec["iid_cross_over_block_cross_median"] = round(rec["influence_cross_cov"]["median_ms"]
                                                             / rec["influence_block_cross_cov"]["median_ms"], 2)
            print(json.dumps(rec), flush=True)

    if args.skip_api:
        return
    import numpy as np

    # ---- (b) the whole curve ---------------------------------------------------------------------------------------------
    block = args.block[0]
    n_levels = len(engine.block_levels(N, block)[0])
    data = txa.DataCentralMomentsVals.from_vals(xv=DeviceDataArray(x, ("rec", "val")), uv=DeviceDataArray(u, ("rec",)),
                                                order=order, central=True)

    def api_curve():
        return txa.beta.factory_extrapmodel(5.6, data).cross_blocking_curve(block)

    ts = _alternate({
        "engine_one_level": lambda: engine.influence_block_cross_cov(x, u, a, b, cu, cx, block),
        "engine_curve": lambda: engine.influence_block_cross_cov(x, u, a, b, cu, cx, block, n_levels=n_levels),
        "cross_blocking_curve": api_curve,
    }, args.reps)
    rec = {**base, "N": N, "what": "curve", "block": block, "levels": n_levels, "result_bytes": 8 * n_levels * (C * nf) ** 2}
    for k, v in ts.items():
        rec[k] = _stats(v)
    print(json.dumps(rec), flush=True)
    del x, u, w, data

    # ---- (c) one correlated series: subsample and take the iid cross covariance, or keep it whole and block ------------------
    Ns = int(args.n_series)
    xs, us = correlated_series(Ns, C, args.corr, seed=5)
    xv, uv = DeviceDataArray(xs, ("rec", "val")), DeviceDataArray(us, ("rec",))
    kept = {}

    def route_decorrelate():
        ud, xd, _, info = timeseries.decorrelate(uv, xv)
        d = txa.DataCentralMomentsVals.from_vals(xv=xd, uv=ud, order=order, central=True)
        kept["n"], kept["g"] = info["n"], info["g"]
        return txa.beta.factory_extrapmodel(5.6, d).derivs_cross_cov()

    def route_block():
        d = txa.DataCentralMomentsVals.from_vals(xv=xv, uv=uv, order=order, central=True)
        return txa.beta.factory_extrapmodel(5.6, d).derivs_cross_cov(block=block)

    ts = _alternate({"decorrelate_then_iid": route_decorrelate, "full_series_blocked": route_block}, max(3, args.reps // 2))
    rec = {**base, "N": Ns, "what": "routes", "block": block, "corr": args.corr, "g_max": round(kept["g"], 3), "n_kept": kept["n"]}
    for k, v in ts.items():
        rec[k] = _stats(v)
    rec["decorrelate_over_blocked_median"] = round(rec["decorrelate_then_iid"]["median_ms"]
                                                   / rec["full_series_blocked"]["median_ms"], 2)
    sd_d = np.sqrt(np.einsum("iicc->ic", route_decorrelate().values))
    sd_b = np.sqrt(np.einsum("iicc->ic", route_block().values))
    rec["std_decorrelated_over_blocked_by_order_median_over_columns"] = [round(float(v), 3) for v in np.median(sd_d / sd_b, axis=1)]
    # the error bar of the sum over the columns of the value itself (order 0): what only the cross blocks give
    rec["std_of_column_sum_decorrelated_over_blocked"] = round(float(np.sqrt(route_decorrelate().values[0, 0].sum()
                                                                             / route_block().values[0, 0].sum())), 3)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
