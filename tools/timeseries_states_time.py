"""The statistical inefficiencies of a state collection, timed against the loop over the states.

Four shapes, all in one process:
  a  64 states x N = 1e6 x C = 4, u = AR(0.9)        (BASELINE config 5's shape)
  b  the same with ragged lengths, uniform in [2e5, 1e6] from a fixed seed
  c  64 states x 1e6 x C = 1
  d  16 states x 1e6 x C = 4 at phi = 0.99           (the scan needs several lag blocks: the kept rows matter)
The series are those of tools/timeseries_time.py: u = AR(phi), x_c = 0.6 u + 0.8 AR(0.7) + 3, made on the device.

Two arms alternate after one warm-up call of each, host clocks around work that ends in a device synchronise:
  states  timeseries.statistical_inefficiencies_states(us, xs)
  loop    [timeseries.statistical_inefficiencies(u, x) for u, x in zip(us, xs)]      (the single-state path, unchanged)
Then the parts of the collection call, each timed alone the same way: the S centres (engine.lag_center per state), the rows
pass (engine.lag_rows_batched with the centres given), every lag block's sums call (engine.lag_sums_batched on the item list
the scan asked for) and its device-to-host copy, and the host scan replayed on the copied arrays.

    python tools/timeseries_states_time.py                       # the four shapes, 7 repetitions
    python tools/timeseries_states_time.py --shapes a --reps 2 --no-loop      # a rocprofv3 --kernel-trace --stats run

One JSON line per shape: median, min and max of every arm and part in ms, the loop's spread (max - min) and whether the
collection call beats the loop by more than three times that spread (DESIGN 7's rule).
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
sys.path.insert(0, str(ROOT / "tools"))

SHAPES = {"a": (64, 4, 0.9, False), "b": (64, 4, 0.9, True), "c": (64, 1, 0.9, False), "d": (16, 4, 0.99, False)}


def _stats(ts):
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


def _timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def _same(a, b):
    return (a.g_u == b.g_u and a.g_max == b.g_max and a.stop_u == b.stop_u and np.array_equal(a.g_x, b.g_x)
            and np.array_equal(a.g_cross, b.g_cross) and np.array_equal(a.stop_x, b.stop_x) and np.array_equal(a.stop_cross, b.stop_cross))


def run(tag, args):
    from timeseries_time import make_series

    from thermoextrap_amd import _build, engine, timeseries

    S, C, phi, ragged = SHAPES[tag]
    N = int(args.n)
    ns = np.random.default_rng(2024).integers(N // 5, N + 1, size=S) if ragged else np.full(S, N)
    us, xs = [], []
    for s, n in enumerate(ns):
        u, x = make_series(int(n), C, phi, 1000 + s)
        us.append(u)
        xs.append(x)
    torch.cuda.synchronize()

    arms = {"states": lambda: timeseries.statistical_inefficiencies_states(us, xs)}
    if not args.no_loop:
        arms["loop"] = lambda: [timeseries.statistical_inefficiencies(u, x) for u, x in zip(us, xs)]
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in arms}
    for _ in range(args.reps):
        for k, fn in arms.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    res = timeseries.statistical_inefficiencies_states(us, xs)
    stops = np.concatenate([np.concatenate([[r.stop_u], r.stop_x, r.stop_cross]) for r in res])
    rec = {"what": "statistical inefficiencies of a state collection", "shape": tag, "S": S, "C": C, "phi": phi,
           "n_min": int(ns.min()), "n_max": int(ns.max()), "n_sum": int(ns.sum()), "reps": args.reps,
           "g_max_min": round(min(r.g_max for r in res), 3), "g_max_max": round(max(r.g_max for r in res), 3),
           "stop_lag_min": int(stops.min()), "stop_lag_max": int(stops.max()),
           "csrc_sha": _build.csrc_sha(), "device": torch.cuda.get_device_name()}
    for k, v in ts.items():
        rec[k] = _stats(v)
    if "loop" in ts:
        a, b = rec["loop"], rec["states"]
        rec["loop_over_states_median"] = round(a["median_ms"] / b["median_ms"], 2)
        rec["loop_minus_states_median_ms"] = round(a["median_ms"] - b["median_ms"], 4)
        rec["loop_spread_ms"] = round(a["max_ms"] - a["min_ms"], 4)
        rec["pays"] = bool(a["median_ms"] - b["median_ms"] > 3 * (a["max_ms"] - a["min_ms"]))
        rec["results_equal"] = bool(all(_same(p, q) for p, q in zip(res, arms["loop"]())))

    # ---- the parts of the collection call
    centers = [engine.lag_center(x, u) for x, u in zip(xs, us)]
    rec["part_centers"] = _stats(_timed(lambda: [engine.lag_center(x, u) for x, u in zip(xs, us)], args.reps))
    rec["part_rows"] = _stats(_timed(lambda: engine.lag_rows_batched(xs, us, centers), args.reps))
    rows = engine.lag_rows_batched(xs, us, centers)
    fetched = []

    def fetch(items, t0, nlags):
        R = engine.lag_sums_batched(rows, items, t0, nlags).cpu().numpy()
        fetched.append((list(items), t0, nlags, R))
        return R

    pairs = [range(2 * C + 1)] * S
    timeseries.scan_lag_sums_states(fetch, ns, pairs)
    blocks = []
    for items, t0, nlags, _ in fetched:
        dev = engine.lag_sums_batched(rows, items, t0, nlags)
        blocks.append({"t0": t0, "nlags": nlags, "items": len(items),
                       "slices": len(engine.lag_item_slices(ns, items, nlags, engine.workspace_budget())),
                       "ws_MB": round(engine.lag_sums_batched_ws_bytes(ns, items, nlags) / 1e6, 1),
                       "sums": _stats(_timed(lambda: engine.lag_sums_batched(rows, items, t0, nlags), args.reps)),
                       "copy": _stats(_timed(lambda: dev.cpu().numpy(), args.reps))})
    rec["part_blocks"] = blocks
    replay = iter(())

    def scan():
        nonlocal replay
        replay = iter(fetched)
        timeseries.scan_lag_sums_states(lambda items, t0, nlags: next(replay)[3], ns, pairs)

    rec["part_host_scan"] = _stats(_timed(scan, args.reps))
    rec["parts_sum_median_ms"] = round(rec["part_centers"]["median_ms"] + rec["part_rows"]["median_ms"] + rec["part_host_scan"]["median_ms"]
                                       + sum(b["sums"]["median_ms"] + b["copy"]["median_ms"] for b in blocks), 4)
    fma = int(ns.sum()) * (3 * C + 1)
    rec["block0_tflops"] = round(2 * fma * 256 / blocks[0]["sums"]["median_ms"] * 1e-9, 2)
    rec["rows_bytes_MB"] = round(rows.rows.numel() / 1e6, 1)
    print(json.dumps(rec), flush=True)
    del us, xs, rows, fetched, centers
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--n", type=float, default=1e6)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-loop", action="store_true")
    args = ap.parse_args()

    import thermoextrap_amd as txa

    txa.require_gpu()
    for tag in args.shapes:
        run(tag, args)


if __name__ == "__main__":
    main()
