"""Timing of timeseries.detect_equilibration(s) against what the package could do before it: statistical_inefficiency
looped over the origins.  The conventions of tools/timeseries_time.py: one process, host clocks around work that ends in a
device synchronise, the median of --reps calls after one warm-up call, one JSON line per shape.

    python tools/equilibration_time.py                    # T = 1e6, 1e7 (one series), T = 1e7 with C = 32; the nskip sweep
    python tools/equilibration_time.py --t 1e7 --c 32 --no-baseline --no-sweep     # one shape (a rocprofv3 --kernel-trace --stats run)

Legs:
  call_ms        detect_equilibration(u) for C = 0, detect_equilibrations(u, x) otherwise, fast=True, 512 origins: the pivots,
                 the lag blocks the scan asks for (each one pass over the samples and one device-to-host copy of
                 [series][origins][lags]), the host loop over (series, origin).
  origin256_ms   engine.lag_origin_sums of all 1 + C series, lags 0 .. 255 (pivots given): centring + transposition, the
                 segment sums, the segment pass, the suffix scan.  The segment pass is 3 MFMAs per step (Q, and X twice) where
                 an auto pair of txm_lag_sums is one: 2 * 3 * T * 256 * (1 + C) FLOP -> TFLOP/s.  origin1024_ms: lags 0 .. 1023.
  loop           the parent's capability: statistical_inefficiency(A[t0:], fast=True) for every origin, every series.  Timed
                 on --loop-origins evenly spaced origins of series u and scaled to all origins and 1 + C series.
  sweep          origin256_ms at T = --sweep-t for nskip = 63 .. 4032: a segment shorter than the stage of 1008 samples still
                 stages whole windows of b and a workgroup per segment; FLOP/s fall with it.
The series are AR(0.9) (x_c: AR(0.7)) plus a transient 5 sigma exp(-n / (0.02 T)).
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from timeseries_time import _timed, ar1_device  # noqa: E402


def make_series(T, C, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    tr = torch.exp(-torch.arange(T, dtype=torch.float64, device="cuda") / (0.02 * T))
    u = ar1_device(T, 1, 0.9, gen)[:, 0] + 5.0 * (1 - 0.81) ** -0.5 * tr + 174.85
    x = None
    if C:
        x = ar1_device(T, C, 0.7, gen)
        x.add_(tr[:, None], alpha=5.0 * (1 - 0.49) ** -0.5).add_(3.0)
    return u.contiguous(), x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--t", type=float, nargs="*", default=None)
    ap.add_argument("--c", type=int, nargs="*", default=None)
    ap.add_argument("--origins", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loop-origins", type=int, default=16)
    ap.add_argument("--sweep-t", type=float, default=2.5e5)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--no-sweep", action="store_true")
    args = ap.parse_args()

    import thermoextrap_amd as txa
    from thermoextrap_amd import _build, engine, timeseries

    txa.require_gpu()
    shapes = [(1_000_000, 0), (10_000_000, 0), (10_000_000, 32)] if args.t is None else [(int(t), c) for t in args.t for c in (args.c or [0])]
    for T, C in shapes:
        u, x = make_series(T, C, 1234)
        nskip = timeseries.pick_nskip(T, None, args.origins)
        run = (lambda: timeseries.detect_equilibrations(u, x, max_origins=args.origins)) if C else (
            lambda: timeseries.detect_equilibration(u, max_origins=args.origins))
        e = timeseries.detect_equilibrations(u, x, max_origins=args.origins)
        call_ms = _timed(run, args.reps)
        center = engine.lag_origin_center(x, u)
        series = list(range(1 + C))
        o256 = _timed(lambda: engine.lag_origin_sums(x, u, series, nskip, 0, 256, center=center), args.reps)
        o1024 = _timed(lambda: engine.lag_origin_sums(x, u, series, nskip, 0, 1024, center=center), args.reps)
        flop = 2 * 3 * T * (1 + C)
        rec = {"T": T, "C": C, "origins": int(e.g_t.shape[1]), "nskip": nskip, "reps": args.reps, "t0": e.t0.tolist(),
               "g": [round(float(v), 4) for v in e.g], "neff": [round(float(v), 1) for v in e.neff], "t0_max": e.t0_max,
               "call_ms": round(call_ms, 3), "origin256_ms": round(o256, 3), "origin1024_ms": round(o1024, 3),
               "origin256_tflops": round(flop * 256 / o256 * 1e-9, 2), "origin1024_tflops": round(flop * 1024 / o1024 * 1e-9, 2),
               "csrc_sha": _build.csrc_sha()}
        if not args.no_baseline:
            picks = [int(v) for v in np.linspace(0, e.g_t.shape[1] - 1, args.loop_origins)]

            def loop():
                return [timeseries.statistical_inefficiency(u[j * nskip:], fast=True) for j in picks]

            g_loop = loop()
            loop_ms = _timed(loop, args.reps)
            scaled = loop_ms / len(picks) * e.g_t.shape[1] * (1 + C)
            rec.update({"loop_origins_timed": picks, "loop_ms_timed": round(loop_ms, 2), "loop_ms_scaled": round(scaled, 1),
                        "loop_over_call": round(scaled / call_ms, 1),
                        "loop_g_max_rel_diff": float(max(abs(g - e.g_t[0, j]) / g for g, j in zip(g_loop, picks)))})
        print(json.dumps(rec), flush=True)
        del u, x, center
        torch.cuda.empty_cache()
    if not args.no_sweep:
        T = int(args.sweep_t)
        u, _ = make_series(T, 0, 99)
        center = engine.lag_origin_center(None, u)
        for nskip in (63, 126, 252, 504, 1008, 2016, 4032):
            ms = _timed(lambda: engine.lag_origin_sums(None, u, [0], nskip, 0, 256, center=center), args.reps)
            print(json.dumps({"sweep_T": T, "nskip": nskip, "origins": -(-(T - 1) // nskip), "origin256_ms": round(ms, 3),
                              "origin256_tflops": round(2 * 3 * T * 256 / ms * 1e-9, 3)}), flush=True)


if __name__ == "__main__":
    main()
