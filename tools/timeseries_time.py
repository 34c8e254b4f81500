"""Timing of timeseries.statistical_inefficiencies and of the lag-sums call, with two baselines a user can write with torch
on the device, all in one process.

    python tools/timeseries_time.py                       # N in {1e6, 1e8} x C in {1, 32} x phi in {0.9, 0.99}
    python tools/timeseries_time.py --n 1e8 --c 32 --phi 0.9 --no-baselines    # one shape (a rocprofv3 --kernel-trace --stats run)

One JSON line per shape.  Times are host clocks around work that ends in a device synchronise, the median of --reps calls
after one warm-up call.  Legs:
  call_ms        the whole statistical_inefficiencies(u, x) call: means, the lag blocks the scan asks for, the host loop.
  lag256_ms      engine.lag_sums of all 2C + 1 pairs, lags 0 .. 255 (means given): centring + transposition, the contraction,
                 the chunk sum.  N * 256 * (3C + 1) FMAs (an auto pair is one product, a cross pair two) -> TFLOP/s, and the
                 fraction of the 78.6 TFLOP/s FP64 matrix peak.  lag1024_ms: the same for lags 0 .. 1023 (four lag tiles
                 share every A operand).
  loop (a)       the per-lag loop (da[:N - t] * db[t:]).sum() on contiguous centred columns.  Timed on --loop-lags lags of
                 three products ((u, u), (x_0, x_0), (x_0, u) one way) and scaled: loop_ms_256 = per product and lag x 256
                 lags x (3C + 1) products; loop_ms_visited = the same per-product time x the lags the plain loop visits for
                 every pair up to its own stop lag.
  fft (b)        zero-padded torch.fft.rfft of every centred series (length 2^ceil(log2(2N))), one product and irfft per
                 pair (the symmetrised cross pair reads lags t and -t of one irfft).  Timed on u and --fft-cols columns and
                 scaled to C columns (every column costs one rfft and two irffts of the same length).  The FFT costs the
                 same at any lag count: fft_break_even_lags = fft_ms / (lag256_ms / 256) is where it overtakes the direct
                 kernel.
The series are AR(1): u = AR(phi), x_c = 0.6 u + 0.8 AR(0.7) + 3, generated on the device by recursive doubling
(y <- y + phi^s shift(y, s), s = 1, 2, 4, ... until phi^s < 1e-9).
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

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

PEAK_TFLOPS = 78.6


def _timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def ar1_device(N, C, phi, gen):
    y = torch.empty((N, C), dtype=torch.float64, device="cuda").normal_(0.0, 1.0, generator=gen)
    s = 1
    while phi**s >= 1e-9:
        z = y.clone()
        z[s:].add_(y[:-s], alpha=phi**s)
        y = z
        s *= 2
    return y


def make_series(N, C, phi, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    u = ar1_device(N, 1, phi, gen)[:, 0].contiguous()
    x = ar1_device(N, C, 0.7, gen)
    x.mul_(0.8).add_(u[:, None], alpha=0.6).add_(3.0)
    return u, x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, nargs="*", default=[1e6, 1e8])
    ap.add_argument("--c", type=int, nargs="*", default=[1, 32])
    ap.add_argument("--phi", type=float, nargs="*", default=[0.9, 0.99])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loop-lags", type=int, default=6)
    ap.add_argument("--fft-cols", type=int, default=2)
    ap.add_argument("--no-baselines", action="store_true")
    args = ap.parse_args()

    import thermoextrap_amd as txa
    from thermoextrap_amd import _build, engine, timeseries

    txa.require_gpu()
    for N in (int(v) for v in args.n):
        for C in args.c:
            for phi in args.phi:
                u, x = make_series(N, C, phi, 1234)
                npairs = 2 * C + 1
                res = timeseries.statistical_inefficiencies(u, x)
                call_ms = _timed(lambda: timeseries.statistical_inefficiencies(u, x), args.reps)
                stops = np.concatenate([[res.stop_u], res.stop_x, res.stop_cross])
                blocks = [b for b in timeseries.lag_blocks(N) if b[0] <= stops.max()]
                center = engine.lag_center(x, u)
                pairs = list(range(npairs))
                lag256_ms = _timed(lambda: engine.lag_sums(x, u, pairs, 0, 256, center=center), args.reps)
                lag1024_ms = _timed(lambda: engine.lag_sums(x, u, pairs, 0, 1024, center=center), args.reps)
                fma = N * (3 * C + 1)
                rec = {
                    "N": N, "C": C, "phi": phi, "pairs": npairs, "reps": args.reps,
                    "g_u": round(res.g_u, 4), "g_max": round(res.g_max, 4), "stop_lag_min": int(stops.min()),
                    "stop_lag_max": int(stops.max()), "lag_blocks": blocks,
                    "call_ms": round(call_ms, 3), "lag256_ms": round(lag256_ms, 3), "lag1024_ms": round(lag1024_ms, 3),
                    "lag256_tflops": round(2 * fma * 256 / lag256_ms * 1e-9, 2),
                    "lag1024_tflops": round(2 * fma * 1024 / lag1024_ms * 1e-9, 2),
                    "lag256_of_peak": round(2 * fma * 256 / lag256_ms * 1e-9 / PEAK_TFLOPS, 3),
                    "lag1024_of_peak": round(2 * fma * 1024 / lag1024_ms * 1e-9 / PEAK_TFLOPS, 3),
                    "csrc_sha": _build.csrc_sha(),
                }
                if not args.no_baselines:
                    # (a) the per-lag loop on contiguous centred columns
                    du = u - u.mean()
                    d0 = x[:, 0].clone()                       # (a copy: C = 1 makes the column a view of x)
                    d0 -= d0.mean()
                    lags = [int(v) for v in np.linspace(1, 255, args.loop_lags)]

                    def loop():
                        acc = []
                        for t in lags:
                            acc.append((du[: N - t] * du[t:]).sum())
                            acc.append((d0[: N - t] * d0[t:]).sum())
                            acc.append((d0[: N - t] * du[t:]).sum())
                        return torch.stack(acc).cpu()

                    per = _timed(loop, args.reps) / (3 * len(lags))
                    visited = int(stops[: 1 + C].sum() + 2 * stops[1 + C:].sum())      # products x lags up to each pair's stop
                    rec.update({"loop_ms_per_product_lag": round(per, 4), "loop_lags_timed": lags, "loop_products_timed": 3,
                                "loop_ms_256": round(per * 256 * (3 * C + 1), 1), "loop_ms_visited": round(per * visited, 1),
                                "loop256_over_lag256": round(per * 256 * (3 * C + 1) / lag256_ms, 1),
                                "loop_visited_over_call": round(per * visited / call_ms, 1)})
                    # (b) the FFT route
                    nfft = 1 << int(np.ceil(np.log2(2 * N)))
                    ncol = min(C, args.fft_cols)
                    try:
                        def fft_u():
                            Fu = torch.fft.rfft(du, n=nfft)
                            r = torch.fft.irfft(Fu * Fu.conj(), n=nfft)[:256] * 2.0
                            return Fu, r

                        def fft_cols(Fu):
                            out = []
                            for c in range(ncol):
                                d = x[:, c].clone()
                                d -= center[1 + c]
                                F = torch.fft.rfft(d, n=nfft)
                                out.append(torch.fft.irfft(F * F.conj(), n=nfft)[:256] * 2.0)
                                cr = torch.fft.irfft(F * Fu.conj(), n=nfft)
                                out.append(cr[:256] + torch.cat([cr[:1], cr[-255:].flip(0)]))
                                del F, cr
                            return out

                        Fu, r_u = fft_u()
                        got = fft_cols(Fu)
                        ref = engine.lag_sums(x, u, [0, 1, 1 + C], 0, 256, center=center)
                        scale = ref[:, :1].abs()
                        fft_err = max(float(((r_u - ref[0]).abs() / scale[0]).max()), float(((got[0] - ref[1]).abs() / scale[1]).max()),
                                      float(((got[1] - ref[2]).abs() / scale[2]).max()))
                        del got
                        fft_u_ms = _timed(lambda: fft_u(), args.reps)
                        fft_c_ms = _timed(lambda: fft_cols(Fu), args.reps)
                        fft_ms = fft_u_ms + fft_c_ms * C / ncol
                        rec.update({"fft_n": nfft, "fft_cols_timed": ncol, "fft_u_ms": round(fft_u_ms, 2),
                                    "fft_per_col_ms": round(fft_c_ms / ncol, 2), "fft_ms": round(fft_ms, 1),
                                    "fft_vs_lag_sums_rel_diff": fft_err, "fft_over_call": round(fft_ms / call_ms, 2),
                                    "fft_over_lag256": round(fft_ms / lag256_ms, 2),
                                    "fft_break_even_lags": int(fft_ms / (lag256_ms / 256))})
                        del Fu
                    except RuntimeError as e:          # (an FFT plan or its work buffer that does not fit)
                        rec.update({"fft_n": nfft, "fft_ms": None, "fft_error": str(e).splitlines()[0][:200]})
                    del du, d0
                print(json.dumps(rec), flush=True)
                del u, x, center
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
