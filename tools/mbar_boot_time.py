"""MBAR bootstrap timing on the device: the batched bootstrap (engine.mbar_bootstrap_solve + mbar_bootstrap_predict)
against the loop a user has to write without it -- per replicate: expanded copies of every state by
``repeat_interleave`` with that replicate's counts, a fresh ``MBARModel``, ``predict``.

    python tools/mbar_boot_time.py                          # K in {4, 8} x N per state in {2.5e5, 2.5e7} x C in {1, 32}
    python tools/mbar_boot_time.py --k 4 --n 25000000 --c 32 --no-loop     # one shape (a rocprofv3 --kernel-trace run)

One JSON line per shape, nrep = 100, 8 targets.  Times are host clocks around work that ends in a device synchronise
(the solves wait for the device at every Newton step by construction): the batched leg is the median of --reps calls
after one warm-up call; the loop leg runs one untimed warm-up replicate, then --loop-reps replicates (all nrep when
N per state <= --loop-full-below, else 4) and is scaled linearly to nrep -- ``loop_replicates_timed`` says which.  Both legs
run in the same process in the same order for every shape: batched, then loop.
``eval_terms_per_s`` = nrep x N_total x K softmax terms of one batched evaluation pass per second (the point kernel's
rate in the same unit: ``point_eval_terms_per_s``, one ``engine.mbar_eval`` pass of the same states).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, nargs="*", default=[4, 8])
    ap.add_argument("--n", type=float, nargs="*", default=[2.5e5, 2.5e7])
    ap.add_argument("--c", type=int, nargs="*", default=[1, 32])
    ap.add_argument("--nrep", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loop-full-below", type=float, default=1e6)
    ap.add_argument("--no-loop", action="store_true")
    args = ap.parse_args()

    import thermoextrap_amd as txa
    from thermoextrap_amd import _build, engine
    from thermoextrap_amd.moments import DeviceDataArray

    txa.require_gpu()
    gen = torch.Generator(device="cuda").manual_seed(0)
    sd, mu, nrep, seed = 10.0, 500.0, args.nrep, 2718
    for K in args.k:
        for n in (int(v) for v in args.n):
            for C in args.c:
                alpha0 = 1.0 + 0.05 * np.arange(K)                  # mean shift sd / 2 between neighbours
                NT = K * n
                us = [torch.randn(n, dtype=torch.float64, device="cuda", generator=gen) * sd + (mu - sd * sd * a) for a in alpha0]
                xs = [torch.randn(n, C, dtype=torch.float64, device="cuda", generator=gen).add_(0.01 * u[:, None]) for u in us]
                targets = alpha0[0] + np.linspace(-0.05, 0.05 * K, 8)
                sol0 = engine.mbar_solve(us, alpha0)
                samplers = [engine.DeviceSampler(seed, nrep, n, rep0=s * nrep) for s in range(K)]
                evals = []
                real = engine.mbar_boot_eval

                def counting(*a, **kw):
                    evals.append(1)
                    return real(*a, **kw)

                engine.mbar_boot_eval = counting
                f = engine.mbar_bootstrap_solve(us, alpha0, samplers, sol0)
                engine.mbar_boot_eval = real
                solve_ms = _timed(lambda: engine.mbar_bootstrap_solve(us, alpha0, samplers, sol0), args.reps)
                b = np.log(n) - alpha0 * sol0.upiv
                g = b[None, :] + f
                g -= g.max(axis=1, keepdims=True)
                eval_ms = _timed(lambda: engine.mbar_boot_eval(us, alpha0, samplers, g, sol0.upiv), args.reps)
                pred_ms = _timed(lambda: engine.mbar_bootstrap_predict(xs, us, alpha0, samplers, f, sol0, targets), args.reps)
                g0 = b + sol0.f
                point_ms = _timed(lambda: engine.mbar_eval(us, alpha0, g0 - g0.max(), sol0.upiv, None), args.reps)
                rec = {
                    "K": K, "n_per_state": n, "N_total": NT, "C": C, "nrep": nrep, "n_alpha": 8,
                    "boot_solve_ms": round(solve_ms, 3), "boot_evaluations": len(evals),
                    "boot_max_df": float(np.abs(f - sol0.f).max()),
                    "boot_eval_pass_ms": round(eval_ms, 3), "eval_terms_per_s": nrep * NT * K / eval_ms * 1e3,
                    "point_eval_pass_ms": round(point_ms, 4), "point_eval_terms_per_s": NT * K / point_ms * 1e3,
                    "boot_predict_ms": round(pred_ms, 3), "boot_total_ms": round(solve_ms + pred_ms, 3),
                    "loop_replicates_timed": 0, "loop_ms_per_replicate": None, "loop_total_ms_scaled_to_nrep": None,
                    "loop_over_boot": None, "csrc_sha": _build.csrc_sha(),
                }
                if not args.no_loop:
                    def one(r):
                        cs = [sm.rows(r, r + 1).freq()[0] for sm in samplers]
                        states = [txa.beta.factory_extrapmodel(beta=a, data=txa.factory_data_values(
                            uv=DeviceDataArray(torch.repeat_interleave(u, c), ("rec",)),
                            xv=DeviceDataArray(torch.repeat_interleave(x, c, dim=0), ("rec", "val")), order=1, central=False))
                            for a, u, x, c in zip(alpha0, us, xs, cs)]
                        return txa.MBARModel(states).predict(targets).values

                    one(0)
                    torch.cuda.synchronize()
                    nloop = nrep if n <= args.loop_full_below else min(4, nrep)
                    t0 = time.perf_counter()
                    for r in range(nloop):
                        one(r)
                    torch.cuda.synchronize()
                    per = (time.perf_counter() - t0) * 1e3 / nloop
                    rec.update(loop_replicates_timed=nloop, loop_ms_per_replicate=round(per, 3),
                               loop_total_ms_scaled_to_nrep=round(per * nrep, 1),
                               loop_over_boot=round(per * nrep / (solve_ms + pred_ms), 2))
                print(json.dumps(rec), flush=True)
                del us, xs, sol0, samplers
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
