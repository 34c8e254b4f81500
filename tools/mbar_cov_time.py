"""Timing of MBAR's asymptotic error bars on the device: the covariance pass (engine.mbar_cov_sums, txm_mbar_cov) next
to ``txm_mbar_predict`` for the same targets in the same process, and next to what a user does without it --
``MBARModel.bootstrap`` with nrep = 100 (the batched solve plus the replicates' predictions).

    python tools/mbar_cov_time.py                                   # K in {4, 8} x 2.5e7 per state x C in {1, 32}
    python tools/mbar_cov_time.py --k 8 --n 25000000 --c 32 --no-boot      # one shape (a rocprofv3 --kernel-trace run)

One JSON line per shape, 8 targets.  Times are host clocks around work that ends in a device synchronise: the median of
--reps calls after one warm-up call.  ``cov_pass_ms`` covers the max pass, the contraction, the finalize and the copy of
the n_alpha x (1 + K + C (1 + K)) sums to the host; ``gram_pass_ms`` is the one evaluation pass at the solution that
gives the sampled block (once per model); ``host_algebra_ms`` the K x K pseudo-inverse and the variances.
``cov_row_col_products_per_s`` = N_total x 8 targets x (K + 1) rows x (C + 1) columns per second.
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
    ap.add_argument("--n", type=float, nargs="*", default=[2.5e7])
    ap.add_argument("--c", type=int, nargs="*", default=[1, 32])
    ap.add_argument("--nrep", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-boot", action="store_true")
    args = ap.parse_args()

    import thermoextrap_amd as txa
    from thermoextrap_amd import _build, engine

    txa.require_gpu()
    gen = torch.Generator(device="cuda").manual_seed(0)
    sd, mu, seed = 10.0, 500.0, 2718
    for K in args.k:
        for n in (int(v) for v in args.n):
            for C in args.c:
                alpha0 = 1.0 + 0.05 * np.arange(K)                  # mean shift sd / 2 between neighbours
                NT = K * n
                us = [torch.randn(n, dtype=torch.float64, device="cuda", generator=gen) * sd + (mu - sd * sd * a) for a in alpha0]
                xs = [torch.randn(n, C, dtype=torch.float64, device="cuda", generator=gen).add_(0.01 * u[:, None]) for u in us]
                targets = alpha0[0] + np.linspace(-0.05, 0.05 * K, 8)
                sol = engine.mbar_solve(us, alpha0)
                ns = np.full(K, float(n))
                means = engine.mbar_predict(xs, us, alpha0, sol.f, sol.logD, targets, upiv=sol.upiv)
                pred_ms = _timed(lambda: engine.mbar_predict(xs, us, alpha0, sol.f, sol.logD, targets, upiv=sol.upiv), args.reps)
                cov_ms = _timed(lambda: engine.mbar_cov_sums(xs, us, alpha0, sol, targets, means), args.reps)
                gram_ms = _timed(lambda: engine.mbar_gram(us, alpha0, sol), args.reps)
                Q, B, yy, b = engine.mbar_cov_sums(xs, us, alpha0, sol, targets, means)
                Gs = engine.mbar_gram(us, alpha0, sol)
                t0 = time.perf_counter()
                var = engine.mbar_mean_variance(Gs, ns, yy, b)
                host_ms = (time.perf_counter() - t0) * 1e3
                rec = {
                    "K": K, "n_per_state": n, "N_total": NT, "C": C, "n_alpha": 8,
                    "cov_pass_ms": round(cov_ms, 3), "predict_ms": round(pred_ms, 3), "cov_over_predict": round(cov_ms / pred_ms, 2),
                    "gram_pass_ms": round(gram_ms, 3), "host_algebra_ms": round(host_ms, 3),
                    "cov_row_col_products_per_s": NT * 8 * (K + 1) * (C + 1) / cov_ms * 1e3,
                    "cov_x_bytes_per_s": NT * C * 8 / cov_ms * 1e3,
                    "err_min": float(np.sqrt(var.min())), "err_max": float(np.sqrt(var.max())),
                    "effective_samples_min": float(1.0 / Q.max()),
                    "nrep": args.nrep, "boot_total_ms": None, "boot_over_cov": None, "boot_std_over_err_median": None,
                    "csrc_sha": _build.csrc_sha(),
                }
                if not args.no_boot:
                    samplers = [engine.DeviceSampler(seed, args.nrep, n, rep0=s * args.nrep) for s in range(K)]

                    def boot():
                        f = engine.mbar_bootstrap_solve(us, alpha0, samplers, sol)
                        return engine.mbar_bootstrap_predict(xs, us, alpha0, samplers, f, sol, targets)

                    boot_ms = _timed(boot, 1)
                    rep = boot().cpu().numpy()                       # (nrep, 8, C)
                    rec.update(boot_total_ms=round(boot_ms, 3), boot_over_cov=round(boot_ms / (cov_ms + gram_ms), 1),
                               boot_std_over_err_median=float(np.median(rep.std(axis=0, ddof=1) / np.sqrt(var))))
                    del samplers
                print(json.dumps(rec), flush=True)
                del us, xs, sol, means
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
