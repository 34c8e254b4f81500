"""MBAR timing on the device: the solve (engine.mbar_solve) and a predict call (engine.mbar_predict), with txm_perturb at
the same (N_total, C, 8 alphas) in the same process as the exp-bound yardstick.

    python tools/mbar_time.py                 # every shape: K in {2, 4, 8}, N per state in {1e5, 1e6, 2.5e7},
                                              # C in {1, 32}, n_alpha in {8, 64}
    python tools/mbar_time.py --n 25000000    # only that N per state (a rocprofv3 --kernel-trace --stats run)

One JSON line per shape.  Times are host clocks around work that ends in a device synchronise, the median of --reps calls
after one warm-up call.  Bytes and exps are what the algorithm needs, computed from the shapes:
  evaluation pass  8 N_total (u) + 8 N_total (logD stored)   K N_total exps (+ N_total logs)
  predict          per tile of <= 8 targets: 16 N_total (max pass: u, logD) + 8 N_total (C + 2) (x, u, logD);
                   n_alpha N_total exps
  txm_perturb      8 N_total (extremes of u) + 8 N_total (C + 1);  8 N_total exps
The samples are Gaussian energies of a common system at neighbouring alpha (mean shift of half a standard deviation) and
observables linear in u plus noise; the states are row slices of one pooled matrix, which txm_perturb reads whole.
"""

from __future__ import annotations

import argparse
import json
import math
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
    ap.add_argument("--k", type=int, nargs="*", default=[2, 4, 8])
    ap.add_argument("--n", type=float, nargs="*", default=[1e5, 1e6, 2.5e7])
    ap.add_argument("--c", type=int, nargs="*", default=[1, 32])
    ap.add_argument("--na", type=int, nargs="*", default=[8, 64])
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()

    import thermoextrap_amd as txa
    from thermoextrap_amd import _build, engine

    txa.require_gpu()
    gen = torch.Generator(device="cuda").manual_seed(0)
    sd, mu = 10.0, 500.0
    for K in args.k:
        for n in (int(v) for v in args.n):
            for C in args.c:
                alpha0 = 1.0 + 0.05 * np.arange(K)                  # mean shift sd^2 * 0.05 = sd / 2 between neighbours
                NT = K * n
                u = torch.empty(NT, dtype=torch.float64, device="cuda")
                for s in range(K):
                    u[s * n:(s + 1) * n] = torch.randn(n, dtype=torch.float64, device="cuda", generator=gen) * sd + (mu - sd * sd * alpha0[s])
                x = torch.randn(NT, C, dtype=torch.float64, device="cuda", generator=gen)
                x.add_(0.01 * u[:, None])
                us = [u[s * n:(s + 1) * n] for s in range(K)]
                xs = [x[s * n:(s + 1) * n] for s in range(K)]
                sol = engine.mbar_solve(us, alpha0)
                solve_ms = _timed(lambda: engine.mbar_solve(us, alpha0), max(1, args.reps // 2))
                g = np.log(n) + sol.f - alpha0 * sol.upiv
                eval_ms = _timed(lambda: engine.mbar_eval(us, alpha0, g - g.max(), sol.upiv, sol.logD), args.reps)
                da8 = np.linspace(-0.05, 0.05 * K, 8)
                perturb_ms = _timed(lambda: engine.perturb(x, u, da8), args.reps)
                for na in args.na:
                    targets = alpha0[0] + np.linspace(-0.05, 0.05 * K, na)
                    pred_ms = _timed(lambda: engine.mbar_predict(xs, us, alpha0, sol.f, sol.logD, targets, upiv=sol.upiv),
                                     args.reps)
                    tiles = math.ceil(na / 8)
                    eval_bytes, eval_exps = 16 * NT, K * NT
                    pred_bytes = tiles * (16 * NT + 8 * NT * (C + 2))
                    pert_bytes = 8 * NT + 8 * NT * (C + 1)
                    rec = {
                        "K": K, "n_per_state": n, "N_total": NT, "C": C, "n_alpha": na,
                        "solve_ms": round(solve_ms, 4), "newton_iterations": sol.iterations, "evaluations": sol.evaluations,
                        "gradient": sol.gradient, "eval_pass_ms": round(eval_ms, 4),
                        "eval_bytes": eval_bytes, "eval_exps": eval_exps,
                        "eval_GBs": round(eval_bytes / eval_ms * 1e-6, 1), "eval_exp_per_s": eval_exps / eval_ms * 1e3,
                        "predict_ms": round(pred_ms, 4), "predict_bytes": pred_bytes, "predict_exps": na * NT,
                        "predict_GBs": round(pred_bytes / pred_ms * 1e-6, 1), "predict_exp_per_s": na * NT / pred_ms * 1e3,
                        "perturb8_ms": round(perturb_ms, 4), "perturb8_bytes": pert_bytes,
                        "perturb8_GBs": round(pert_bytes / perturb_ms * 1e-6, 1), "perturb8_exp_per_s": 8 * NT / perturb_ms * 1e3,
                        "predict8_over_perturb8": None,
                        "csrc_sha": _build.csrc_sha(),
                    }
                    if na == 8:
                        rec["predict8_over_perturb8"] = round(pred_ms / perturb_ms, 3)
                    print(json.dumps(rec), flush=True)
                del u, x, us, xs, sol
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
