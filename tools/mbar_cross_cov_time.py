"""Timing of MBAR's covariance across columns and targets on the device: the Gram pass (txm_mbar_cross_cov, both modes)
next to txm_mbar_cov on the same operands in the same process -- the pass it follows, and the yardstick: at C = 32 in
same-alpha mode both issue 3 x 8 x N / 4 FP64 MFMAs -- and next to what a user did without it, ``MBARModel.bootstrap`` with
nrep = 100 (the batched solve, the replicates' predictions) and a covariance over ``rep``.

    python tools/mbar_cross_cov_time.py                             # K in {4, 8} x 2.5e7 per state x C in {1, 32}
    python tools/mbar_cross_cov_time.py --k 8 --c 32 --no-boot      # one shape (a rocprofv3 --kernel-trace run)

One JSON line per (shape, mode), 8 targets.  Times are host clocks around work that ends in a device synchronise: the
median of --reps calls after one warm-up call; the two device passes are timed through the C ABI alone (no copy of the
result to the host), ``engine_ms`` is engine.mbar_cross_cov_sums whole (both passes and the copies).  Counted from the shapes:
``mfma`` = tile pairs x row targets x 8 accumulators x ceil(N_s / 64) x 16 per state, 2048 FLOP each; ``exps`` = one per
(sample, target) and workgroup that visits the sample; ``bytes_min`` = x, u and logD once (what HBM must deliver),
``bytes_requested`` = what the workgroups load (each pair reads its two column tiles again: the caches' share).  ``bound``
names the larger of mfma FLOP / 78.6 TFLOP/s (the FP64 matrix peak) and bytes_min / 8 TB/s, ``share_of_bound`` that time over
the measured one.
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

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

PEAK_FLOPS, PEAK_BYTES = 78.6e12, 8.0e12


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


def counts(ns, C, na, cross):
    """(mfma, exps, bytes_min, bytes_requested) of one Gram pass from the shapes."""
    T = -(-C // 16)
    pairs, rows = T * (T + 1) // 2, (na if cross else 1)
    NA = 1 if na == 1 else 2 if na == 2 else 4 if na <= 4 else 8
    steps = sum(-(-n // 64) * 16 for n in ns)
    N = sum(ns)
    cols = sum(min(16, C - 16 * i) + (0 if i == j else min(16, C - 16 * j)) for i in range(T) for j in range(i, T))
    return (pairs * rows * NA * steps, pairs * rows * NA * N, N * (C + 2) * 8, rows * N * (cols + 2 * pairs) * 8)


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
    from thermoextrap_amd import _build, _lib, engine

    txa.require_gpu()
    L = _lib.load()
    dp = ct.POINTER(ct.c_double)
    gen = torch.Generator(device="cuda").manual_seed(0)
    sd, mu, seed = 10.0, 500.0, 2718
    for K in args.k:
        for n in (int(v) for v in args.n):
            for C in args.c:
                alpha0 = 1.0 + 0.05 * np.arange(K)                  # mean shift sd / 2 between neighbours
                us = [torch.randn(n, dtype=torch.float64, device="cuda", generator=gen) * sd + (mu - sd * sd * a) for a in alpha0]
                xs = [torch.randn(n, C, dtype=torch.float64, device="cuda", generator=gen).add_(0.01 * u[:, None]) for u in us]
                targets = np.ascontiguousarray(alpha0[0] + np.linspace(-0.05, 0.05 * K, 8))
                sol = engine.mbar_solve(us, alpha0)
                ns = [n] * K
                means = engine.mbar_predict(xs, us, alpha0, sol.f, sol.logD, targets, upiv=sol.upiv).contiguous()
                tab, keep, nsf, _ = engine._mbar_table(us, xs)
                a0 = np.ascontiguousarray(alpha0, dtype=np.float64)
                g = np.ascontiguousarray(engine.mbar_solution_g(nsf, a0, sol)[0])
                nbytes = L.txm_mbar_cov_ws_bytes(K, C, 8)
                ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
                out = torch.empty((8, 1 + K + C * (1 + K)), dtype=torch.float64, device="cuda")
                lnw = torch.empty(8, dtype=torch.float64, device="cuda")
                gram = torch.empty((8 * C) ** 2, dtype=torch.float64, device="cuda")

                def cov_pass():
                    _lib.check(L.txm_mbar_cov(tab, K, C, float(sol.upiv), a0.ctypes.data_as(dp), g.ctypes.data_as(dp),
                                              engine._ptr(sol.logD), targets.ctypes.data_as(dp), 8, engine._ptr(means),
                                              engine._ptr(out), engine._ptr(lnw), engine._ptr(ws), nbytes, engine._stream()),
                               "txm_mbar_cov")

                def gram_pass(cross):
                    _lib.check(L.txm_mbar_cross_cov(tab, K, C, float(sol.upiv), engine._ptr(sol.logD), targets.ctypes.data_as(dp),
                                                    8, engine._ptr(means), engine._ptr(lnw), cross, engine._ptr(gram),
                                                    engine._ptr(ws), nbytes, engine._stream()), "txm_mbar_cross_cov")

                cov_ms = _timed(cov_pass, args.reps)
                boot_ms = boot_cov_ms = None
                if not args.no_boot:
                    def boot(nrep):
                        samplers = [engine.DeviceSampler(seed, nrep, n, rep0=s * nrep) for s in range(K)]
                        f = engine.mbar_bootstrap_solve(us, alpha0, samplers, sol)
                        rep = engine.mbar_bootstrap_predict(xs, us, alpha0, samplers, f, sol, targets)      # (nrep, 8, C)
                        return torch.cov(rep.reshape(nrep, -1).T).cpu()

                    boot(2)                                          # warm-up: code objects, allocations
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    boot(args.nrep)
                    torch.cuda.synchronize()
                    boot_ms = (time.perf_counter() - t0) * 1e3
                for cross in (0, 1):
                    plan = (ct.c_int64 * 4)()
                    _lib.check(L.txm_mbar_cross_cov_plan(K, C, 8, cross, n, nbytes, plan), "txm_mbar_cross_cov_plan")
                    cov_pass()
                    ms = _timed(lambda: gram_pass(cross), args.reps)
                    eng_ms = _timed(lambda: engine.mbar_cross_cov_sums(xs, us, alpha0, sol, targets, means, cross_alpha=bool(cross)),
                                    args.reps)
                    mfma, exps, bmin, breq = counts(ns, C, 8, cross)
                    t_flop, t_byte = mfma * 2048 / PEAK_FLOPS * 1e3, bmin / PEAK_BYTES * 1e3
                    rec = {
                        "K": K, "n_per_state": n, "N_total": K * n, "C": C, "n_alpha": 8, "cross_alpha": cross,
                        "plan": {"T": plan[0], "pairs": plan[1], "sample_workgroups": plan[2], "ws_bytes_used": plan[3],
                                 "workgroups": plan[1] * plan[2] * (8 if cross else 1)},
                        "gram_pass_ms": round(ms, 3), "mbar_cov_pass_ms": round(cov_ms, 3), "gram_over_cov": round(ms / cov_ms, 2),
                        "engine_ms": round(eng_ms, 3),
                        "mfma": mfma, "exps": exps, "bytes_min": bmin, "bytes_requested": breq,
                        "mfma_tflops": round(mfma * 2048 / ms * 1e-9, 2), "bytes_min_tb_per_s": round(bmin / ms * 1e-9, 3),
                        "bound": "matrix pipe" if t_flop >= t_byte else "HBM", "share_of_bound": round(max(t_flop, t_byte) / ms, 3),
                        "nrep": args.nrep, "boot_total_ms": None if boot_ms is None else round(boot_ms, 1),
                        "boot_over_engine": None if boot_ms is None else round(boot_ms / eng_ms, 1),
                        "csrc_sha": _build.csrc_sha(),
                    }
                    print(json.dumps(rec), flush=True)
                del us, xs, sol, means, keep, ws, out, gram
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
