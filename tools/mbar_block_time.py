"""Timing of the blocked (batch-means) MBAR error bars on the device: the block pass (txm_mbar_block_cov through the C
ABI) next to ``txm_mbar_cov``'s pass on the same operands in the same process, and the whole blocked route next to the
route it replaces, ``timeseries.decorrelate_states`` -> a new solve on the subsample -> the Theta-form error bar.

    python tools/mbar_block_time.py                          # K in {4, 8} x 2.5e7 per state x C in {1, 32}, B = 1024
    python tools/mbar_block_time.py --k 4 --n 1000000 --c 1  # one shape

One JSON line per shape, 8 targets.  Times are host clocks around work that ends in a device synchronise: the median of
--reps calls after one warm-up call.  The energies are moving averages of 8 white-noise values (statistical inefficiency
about 8), the observables 0.02 (c + 1) u plus white noise.

  cov_pass_ms         txm_mbar_cov (max pass, contraction, final kernel), outputs left on the device
  block_pass_ms       txm_mbar_block_cov with ``levels`` levels: block sums, centring, merges, Gram passes
  blocked_call_ms     what ``MBARModel.predict_with_error(block=B)`` does behind the cached solve: predict, both passes,
                      the copies to the host and the host algebra l^T Gamma l
  theta_call_ms       the same for ``predict_with_error()`` on the full data (predict, txm_mbar_cov, host algebra)
  block_lengths_ms    timeseries.block_lengths (what proposes B; the lag scan decorrelate_states needs as well)
  decorrelate_ms, solve_sub_ms, theta_sub_call_ms, n_sub      the route without blocks: subsample every state by its
                      statistical inefficiency, solve MBAR anew on the subsample, Theta-form error bar there
  solve_full_ms       the solve on the full data (both routes need it for the mean; a model caches it)
The decorrelate route is timed for C <= --route-c-max only (its lag scan runs over 2 C + 1 series per state).
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


def _timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), max(ts) - min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, nargs="*", default=[4, 8])
    ap.add_argument("--n", type=float, nargs="*", default=[2.5e7])
    ap.add_argument("--c", type=int, nargs="*", default=[1, 32])
    ap.add_argument("--block", type=int, default=1024)
    ap.add_argument("--levels", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--route-c-max", type=int, default=1)
    args = ap.parse_args()

    import thermoextrap_amd as txa
    from thermoextrap_amd import _build, engine, timeseries

    txa.require_gpu()
    L = engine._L()
    gen = torch.Generator(device="cuda").manual_seed(0)
    sd, mu, w = 10.0, 500.0, 8
    dp, ip = ct.POINTER(ct.c_double), ct.POINTER(ct.c_int64)
    for K in args.k:
        for n in (int(v) for v in args.n):
            alpha0 = 1.0 + 0.05 * np.arange(K)                  # mean shift sd / 2 between neighbours
            us = []
            for a in alpha0:
                z = torch.randn(n + w, dtype=torch.float64, device="cuda", generator=gen).cumsum(0)
                us.append(((z[w:] - z[:-w]) / np.sqrt(w)) * sd + (mu - sd * sd * a))
                del z
            targets = alpha0[0] + np.linspace(-0.05, 0.05 * K, 8)
            t0 = time.perf_counter()
            sol = engine.mbar_solve(us, alpha0)
            torch.cuda.synchronize()
            solve_ms = (time.perf_counter() - t0) * 1e3
            ns = np.full(K, float(n))
            Gs = engine.mbar_gram(us, alpha0, sol)
            pinv = engine.mbar_reduced_pinv(Gs, ns)
            for C in args.c:
                xs = [0.02 * (1 + torch.arange(C, dtype=torch.float64, device="cuda"))[None, :] * u[:, None] +
                      0.1 * torch.randn((n, C), dtype=torch.float64, device="cuda", generator=gen) for u in us]
                means = engine.mbar_predict(xs, us, alpha0, sol.f, sol.logD, targets, upiv=sol.upiv)
                tab, keep, _, _ = engine._mbar_table(us, xs)
                a0 = np.ascontiguousarray(alpha0, dtype=np.float64)
                g, _ = engine.mbar_solution_g(ns, a0, sol)
                g = np.ascontiguousarray(g)
                al = np.ascontiguousarray(targets, dtype=np.float64)
                blk = np.full(K, args.block, dtype=np.int64)
                n64 = np.full(K, n, dtype=np.int64)
                M = engine.mbar_block_width(K, 8, C)
                out = torch.empty((8, 1 + K + C * (1 + K)), dtype=torch.float64, device="cuda")
                lnw = torch.empty(8, dtype=torch.float64, device="cuda")
                gamma = torch.empty((args.levels, M, M), dtype=torch.float64, device="cuda")
                nbl = torch.empty((args.levels, K), dtype=torch.int64, device="cuda")
                cbytes = L.txm_mbar_cov_ws_bytes(K, C, 8)
                wsc = engine.workspace(cbytes, tag="mbar_cov")
                plan = (ct.c_int64 * 7)()
                engine.check(L.txm_mbar_block_cov_plan(n64.ctypes.data_as(ip), blk.ctypes.data_as(ip), K, C, 8, args.levels,
                                                       ct.c_size_t(-1).value, plan), "txm_mbar_block_cov_plan")
                wsb = engine.workspace(int(plan[5]), tag="mbar_block")

                def cov_pass():
                    engine.check(L.txm_mbar_cov(tab, K, C, float(sol.upiv), a0.ctypes.data_as(dp), g.ctypes.data_as(dp),
                                                engine._ptr(sol.logD), al.ctypes.data_as(dp), 8, engine._ptr(means),
                                                engine._ptr(out), engine._ptr(lnw), engine._ptr(wsc), cbytes, engine._stream()),
                                 "txm_mbar_cov")

                def block_pass():
                    engine.check(L.txm_mbar_block_cov(tab, K, C, float(sol.upiv), a0.ctypes.data_as(dp), g.ctypes.data_as(dp),
                                                      engine._ptr(sol.logD), al.ctypes.data_as(dp), 8, engine._ptr(means),
                                                      engine._ptr(lnw), blk.ctypes.data_as(ip), args.levels, engine._ptr(gamma),
                                                      engine._ptr(nbl), engine._ptr(wsb), int(plan[5]), engine._stream()),
                                 "txm_mbar_block_cov")

                def blocked_call():
                    mn = engine.mbar_predict(xs, us, alpha0, sol.f, sol.logD, targets, upiv=sol.upiv)
                    res = engine.mbar_block_gamma(xs, us, alpha0, sol, targets, mn, args.block, n_levels=args.levels)
                    Lm = engine.mbar_block_coef_mean(Gs, ns, res.b, pinv=pinv)
                    return engine.mbar_block_variance(res.gamma[0], Lm)

                def theta_call(xs_, us_, sol_, Gs_, ns_, pinv_):
                    mn = engine.mbar_predict(xs_, us_, alpha0, sol_.f, sol_.logD, targets, upiv=sol_.upiv)
                    _, _, yy, b = engine.mbar_cov_sums(xs_, us_, alpha0, sol_, targets, mn)
                    return engine.mbar_mean_variance(Gs_, ns_, yy, b, pinv=pinv_)

                cov_ms, cov_spread = _timed(cov_pass, args.reps)
                blk_ms, blk_spread = _timed(block_pass, args.reps)
                call_ms, _ = _timed(blocked_call, args.reps)
                theta_ms, _ = _timed(lambda: theta_call(xs, us, sol, Gs, ns, pinv), args.reps)
                var_b = blocked_call()
                var_t = theta_call(xs, us, sol, Gs, ns, pinv)
                rec = {
                    "K": K, "n_per_state": n, "N_total": K * n, "C": C, "n_alpha": 8, "block": args.block,
                    "levels": args.levels, "M": M, "blocks": int(plan[1]), "gram_workgroups": int(plan[4]),
                    "ws_block_MB": round(int(plan[5]) / 1e6, 1), "cov_pass_ms": round(cov_ms, 3),
                    "cov_pass_spread_ms": round(cov_spread, 3), "block_pass_ms": round(blk_ms, 3),
                    "block_pass_spread_ms": round(blk_spread, 3), "block_over_cov": round(blk_ms / cov_ms, 2),
                    "blocked_call_ms": round(call_ms, 3), "theta_call_ms": round(theta_ms, 3),
                    "solve_full_ms": round(solve_ms, 1), "var_blocked_over_theta": round(float(np.median(var_b / var_t.reshape(-1))), 2),
                    "block_lengths_ms": None, "decorrelate_ms": None, "solve_sub_ms": None, "theta_sub_call_ms": None,
                    "n_sub": None, "var_sub_over_blocked": None, "csrc_sha": _build.csrc_sha(),
                }
                if C <= args.route_c_max:
                    t0 = time.perf_counter()
                    timeseries.block_lengths(us, xs)
                    torch.cuda.synchronize()
                    rec["block_lengths_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                    t0 = time.perf_counter()
                    dec = timeseries.decorrelate_states(us, xs)
                    torch.cuda.synchronize()
                    rec["decorrelate_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                    us2 = [d[0].tensor.contiguous() for d in dec]
                    xs2 = [d[1].tensor.contiguous() for d in dec]
                    t0 = time.perf_counter()
                    sol2 = engine.mbar_solve(us2, alpha0)
                    torch.cuda.synchronize()
                    rec["solve_sub_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                    ns2 = np.array([float(u.shape[0]) for u in us2])
                    Gs2 = engine.mbar_gram(us2, alpha0, sol2)
                    pinv2 = engine.mbar_reduced_pinv(Gs2, ns2)
                    sub_ms, _ = _timed(lambda: theta_call(xs2, us2, sol2, Gs2, ns2, pinv2), args.reps)
                    var_s = theta_call(xs2, us2, sol2, Gs2, ns2, pinv2)
                    rec.update(theta_sub_call_ms=round(sub_ms, 3), n_sub=[int(v) for v in ns2],
                               var_sub_over_blocked=round(float(np.median(var_s.reshape(-1) / var_b)), 2))
                    del dec, us2, xs2, sol2
                print(json.dumps(rec), flush=True)
                del xs, means, keep, gamma
                torch.cuda.empty_cache()
            del us, sol
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
