"""Timing of MBAR's reweighted histograms on the device: the histogram pass (engine.mbar_hist_sums, txm_mbar_hist) next
to ``txm_mbar_predict`` for the same targets in the same process and -- at nbins = 32 -- next to the only other route,
``predict_with_covariance``'s passes over the materialised N x nbins indicator matrix, and to ``txm_mbar_cov``'s pass at
C = 32 on that matrix.

    python tools/mbar_hist_time.py                              # K in {4, 8} x 2.5e7 per state x nbins in {32, 128, 1023}
    python tools/mbar_hist_time.py --k 8 --n 25000000 --nbins 128 --no-indicator     # one shape

One JSON line per shape, 8 targets.  Times are host clocks around work that ends in a device synchronise: the median of
--reps calls after one warm-up call.  ``hist_pass_ms`` covers the max pass, the contraction, the two final kernels and the
copy of the n_alpha x (K + 2) x (nbins + 1) sums to the host, for uniformly random bin indices; ``hist_pass_sorted_ms`` the
same for indices sorted along the samples.  ``histogram_ms`` / ``histogram_nocov_ms`` are the steps of
``MBARModel.histogram`` behind the cached solve at engine level: ``bin_index`` of the energies on the device, the pass, the
variances and (with cov) the nbins x nbins covariance per target on the host; the K x K pseudo-inverse is taken once
outside, as the model caches it.  ``indicator_*``: predict, txm_mbar_cov and txm_mbar_cross_cov on the indicator matrix.
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
    return statistics.median(ts), max(ts) - min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, nargs="*", default=[4, 8])
    ap.add_argument("--n", type=float, nargs="*", default=[2.5e7])
    ap.add_argument("--nbins", type=int, nargs="*", default=[32, 128, 1023])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-indicator", action="store_true")
    args = ap.parse_args()

    import thermoextrap_amd as txa
    from thermoextrap_amd import _build, engine

    txa.require_gpu()
    gen = torch.Generator(device="cuda").manual_seed(0)
    sd, mu = 10.0, 500.0
    for K in args.k:
        for n in (int(v) for v in args.n):
            alpha0 = 1.0 + 0.05 * np.arange(K)                  # mean shift sd / 2 between neighbours
            NT = K * n
            us = [torch.randn(n, dtype=torch.float64, device="cuda", generator=gen) * sd + (mu - sd * sd * a) for a in alpha0]
            x1 = [u[:, None] for u in us]
            targets = alpha0[0] + np.linspace(-0.05, 0.05 * K, 8)
            sol = engine.mbar_solve(us, alpha0)
            ns = np.full(K, float(n))
            Gs = engine.mbar_gram(us, alpha0, sol)
            pinv = engine.mbar_reduced_pinv(Gs, ns)
            pred_ms, _ = _timed(lambda: engine.mbar_predict(x1, us, alpha0, sol.f, sol.logD, targets, upiv=sol.upiv), args.reps)
            lo, hi = min(float(u.min()) for u in us), max(float(u.max()) for u in us)
            for nb in args.nbins:
                edges = np.histogram_bin_edges(np.empty(0), bins=nb, range=(lo, hi))
                rnd = [torch.randint(0, nb, (n,), dtype=torch.int32, device="cuda", generator=gen) for _ in us]
                srt = [torch.sort(b).values for b in rnd]
                pass_ms, spread = _timed(lambda: engine.mbar_hist_sums(rnd, us, alpha0, sol, targets, nb), args.reps)
                sorted_ms, _ = _timed(lambda: engine.mbar_hist_sums(srt, us, alpha0, sol, targets, nb), args.reps)
                del rnd, srt

                def whole(cov):
                    idx = [engine.bin_index(u, edges) for u in us]
                    H, S, T, _, _, _ = engine.mbar_hist_sums(idx, us, alpha0, sol, targets, nb)
                    var = engine.mbar_hist_variance(Gs, ns, H, S, T, pinv=pinv)
                    return var, (engine.mbar_hist_covariance(Gs, ns, H, S, T, pinv=pinv) if cov else None)

                call_ms, _ = _timed(lambda: whole(True), args.reps)
                nocov_ms, _ = _timed(lambda: whole(False), args.reps)
                energy_ms, _ = _timed(lambda: engine.mbar_hist_sums([engine.bin_index(u, edges) for u in us], us, alpha0, sol,
                                                                    targets, nb), args.reps)
                rec = {
                    "K": K, "n_per_state": n, "N_total": NT, "nbins": nb, "n_alpha": 8,
                    "hist_pass_ms": round(pass_ms, 3), "hist_pass_spread_ms": round(spread, 3),
                    "hist_pass_sorted_ms": round(sorted_ms, 3), "histogram_ms": round(call_ms, 3),
                    "histogram_nocov_ms": round(nocov_ms, 3), "bin_index_plus_pass_ms": round(energy_ms, 3),
                    "predict_ms": round(pred_ms, 3), "hist_over_predict": round(pass_ms / pred_ms, 2),
                    "mfma_per_s": (NT / 4) * 8 * (nb // 16 + 1) * -(-(K + 2) // 16) / pass_ms * 1e3,
                    "indicator_predict_ms": None, "indicator_cov_pass_ms": None, "indicator_route_ms": None,
                    "indicator_route_over_hist": None, "cov_pass_over_hist": None, "csrc_sha": _build.csrc_sha(),
                }
                if nb == 32 and not args.no_indicator:
                    xs = []
                    for u in us:
                        idx = engine.bin_index(u, edges).to(torch.int64)
                        m = torch.zeros((n, nb), dtype=torch.float64, device="cuda")
                        m.scatter_(1, idx.clamp_(0, nb - 1)[:, None], 1.0)
                        xs.append(m)
                        del idx
                    means = engine.mbar_predict(xs, us, alpha0, sol.f, sol.logD, targets, upiv=sol.upiv)
                    ipred, _ = _timed(lambda: engine.mbar_predict(xs, us, alpha0, sol.f, sol.logD, targets, upiv=sol.upiv), args.reps)
                    icov, _ = _timed(lambda: engine.mbar_cov_sums(xs, us, alpha0, sol, targets, means), args.reps)
                    iroute, _ = _timed(lambda: engine.mbar_cross_cov_sums(xs, us, alpha0, sol, targets, means), args.reps)
                    rec.update(indicator_predict_ms=round(ipred, 3), indicator_cov_pass_ms=round(icov, 3),
                               indicator_route_ms=round(ipred + iroute, 3),
                               indicator_route_over_hist=round((ipred + iroute) / pass_ms, 2),
                               cov_pass_over_hist=round(icov / pass_ms, 2))
                    del xs, means
                    torch.cuda.empty_cache()
                print(json.dumps(rec), flush=True)
            del us, x1, sol
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
