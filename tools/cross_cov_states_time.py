"""The cross-column delta-method covariance of a state collection, timed at BASELINE config 5's shape:
64 states x N = 1e6 samples x 4 observables, order 3, the generator of tools/bench_states.py.

Three arms alternate inside one process after a warm-up call each, fresh models in every repetition (nothing cached: a
caller's first call):
  (a) loop      [st.derivs_cross_cov() for st in coll] -- a copy to the host, the host algebra and the three launches of
                txm_influence_cross_cov PER STATE;
  (b) batched   StateCollection.derivs_cross_cov() -- one copy, the host algebra, ONE txm_influence_cross_cov_batched
                launch set for all states;
  (d) bootstrap coll.resample(nrep=1000) -> derivs() -> the covariance over rep of all (column, order) pairs per state:
                the only route to the cross blocks of a collection without the delta method.
Then (c), the three batched kernels alone (engine.influence_cross_cov_batched between HIP events), with the bytes they have
to read, 8 (C + 1) sum_s n_s.  A second run has ragged states, n_s uniform in [2e5, 1e6] from a fixed seed -- what
timeseries.decorrelate leaves.

    python tools/cross_cov_states_time.py                 # both runs, 10 repetitions
    python tools/cross_cov_states_time.py --n 1e5 --reps 3

One JSON line per run: median, min and max of every arm in ms (host clocks around work that ends in a copy to the host and a
device synchronise).  At these sizes every state's budget binds (q = 8 CUs / 64 workgroups against 3907 shares), so (a)
and (b) agree to rounding, not bit for bit: the largest deviation relative to the diagonal scale is printed.
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


def _stats(ts):
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


def _alternate(arms: dict, reps: int) -> dict:
    for fn in arms.values():          # one warm-up call of every arm
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


def run(args, ns, tag):
    import bench_states
    import thermoextrap_amd as txa
    from thermoextrap_amd import _build, engine
    from thermoextrap_amd.moments import DeviceDataArray

    S, C, order = len(ns), args.c, args.order
    datas = []
    for s, n in enumerate(ns):
        xx, uu = bench_states._state_xu(torch, s, int(ns.max()), C)      # the generator's stream of state s, cut to n_s samples
        xx, uu = xx[:n].contiguous(), uu[:n].contiguous()
        datas.append(txa.DataCentralMomentsVals.from_vals(xv=DeviceDataArray(xx, ("rec", "val")), uv=DeviceDataArray(uu, ("rec",)),
                                                          order=order, central=True))
    torch.cuda.synchronize()

    def fresh():
        return txa.models.StateCollection([txa.beta.factory_extrapmodel(1.0 + 0.1 * s, d) for s, d in enumerate(datas)])

    seeds = iter(range(100, 1 << 30))
    n_ord = order + 1

    def bootstrap():
        boot = fresh().resample({"nrep": args.nrep, "device": True, "seed": next(seeds)})
        out = []
        for m in boot:
            d = m.derivs().transpose("rep", "val", "order").values.reshape(args.nrep, C * n_ord)
            out.append(np.cov(d, rowvar=False))
        return out

    arms = {
        "a_loop": lambda: [st.derivs_cross_cov() for st in fresh()],
        "b_batched": lambda: fresh().derivs_cross_cov(),
        "d_bootstrap": bootstrap,
    }
    ts = _alternate(arms, args.reps)
    q = engine._L().txm_influence_cross_cov_batched_grid(S, 10**12, C)
    rec = {"what": "derivs_cross_cov of a state collection", "states": tag, "S": S, "C": C, "order": order,
           "n_min": int(ns.min()), "n_max": int(ns.max()), "n_sum": int(ns.sum()), "nrep_bootstrap": args.nrep, "reps": args.reps,
           "q_workgroups_per_state": int(q), "states_capped": int(sum(-(-int(n) // 256) > q for n in ns)),
           "workspace_MB": round(engine._L().txm_influence_cross_cov_batched_ws_bytes(S, int(ns.max()), C, n_ord, n_ord) / 1e6, 2),
           "csrc_sha": _build.csrc_sha(), "device": torch.cuda.get_device_name()}
    for k, v in ts.items():
        rec[k] = _stats(v)
    a, b = rec["a_loop"], rec["b_batched"]
    rec["loop_over_batched_median"] = round(a["median_ms"] / b["median_ms"], 2)
    rec["loop_minus_batched_median_ms"] = round(a["median_ms"] - b["median_ms"], 4)
    rec["loop_spread_ms"] = round(a["max_ms"] - a["min_ms"], 4)
    rec["ab_rule_met"] = bool(a["median_ms"] - b["median_ms"] > 3.0 * (a["max_ms"] - a["min_ms"]))
    rec["bootstrap_over_batched_median"] = round(rec["d_bootstrap"]["median_ms"] / b["median_ms"], 2)
    # the two paths against each other: the same sums in another order where a state's budget binds
    loop = np.stack([st.derivs_cross_cov().values for st in fresh()])                     # [S, i, j, c, c']
    bat = fresh().derivs_cross_cov().values
    diag = np.sqrt(np.abs(np.einsum("siicc->sic", loop)))
    scale = diag[:, :, None, :, None] * diag[:, None, :, None, :]
    rec["bits_equal"] = bool(np.array_equal(loop, bat))
    rec["max_dev_over_diagonal_scale"] = float((np.abs(loop - bat) / scale).max())

    # ---- (c) the three batched kernels alone
    xs = [d.xv.tensor for d in datas]
    us = [d.uv.tensor for d in datas]
    st = torch.stack([d.dxduave.device_values.reshape(-1, 2, n_ord) for d in datas])
    cu, cx = st[:, 0, 0, 1].contiguous(), st[:, :, 1, 0].contiguous()
    gen = torch.Generator(device="cuda").manual_seed(11)
    ca = torch.randn((S, C, n_ord, n_ord), dtype=torch.float64, device="cuda", generator=gen)
    cb = torch.randn((S, C, n_ord, n_ord), dtype=torch.float64, device="cuda", generator=gen)
    engine.influence_cross_cov_batched(xs, us, ca, cb, cu, cx)
    evs = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        engine.influence_cross_cov_batched(xs, us, ca, cb, cu, cx)
        e1.record()
        evs.append((e0, e1))
    torch.cuda.synchronize()
    kt = [e0.elapsed_time(e1) for e0, e1 in evs]
    nbytes = 8 * int(ns.sum()) * (C + 1)
    ks = _stats(kt)
    rec["c_kernels"] = {**ks, "bytes": nbytes, "TBs_at_median": round(nbytes / ks["median_ms"] * 1e-9, 3),
                        "measured": "HIP events around engine.influence_cross_cov_batched (table upload + three launches)"}
    # one state's single call alone, for the loop's floor
    evs = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        engine.influence_cross_cov(xs[0], us[0], ca[0], cb[0], float(cu[0]), cx[0])
        e1.record()
        evs.append((e0, e1))
    torch.cuda.synchronize()
    rec["single_call_state0"] = _stats([e0.elapsed_time(e1) for e0, e1 in evs][1:] or [0.0])
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--states", type=int, default=64)
    ap.add_argument("--n", type=float, default=1e6)
    ap.add_argument("--c", type=int, default=4)
    ap.add_argument("--order", type=int, default=3)
    ap.add_argument("--nrep", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()

    import thermoextrap_amd as txa

    txa.require_gpu()
    N = int(args.n)
    run(args, np.full(args.states, N, dtype=np.int64), "one N")
    ragged = np.random.default_rng(2024).integers(N // 5, N + 1, size=args.states)
    run(args, ragged, "ragged N, uniform in [N / 5, N]")


if __name__ == "__main__":
    main()
