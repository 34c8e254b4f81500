#!/usr/bin/env python
"""Time the HBM-bound reduce (txm_reduce_vals) at the north-star shape:  TXM_LIBRARY=<variant.so> python tools/reduce_time.py [N] [C] [order] [--weighted[=sparse]]
(without the flag: the unweighted protocol of the committed profiles, unchanged.  --weighted: engine.reduce_vals with uniform weights, 3 warm-up
calls, 25 timed -- the cost check of the weighted pivot; --weighted=sparse: one row in 1000 carries weight, so the pivot's subsample holds about one
weighted row and every series takes the all-rows pass)"""
import os, sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch
import thermoextrap_amd as txa
from thermoextrap_amd import engine
from bench import make_data
wmode = next((a for a in sys.argv if a.startswith("--weighted")), None)
sys.argv = [a for a in sys.argv if not a.startswith("--weighted")]
N = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
C = int(sys.argv[2]) if len(sys.argv) > 2 else 32
order = int(sys.argv[3]) if len(sys.argv) > 3 else 4
txa.require_gpu(0)
x, u = make_data(N, C, 3, torch)
b = 8.0 * N * (C + 1)
if wmode:
    w = 0.05 + torch.rand(N, dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(7))
    if wmode == "--weighted=sparse":
        w[torch.rand(N, device="cuda", generator=torch.Generator(device="cuda").manual_seed(8)) >= 1e-3] = 0.0
    for _ in range(3):
        engine.reduce_vals(x, u, order, w=w)
    torch.cuda.synchronize()
    ts = []
    for _ in range(25):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); engine.reduce_vals(x, u, order, w=w); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    print(f"{os.path.basename(os.environ.get('TXM_LIBRARY', 'default')):30s} reduce N={N:.0e} C={C} order={order} {wmode[2:]}: median {ts[12]:7.3f} ms = {(b + 8.0 * N) / ts[12] / 1e9:6.2f} TB/s  (min {ts[0]:.3f}, max {ts[-1]:.3f}, 25 runs)", flush=True)
    sys.exit(0)
engine.reduce_vals(x, u, order); torch.cuda.synchronize()
ts = []
for _ in range(15):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); engine.reduce_vals(x, u, order); e1.record(); torch.cuda.synchronize()
    ts.append(e0.elapsed_time(e1))
ts.sort()
print(f"{os.path.basename(os.environ.get('TXM_LIBRARY', 'default')):30s} reduce N={N:.0e} C={C} order={order}: median {ts[7]:7.3f} ms = {b / ts[7] / 1e9:6.2f} TB/s  (min {ts[0]:.3f})", flush=True)
