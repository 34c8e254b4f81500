"""Writes tests/golden/resample_fp64_parent.npz: inputs and outputs of the FP64 bootstrap (txm_resample_vals, path "fp64")
on three small shapes -- an unweighted and a weighted scale-mode call and a weighted parity-mode call.  Run once on an
MI355X with the build BEFORE the finalize kernels learned the empty state (`python tests/golden/make_resample_golden.py`);
tests/test_resample_kernel_gpu.py holds every later build to these bits: a replicate whose weight sum is not zero is not to
change.  Do not regenerate it to make that test pass."""

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent


def make_inputs():
    rng = np.random.default_rng(20261019)

    def gas(N, C):
        u = rng.normal(174.85, 5.31, N)
        x = rng.normal(0.0, 1.0, C)[None, :] + rng.normal(1e-3, 5e-4, C)[None, :] * u[:, None] + rng.normal(0, 0.05, (N, C))
        return x, u

    d = {}
    d["in_x1"], d["in_u1"] = gas(2053, 5)           # unweighted, device sampler, two powers per column
    d["in_x2"], d["in_u2"] = gas(1100, 33)          # weighted, device sampler, two column groups
    d["in_w2"] = rng.random(1100) + 0.05
    d["in_x3"], d["in_u3"] = gas(777, 3)            # weighted, explicit counts, shorter than one sampler tile
    d["in_w3"] = rng.random(777) + 0.05
    d["in_f3"] = rng.multinomial(777, np.full(777, 1.0 / 777), size=17).astype(np.int64)
    return d


def compute(eng, d):
    import torch

    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()  # noqa: E731
    out = {}
    out["out_scale_unweighted"] = eng.resample_vals(dev(d["in_x1"]), dev(d["in_u1"]), 4, sampler=eng.DeviceSampler(11, 17, len(d["in_u1"])),
                                                    path="fp64")
    out["out_scale_weighted"] = eng.resample_vals(dev(d["in_x2"]), dev(d["in_u2"]), 3, w=dev(d["in_w2"]),
                                                  sampler=eng.DeviceSampler(12, 65, len(d["in_u2"]), rep0=7), path="fp64")
    out["out_explicit_weighted"] = eng.resample_vals(dev(d["in_x3"]), dev(d["in_u3"]), 8, w=dev(d["in_w3"]), freq=dev(d["in_f3"]))
    return {k: v.cpu().numpy() for k, v in out.items()}


if __name__ == "__main__":
    sys.path.insert(0, str(HERE.parent.parent))
    import thermoextrap_amd as txa
    from thermoextrap_amd import engine

    txa.require_gpu()
    d = make_inputs()
    dest = Path(sys.argv[1]) if len(sys.argv) > 1 else HERE / "resample_fp64_parent.npz"
    np.savez(dest, **d, **compute(engine, d))
    print("wrote", dest)
