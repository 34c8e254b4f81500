"""Writes tests/golden/reduce_unweighted_parent.npz: inputs and outputs of the UNWEIGHTED reduction entry points on a few
small shapes, one per kernel of txm_reduce.hip.  Run once on an MI355X with the build BEFORE the weighted pivot
(`python tests/golden/make_reduce_golden.py`); tests/test_reduce_kernels_gpu.py holds every later build to these bits --
the unweighted kernels and their launch sequence are not to change.  Do not regenerate it to make that test pass."""

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent


def make_inputs():
    rng = np.random.default_rng(20261018)

    def gas(N, C):
        u = rng.normal(174.85, 5.31, N)
        x = rng.normal(0.0, 1.0, C)[None, :] + rng.normal(1e-3, 5e-4, C)[None, :] * u[:, None] + rng.normal(0, 0.05, (N, C))
        return x, u

    d = {}
    d["in_x1"], d["in_u1"] = gas(301, 5)            # row-major, VEC = 1
    d["in_x2"], d["in_u2"] = gas(2051, 8)           # row-major, VEC = 2, several blocks
    d["in_x3"], d["in_u3"] = gas(1000, 3)           # (val, rec)
    d["in_rows"] = rng.normal(3.0, 1.5, (3, 777))   # 1-D
    d["in_x4"], d["in_u4"] = gas(500, 4)            # batched, with x2[:500, :4] as the other state
    return d


def compute(eng, d):
    import torch

    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).cuda()  # noqa: E731
    out = {}
    out["out_rowmajor_vec1"] = eng.reduce_vals(dev(d["in_x1"]), dev(d["in_u1"]), 4)
    out["out_rowmajor_vec2"] = eng.reduce_vals(dev(d["in_x2"]), dev(d["in_u2"]), 3)
    out["out_colmajor"] = eng.reduce_vals(dev(d["in_x3"].T).t(), dev(d["in_u3"]), 4)
    out["out_single_series"] = eng.reduce_vals(dev(d["in_x3"][:, 0]), dev(d["in_u3"]), 8)
    out["out_1d"] = eng.reduce_vals_1d(dev(d["in_rows"]), 4)
    out["out_batched"] = eng.reduce_vals_batched([dev(d["in_x4"]), dev(d["in_x2"][:500, :4])],
                                                 [dev(d["in_u4"]), dev(d["in_u2"][:500])], 2)
    st = torch.zeros((5, 2, 5), dtype=torch.float64, device="cuda")
    eng.push_vals(st, dev(d["in_x1"][:100]), dev(d["in_u1"][:100]))
    out["out_push"] = eng.push_vals(st, dev(d["in_x1"][100:]), dev(d["in_u1"][100:]))
    piv = eng.reduce_pivot(dev(d["in_x2"][:1000]), dev(d["in_u2"][:1000]))
    sums = torch.stack([eng.reduce_sums(dev(d["in_x2"][a:b]), dev(d["in_u2"][a:b]), 3, piv) for a, b in ((0, 1000), (1000, 2051))])
    out["out_pivot"] = piv
    out["out_sharded"] = eng.sums_to_state(sums, piv)
    return {k: v.cpu().numpy() for k, v in out.items()}


if __name__ == "__main__":
    sys.path.insert(0, str(HERE.parent.parent))
    import thermoextrap_amd as txa
    from thermoextrap_amd import engine

    txa.require_gpu()
    d = make_inputs()
    dest = Path(sys.argv[1]) if len(sys.argv) > 1 else HERE / "reduce_unweighted_parent.npz"
    np.savez(dest, **d, **compute(engine, d))
    print("wrote", dest)
