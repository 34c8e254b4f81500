"""Differential tests of txm_mbar_hist (txm_mbar_hist.hip) through the C ABI against the long-double restatement
tests/_mbar_hist_ref.py hist_sums.  g is NOT a solution (the thermodynamic-integration start plus noise) and logD is made on
the host, as in group E of tests/test_mbar_kernels_gpu.py: no other device kernel supplies an input.

Tolerances (derived, not measured; that file's):

  every entry of out   |hip - ref| <= 1e-12 sum_n kappa_n |term_n| + floor
  lnw_a                |hip - ref| <= 1e-12 kappa (1 + |ref|)

with the same kappa_n for the row of v_a^2 and the floors of tests/_mbar_hist_ref.py (derivation in its header).  Exact
claims: a column no sample fell into is 0.0; two calls give equal bits; the histogram row, the outside class included, sums
to 1 within (nbins + 2) 2^-52 -- one rounding per quotient and one per addition of the denominator, doubled.

Shapes: the smallest at which each index expression can go wrong.  Per-state counts 1, 63, 64, 65, 257 and 1000 mixed in
one call (a state ends inside a 64-sample tile; several grid-stride turns; more sample workgroups than one); K + 2 rows at
the row-tile edges (K = 14: 16 rows, one tile; 15: two; 17; 64: five); nbins + 1 columns at the bin-tile edges (15: one
full tile; 16 and 17: the outside class alone in, or second in, a second tile; 1023: 64 tiles, 16 groups of 4 with eight
targets and 2 groups of 32 with one); one and eight targets.  Every case runs under the smallest plan (one sample
workgroup) and under the full one, in guard-banded workspaces with NaN scratch and a guard-banded output.
"""

import ctypes as ct

import numpy as np
import pytest
import torch

import _mbar_hist_ref as hr
from _bands import Banded
from oracle import mbar_oracle as mo
from test_mbar_oracle_cpu import eval_inputs, steps, targets_for

pytestmark = pytest.mark.gpu
TOL = 1e-12
LD = np.longdouble
SIZE_MAX = ct.c_size_t(-1).value
MIX = [1000, 1, 63, 64, 65, 257]


def mixed(K):
    return [MIX[k % 6] if k < 6 else 20 + 3 * k for k in range(K)]


# name -> (K, nbins, n_alpha, bin pattern)
CASES = {
    "K1_nb1_na1_one_bin": (1, 1, 1, "one_bin"),
    "K3_nb15_na8_random": (3, 15, 8, "random"),
    "K14_nb16_na1_sorted": (14, 16, 1, "sorted"),
    "K15_nb17_na8_all_outside": (15, 17, 8, "all_outside"),
    "K17_nb100_na8_beyond": (17, 100, 8, "beyond"),
    "K3_nb100_na1_one_bin": (3, 100, 1, "one_bin"),
    "K64_nb1023_na8_random": (64, 1023, 8, "random"),
    "K64_nb1023_na1_sorted": (64, 1023, 1, "sorted"),
}
_cache = {}


def bin_pattern(kind, ns, nbins, rng):
    N = sum(ns)
    if kind == "one_bin":
        flat = np.full(N, nbins // 2)
    elif kind == "all_outside":
        flat = np.where(np.arange(N) % 2 == 0, -1, nbins)
    elif kind == "sorted":                     # along the pooled samples: whole 4-sample steps share a bin tile
        flat = (np.arange(N) * nbins) // N
    elif kind == "random":
        flat = rng.integers(0, nbins, N)
    elif kind == "beyond":                     # negative indices and indices >= nbins among the bins
        flat = rng.integers(-7, nbins + 9, N)
        flat[:3] = [np.iinfo(np.int32).min, np.iinfo(np.int32).max, nbins]
    else:
        raise KeyError(kind)
    return [np.ascontiguousarray(b, dtype=np.int32) for b in np.split(flat, np.cumsum(ns)[:-1])]


def reference(name):
    """(inputs, hist_sums of them), once per process: the tests that share it leave it unchanged."""
    if name not in _cache:
        K, nbins, na, kind = CASES[name]
        ns = mixed(K)
        a0 = steps(K, 0.1 if K <= 3 else 0.01)
        us, _, upiv, g = eval_inputs(a0, ns, seed=7000 + 16 * K + na)
        targets = targets_for(a0, na)
        logD = np.ascontiguousarray(mo.eval_sums(us, a0, g, upiv).logD, dtype=np.float64)
        bins = bin_pattern(kind, ns, nbins, np.random.default_rng(K + nbins))
        case = (a0, ns, us, bins, upiv, g, targets, logD, nbins)
        _cache[name] = (case, hr.hist_sums(us, bins, a0, g, upiv, targets, logD, nbins))
    return _cache[name]


@pytest.fixture(scope="module")
def eng(txm):
    from thermoextrap_amd import engine

    return engine


def run(eng, case, ws_bytes):
    """(out, lnw, plan) of one call in a guard-banded workspace of exactly ws_bytes (NaN scratch) with out and lnw in
    guard-banded buffers of their own."""
    from thermoextrap_amd import _lib

    L = _lib.load()
    a0, ns, us, bins, upiv, g, targets, logD, nbins = case
    K, na = len(ns), len(targets)
    ud = [torch.as_tensor(u, dtype=torch.float64).cuda() for u in us]
    bd = [torch.as_tensor(b).cuda() for b in bins]
    tab, keep, _, _ = eng._mbar_table(ud)
    btab = (ct.c_void_p * K)(*[b.data_ptr() for b in bd])
    a0 = np.ascontiguousarray(a0, dtype=np.float64)
    g = np.ascontiguousarray(g, dtype=np.float64)
    al = np.ascontiguousarray(targets, dtype=np.float64)
    ld = torch.as_tensor(logD).cuda()
    plan = (ct.c_int64 * 4)()
    assert L.txm_mbar_hist_plan(K, nbins, na, max(ns), ws_bytes, plan) == 0, _lib.last_error()
    assert plan[3] <= ws_bytes
    ws = Banded(ws_bytes, "nan")
    out = Banded(na * (K + 2) * (nbins + 1) * 8, "value")
    lnw = Banded(na * 8, "value")
    dp = ct.POINTER(ct.c_double)
    rc = L.txm_mbar_hist(tab, btab, K, nbins, float(upiv), a0.ctypes.data_as(dp), g.ctypes.data_as(dp), eng._ptr(ld),
                         al.ctypes.data_as(dp), na, ct.c_void_p(out.ptr), ct.c_void_p(lnw.ptr), ct.c_void_p(ws.ptr),
                         ws_bytes, eng._stream())
    torch.cuda.synchronize()
    assert rc == 0, _lib.last_error()
    del keep
    assert ws.check() and out.check() and lnw.check(), "txm_mbar_hist wrote outside its workspace or its outputs"
    assert out.unwritten() == 0 and lnw.unwritten() == 0
    return out.view().cpu().numpy().reshape(na, K + 2, nbins + 1), lnw.view().cpu().numpy(), list(plan)


def plans(case):
    """(smallest bytes, full bytes, expected bin tiles per workgroup and groups) from txm_mbar_hist_plan and the shapes."""
    from thermoextrap_amd import _lib

    L = _lib.load()
    _, ns, _, _, _, _, targets, _, nbins = case
    K, na = len(ns), len(targets)
    p = (ct.c_int64 * 4)()
    assert L.txm_mbar_hist_plan(K, nbins, na, max(ns), 0, p) == -3
    least = int(p[3])
    assert L.txm_mbar_hist_plan(K, nbins, na, max(ns), SIZE_MAX, p) == 0
    NT = nbins // 16 + 1
    bt = min(NT, 32 // (1 if na == 1 else 2 if na == 2 else 4 if na <= 4 else 8))
    assert list(p)[:2] == [bt, -(-NT // bt)]
    return least, int(p[3]), list(p)


def check(name, out, lnw, ref, nbins):
    K = out.shape[1] - 2
    assert np.all(np.isfinite(out)) and np.all(np.isfinite(lnw)) and np.all(out >= 0)
    q = np.abs(out.astype(LD) - ref.out) / (ref.bound + ref.floor / LD(TOL))
    worst = {"T": float(q[:, :K].max()), "H": float(q[:, K].max()), "S": float(q[:, K + 1].max()),
             "lnw": float(np.max(np.abs(lnw.astype(LD) - ref.lnw) / (LD(ref.kappa) * (1 + np.abs(ref.lnw)))))}
    rowsum = float(np.max(np.abs(out[:, K].astype(LD).sum(axis=1) - 1)))
    print(f"\n{name}: worst |hip - ref| / bound-sum: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()) +
          f"; |sum_b H - 1| {rowsum:.2e} (allowed {(nbins + 2) * 2.0 ** -52:.2e})")
    for key, v in worst.items():
        assert v <= TOL, (name, key, v)
    empty = ref.count == 0
    assert not out[:, :, empty].any(), "a column no sample fell into is not exactly 0.0"
    assert np.all(out[:, K][:, ~empty] > 0)
    assert rowsum <= (nbins + 2) * 2.0 ** -52


@pytest.mark.parametrize("name", list(CASES))
def test_hist_against_long_double_under_both_plans(eng, name):
    case, ref = reference(name)
    ns, nbins = case[1], case[8]
    least, full_bytes, full = plans(case)
    assert max(ns) == 1000 and full[2] == 4 and full_bytes > least       # one sample workgroup per 256 samples
    out_f, lnw_f, plan_f = run(eng, case, full_bytes)
    assert plan_f == full
    check(name + " (full plan)", out_f, lnw_f, ref, nbins)
    out_s, lnw_s, plan_s = run(eng, case, least)
    assert plan_s[:2] == full[:2] and plan_s[2] == 1 and plan_s[3] == least
    check(name + " (smallest plan)", out_s, lnw_s, ref, nbins)
    # no atomics: two calls under one plan give the same bits
    again, lnw_again, _ = run(eng, case, full_bytes)
    assert np.array_equal(again, out_f) and np.array_equal(lnw_again, lnw_f)
