"""Differential tests of the four MBAR entry points -- txm_mbar_eval, txm_mbar_predict (txm_mbar.hip), txm_mbar_boot_eval,
txm_mbar_boot_predict (txm_mbar_boot.hip) -- and of the covariance pass txm_mbar_cov (txm_mbar_cov.hip, group E) against
the long-double restatement oracle/mbar_oracle.py, on every path of their dispatch.  tests/test_mbar_gpu.py and tests/test_mbar_boot_gpu.py reach these kernels through the converged Newton
solve only: a wrong Hessian or objective still converges, and only near-solution log-weights are ever seen.  Here g is
NOT a solution (the thermodynamic-integration start plus N(0, 0.5) noise per state; for the bootstrap an independent
noise row per replicate around gref, so min_k (g^r - gref)_k is non-zero and differs between rows), and S, every entry
of H, the objective and every sample's logD are compared one by one.

Inputs and case tables live in tests/test_mbar_oracle_cpu.py, which proves without a GPU what the tolerances assume (no
p_kn below 1e-9 and no kappa_n above 2 in the ordinary cases; p below 1e-308 in the poor-overlap case).  Every case
asserts, from the dispatch arithmetic restated here and the device's number of compute units, that it takes the path it
is named for.

Tolerances (derived, not measured; README "Tolerances").  A sum is held to the first-order bound of its own sum:

  S, H, obj   |hip - ref| <= 1e-12 sum_n kappa_n |term_n| + N_total max_n c_n 2^-1022
  logD_n      |hip - ref| <= 1e-12 kappa_n (1 + |logD_n|)
  averages    |hip - ref| <= 1e-12 kappa sum c w |x| / sum c w     (kappa: the largest kappa_n among the samples whose
                                                                     c w is above 1e-30 of the largest)

with kappa_n = 1 + max_k(|g_k| + |alpha0_k ut_n|) / 64 (for the averages also over the targets' |a ut_n| + |logD_n|).  A
device exponent carries at most eps (|g_k| + 2 |alpha0_k ut_n|) of absolute error -- one rounding in u - upiv, one in the
fma -- a relative weight error of at most 128 eps kappa_n = 2.8e-14 kappa_n; 1e-12 leaves about 30x for the ulps of exp,
log and the divide and for the summation (a few hundred terms per lane plus the tree).  Weighted terms carry c_n.  The
absolute floor stands for terms the device flushes to zero; it is the larger part of a bound in the poor-overlap case
alone.  Bit-for-bit claims (``active`` subsets, ``rows``, ``logD=None``) are held with array_equal.  Every case prints
its worst ratio |hip - ref| / bound-sum (run with -s).

Group E: txm_mbar_cov.  Q_a, every B_ak, yy_ac and b_kac, with g, logD and the centres made on the host (no other device
kernel supplies an input), at the smallest shapes where each tile-index expression of the MFMA kernel and of its final
kernel can go wrong: state rows in row tiles 1 to 4 (K = 17 ... 64), the row of ones at index 0, 1 and 15 of its tile, the
column of ones at index 15 of a group and alone behind full groups, RT >= 2 together with NCG >= 2, the workgroup cap
binding (more than four grid-stride turns) and clamped to one.

  Q, B, yy, b   |hip - ref| <= 1e-12 sum_n kappa_n |term_n| + floor
  lnw_a         |hip - ref| <= 1e-12 kappa (1 + |ref|)                  (kappa: the largest kappa_n)

The floor, from the kernel's own expressions.  A sample enters a matrix-pipe row as pm * va with pm = p_kn <= 1 and
va = e^{-a ut_n - logD_n - M_a} <= 1 (M_a is the exact maximum, so sum_n va >= 1 -- ``den`` of the restatement).  Where
the true product is below 2^-1022 -- because p_kn underflowed in the softmax, because va did, or because only their
product does -- the device holds a subnormal or zero in its place: an absolute error of at most 2^-1022 per sample,
times |d_nc| in b (times 1 in B).  The VALU side squares t = va d_nc: t^2 below 2^-1022 is lost in the same way (Q: d = 1).
These errors are made BEFORE the final kernel divides by N_k sum_n va (B, b) or (sum_n va)^2 (Q, yy), so

  floor(B_ak) = 2^-1022 N_total / (N_k den_a)        floor(b_kac) = 2^-1022 sum_n |d_nc| / (N_k den_a)
  floor(Q_a) = floor(yy_ac) = 2^-1022 N_total / den_a^2

(tests/test_mbar_oracle_cpu.py cov_floor).  The CPU module asserts that it is below 1e-250 of every bound in the ordinary
cases and the larger part of some B and b bounds in the poor-overlap case.  lnw needs none: sum_n va >= 1.
"""

import ctypes as ct

import numpy as np
import pytest
import torch

from oracle import mbar_oracle as mo
from test_mbar_oracle_cpu import (BOOT_EVAL_CASES, BOOT_NREP, BOOT_PREDICT_CASES, COV_CASES, COV_POOR, EVAL_CASES,
                                  EVAL_NOLOGD, PREDICT_CASES, boot_eval_case, boot_predict_case, cov_floor,
                                  cov_reference, eval_case, poor_overlap_inputs, poor_overlap_predict_inputs,
                                  predict_case)

pytestmark = pytest.mark.gpu
TOL = 1e-12
LD = np.longdouble
TINY = 2.0 ** -1022


@pytest.fixture(scope="module")
def eng(txm):
    from thermoextrap_amd import engine

    return engine


@pytest.fixture(scope="module")
def cus(txm):
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).cuda()


def cdiv(a, b):
    return -(-a // b)


def dev_x(xs, pitch=None, col0=0):
    """Each state's x on the device; with ``pitch`` as columns [col0, col0 + C) of rows of ``pitch`` doubles, NaN elsewhere."""
    if pitch is None:
        return [dev(x) for x in xs]
    out = []
    for x in xs:
        wide = torch.full((len(x), pitch), float("nan"), dtype=torch.float64, device="cuda")
        wide[:, col0:col0 + x.shape[1]] = dev(x)
        out.append(wide[:, col0:col0 + x.shape[1]])
    return out


def ratio(got, want, scale, floor=0.0):
    """max |got - want| / (scale + floor / TOL) over the entries, in long double; every entry of got must be finite."""
    assert np.all(np.isfinite(got))
    return float(np.max(np.abs(np.asarray(got, dtype=LD) - want) / (np.asarray(scale, dtype=LD) + LD(floor) / LD(TOL))))


def eval_ratios(S, H, obj, ref, floor):
    return {"S": ratio(S, ref.S, ref.S_bound, floor), "H": ratio(H, ref.H, ref.H_bound, floor),
            "obj": ratio(obj, ref.obj, ref.obj_bound, floor)}


def show(name, worst):
    print(f"\n{name}: worst |hip - ref| / bound-sum: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for key, v in worst.items():
        assert v <= TOL, (name, key, v)


# ---- group A: txm_mbar_eval ---------------------------------------------------------------------------------------------
def eval_plan(K, ns, cus):
    """txm_mbar_eval's launch: which kernel, how many blocks per state, whether the cap binds, how many grid-stride turns
    the largest state takes, and how many rounds of the LDS kernel's triangle-ownership loop own an entry."""
    nmax, cap = max(ns), max(1, cus * 8 // K)
    if K <= 8:
        kernel, per_turn = ("reg", K), 256
    else:
        kernel, per_turn = ("lds", 16 if K <= 16 else 32 if K <= 32 else 64), 64
    want = cdiv(nmax, per_turn * 4)
    gx = max(1, min(want, cap))
    return {"kernel": kernel, "gx": gx, "capped": want > cap, "turns": cdiv(nmax, gx * per_turn),
            "rounds": cdiv(K * (K + 1) // 2, 256)}


EVAL_PATHS = {**{f"reg_K{K}": {"kernel": ("reg", K)} for K in range(1, 9)},
              "reg_K8_block_cap": {"kernel": ("reg", 8), "capped": True},
              "lds16_K9": {"kernel": ("lds", 16), "rounds": 1}, "lds16_K16": {"kernel": ("lds", 16), "rounds": 1},
              "lds32_K17": {"kernel": ("lds", 32), "rounds": 1}, "lds32_K24": {"kernel": ("lds", 32), "rounds": 2},
              "lds32_K32": {"kernel": ("lds", 32), "rounds": 3}, "lds64_K33": {"kernel": ("lds", 64), "rounds": 3},
              "lds64_K64_block_cap": {"kernel": ("lds", 64), "rounds": 9, "capped": True}}


def run_eval(eng, us, a0, g, upiv, with_logD=True):
    ud = [dev(u) for u in us]
    logD = torch.full((sum(len(u) for u in us),), float("nan"), dtype=torch.float64, device="cuda") if with_logD else None
    S, H, obj = eng.mbar_eval(ud, a0, g, upiv, logD)
    return S, H, obj, (logD.cpu().numpy() if with_logD else None)


def check_logD(logD, ref):
    assert np.all(np.isfinite(logD))
    q = np.abs(logD.astype(LD) - ref.logD) / (ref.kappa * (1.0 + np.abs(ref.logD)))
    return float(q.max())


@pytest.mark.parametrize("name", list(EVAL_CASES))
def test_eval_against_long_double(eng, cus, name):
    a0, ns, us, upiv, g = eval_case(name, cus)
    K = len(ns)
    plan = eval_plan(K, ns, cus)
    for key, v in EVAL_PATHS[name].items():
        assert plan[key] == v, (name, key, plan)
    if name.startswith("reg_") and K <= 8 and "cap" not in name:
        assert plan["gx"] > 1 and plan["turns"] > 1                 # several blocks, several grid-stride turns
    if "cap" in name:
        assert plan["turns"] > 4
    S, H, obj, logD = run_eval(eng, us, a0, g, upiv)
    assert np.array_equal(H, H.T)
    ref = mo.eval_sums(us, a0, g, upiv)
    worst = eval_ratios(S, H, obj, ref, sum(ns) * TINY)
    worst["logD"] = check_logD(logD, ref)                           # per sample across the state offsets
    show(name, worst)


@pytest.mark.parametrize("name", list(EVAL_NOLOGD))
def test_eval_without_logD_gives_the_same_bits(eng, cus, name):
    a0, ns, us, upiv, g = eval_case(name, cus)
    assert eval_plan(len(ns), ns, cus)["kernel"] == (("reg", 5) if name == "nologd_K5" else ("lds", 16))
    S, H, obj, _ = run_eval(eng, us, a0, g, upiv)
    S2, H2, obj2, _ = run_eval(eng, us, a0, g, upiv, with_logD=False)
    assert np.array_equal(S, S2) and np.array_equal(H, H2) and obj == obj2
    show(name, eval_ratios(S2, H2, obj2, mo.eval_sums(us, a0, g, upiv), sum(ns) * TINY))


def test_eval_poor_overlap(eng, cus):
    """alpha0 = [0.1, 10], energies 190 apart: every p of the other state is below 1e-308 and the device flushes it; H_01
    is then held by the floor N_total 2^-1022 alone, everything else by its own bound (kappa_n reaches about 17)."""
    a0, us, _, upiv, g = poor_overlap_inputs()
    ns = [len(u) for u in us]
    assert eval_plan(2, ns, cus)["kernel"] == ("reg", 2)
    S, H, obj, logD = run_eval(eng, us, a0, g, upiv)
    assert np.array_equal(H, H.T)
    ref = mo.eval_sums(us, a0, g, upiv)
    floor = sum(ns) * TINY
    assert TOL * float(ref.H_bound[0, 1]) < floor and TOL * float(ref.H_bound[0, 0]) > 1e100 * floor
    worst = eval_ratios(S, H, obj, ref, floor)
    worst["logD"] = check_logD(logD, ref)
    show("poor_overlap_K2", worst)


# ---- group B: txm_mbar_predict ------------------------------------------------------------------------------------------
def predict_plan(K, ns, C, na, pitches, aligned, cus):
    """txm_mbar_predict's launch: VEC, log2 lanes per row, column chunks, blocks per state, and per column chunk whether
    the lanes of a row share the targets' weights."""
    vec = 2 if (C % 2 == 0 and all(p % 2 == 0 for p in pitches) and all(aligned)) else 1
    lanes, l2 = cdiv(C, vec), 0
    while (1 << l2) < lanes and l2 < 8:
        l2 += 1
    lpr, cpc = 1 << l2, (1 << l2) * vec
    chunks, cap = cdiv(C, cpc), max(1, cus * 8 // K)
    want = cdiv(max(ns), (256 >> l2) * 4)
    share = [lpr >= na and lpr <= 64 and na > 1 and cdiv(C - ch * cpc, vec) >= na for ch in range(chunks)]
    return {"vec": vec, "l2": l2, "chunks": chunks, "gx": max(1, min(want, cap)), "capped": want > cap, "na": na,
            "share": share}


def spec_plan(name, cus):
    """The plan from the case's table entry alone (a torch allocation is 16-byte aligned; a 1-sample state has pitch C)."""
    K, nsf, C, na, pitch, col0 = PREDICT_CASES[name]
    ns = nsf(cus)[:K]
    return predict_plan(K, ns, C, na, [(pitch or C) if n > 1 else C for n in ns], [col0 % 2 == 0] * K, cus)


PREDICT_PATHS = {"C600_na2_two_chunks": {"vec": 2, "l2": 8, "chunks": 2},
                 "C300_na3_odd_pitch_grid_cap": {"vec": 1, "l2": 8, "chunks": 2, "capped": True},
                 "C6_na5_pitch8_keeps_vec2": {"vec": 2, "l2": 2}, "C2_na2_odd_pitch": {"vec": 1, "l2": 1},
                 "C10_na4_odd_pitch": {"vec": 1, "l2": 4}, "C8_na4_slice_8_mod_16": {"vec": 1, "l2": 3},
                 "C5_na4": {"vec": 1, "l2": 3, "share": [True]}, "C5_na8": {"vec": 1, "l2": 3, "share": [False]},
                 "C257_na2": {"vec": 1, "l2": 8, "chunks": 2}, "C514_na2": {"vec": 2, "l2": 8, "chunks": 2}}


def test_predict_cases_cover_the_dispatch(cus):
    plans = {name: spec_plan(name, cus) for name in PREDICT_CASES}
    assert {(p["vec"], p["l2"]) for p in plans.values()} == {(v, l) for v in (1, 2) for l in range(9)}
    seen = {(p["na"], s) for p in plans.values() for s in p["share"]}
    assert {(na, s) for na in range(2, 9) for s in (True, False)} <= seen and (1, False) in seen
    for v in (1, 2):
        assert any(p["vec"] == v and p["chunks"] > 1 for p in plans.values())
    assert any(p["capped"] for p in plans.values())
    for name, want in PREDICT_PATHS.items():
        for key, v in want.items():
            assert plans[name][key] == v, (name, key, plans[name])


@pytest.mark.parametrize("name", list(PREDICT_CASES))
def test_predict_against_long_double(eng, cus, name):
    """logD is the oracle's, rounded to float64 and uploaded: the contraction is tested independently of group A."""
    K, _, C, na, pitch, col0 = PREDICT_CASES[name]
    a0, ns, us, xs, upiv, g, targets = predict_case(name, cus)
    ud, xd = [dev(u) for u in us], dev_x(xs, pitch, col0)
    tab, keep, _, C2 = eng._mbar_table(ud, xd)
    plan = predict_plan(K, ns, C2, na, [tab[s].ldx_s for s in range(K)], [tab[s].x % 16 == 0 for s in range(K)], cus)
    assert C2 == C and plan == spec_plan(name, cus), (plan, spec_plan(name, cus))
    if pitch is not None:
        assert all(tab[s].ldx_s == pitch for s in range(K) if ns[s] > 1)
    if col0:
        assert all(tab[s].x % 16 == 8 for s in range(K))
    del keep
    ld64 = np.asarray(mo.eval_sums(us, a0, g, upiv).logD, dtype=np.float64)
    out = eng.mbar_predict(xd, ud, a0, None, dev(ld64), targets, upiv=upiv).cpu().numpy()
    ref = mo.predict(us, xs, a0, upiv, targets, logD=ld64)
    assert out.shape == (na, C)
    show(name, {"avg": ratio(out, ref.avg.astype(LD), ref.kappa[:, None] * ref.scale)})


@pytest.mark.parametrize("C,share", [(1, False), (3, True)])
def test_predict_poor_overlap_needs_each_targets_own_maximum(eng, cus, C, share):
    """Targets whose maxima M_a lie 950 apart (tests/test_mbar_oracle_cpu.py proves it), on the path where every lane
    forms all NA weights and on the one where the lanes of a row share them.  A quotient is unchanged when its weights are
    shifted by a constant, so the ordinary cases cannot see which M_a a weight was shifted by; here e^{. - M_0} of
    target 1 overflows."""
    a0, us, xs, upiv, g, targets = poor_overlap_predict_inputs(C)
    ns = [len(u) for u in us]
    plan = predict_plan(2, ns, C, len(targets), [C, C], [True, True], cus)
    assert plan["vec"] == 1 and plan["share"] == [share], plan
    ld64 = np.asarray(mo.eval_sums(us, a0, g, upiv).logD, dtype=np.float64)
    out = eng.mbar_predict(dev_x(xs), [dev(u) for u in us], a0, None, dev(ld64), targets, upiv=upiv).cpu().numpy()
    ref = mo.predict(us, xs, a0, upiv, targets, logD=ld64)
    assert ref.kappa.max() > 2.0
    show(f"poor_overlap_C{C}_na3", {"avg": ratio(out, ref.avg.astype(LD), ref.kappa[:, None] * ref.scale)})


# ---- groups C and D: the bootstrap --------------------------------------------------------------------------------------
def boot_plan(K, ns, nrep):
    """txm_mbar_boot_eval's work units: the kernel, each state's sampler tiles per chunk (a chunk is one wave's work; at
    most 256 / K chunks per state) and the waves left over in the last group of four."""
    cap = max(1, 256 // K)
    tiles = [cdiv(n, 1024) for n in ns]
    tpc = [cdiv(t, min(t, cap)) for t in tiles]
    kernel = ("reg", K) if K <= 8 else ("lds", 16 if K <= 16 else 32 if K <= 32 else 64)
    return {"kernel": kernel, "tpc": max(tpc), "rounds": cdiv(K * (K + 1) // 2, 64), "remainder": nrep % 4}


def samplers_and_counts(eng, ns, nrep, seed):
    """One DeviceSampler per state (stream offset s * nrep) and the (nrep, N_total) counts they regenerate."""
    sm = [eng.DeviceSampler(seed, nrep, n, rep0=s * nrep) for s, n in enumerate(ns)]
    fr = [m.freq().cpu().numpy() for m in sm]
    for f, n in zip(fr, ns):
        assert f.shape == (nrep, n) and np.all(f.sum(axis=1) == n) and f.min() >= 0
    return sm, np.concatenate(fr, axis=1)


BOOT_EVAL_PATHS = {"reg_K1_nrep1": ("reg", 1), "reg_K2_nrep3": ("reg", 2), "reg_K5_nrep5": ("reg", 5),
                   "reg_K8_nrep6_tpc2": ("reg", 8), "lds16_K9_nrep3": ("lds", 16), "lds16_K16_nrep5": ("lds", 16),
                   "lds32_K17_nrep1": ("lds", 32), "lds32_K32_nrep6": ("lds", 32), "lds64_K33_nrep5": ("lds", 64),
                   "lds64_K64_nrep3_tpc2": ("lds", 64)}
_boot_cache = {}


def boot_eval_all(eng, name):
    """Inputs, samplers, counts and the all-rows device result of a group C case, once per module."""
    if name not in _boot_cache:
        K, nrep, ns, _ = BOOT_EVAL_CASES[name]
        a0, ns, us, upiv, gref, g = boot_eval_case(name)
        sm, counts = samplers_and_counts(eng, ns, nrep, seed=9000 + K)
        ud = [dev(u) for u in us]
        _boot_cache[name] = (a0, ns, us, ud, upiv, g, sm, counts, eng.mbar_boot_eval(ud, a0, sm, g, upiv))
    return _boot_cache[name]


def boot_eval_worst(a0, us, upiv, g, counts, rows, got):
    S, H, obj = got
    worst = {}
    for i, r in enumerate(rows):
        ref = mo.eval_sums(us, a0, g[r], upiv, counts[r])
        assert np.array_equal(H[i], H[i].T)
        for key, v in eval_ratios(S[i], H[i], obj[i], ref, counts.shape[1] * counts[r].max() * TINY).items():
            worst[key] = max(worst.get(key, 0.0), v)
    return worst


@pytest.mark.parametrize("name", list(BOOT_EVAL_CASES))
def test_boot_eval_against_long_double(eng, name):
    K, nrep, ns, _ = BOOT_EVAL_CASES[name]
    plan = boot_plan(K, ns, nrep)
    assert plan["kernel"] == BOOT_EVAL_PATHS[name] and (plan["tpc"] > 1) == ("tpc2" in name), plan
    if name in ("reg_K5_nrep5", "reg_K8_nrep6_tpc2"):
        assert nrep > 4 and plan["remainder"] != 0                  # a full group of four waves and a partial one
    if name == "lds64_K64_nrep3_tpc2":
        assert plan["rounds"] == 33
    a0, ns, us, ud, upiv, g, sm, counts, got = boot_eval_all(eng, name)
    assert counts.max() >= 3 and (counts == 0).any()
    show(name, boot_eval_worst(a0, us, upiv, g, counts, range(nrep), got))


@pytest.mark.parametrize("name", ["reg_K8_nrep6_tpc2", "lds32_K32_nrep6"])
def test_boot_eval_active_subset_and_rows_give_the_same_bits(eng, name):
    """An unordered ``active`` subset that is no multiple of four, and replicates [2, 5) as a sampler of their own
    (rep0 > 0 in every state): the rows of the all-rows call, bit for bit, and the oracle's."""
    a0, ns, us, ud, upiv, g, sm, counts, (S, H, obj) = boot_eval_all(eng, name)
    act = [4, 0, 2]
    Sa, Ha, oa = eng.mbar_boot_eval(ud, a0, sm, g, upiv, active=act)
    assert np.array_equal(Sa, S[act]) and np.array_equal(Ha, H[act]) and np.array_equal(oa, obj[act])
    show(name + " active [4, 0, 2]", boot_eval_worst(a0, us, upiv, g, counts, act, (Sa, Ha, oa)))
    sub = [m.rows(2, 5) for m in sm]
    assert all(m.rep0 == s * len(g) + 2 for s, m in enumerate(sub))
    Sr, Hr, orr = eng.mbar_boot_eval(ud, a0, sub, np.ascontiguousarray(g[2:5]), upiv)
    assert np.array_equal(Sr, S[2:5]) and np.array_equal(Hr, H[2:5]) and np.array_equal(orr, obj[2:5])


def boot_predict_plan(K, ns, C, na):
    """txm_mbar_boot_predict's launch: log2 lanes per row, column chunks, the padded target count, the pipelined gather."""
    l2 = 0
    while (1 << l2) < C and l2 < 6:
        l2 += 1
    return {"l2": l2, "chunks": cdiv(C, 1 << l2), "pad": 1 if na <= 1 else 2 if na <= 2 else 4 if na <= 4 else 8,
            "pipe": l2 >= 3, "tpc": boot_plan(K, ns, BOOT_NREP)["tpc"]}


BOOT_PREDICT_PATHS = {
    "K3_C1_na1": {"pad": 1, "pipe": False, "chunks": 1}, "K3_C2_na2": {"pad": 2, "pipe": False},
    "K3_C3_na3": {"pad": 4, "pipe": False}, "K3_C4_na4_pitch7": {"pad": 4, "pipe": False, "l2": 2},
    "K3_C8_na5": {"pad": 8, "pipe": True, "l2": 3}, "K3_C33_na7": {"pad": 8, "pipe": True, "l2": 6, "chunks": 1},
    "K3_C64_na8": {"pad": 8, "pipe": True, "chunks": 1}, "K3_C65_na2_two_chunks": {"pad": 2, "pipe": True, "chunks": 2},
    "K3_C130_na3_three_chunks_pitch136": {"pad": 4, "pipe": True, "chunks": 3},
    "K12_C8_na5": {"pad": 8, "pipe": True}, "K12_C3_na7": {"pad": 8, "pipe": False},
    "K64_C2_na1_tpc2": {"pad": 1, "pipe": False, "tpc": 2}}


def boot_predict_raw(eng, us, xd, a0, sm, g, gref, upiv, targets):
    """txm_mbar_boot_predict through the C ABI, as engine.mbar_bootstrap_predict calls it, with g and gref chosen freely."""
    from thermoextrap_amd import _lib

    L = _lib.load()
    ud = [dev(u) for u in us]
    tab, stab, keep, ns, C, nrep = eng._mbar_boot_tables(ud, sm, xd)
    K, na = len(us), len(targets)
    a0 = np.ascontiguousarray(a0, dtype=np.float64)
    gref = np.ascontiguousarray(gref, dtype=np.float64)
    gd = dev(g)
    out = torch.full((nrep, na, C), float("nan"), dtype=torch.float64, device="cuda")
    nbytes = L.txm_mbar_boot_ws_bytes(K, C, na, int(ns.sum()), nrep)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    dp = ct.POINTER(ct.c_double)
    rc = L.txm_mbar_boot_predict(tab, stab, K, C, float(upiv), a0.ctypes.data_as(dp), eng._ptr(gd), gref.ctypes.data_as(dp),
                                 targets.ctypes.data_as(dp), na, eng._ptr(out), eng._ptr(ws), nbytes, eng._stream())
    torch.cuda.synchronize()
    assert rc == 0, _lib.last_error()
    pitches = [tab[s].ldx_s for s in range(K)]
    del keep
    return out.cpu().numpy(), pitches


@pytest.mark.parametrize("name", list(BOOT_PREDICT_CASES))
def test_boot_predict_against_long_double(eng, name):
    K, ns, C, na, pitch = BOOT_PREDICT_CASES[name]
    plan = boot_predict_plan(K, ns, C, na)
    for key, v in BOOT_PREDICT_PATHS[name].items():
        assert plan[key] == v, (name, key, plan)
    a0, ns, us, xs, upiv, gref, g, targets = boot_predict_case(name)
    assert 1 in ns and (targets.min() < min(a0) or targets.max() > max(a0))   # a 1-sample state, a target outside the range
    sm, counts = samplers_and_counts(eng, ns, BOOT_NREP, seed=9500 + K + C)
    out, pitches = boot_predict_raw(eng, us, dev_x(xs, pitch), a0, sm, g, gref, upiv, targets)
    if pitch is not None:
        assert all(p == pitch for p, n in zip(pitches, ns) if n > 1)
    worst = 0.0
    for r in range(BOOT_NREP):
        ref = mo.predict(us, xs, a0, upiv, targets, g=g[r], counts=counts[r])
        worst = max(worst, ratio(out[r], ref.avg.astype(LD), ref.kappa[:, None] * ref.scale))
    show(name, {"avg": worst})


def test_boot_predict_cases_cover_the_dispatch():
    plans = {name: boot_predict_plan(c[0], c[1], c[2], c[3]) for name, c in BOOT_PREDICT_CASES.items()}
    assert {c[3] for c in BOOT_PREDICT_CASES.values()} == {1, 2, 3, 4, 5, 7, 8}
    assert {c[2] for c in BOOT_PREDICT_CASES.values()} >= {1, 2, 3, 4, 8, 33, 64, 65, 130}
    assert {p["pad"] for p in plans.values()} == {1, 2, 4, 8} and {p["chunks"] for p in plans.values()} == {1, 2, 3}
    assert {(p["pad"], p["pipe"]) for p in plans.values()} >= {(1, False), (2, False), (2, True), (4, False), (4, True),
                                                               (8, False), (8, True)}


# ---- group E: txm_mbar_cov ------------------------------------------------------------------------------------------------
def cov_plan(K, C, na, ns, cus):
    """txm_mbar_cov's launch: row tiles and column groups (the states plus a row of ones, the observables plus a column of
    ones), where the ones sit as (tile, index), workgroups per (state, row tile, column group) and their cap, grid-stride
    turns of the largest state, the target template."""
    RT, NCG = K // 16 + 1, C // 16 + 1
    cap = max(1, cus * 8 // (K * NCG * RT))
    want = cdiv(max(ns), 256)
    gx = max(1, min(want, cap))
    return {"RT": RT, "NCG": NCG, "cap": cap, "gx": gx, "capped": want > cap, "turns": cdiv(max(ns), gx * 64),
            "NA": 1 if na == 1 else 2 if na == 2 else 4 if na <= 4 else 8, "ones_row": (K // 16, K % 16),
            "ones_col": (C // 16, C % 16)}


COV_PATHS = {
    "K16_C15_na8": {"RT": 2, "NCG": 1, "NA": 8, "ones_row": (1, 0), "ones_col": (0, 15), "capped": False},
    "K17_C1_na1": {"RT": 2, "NCG": 1, "NA": 1, "ones_row": (1, 1), "capped": False},
    "K31_C15_na2": {"RT": 2, "NCG": 1, "NA": 2, "ones_row": (1, 15), "ones_col": (0, 15), "capped": False},
    "K32_C16_na3": {"RT": 3, "NCG": 2, "NA": 4, "ones_row": (2, 0), "ones_col": (1, 0), "capped": False},
    "K33_C31_na4_pitch37": {"RT": 3, "NCG": 2, "NA": 4, "ones_row": (2, 1), "ones_col": (1, 15), "capped": False},
    "K48_C32_na5": {"RT": 4, "NCG": 3, "NA": 8, "ones_row": (3, 0), "ones_col": (2, 0), "capped": False},
    "K64_C17_na8_block_cap": {"RT": 5, "NCG": 2, "NA": 8, "ones_row": (4, 0), "capped": True},
    "K64_C*_na2_cap_one": {"RT": 5, "NA": 2, "cap": 1, "gx": 1},
    "K8_C3_na8_block_cap": {"RT": 1, "NCG": 1, "NA": 8, "capped": True},
    COV_POOR: {"RT": 1, "NCG": 1, "NA": 4, "capped": False},
}
COV_BAND, COV_FILL = 4096, 0xA5


def cov_raw(eng, case):
    """(out (n_alpha, 1 + K + C (1 + K)), lnw) of txm_mbar_cov through the C ABI with the case's host-made g, logD and
    centres.  out and lnw start as NaN; the workspace is txm_mbar_cov_ws_bytes long plus a band of COV_BAND bytes in the
    same tensor, which must come back untouched."""
    from thermoextrap_amd import _lib

    L = _lib.load()
    a0, ns, us, xs, upiv, g, targets, logD, means, pitch = case
    K, C, na = len(ns), xs[0].shape[1], len(targets)
    ud, xd = [dev(u) for u in us], dev_x(xs, pitch)
    tab, keep, _, C2 = eng._mbar_table(ud, xd)
    assert C2 == C and means.shape == (na, C) and logD.shape == (sum(ns),)
    if pitch is not None:
        assert all(tab[s].ldx_s == pitch for s in range(K) if ns[s] > 1)
    a0 = np.ascontiguousarray(a0, dtype=np.float64)
    g = np.ascontiguousarray(g, dtype=np.float64)
    al = np.ascontiguousarray(targets, dtype=np.float64)
    ld, mean = dev(logD), dev(means)
    out = torch.full((na, 1 + K + C * (1 + K)), float("nan"), dtype=torch.float64, device="cuda")
    lnw = torch.full((na,), float("nan"), dtype=torch.float64, device="cuda")
    nbytes = L.txm_mbar_cov_ws_bytes(K, C, na)
    assert nbytes > 0
    ws = torch.full((nbytes + COV_BAND,), COV_FILL, dtype=torch.uint8, device="cuda")
    dp = ct.POINTER(ct.c_double)
    rc = L.txm_mbar_cov(tab, K, C, float(upiv), a0.ctypes.data_as(dp), g.ctypes.data_as(dp), eng._ptr(ld),
                        al.ctypes.data_as(dp), na, eng._ptr(mean), eng._ptr(out), eng._ptr(lnw), eng._ptr(ws), nbytes,
                        eng._stream())
    torch.cuda.synchronize()
    assert rc == 0, _lib.last_error()
    del keep
    assert bool((ws[nbytes:] == COV_FILL).all()), "txm_mbar_cov wrote past txm_mbar_cov_ws_bytes"
    out, lnw = out.cpu().numpy(), lnw.cpu().numpy()
    assert np.all(np.isfinite(out)) and np.all(np.isfinite(lnw))
    return out, lnw


def cov_worst(out, lnw, ref, ns):
    na, K = ref.B.shape
    C = ref.yy.shape[1]
    rest = out[:, 1 + K:].reshape(na, C, 1 + K)
    got = {"Q": out[:, 0], "B": out[:, 1:1 + K], "yy": rest[:, :, 0], "b": rest[:, :, 1:]}
    floor = cov_floor(ref, ns)
    worst = {key: float(np.max(np.abs(v.astype(LD) - getattr(ref, key)) / (getattr(ref, key + "_bound") + floor[key] / LD(TOL))))
             for key, v in got.items()}
    worst["lnw"] = float(np.max(np.abs(lnw.astype(LD) - ref.lnw) / (LD(ref.kappa) * (1 + np.abs(ref.lnw)))))
    return worst


def cov_path(name, case, cus):
    """The launch plan of a group E case, asserted to be the path the case is named for."""
    ns, C, na = case[1], case[3][0].shape[1], len(case[6])
    K = len(ns)
    plan = cov_plan(K, C, na, ns, cus)
    for key, v in COV_PATHS[name].items():
        assert plan[key] == v, (name, key, plan)
    if "block_cap" in name:
        assert plan["gx"] == plan["cap"] and plan["turns"] > 4 and max(ns) == plan["cap"] * 256 + 77
    if "cap_one" in name:
        assert K * plan["NCG"] * plan["RT"] > cus * 8 and plan["cap"] == 1 and plan["turns"] == cdiv(max(ns), 64) > 1
    if name in ("K32_C16_na3", "K33_C31_na4_pitch37", "K48_C32_na5", "K64_C17_na8_block_cap", "K64_C*_na2_cap_one"):
        assert plan["RT"] >= 2 and plan["NCG"] >= 2
    return plan


@pytest.mark.parametrize("name", list(COV_CASES) + [COV_POOR])
def test_cov_against_long_double(eng, cus, name):
    case, ref = cov_reference(name, cus)
    cov_path(name, case, cus)
    ns = case[1]
    if name == COV_POOR:
        assert ref.p_min < 1e-308 and ref.kappa > 2.0
    else:
        assert ref.p_min >= 1e-9 and ref.kappa <= 2.0
    out, lnw = cov_raw(eng, case)
    show(name, cov_worst(out, lnw, ref, ns))
    # the structure the maths promises for any g: sum_k N_k B_ak = 1, to the sum of the B bounds
    N = np.asarray(ns, dtype=LD)
    assert np.all(np.abs(out[:, 1:1 + len(ns)].astype(LD) @ N - 1) <= TOL * (ref.B_bound @ N) + cov_floor(ref, ns)["B"] @ N)


@pytest.mark.parametrize("name", ["K64_C17_na8_block_cap", "K64_C*_na2_cap_one"])
def test_cov_capped_calls_stay_in_their_workspace_and_repeat_their_bits(eng, cus, name):
    """Where K * cap * NCG * RT partial tiles are most: the band behind the workspace is untouched (cov_raw) and, no
    atomics being used, two calls give equal bits."""
    case, _ = cov_reference(name, cus)
    cov_path(name, case, cus)
    a, b = cov_raw(eng, case), cov_raw(eng, case)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
