"""The long-double references of oracle/mbar_oracle.py (eval_sums, predict, cov_sums) pinned to mpmath at 50 digits, and
the input generators of tests/test_mbar_kernels_gpu.py checked without a GPU.

The mpmath side is scalar loops straight from the definitions (no maximum is subtracted: mpmath's exponent range has no
end).  The agreement demanded is the one tests/test_tail_oracle_cpu.py demands of tail_oracle.py: a few long-double
ulps of each sum's own bound.  A long-double exponent g_k - alpha0_k ut_n carries eps_ld (|g_k| + 2 |alpha0_k ut_n|)
<= 128 eps_ld kappa_n, a relative error of the weight; exp, log, the divide and the summation of a few hundred terms add
tens of eps_ld: 200 eps_ld = 2.2e-17 of the bound (which carries kappa_n) covers both.

The generators.  Every case of the GPU module draws its inputs here (``eval_inputs``, ``boot_g``), so that this module
can show, on the CPU, what the GPU tolerances assume: in every ordinary case no p_kn is below 1e-9 (no underflow floor
is active: the floor of the bound matters in the poor-overlap case alone) and no kappa_n is above 2; and the poor-overlap
case really has p below 1e-308, which float64 flushes.  Sizes that depend on the device (a state large enough for a grid
cap to bind) are functions of the number of compute units; here they are taken at 256.

The fifth table, COV_CASES, feeds group E of the GPU module (txm_mbar_cov).  No device kernel supplies an input there:
logD is the long-double logD at the case's g rounded once to float64, the centres are mo.predict's at that logD.
``cov_floor`` is the absolute floor of group E (derived in the GPU module's header); here it is shown to be negligible
in every ordinary case and to be the larger part of a bound in the poor-overlap case.
"""

import mpmath as mp
import numpy as np
import pytest

from oracle import mbar_oracle as mo

LD = np.longdouble
mp.mp.dps = 50
F = mp.mpf
PIN = 200 * mo.EPS_LD
CUS = 256          # compute units assumed where no device is there to ask


# ---------------------------------------------------------------------------
# generators shared with tests/test_mbar_kernels_gpu.py
# ---------------------------------------------------------------------------
def gauss_us(a0, ns, rng, mu=50.0, sd=2.0):
    """Gaussian energies: state k is N(mu - sd^2 alpha0_k, sd) (problem() of tests/test_mbar_cov_gpu.py)."""
    return [rng.normal(mu - sd * sd * a, sd, n) for a, n in zip(a0, ns)]


def gauss_xs(us, C, rng, mu=50.0):
    """C columns of mixed offset and scale, correlated with u."""
    off, slope = rng.normal(0.0, 3.0, C), rng.normal(0.05, 0.02, C)
    return [off[None, :] + slope[None, :] * (u[:, None] - mu) + rng.normal(0, 0.3, (len(u), C)) for u in us]


def ti_g(us, a0, upiv):
    """ln N + f_TI - alpha0 upiv shifted to max 0: the solver's starting point (trapezoid over the states sorted by
    alpha0), not a solution."""
    a0 = np.asarray(a0, dtype=np.float64)
    means = np.array([u.mean() for u in us])
    order = np.argsort(a0, kind="stable")
    f = np.zeros(len(a0))
    for i in range(1, len(order)):
        p, q = order[i - 1], order[i]
        f[q] = f[p] + (a0[q] - a0[p]) * 0.5 * (means[p] + means[q])
    g = np.log([len(u) for u in us]) + f - a0 * upiv
    return g - g.max()


def eval_inputs(a0, ns, seed, C=0, mu=50.0, sd=2.0, us=None):
    """(us, xs or None, upiv, g): g is ti_g plus N(0, 0.5) noise per state -- any g but a solution."""
    rng = np.random.default_rng(seed)
    if us is None:
        us = gauss_us(a0, ns, rng, mu, sd)
    xs = gauss_xs(us, C, rng, mu) if C else None
    upiv = float(np.concatenate(us).mean())
    g = ti_g(us, a0, upiv) + rng.normal(0.0, 0.5, len(a0))
    return us, xs, upiv, np.ascontiguousarray(g)


def boot_g(gref, nrep, seed):
    """An independent noise row per replicate around gref: N(0, 0.5) clipped to +-1.5, so min_k (g^r - gref)_k is not
    zero and differs between rows."""
    rng = np.random.default_rng(seed)
    d = np.clip(rng.normal(0.0, 0.5, (nrep, len(gref))), -1.5, 1.5)
    return np.ascontiguousarray(np.asarray(gref)[None, :] + d)


def poor_overlap_inputs(n=3000, seed=7):
    """alpha0 = [0.1, 10], energies about 190 apart (tests/test_mbar_gpu.py test_poor_overlap_notebook_shape, reduced):
    the weight of a sample in the other state is e^-1900."""
    rng = np.random.default_rng(seed)
    a0 = [0.1, 10.0]
    us = [rng.normal(200.0, 6.0, n), rng.normal(10.0, 0.3, n)]
    return (a0,) + eval_inputs(a0, [n, n], seed + 1, us=us)


POOR_TARGETS = np.array([0.1, 20.0, 10.0])


def poor_overlap_predict_inputs(C, n=300):
    """The poor-overlap pair with C columns and targets on both sampled alpha0 and at 20: the targets' maxima
    M_a = max_n(-a ut_n - logD_n) lie some 950 apart, so a weight shifted by another target's maximum overflows."""
    a0, us, _, upiv, g = poor_overlap_inputs(n=n)
    return a0, us, gauss_xs(us, C, np.random.default_rng(600 + C), mu=100.0), upiv, g, POOR_TARGETS


def steps(K, d):
    return list(1.0 + d * np.arange(K))


def targets_for(a0, n):
    """n targets: one on a sampled alpha0, one below and one above the sampled range, the rest inside it."""
    lo, hi = min(a0), max(a0)
    t = [a0[len(a0) // 2], lo - 0.15, hi + 0.15] + list(np.linspace(lo, hi, max(n - 3, 1) + 2)[1:-1])
    return np.ascontiguousarray(t[:n] if n > 1 else [hi + 0.15], dtype=np.float64)


def reg_cap(K, cus):
    """One state above cap * 1024 samples (cap = cus * 8 / K blocks per state), so the register kernel's block cap binds."""
    return max(1, cus * 8 // K) * 1024 + 777


def lds_cap(K, cus):
    return max(1, cus * 8 // K) * 256 + 77


RAGGED8 = [2500, 1, 63, 64, 65, 255, 257, 300]


def _lds64_ns(K):
    ns = [40 + 13 * k for k in range(K)]
    ns[1:6] = [1, 63, 64, 65, 257]
    return ns


# group A: name -> (alpha0 step d, ns(cus))
EVAL_CASES = {f"reg_K{K}": (0.1, lambda cus, K=K: RAGGED8[:K]) for K in range(1, 9)}
EVAL_CASES.update({
    "reg_K8_block_cap": (0.1, lambda cus: [1, 63, reg_cap(8, cus), 64, 65, 255, 257, 300]),
    "lds16_K9": (0.04, lambda cus: [1, 1000] + [50 + 7 * k for k in range(2, 9)]),
    "lds16_K16": (0.04, lambda cus: [50 + 7 * k for k in range(14)] + [1, 1000]),
    "lds32_K17": (0.02, lambda cus: [1] + [100 + 7 * k for k in range(1, 17)]),
    "lds32_K24": (0.02, lambda cus: [100 + 7 * k for k in range(24)]),
    "lds32_K32": (0.02, lambda cus: [100 + 7 * k for k in range(31)] + [1]),
    "lds64_K33": (0.01, lambda cus: _lds64_ns(33)),
    "lds64_K64_block_cap": (0.01, lambda cus: _lds64_ns(63) + [lds_cap(64, cus)]),
})
EVAL_NOLOGD = {"nologd_K5": EVAL_CASES["reg_K5"], "nologd_K12": (0.04, lambda cus: [1, 1000] + [50 + 7 * k for k in range(2, 12)])}


def eval_case(name, cus=CUS):
    """(a0, ns, us, upiv, g) of a group A case."""
    d, nsf = {**EVAL_CASES, **EVAL_NOLOGD}[name]
    ns = nsf(cus)
    a0 = steps(len(ns), d)
    us, _, upiv, g = eval_inputs(a0, ns, seed=1000 + len(ns) + len(name))
    return a0, ns, us, upiv, g


# group B: name -> (K, ns(cus), C, n_alpha, row pitch or None, first column of the slice)
def _pcap(cus):
    return [max(1, cus * 8 // 2) * 4 + 37, 1]


PREDICT_CASES = {}
for _C, _na in [(1, 1), (3, 2), (5, 4), (5, 8), (9, 3), (17, 8), (33, 6), (65, 7), (129, 8), (257, 2),      # VEC = 1
                (2, 1), (4, 2), (6, 3), (10, 4), (18, 5), (34, 6), (66, 7), (130, 8), (258, 3), (514, 2),  # VEC = 2
                (1, 4), (3, 5), (3, 6), (1, 8)]:                                                             # no share
    PREDICT_CASES[f"C{_C}_na{_na}"] = (3 if _C % 3 else 2, lambda cus: [257, 1, 700], _C, _na, None, 0)
PREDICT_CASES.update({
    "C600_na2_two_chunks": (2, lambda cus: [300, 65], 600, 2, None, 0),
    "C300_na3_odd_pitch_grid_cap": (2, _pcap, 300, 3, 301, 0),
    "C6_na5_pitch8_keeps_vec2": (3, lambda cus: [257, 1, 700], 6, 5, 8, 0),
    "C2_na2_odd_pitch": (3, lambda cus: [257, 1, 700], 2, 2, 3, 0),
    "C10_na4_odd_pitch": (2, lambda cus: [300, 65], 10, 4, 13, 0),
    "C8_na4_slice_8_mod_16": (3, lambda cus: [257, 5, 700], 8, 4, 10, 1),
})


def predict_case(name, cus=CUS):
    K, nsf, C, na, pitch, col0 = PREDICT_CASES[name]
    ns = nsf(cus)[:K]
    a0 = steps(K, 0.3 if K == 2 else 0.2)
    us, xs, upiv, g = eval_inputs(a0, ns, seed=2000 + C * 8 + na, C=C)
    return a0, ns, us, xs, upiv, g, targets_for(a0, na)


# group C: name -> (K, nrep, ns, alpha0 step)
def _boot_ns(K, first):
    return (first + [30 + 3 * k for k in range(K)])[:K]


BOOT_EVAL_CASES = {
    "reg_K1_nrep1": (1, 1, [3 * 1024 + 5], 0.1),
    "reg_K2_nrep3": (2, 3, [1, 1025], 0.1),
    "reg_K5_nrep5": (5, 5, [1, 700, 1024, 1025, 3 * 1024 + 5], 0.1),
    "reg_K8_nrep6_tpc2": (8, 6, [33 * 1024 + 5, 1, 700, 1024, 1025, 63, 64, 65], 0.1),
    "lds16_K9_nrep3": (9, 3, _boot_ns(9, [700, 1, 1025]), 0.04),
    "lds16_K16_nrep5": (16, 5, _boot_ns(16, [1024, 1, 3 * 1024 + 5]), 0.04),
    "lds32_K17_nrep1": (17, 1, _boot_ns(17, [1025, 1, 700]), 0.02),
    "lds32_K32_nrep6": (32, 6, _boot_ns(32, [1, 1025, 700]), 0.02),
    "lds64_K33_nrep5": (33, 5, _boot_ns(33, [700, 1, 1024, 1025]), 0.01),
    "lds64_K64_nrep3_tpc2": (64, 3, _boot_ns(64, [5 * 1024 + 7, 1, 700, 1025]), 0.01),
}


def boot_eval_case(name):
    """(a0, ns, us, upiv, gref, g (nrep, K))."""
    K, nrep, ns, d = BOOT_EVAL_CASES[name]
    a0 = steps(K, d)
    us, _, upiv, gref = eval_inputs(a0, ns, seed=3000 + K * 8 + nrep)
    return a0, ns, us, upiv, gref, boot_g(gref, nrep, seed=3500 + K)


# group D: name -> (K, ns, C, n_alpha, row pitch or None); nrep = 5 throughout
_D3 = [1, 700, 1025]
BOOT_PREDICT_CASES = {
    "K3_C1_na1": (3, _D3, 1, 1, None), "K3_C2_na2": (3, _D3, 2, 2, None), "K3_C3_na3": (3, _D3, 3, 3, None),
    "K3_C4_na4_pitch7": (3, _D3, 4, 4, 7), "K3_C8_na5": (3, _D3, 8, 5, None), "K3_C33_na7": (3, _D3, 33, 7, None),
    "K3_C64_na8": (3, _D3, 64, 8, None), "K3_C65_na2_two_chunks": (3, _D3, 65, 2, None),
    "K3_C130_na3_three_chunks_pitch136": (3, _D3, 130, 3, 136),
    "K12_C8_na5": (12, _boot_ns(12, [1025, 1, 700]), 8, 5, None), "K12_C3_na7": (12, _boot_ns(12, [1025, 1, 700]), 3, 7, None),
    "K64_C2_na1_tpc2": (64, _boot_ns(64, [5 * 1024 + 7, 1, 700]), 2, 1, None),
}
BOOT_NREP = 5


def boot_predict_case(name):
    """(a0, ns, us, xs, upiv, gref, g (nrep, K), targets)."""
    K, ns, C, na, pitch = BOOT_PREDICT_CASES[name]
    a0 = steps(K, {3: 0.2, 12: 0.04, 64: 0.01}[K])
    us, xs, upiv, gref = eval_inputs(a0, ns, seed=4000 + K * 8 + C, C=C)
    return a0, ns, us, xs, upiv, gref, boot_g(gref, BOOT_NREP, seed=4500 + K + C), targets_for(a0, na)


# group E (txm_mbar_cov): name -> (alpha0 step, ns(cus), C or C(cus), n_alpha, row pitch or None)
def cov_cap(K, C, cus):
    """txm_mbar_cov's workgroups per (state, row tile, column group): about cus * 8 in all."""
    return max(1, cus * 8 // (K * (C // 16 + 1) * (K // 16 + 1)))


def cov_cap_one_C(cus):
    """The smallest C = 4 mod 16 at which 64 states (RT = 5) have K * NCG * RT > cus * 8: 100 on 256 compute units."""
    return 16 * (cus * 8 // (64 * 5)) + 4


def _cov64_ns(big):
    ns = [20 + 3 * k for k in range(64)]
    ns[0], ns[5] = 1, big
    return ns


COV_CASES = {
    "K16_C15_na8": (0.02, lambda cus: _boot_ns(16, [257, 1, 63]), 15, 8, None),
    "K17_C1_na1": (0.02, lambda cus: _lds64_ns(17), 1, 1, None),
    "K31_C15_na2": (0.02, lambda cus: _boot_ns(31, [1, 257]), 15, 2, None),
    "K32_C16_na3": (0.02, lambda cus: _boot_ns(32, [63, 64, 65]), 16, 3, None),
    "K33_C31_na4_pitch37": (0.01, lambda cus: _boot_ns(33, [1, 63, 64, 65, 257]), 31, 4, 37),
    "K48_C32_na5": (0.01, lambda cus: _boot_ns(48, [257, 1]), 32, 5, None),
    "K64_C17_na8_block_cap": (0.01, lambda cus: _cov64_ns(cov_cap(64, 17, cus) * 256 + 77), 17, 8, None),
    "K64_C*_na2_cap_one": (0.01, lambda cus: _cov64_ns(65), cov_cap_one_C, 2, None),
    "K8_C3_na8_block_cap": (0.1, lambda cus: [1, 63, cov_cap(8, 3, cus) * 256 + 77, 64, 65, 255, 257, 300], 3, 8, None),
}
COV_POOR = "poor_overlap_K2_C3"
COV_TINY = LD(2.0 ** -1022)
_cov_cache = {}


def cov_case(name, cus=CUS):
    """(a0, ns, us, xs, upiv, g, targets, logD, means, pitch) of a group E case; logD and means are made on the host."""
    if name == COV_POOR:
        a0, us, xs, upiv, g, targets = poor_overlap_predict_inputs(3)
        ns, pitch = [len(u) for u in us], None
    else:
        d, nsf, C, na, pitch = COV_CASES[name]
        ns, C = nsf(cus), (C(cus) if callable(C) else C)
        a0 = steps(len(ns), d)
        us, xs, upiv, g = eval_inputs(a0, ns, seed=5000 + len(ns) * 8 + na, C=C)
        targets = targets_for(a0, na)
    logD = np.ascontiguousarray(mo.eval_sums(us, a0, g, upiv).logD, dtype=np.float64)
    means = np.ascontiguousarray(mo.predict(us, xs, a0, upiv, targets, logD=logD).avg)
    return a0, ns, us, xs, upiv, g, targets, logD, means, pitch


def cov_reference(name, cus=CUS):
    """(cov_case(name), mo.cov_sums of it), once per process: the tests that share it leave it unchanged."""
    if (name, cus) not in _cov_cache:
        case = cov_case(name, cus)
        a0, ns, us, xs, upiv, g, targets, logD, means, _ = case
        _cov_cache[name, cus] = (case, mo.cov_sums(us, xs, a0, g, upiv, targets, means, logD))
    return _cov_cache[name, cus]


def cov_floor(ref, ns):
    """The absolute floor of every entry of Q, B, yy, b (long double; derivation: tests/test_mbar_kernels_gpu.py): a
    sample's product below 2^-1022 is lost before the division by N_k sum_n v_an, resp. (sum_n v_an)^2."""
    N, Nk = LD(sum(ns)), mo._ld(ns)
    q = COV_TINY * N / ref.den ** 2
    return {"Q": q, "B": COV_TINY * N / (ref.den[:, None] * Nk[None, :]), "yy": np.broadcast_to(q[:, None], ref.yy.shape),
            "b": COV_TINY * ref.dabs[:, :, None] / (ref.den[:, None, None] * Nk[None, None, :])}


# ---------------------------------------------------------------------------
# the pin to mpmath
# ---------------------------------------------------------------------------
def mp_sums(us, a0, g, upiv, counts):
    """S, H, obj, logD and each sum's kappa-weighted bound in mpmath, from the definitions."""
    K = len(a0)
    ut = [F(float(v)) - F(upiv) for u in us for v in u]
    kap = [1 + max(abs(F(float(gk))) + abs(F(float(ak)) * t) for gk, ak in zip(g, a0)) / 64 for t in ut]
    c = [F(1)] * len(ut) if counts is None else [F(int(v)) for v in counts]
    S, Sb = [F(0)] * K, [F(0)] * K
    H, Hb = [[F(0)] * K for _ in range(K)], [[F(0)] * K for _ in range(K)]
    obj = objb = F(0)
    lds = []
    for t, kn, cn in zip(ut, kap, c):
        e = [mp.exp(F(float(gk)) - F(float(ak)) * t) for gk, ak in zip(g, a0)]
        D = mp.fsum(e)
        p = [v / D for v in e]
        ld = mp.log(D)
        lds.append(ld)
        obj += cn * ld
        objb += cn * kn * abs(ld)
        for j in range(K):
            S[j] += cn * p[j]
            Sb[j] += cn * kn * p[j]
            for k in range(K):
                H[j][k] += cn * p[j] * p[k]
                Hb[j][k] += cn * kn * p[j] * p[k]
    return S, Sb, H, Hb, obj, objb, lds, kap


def mp_predict(us, xs, upiv, targets, lds, counts):
    ut = [F(float(v)) - F(upiv) for u in us for v in u]
    x = [row for v in xs for row in v]
    c = [F(1)] * len(ut) if counts is None else [F(int(v)) for v in counts]
    out = []
    for a in targets:
        w = [cn * mp.exp(-F(float(a)) * t - ld) for t, ld, cn in zip(ut, lds, c)]
        den = mp.fsum(w)
        C = len(x[0])
        out.append(([mp.fsum(wn * F(float(r[col])) for wn, r in zip(w, x)) / den for col in range(C)],
                    [mp.fsum(wn * abs(F(float(r[col]))) for wn, r in zip(w, x)) / den for col in range(C)]))
    return out


def _pin_problem(a0, us, xs, upiv, g, counts, targets):
    ev = mo.eval_sums(us, a0, g, upiv, counts)
    S, Sb, H, Hb, obj, objb, lds, kap = mp_sums(us, a0, g, upiv, counts)
    K = len(a0)
    lim, rel = F(PIN), F(1e-15)              # the bounds carry kappa_n as float64
    def q(v):                                  # a long double through 25 digits (it holds 19.3; float64 has no 1e-349)
        return F(np.format_float_scientific(LD(v), precision=24, unique=False))

    assert np.allclose(ev.kappa, [float(v) for v in kap], rtol=1e-15, atol=0)
    for j in range(K):
        assert abs(q(ev.S[j]) - S[j]) <= lim * Sb[j], ("S", j)
        assert abs(q(ev.S_bound[j]) - Sb[j]) <= rel * Sb[j]
        for k in range(K):
            assert abs(q(ev.H[j, k]) - H[j][k]) <= lim * Hb[j][k], ("H", j, k)
            assert abs(q(ev.H_bound[j, k]) - Hb[j][k]) <= rel * Hb[j][k]
            assert ev.H[j, k] == ev.H[k, j]
    assert abs(q(ev.obj) - obj) <= lim * objb and abs(q(ev.obj_bound) - objb) <= rel * objb
    for n, ld in enumerate(lds):
        assert abs(q(ev.logD[n]) - ld) <= lim * kap[n] * (1 + abs(ld)), ("logD", n)
    # predict, both forms: from the float64 logD a kernel would read, and from g with the counts
    ld64 = np.asarray(ev.logD, dtype=np.float64)
    forms = [(mo.predict(us, xs, a0, upiv, targets, logD=ld64), [F(float(v)) for v in ld64], None),
             (mo.predict(us, xs, a0, upiv, targets, g=g, counts=counts), lds, counts)]
    for got, ldm, cnt in forms:
        want = mp_predict(us, xs, upiv, targets, ldm, cnt)
        assert np.all(got.kappa >= 1.0) and np.all(got.kappa <= got.kappa_n.max())
        for a in range(len(targets)):
            for col in range(xs[0].shape[1]):
                v, s = want[a]
                # the float64 returned is the rounding of a long double: half an ulp of the value on top of the pin
                assert abs(F(float(got.avg[a, col])) - v[col]) <= (lim * F(float(got.kappa[a])) + F(2) ** -53) * s[col], (a, col)
                assert abs(F(float(got.scale[a, col])) - s[col]) <= F(1e-15) * s[col]
    return ev


def mp_cov(us, xs, a0, g, upiv, targets, means, logD):
    """Per target (Q, B, yy, b, lnw) and the kappa-weighted bounds of the first four, in mpmath from the definitions."""
    K, C = len(a0), xs[0].shape[1]
    ut = [F(float(v)) - F(upiv) for u in us for v in u]
    x = [[F(float(v)) for v in row] for xv in xs for row in xv]
    ld = [F(float(v)) for v in logD]
    Nk = [F(len(u)) for u in us]
    amax = max(abs(F(float(a))) for a in targets)
    kap = [1 + max(max(abs(F(float(gk))) + abs(F(float(ak)) * t) for gk, ak in zip(g, a0)), amax * abs(t) + abs(l)) / 64
           for t, l in zip(ut, ld)]
    W = []
    for t in ut:
        e = [mp.exp(F(float(gk)) - F(float(ak)) * t) for gk, ak in zip(g, a0)]
        D = mp.fsum(e)
        W.append([v / D / n for v, n in zip(e, Nk)])
    out = []
    for i, a in enumerate(targets):
        v = [mp.exp(-F(float(a)) * t - l) for t, l in zip(ut, ld)]
        den = mp.fsum(v)
        wa = [vn / den for vn in v]
        d = [[xn[c] - F(float(means[i][c])) for c in range(C)] for xn in x]
        val = {"Q": mp.fsum(w * w for w in wa), "B": [mp.fsum(Wn[k] * w for Wn, w in zip(W, wa)) for k in range(K)],
               "yy": [mp.fsum((w * dn[c]) ** 2 for w, dn in zip(wa, d)) for c in range(C)],
               "b": [[mp.fsum(Wn[k] * w * dn[c] for Wn, w, dn in zip(W, wa, d)) for k in range(K)] for c in range(C)],
               "lnw": mp.log(den)}
        bnd = {"Q": mp.fsum(kn * w * w for kn, w in zip(kap, wa)),
               "B": [mp.fsum(kn * Wn[k] * w for kn, Wn, w in zip(kap, W, wa)) for k in range(K)],
               "yy": [mp.fsum(kn * (w * dn[c]) ** 2 for kn, w, dn in zip(kap, wa, d)) for c in range(C)],
               "b": [[mp.fsum(kn * Wn[k] * w * abs(dn[c]) for kn, Wn, w, dn in zip(kap, W, wa, d)) for k in range(K)]
                     for c in range(C)]}
        out.append((val, bnd))
    return out, kap


def _pin_cov(a0, us, xs, upiv, g, targets):
    """mo.cov_sums against mp_cov at the host-made logD and centres of a group E case."""
    logD = np.asarray(mo.eval_sums(us, a0, g, upiv).logD, dtype=np.float64)
    means = mo.predict(us, xs, a0, upiv, targets, logD=logD).avg
    got = mo.cov_sums(us, xs, a0, g, upiv, targets, means, logD)
    want, kap = mp_cov(us, xs, a0, g, upiv, targets, means, logD)
    lim, rel = F(PIN), F(1e-15)
    def q(v):
        return F(np.format_float_scientific(LD(v), precision=24, unique=False))

    assert np.allclose(got.kappa_n, [float(v) for v in kap], rtol=1e-15, atol=0) and got.kappa == got.kappa_n.max()
    K, C = len(a0), xs[0].shape[1]
    for i, (val, bnd) in enumerate(want):
        pairs = [("Q", got.Q[i], got.Q_bound[i], val["Q"], bnd["Q"])]
        pairs += [(("B", k), got.B[i, k], got.B_bound[i, k], val["B"][k], bnd["B"][k]) for k in range(K)]
        pairs += [(("yy", c), got.yy[i, c], got.yy_bound[i, c], val["yy"][c], bnd["yy"][c]) for c in range(C)]
        pairs += [(("b", c, k), got.b[i, c, k], got.b_bound[i, c, k], val["b"][c][k], bnd["b"][c][k])
                  for c in range(C) for k in range(K)]
        for key, v, vb, w, wb in pairs:
            assert abs(q(v) - w) <= lim * wb, (i, key)
            assert abs(q(vb) - wb) <= rel * wb, (i, key)
        assert abs(q(got.lnw[i]) - val["lnw"]) <= lim * F(got.kappa) * (1 + abs(val["lnw"])), (i, "lnw")
        shift = q((-LD(targets[i]) * mo.pooled_ut(us, upiv) - mo._ld(logD)).max())      # den is sum_n v_an over its largest term
        assert abs(q(got.den[i]) - mp.exp(val["lnw"] - shift)) <= rel * q(got.den[i]) and got.den[i] >= 1
    return got


def test_long_double_is_80_bit():
    assert np.finfo(LD).eps < 1.1e-19


@pytest.mark.parametrize("K", [1, 3, 9])
def test_oracle_vs_mpmath(K):
    a0 = steps(K, 0.7 / max(K - 1, 1) if K > 1 else 0.0)
    ns = [40 + (3 * k) % 5 for k in range(K)]
    us, xs, upiv, g = eval_inputs(a0, ns, seed=K, C=2)
    ev = _pin_problem(a0, us, xs, upiv, g, None, targets_for(a0, 4))
    assert ev.p_min >= 1e-9 and ev.kappa.max() <= 2.0


def test_weighted_oracle_vs_mpmath():
    """Counts with zeros and a 3 (a bootstrap replicate's), log-weights off the reference row."""
    a0, ns = steps(3, 0.2), [41, 1, 38]
    us, xs, upiv, gref = eval_inputs(a0, ns, seed=77, C=3)
    rng = np.random.default_rng(78)
    counts = np.concatenate([rng.multinomial(n, np.full(n, 1.0 / n)) for n in ns])
    counts[:4] = [0, 3, 0, 1]
    assert (counts == 0).sum() > 10 and (counts == 3).any()
    _pin_problem(a0, us, xs, upiv, boot_g(gref, 2, 79)[1], counts, targets_for(a0, 3))


def test_poor_overlap_oracle_vs_mpmath():
    a0, us, _, upiv, g = poor_overlap_inputs(n=40)
    xs = gauss_xs(us, 2, np.random.default_rng(5), mu=100.0)
    ev = _pin_problem(a0, us, xs, upiv, g, None, np.array([0.1, 10.0, 3.0]))
    assert ev.p_min < 1e-308


def test_cov_oracle_vs_mpmath():
    """An ordinary problem with state rows in a second tile of 16 (K = 17, 3 to 5 samples per state)."""
    a0, ns = steps(17, 0.02), [3 + k % 3 for k in range(17)]
    us, xs, upiv, g = eval_inputs(a0, ns, seed=517, C=2)
    got = _pin_cov(a0, us, xs, upiv, g, targets_for(a0, 3))
    assert got.p_min >= 1e-9 and got.kappa <= 2.0


def test_cov_oracle_vs_mpmath_poor_overlap():
    a0, us, _, upiv, g = poor_overlap_inputs(n=30)
    xs = gauss_xs(us, 2, np.random.default_rng(6), mu=100.0)
    got = _pin_cov(a0, us, xs, upiv, g, POOR_TARGETS)
    assert got.p_min < 1e-308 and got.kappa > 2.0


# ---------------------------------------------------------------------------
# what the GPU tolerances assume of their inputs
# ---------------------------------------------------------------------------
def _ordinary(a0, us, upiv, g, targets=None):
    ut = mo.pooled_ut(us, upiv)
    t = mo.exponents(a0, g, ut)
    m = t.max(axis=0)
    ld = m + np.log(np.exp(t - m).sum(axis=0))
    p_min = float(np.exp(t - ld).min())
    assert p_min >= 1e-9, p_min
    assert mo.kappa(a0, g, ut, targets, ld).max() <= 2.0


@pytest.mark.parametrize("name", list(EVAL_CASES) + list(EVAL_NOLOGD))
def test_eval_case_inputs_are_ordinary(name):
    a0, ns, us, upiv, g = eval_case(name)
    assert [len(u) for u in us] == ns and max(a0) - min(a0) <= 0.7 + 1e-12
    off = g - ti_g(us, a0, upiv)                                            # not the starting point, not a constant off it
    assert abs(off).max() > 0.05 and (len(a0) == 1 or np.ptp(off) > 0.05)
    _ordinary(a0, us, upiv, g)


@pytest.mark.parametrize("name", list(PREDICT_CASES))
def test_predict_case_inputs_are_ordinary(name):
    a0, ns, us, xs, upiv, g, targets = predict_case(name)
    assert [len(u) for u in us] == ns and xs[0].shape[1] == PREDICT_CASES[name][2]
    _ordinary(a0, us, upiv, g, targets)


@pytest.mark.parametrize("name", list(BOOT_EVAL_CASES))
def test_boot_eval_case_inputs_are_ordinary(name):
    a0, ns, us, upiv, gref, g = boot_eval_case(name)
    d = (g - gref[None, :]).min(axis=1)
    assert np.all(d != 0.0) and (len(d) == 1 or len(set(d)) == len(d)) and abs(g - gref).max() <= 1.5
    for row in g:
        _ordinary(a0, us, upiv, row)


@pytest.mark.parametrize("name", list(BOOT_PREDICT_CASES))
def test_boot_predict_case_inputs_are_ordinary(name):
    a0, ns, us, xs, upiv, gref, g, targets = boot_predict_case(name)
    d = (g - gref[None, :]).min(axis=1)
    assert np.all(d != 0.0) and len(set(d)) == len(d) and abs(g - gref).max() <= 1.5
    for row in g:
        _ordinary(a0, us, upiv, row, targets)


def test_poor_overlap_targets_need_their_own_shift():
    """What makes the per-target maximum of txm_mbar_predict visible: the quotient does not change when a target's
    weights are shifted by a constant, so only an overflow (beyond e^709.78) can show that a wrong one was used."""
    a0, us, xs, upiv, g, targets = poor_overlap_predict_inputs(1)
    ut = mo.pooled_ut(us, upiv)
    ld = mo.eval_sums(us, a0, g, upiv).logD
    M = [float((-LD(a) * ut - ld).max()) for a in targets]
    assert M[1] - M[0] > 745.0 and abs(M[2] - M[0]) < 10.0


def test_poor_overlap_case_underflows_float64():
    a0, us, _, upiv, g = poor_overlap_inputs()
    ev = mo.eval_sums(us, a0, g, upiv)
    K0 = len(us[0])
    ut = mo.pooled_ut(us, upiv)
    p1_in_state0 = np.exp(mo.exponents(a0, g, ut)[1, :K0] - ev.logD[:K0])
    assert float(p1_in_state0.max()) < 1e-308 and ev.kappa.max() > 2.0


# ---- group E: txm_mbar_cov ------------------------------------------------------------------------------------------------
def test_cov_cases_hold_the_sizes_and_shapes_they_are_named_for():
    sizes = set()
    for name, (d, nsf, C, na, pitch) in COV_CASES.items():
        ns, C = nsf(CUS), (C(CUS) if callable(C) else C)
        sizes |= set(ns)
        K = len(ns)
        assert name.startswith(f"K{K}_") and f"_na{na}" in name and (f"_C{C}_" in name or "_C*_" in name)
        assert (pitch is None) == ("pitch" not in name) and (pitch is None or pitch > C)
        if K == 64:
            assert 6500 <= sum(ns) - max(ns) <= 7500                          # the reference stays near a second
    assert {1, 63, 64, 65, 257} <= sizes
    assert cov_cap_one_C(256) == 100 and 64 * 7 * 5 > 256 * 8 >= 64 * 6 * 5 and cov_cap(64, 100, 256) == 1
    assert cov_cap(64, 17, 256) == 3 and cov_cap(8, 3, 256) == 256


@pytest.mark.parametrize("name", list(COV_CASES))
def test_cov_case_inputs_are_ordinary(name):
    """What group E's tolerance assumes, from the reference alone; and that its floor is nothing here."""
    (a0, ns, us, xs, upiv, g, targets, logD, means, _), ref = cov_reference(name)
    assert [len(u) for u in us] == ns and means.shape == (len(targets), xs[0].shape[1]) and logD.shape == (sum(ns),)
    off = g - ti_g(us, a0, upiv)
    assert abs(off).max() > 0.05 and np.ptp(off) > 0.05                      # not a solution, not a constant off the start
    assert ref.p_min >= 1e-9, ref.p_min
    assert ref.kappa <= 2.0, ref.kappa
    floor = cov_floor(ref, ns)
    for key in ("Q", "B", "yy", "b"):
        bnd = getattr(ref, key + "_bound")
        assert np.all(bnd > 0) and np.all(floor[key] <= LD(1e-250) * 1e-12 * bnd), key


@pytest.mark.parametrize("name", list(COV_CASES) + [COV_POOR])
def test_cov_reference_weights_sum_to_one(name):
    """sum_k N_k B_ak = sum_n W_na sum_k p_kn = 1 for any g: a softmax sums to one."""
    (a0, ns, *_), ref = cov_reference(name)
    one = ref.B @ mo._ld(ns)
    print(f"\n{name}: sum_k N_k B_ak - 1: {float(np.abs(one - 1).max()):.1e}; p_min {ref.p_min:.1e}, kappa {ref.kappa:.3f}")
    assert np.all(np.abs(one - 1) <= len(ns) * 64 * mo.EPS_LD)


def test_cov_poor_overlap_case_needs_the_floor():
    """The one case where the floor is the larger part of a bound: p_kn underflows float64, and so do products p_kn v_an."""
    (a0, ns, us, xs, upiv, g, targets, logD, means, _), ref = cov_reference(COV_POOR)
    assert ref.p_min < 1e-308 and ref.kappa > 2.0
    floor = cov_floor(ref, ns)
    assert np.any(floor["B"] > 1e-12 * ref.B_bound) and np.any(floor["b"] > 1e-12 * ref.b_bound)
    assert np.all(floor["Q"] < 1e-200 * ref.Q_bound) and np.all(floor["yy"] < 1e-200 * ref.yy_bound)
    big = floor["B"] <= 1e-200 * ref.B_bound                                 # and entries the floor does not touch
    assert big.any() and np.all(ref.B[big] > 0)
