"""Differential tests of txm_mbar_block_cov (txm_mbar_block.hip) through the C ABI against the long-double restatement
tests/_mbar_block_ref.py.  g is NOT a solution (the thermodynamic-integration start plus noise) and logD, mean and lnw are
made on the host, as in group E of tests/test_mbar_kernels_gpu.py: no other device kernel supplies an input.

Tolerances (derived, not measured):

  every centred block sum   |hip - ref| <= 1e-12 (b_beta + (len_beta / n_s) sum_{beta' in s} b_beta'),
                            b_beta = sum_{n in beta} kappa_n |t_n|,
                            kappa_n = 1 + max(|g_k| + |a0_k ut_n|, |a ut_n| + |logD_n|) / 64 + max_a |lnw_a| / 64
  every entry of Gamma_l    |hip - ref| <= 1e-12 sum_beta beta_beta(i) beta_beta(j),
                            beta_beta = sum_{n in beta} |t_n| + (len_beta / n_s) sum_{n in s} |t_n|

kappa_n is the README's MBAR rule (an exponent g_k - a0_k ut or -a ut - logD carries eps (|g_k| + 2 |a0_k ut|), a relative
error of the weight of at most 128 eps kappa_n) plus the subtraction of lnw_a from the exponent, one more rounding of size
eps |lnw_a|.  x is centred on the mean itself inside the pass (d = x - mean_ac, one rounding, relative to |d|): there is
no pivot and no correction term, so nothing is added for one.  The block sums themselves are not an output: after a call
with n_levels = 1 the workspace still holds the centred sums at the offset the plan names, and the test reads them there;
the bound of a centred sum is the block's own plus its share of the state's.

Exact claims: Gamma_l is symmetric; two calls give equal bits; the centred sums of a state with one block are 0.0, and so
is Gamma when every state has one block; nblocks is the restatement's.

Shapes: the smallest at which each index expression can go wrong.  Ragged states (1000, 777, 1300) with B = 64 (short
last blocks), B = 1 (more blocks than a chunk of 1024 and more units than the grid), B above every n_s (one block each)
and B = n_s for one state only; K at 1, 2, 3, 8, 9, 17 and 64 (fewer states than the four lanes of a record; the LDS row
of all 64); C at 1, 15, 16, 17 and 33 (C + 1 at and around a power of two: 2, 16, 32 and 64 lanes a row, M across the
16-column tiles and, at K = 64 with eight targets, across a second macro tile); one and eight targets; five levels from
odd block counts, so that an unpaired block survives every level, and down to a state's last block; blocks above 4096
records, which are summed in pieces (a short last block leaves a piece empty).  Every case runs in a guard-banded
workspace of exactly the plan's bytes with NaN scratch, under the smallest plan and -- where it differs -- the full one.
"""

import ctypes as ct

import numpy as np
import pytest
import torch

import _mbar_block_ref as br
from _bands import Banded
from oracle import mbar_oracle as mo
from test_mbar_oracle_cpu import eval_inputs, steps, targets_for

pytestmark = pytest.mark.gpu
TOL = 1e-12
LD = np.longdouble
SIZE_MAX = ct.c_size_t(-1).value
RAGGED = [1000, 777, 1300]
MIX = [1000, 1, 63, 64, 65, 257]


def sizes(K):
    if K <= 3:
        return RAGGED[:K]
    return [MIX[k % 6] if k < 6 else 20 + 3 * k for k in range(K)]


# name -> (K, C, n_alpha, ns or None, block, n_levels)
CASES = {
    "K3_C1_na1_B64": (3, 1, 1, None, 64, 1),
    "K3_C15_na8_B1": (3, 15, 8, None, 1, 1),
    "K3_C16_na1_B_above_every_state": (3, 16, 1, None, 5000, 1),
    "K3_C17_na8_B_one_state_whole": (3, 17, 8, None, [64, 777, 64], 1),
    "K3_C1_na8_odd_counts_L5": (3, 1, 8, None, [7, 9, 11], 5),
    "K1_C33_na1_B64_L5": (1, 33, 1, None, 64, 5),
    "K2_C1_na8_B64": (2, 1, 8, None, 64, 1),
    "K8_C1_na1_B64": (8, 1, 1, None, 64, 1),
    "K9_C16_na8_B64_L5": (9, 16, 8, None, 64, 5),
    "K17_C15_na8_B1": (17, 15, 8, None, 1, 1),
    "K64_C33_na8_B64": (64, 33, 8, None, 64, 1),
    "K3_C1_na1_pieces": (3, 1, 1, [9000, 5000, 300], 4500, 1),
    "K3_C17_na1_pieces_L5": (3, 17, 1, [13000, 4097, 300], [4097, 2000, 7], 5),
}
_cache = {}


def reference(name):
    """(inputs, restatement), once per process: the tests that share it leave it unchanged."""
    if name not in _cache:
        K, C, na, ns, block, nl = CASES[name]
        ns = sizes(K) if ns is None else ns
        a0 = steps(K, 0.1 if K <= 3 else 0.01)
        us, xs, upiv, g = eval_inputs(a0, ns, seed=9000 + 16 * K + na + C, C=C)
        targets = targets_for(a0, na)
        logD = np.ascontiguousarray(mo.eval_sums(us, a0, g, upiv).logD, dtype=np.float64)
        means = np.ascontiguousarray(mo.predict(us, xs, a0, upiv, targets, logD=logD).avg, dtype=np.float64)
        ut = mo.pooled_ut(us, upiv)
        lnw = []
        for a in targets:
            ex = -LD(a) * ut - logD.astype(LD)
            lnw.append(ex.max() + np.log(np.exp(ex - ex.max()).sum()))
        lnw = np.ascontiguousarray(np.array(lnw, dtype=LD), dtype=np.float64)
        r = br.rows(us, xs, a0, g, upiv, targets, logD, means, lnw)
        blk = [block] * K if np.ndim(block) == 0 else list(block)
        case = (a0, ns, us, xs, upiv, g, targets, logD, means, lnw, blk, nl)
        _cache[name] = (case, br.gammas(r.t, r.kappa, ns, blk, nl))
    return _cache[name]


@pytest.fixture(scope="module")
def eng(txm):
    from thermoextrap_amd import engine

    return engine


def plan_of(case, ws_bytes):
    from thermoextrap_amd import _lib

    L = _lib.load()
    a0, ns, us, xs, upiv, g, targets, logD, means, lnw, blk, nl = case
    K = len(ns)
    p = (ct.c_int64 * 7)()
    rc = L.txm_mbar_block_cov_plan((ct.c_int64 * K)(*ns), (ct.c_int64 * K)(*blk), K, xs[0].shape[1], len(targets), nl,
                                   ws_bytes, p)
    return rc, list(p)


def run(eng, case, ws_bytes):
    """(gamma, nblocks, centred level-0 sums or None) of one call in a guard-banded workspace of exactly ws_bytes (NaN
    scratch) with gamma and nblocks in guard-banded buffers of their own."""
    from thermoextrap_amd import _lib

    L = _lib.load()
    a0, ns, us, xs, upiv, g, targets, logD, means, lnw, blk, nl = case
    K, na, C = len(ns), len(targets), xs[0].shape[1]
    M = K + na * (C + 1)
    ud = [torch.as_tensor(u, dtype=torch.float64).cuda() for u in us]
    xd = [torch.as_tensor(x, dtype=torch.float64).cuda() for x in xs]
    tab, keep, _, _ = eng._mbar_table(ud, xd)
    a0 = np.ascontiguousarray(a0, dtype=np.float64)
    g = np.ascontiguousarray(g, dtype=np.float64)
    al = np.ascontiguousarray(targets, dtype=np.float64)
    ld, md, wd = (torch.as_tensor(v).cuda() for v in (logD, means, lnw))
    rc, plan = plan_of(case, ws_bytes)
    assert rc == 0 and plan[5] <= ws_bytes and plan[0] == M
    ws = Banded(ws_bytes, "nan")
    gam = Banded(nl * M * M * 8, "value")
    nbl = Banded(nl * K * 8, "value", dtype=torch.int64)
    dp = ct.POINTER(ct.c_double)
    rc = L.txm_mbar_block_cov(tab, K, C, float(upiv), a0.ctypes.data_as(dp), g.ctypes.data_as(dp), eng._ptr(ld),
                              al.ctypes.data_as(dp), na, eng._ptr(md), eng._ptr(wd), (ct.c_int64 * K)(*blk), nl,
                              ct.c_void_p(gam.ptr), ct.c_void_p(nbl.ptr), ct.c_void_p(ws.ptr), ws_bytes, eng._stream())
    torch.cuda.synchronize()
    assert rc == 0, _lib.last_error()
    del keep
    assert ws.check() and gam.check() and nbl.check(), "txm_mbar_block_cov wrote outside its workspace or its outputs"
    assert gam.unwritten() == 0 and nbl.unwritten() == 0
    Tc = None
    if nl == 1:
        Tc = ws.view(torch.float64)[plan[6] // 8:plan[6] // 8 + plan[1] * M].cpu().numpy().reshape(plan[1], M)
    return gam.view().cpu().numpy().reshape(nl, M, M), nbl.view(torch.int64).cpu().numpy().reshape(nl, K), Tc, plan


def check(name, case, ref, gamma, nblocks, Tc):
    ns, blk = case[1], case[10]
    assert np.all(np.isfinite(gamma))
    assert np.array_equal(nblocks, ref.nblocks)
    assert np.array_equal(gamma, np.swapaxes(gamma, -1, -2)), "Gamma is not exactly symmetric"
    q = np.abs(gamma.astype(LD) - ref.gamma)
    ok = q <= LD(TOL) * ref.bound
    worst = float(np.max(np.where(ref.bound > 0, q / np.where(ref.bound > 0, ref.bound, 1), 0)))
    line = f"\n{name}: worst |Gamma - ref| / bound-sum {worst:.2e}"
    for l in range(len(gamma)):
        if np.all(ref.nblocks[l] == 1):
            assert not gamma[l].any(), "every state has one block, Gamma is not exactly 0.0"
    if Tc is not None:
        bounds = br.block_bounds(ns, blk)
        st = np.array([s for s, _, _ in bounds])
        ln = np.array([hi - lo for _, lo, hi in bounds], dtype=LD)
        want = br.centre(ref.T, bounds, ns)
        tb = np.array(ref.T_bound, dtype=LD)
        for s in range(len(ns)):
            sel = st == s
            tb[sel] += (ln[sel] / LD(ns[s]))[:, None] * ref.T_bound[sel].sum(axis=0)[None, :]
            if sel.sum() == 1:
                assert not Tc[sel].any(), "a state with one block is not centred to exactly 0.0"
                want[sel] = 0
        d = np.abs(Tc.astype(LD) - want)
        line += f", centred block sums {float(np.max(d / np.where(tb > 0, tb, 1))):.2e}"
        print(line)
        assert np.all(d <= LD(TOL) * tb), name
    else:
        print(line)
    assert np.all(ok), (name, worst)


@pytest.mark.parametrize("name", list(CASES))
def test_block_cov_against_long_double(eng, name):
    case, ref = reference(name)
    rc, least = plan_of(case, 0)
    assert rc == -3 and least[4] == 0
    rc, full = plan_of(case, SIZE_MAX)
    assert rc == 0 and full[:4] == least[:4] and full[4] >= 1 and full[5] >= least[5]
    assert full[1] == int(ref.nblocks[0].sum()) and full[5] >= 8 * full[1] * full[0]
    gamma, nblocks, Tc, plan = run(eng, case, full[5])
    assert plan == full
    check(name + " (full plan)", case, ref, gamma, nblocks, Tc)
    if least[5] < full[5]:                                  # more than 256 blocks: several block workgroups in the Gram pass
        g1, n1, T1, p1 = run(eng, case, least[5])
        assert p1[4] == 1 and p1[5] == least[5]
        check(name + " (smallest plan)", case, ref, g1, n1, T1)
        if T1 is not None:
            assert np.array_equal(T1, Tc)                   # the block sums do not depend on the plan
    # no atomics: two calls under one plan give the same bits
    again, _, T2, _ = run(eng, case, full[5])
    assert np.array_equal(again, gamma) and (Tc is None or np.array_equal(T2, Tc))


def test_refusals_come_before_anything_is_enqueued(eng):
    from thermoextrap_amd import _lib

    L = _lib.load()
    case, _ = reference("K3_C1_na1_B64")
    rc, least = plan_of(case, 0)
    a0, ns, us, xs, upiv, g, targets, logD, means, lnw, blk, nl = case
    K = 3
    ud = [torch.as_tensor(u, dtype=torch.float64).cuda() for u in us]
    xd = [torch.as_tensor(x, dtype=torch.float64).cuda() for x in xs]
    tab, keep, _, _ = eng._mbar_table(ud, xd)
    ld, md, wd = (torch.as_tensor(v).cuda() for v in (logD, means, lnw))
    dp = ct.POINTER(ct.c_double)
    a0 = np.ascontiguousarray(a0, dtype=np.float64)
    g = np.ascontiguousarray(g, dtype=np.float64)
    al = np.ascontiguousarray(targets, dtype=np.float64)
    ws = Banded(least[5], "nan")
    gam = Banded(5 * 5 * 8, "value")
    nbl = Banded(3 * 8, "value", dtype=torch.int64)

    def call(ws_bytes, block, n_levels=1):
        return L.txm_mbar_block_cov(tab, K, 1, float(upiv), a0.ctypes.data_as(dp), g.ctypes.data_as(dp), eng._ptr(ld),
                                    al.ctypes.data_as(dp), 1, eng._ptr(md), eng._ptr(wd), (ct.c_int64 * K)(*block), n_levels,
                                    ct.c_void_p(gam.ptr), ct.c_void_p(nbl.ptr), ct.c_void_p(ws.ptr), ws_bytes, eng._stream())

    assert call(least[5] - 1, blk) == -3 and b"smallest" in L.txm_last_error()
    assert call(least[5], [64, 0, 64]) == -1
    assert call(least[5], blk, n_levels=33) == -1
    torch.cuda.synchronize()
    assert ws.holds_fill() and gam.unwritten() == 25 and nbl.unwritten() == 3
    del keep
