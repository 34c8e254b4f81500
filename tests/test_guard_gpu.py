"""The precision guard of the int8 bootstrap and its FP64 fallback, on every kernel that can meet it.

The guard (txm_resample_i8.h I8_GUARD, i8_table_kernel in txm_resample_i8.hip) flags every scaling window whose top-power
scale wmax * max|du|^J (times max|dx_c| for a column) exceeds I8_GUARD * sqrt(n) times the window's typical monomial (the
smallest group mean of |w du^J| or |w du^J dx_c|).  The FP64 kernel contracts the flagged windows in listed mode and
resample_finalize_i8_kernel / resample_finalize_y_kernel add its sums behind the int8 slots, in whichever slot layout the
int8 kernel of the call wrote.  Outlier data only reach that merge, so these tests put one outlier into u, into one
observable column, into the second matrix or into the weights and hold the result to the ORACLE (the long-double
definition `orc.truth_cov` on the materialised frequency rows) for replicates that drew the outlier and replicates that
did not, with the scale of the clean data.  Every case pins the kernel it means to reach (`resample_info()`) and how
many windows the guard sent to the FP64 kernel, so that a change of the dispatch rule fails here instead of moving the
case off its kernel.  Where the suite holds the table-fed kernel equal to the fused one bit for bit on clean data, it
must be equal on the dirty data too.

The threshold itself is restated on the host (`guard_ratios`): the window size of plan_i8, the sub-block statistics of
i8_stats_kernel (64 fine groups for a window of one sub-block, four per sub-block otherwise) and the test of
i8_table_kernel.  One sample is placed at 0.8 and at 1.25 times the threshold; the library must count exactly the
windows the restatement flags.
"""

import math

import numpy as np
import pytest
import torch

from test_i8_gpu import TOL, data, scale, truth_err

pytestmark = pytest.mark.gpu

SM_T = 1024          # samples per sampler tile (txm_sampler.h)
I8_GUARD = 275.0     # txm_resample_i8.h


@pytest.fixture(scope="module")
def eng(txm):
    from thermoextrap_amd import engine

    return engine


def tol(order):
    """The int8 path's contract against the oracle, relative to |truth| + the clean data's natural scale."""
    return TOL * max(1.0, 4.0 ** (order - 5))


def drew(freq, i):
    """(first replicate that did not draw sample i, first replicate that did)."""
    f = freq[:, i].cpu().numpy()
    without, with_ = np.flatnonzero(f == 0), np.flatnonzero(f > 0)
    assert len(without) and len(with_), "the seed gives no replicate on one side of the outlier"
    return int(without[0]), int(with_[0])


def y_means_err(ym, y, freq, reps, w, ysc):
    """max over `reps` of |ym[r] - sum f w y / sum f w| / (|want| + ysc), the reference sums in long double."""
    yh = y.cpu().numpy().astype(np.longdouble)
    wh = None if w is None else w.cpu().numpy().astype(np.longdouble)
    worst = 0.0
    for r in reps:
        f = freq[r].cpu().numpy().astype(np.longdouble)
        fw = f if wh is None else f * wh
        want = (fw[:, None] * yh).sum(axis=0) / fw.sum()
        e = np.abs(ym[r].cpu().numpy().astype(np.longdouble) - want) / (np.abs(want) + ysc)
        worst = max(worst, float(e.max()))
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# 1. fallback matrix: kernel x order x outlier site x options
OUT_U, OUT_X = 5.0e5, 4.0e4     # ~1e5 sigma in u and in an observable (order 0 looks at x alone)

MATRIX = [
    # N, C, order, site, column, weighted, y, rep0, nrep
    (150_000, 32, 0, "x", 7, False, False, 0, 64),       # wide, order 0: one row set
    (150_000, 32, 1, "u", 0, True, True, 7, 64),         # wide + y, the u row flags the window
    (120_000, 48, 3, "x", 40, False, False, 0, 70),      # second (16-column) group only; 3 + 1 row sets on the table kernel
    (120_000, 48, 5, "w", 0, True, True, 3, 64),         # two passes, one weight 1e8 x the rest, y
    (100_001, 40, 7, "u", 0, False, False, 0, 64),       # narrow tail group (32 + 8), order 7 in two passes
    (100_001, 40, 3, "y", 36, True, True, 5, 64),        # the tail with y runs the wide variant; only y's flags
    (150_000, 32, 7, "y", 31, False, True, 11, 65),      # y only, order 7, ragged replicate group
    (100_001, 40, 0, "w", 0, True, True, 0, 64),         # order 0 with a tail group and y
    (120_000, 48, 1, "x", 5, False, False, 2, 64),       # first group only
    (150_000, 2, 1, "u", 0, False, False, 0, 64),        # narrow, CPAD 4 (a 4-double row pitch lets the table kernel's DMA in)
    (150_000, 2, 5, "x", 1, True, False, 6, 64),
    (150_000, 4, 3, "x", 2, True, False, 9, 64),
    (150_000, 8, 5, "w", 0, True, False, 0, 64),
    (150_000, 8, 7, "u", 0, True, True, 2, 64),          # narrow call with y: y bootstrapped on its own behind it
    (150_000, 12, 7, "u", 0, False, False, 4, 64),       # four column quads, eight powers: two passes
    (150_000, 16, 5, "x", 15, False, False, 0, 70),      # four quads, six powers: two passes
    (100_001, 16, 1, "w", 0, True, False, 1, 64),
]


def dirty_case(N, C, seed, site, col, weighted, withy):
    """(clean, dirty) operands: data() of the sibling tests with bounded noise -- whose windows the guard never flags, so that
    the flagged windows are exactly the outlier's -- and one outlier at sample i_out."""
    if C == 2:                                  # a (N, 2) view of a 4-column array: row pitch 4 (what the narrow table DMA needs)
        xf, u = data(N, 4, seed, bounded=True)
        x = xf[:, :2]
    else:
        x, u = data(N, C, seed, bounded=True)
    g = torch.Generator(device="cuda").manual_seed(seed + 1)
    w = (0.25 + torch.rand(N, generator=g, dtype=torch.float64, device="cuda")) if weighted else None
    y = (0.5 * x + 0.3 * torch.rand(N, C, generator=g, dtype=torch.float64, device="cuda")) if withy else None
    clean = (x.clone(), u.clone(), None if w is None else w.clone(), None if y is None else y.clone())
    i = N // 3 + 37
    if site == "u":
        u[i] += OUT_U
    elif site == "x":
        x[i, col] += OUT_X
    elif site == "y":
        y[i, col] += OUT_X
    else:
        w[i] *= 1.0e8
    return clean, (x, u, w, y), i


def groups_hit(C, site, col):
    """Column groups of 32 whose outlier window the guard must flag: u and w enter every group's statistic, x and y only their own."""
    return (C + 31) // 32 if site in ("u", "w") else 1


@pytest.mark.parametrize("N,C,order,site,col,weighted,withy,rep0,nrep", MATRIX,
                         ids=[f"C{c[1]}-o{c[2]}-{c[3]}{'-w' if c[5] else ''}{'-y' if c[6] else ''}-r{c[7]}" for c in MATRIX])
def test_fallback_matrix(eng, orc, N, C, order, site, col, weighted, withy, rep0, nrep):
    K = order + 1
    seed = 100 + 7 * C + order
    (xc, uc, wc, yc), (x, u, w, y), i_out = dirty_case(N, C, seed, site, col, weighted, withy)
    s = eng.DeviceSampler(seed * 13 + 1, nrep, N, rep0=rep0)
    # the clean data of the same shape: nothing flagged
    eng.resample_vals(xc, uc, order, sampler=s, w=wc, y=yc, path="int8_fused")
    base = eng.resample_info()["windows_fp64"]
    assert base == 0, base
    hit = groups_hit(C, site, col)
    res = {}
    for path in ("int8_fused", "int8_table"):
        out = eng.resample_vals(x, u, order, sampler=s, w=w, y=y, path=path)
        info = eng.resample_info()
        print(f"{path}: kernel {info['kernel']}, windows_fp64 {info['windows_fp64']} of {info['windows']} (clean data: {base})")
        assert info["path"] == "int8" and info["kernel"] == path, info
        # the outlier's window in every column group it enters, and nothing else
        assert info["windows_fp64"] == hit, (info, hit)
        res[path] = out if withy else (out, None)
    (got, ym), (tab, ymt) = res["int8_fused"], res["int8_table"]
    # the same int8 sums and the same FP64 listed sums, merged by the finalize in the table kernel's slot layout: same bits
    assert torch.equal(tab, got)
    if withy:
        assert torch.equal(ymt, ym)
    assert torch.isfinite(got).all()
    freq = s.freq()
    reps = drew(freq, i_out)
    sc = scale(xc, uc, K).cpu().numpy()
    e = truth_err(orc, got, x, u, order, freq, reps, w=w, sc=sc)
    print(f"oracle: max err {e:.3e} (replicates {reps}: without / with the outlier), bound {tol(order):.1e}")
    assert e < tol(order), e
    if withy:
        ey = y_means_err(ym, y, freq, reps, w, float(yc.std()))
        print(f"y means: max err {ey:.3e}")
        assert ey < 1e-12, ey


BATCHED = [
    # S, N, C, order, state with the outlier, site, weighted
    (3, 150_000, 4, 1, 1, "u", False),
    (3, 150_000, 12, 7, 2, "x", True),
    (4, 120_000, 8, 3, 3, "w", True),
]


@pytest.mark.parametrize("S,N,C,order,sd,site,weighted", BATCHED)
def test_fallback_batched_narrow(eng, orc, S, N, C, order, sd, site, weighted):
    """The batched narrow launch (state on a grid axis): the outlier state's window goes to the FP64 kernel, every state
    equals its single call at rep0 = s * nrep bit for bit, and the outlier state meets the oracle on both sides."""
    nrep, K = 64, order + 1
    xs, us, ws = [], [], []
    for st in range(S):
        x, u = data(N, C, 300 + st, bounded=True)
        xs.append(x)
        us.append(u)
        ws.append(0.25 + torch.rand(N, generator=torch.Generator(device="cuda").manual_seed(400 + st), dtype=torch.float64, device="cuda"))
    ws = ws if weighted else None
    xc, uc = xs[sd].clone(), us[sd].clone()
    wc = ws[sd].clone() if ws is not None else None
    i_out = N // 2 + 11
    if site == "u":
        us[sd][i_out] += OUT_U
    elif site == "x":
        xs[sd][i_out, C // 2] += OUT_X
    else:
        ws[sd][i_out] *= 1.0e8
    smp = eng.DeviceSampler(55, S * nrep, N)
    got = eng.resample_vals_batched(xs, us, order, nrep=nrep, sampler=smp, ws=ws, path="int8")
    bi = eng.batched_info()
    eng.resample_vals(xc, uc, order, sampler=eng.DeviceSampler(55, nrep, N, rep0=sd * nrep), w=None if ws is None else wc, path="int8")
    base = eng.resample_info()["windows_fp64"]
    print(f"batched: {bi} (state {sd} on clean data: {base} windows flagged)")
    assert base == 0, base
    assert bi["path"] == "int8", bi
    total = 0
    for st in range(S):
        one = eng.resample_vals(xs[st], us[st], order, sampler=eng.DeviceSampler(55, nrep, N, rep0=st * nrep),
                                w=None if ws is None else ws[st], path="int8")
        info = eng.resample_info()
        assert info["path"] == "int8" and info["kernel"] == "int8_fused", info
        total += info["windows_fp64"]
        assert info["windows_fp64"] == (1 if st == sd else 0), (st, info)
        assert torch.equal(got[st], one), st
    assert bi["windows_fp64"] == total == 1, (bi, total)
    freq = smp.freq()[sd * nrep:(sd + 1) * nrep]
    reps = drew(freq, i_out)
    e = truth_err(orc, got[sd], xs[sd], us[sd], order, freq, reps, w=None if ws is None else ws[sd],
                  sc=scale(xc, uc, K).cpu().numpy())
    print(f"oracle (state {sd}): max err {e:.3e}")
    assert e < tol(order), e


# ---------------------------------------------------------------------------------------------------------------------
# 2. the threshold itself
def win_tiles(N):
    """plan_i8 (txm_resample.hip): 256-tile windows, quartered while there would be fewer than 256 of them, down to 4 tiles."""
    ntiles, wt = -(-N // SM_T), 256
    while wt > 4 and ntiles < 256 * wt:
        wt //= 4
    return wt


def guard_ratios(x, u, w, pivot, J, lo=0, hi=None):
    """Host restatement of the guard on windows [lo, hi): (ratio of the u row, ratios of the columns (nw, C), samples per
    window), ratio = statistic / (I8_GUARD sqrt(n)); a window is flagged where any ratio exceeds 1.

    i8_stats_kernel, per sub-block of min(16, win_tiles) tiles: u row groups by row phase mod 256 (thread tid walks rows
    i0 + tid, + 256, ...) -- 64 groups of four threads for a window of one sub-block, four of 64 otherwise; column groups by
    quarter of the sub-block x row phase mod 16 (64 groups), or by quarter alone (four).  Group means of |w du^J|
    (|w du^J dx_c|), their minimum over the window; i8_table_kernel: mtop = wmax max|du|^J (wmax = 1 unweighted)."""
    N, C = x.shape
    wt = win_tiles(N)
    st = min(wt, 16)
    nsub = wt // st
    fine = nsub == 1
    ws, ss = wt * SM_T, st * SM_T
    nwin = -(-N // ws)
    hi = nwin if hi is None else hi
    ru, rx, nn = [], [], []
    step = max(1, (1 << 22) // ws)                 # a few million rows at a time
    for a in range(lo, hi, step):
        b = min(hi, a + step)
        i0, i1 = a * ws, min(b * ws, N)
        du = np.abs(u[i0:i1] - pivot[0])
        dx = np.abs(x[i0:i1] - pivot[1:][None, :])
        wa = np.abs(w[i0:i1]) if w is not None else None
        mono = du ** J if wa is None else wa * du ** J
        loc = np.arange(i0, i1, dtype=np.int64)
        sb = loc // ss - a * nsub                   # sub-block within this stretch
        lr = loc % ss
        nsb = int(sb[-1]) + 1
        ug = (lr % 256) // (4 if fine else 64)
        gu = 64 if fine else 4
        xg = (lr // (ss // 4)) * 16 + lr % 16 if fine else lr // (ss // 4)
        ku, kx = sb * gu + ug, sb * gu + xg

        def group_min(key, vals):
            cnt = np.bincount(key, minlength=nsb * gu)
            s = np.bincount(key, weights=vals, minlength=nsb * gu)
            m = np.where(cnt > 0, s / np.maximum(cnt, 1), np.inf).reshape(nsb, gu).min(axis=1)
            m = np.concatenate([m, np.full((-nsb) % nsub, np.inf)])
            return m.reshape(-1, nsub).min(axis=1)      # per window

        starts = np.arange(0, i1 - i0, ws)
        dumax = np.maximum.reduceat(du, starts)
        wmax = np.maximum.reduceat(wa, starts) if wa is not None else 1.0
        n = np.diff(np.append(starts, i1 - i0)).astype(np.float64)
        theta = I8_GUARD * np.sqrt(n)
        mtop = wmax * dumax ** J
        ru.append(mtop / (theta * group_min(ku, mono)))
        mx = np.maximum.reduceat(dx, starts, axis=0)
        gx = np.stack([group_min(kx, mono * dx[:, c]) for c in range(C)], axis=1)
        rx.append(mtop[:, None] * mx / (theta[:, None] * gx))
        nn.append(n)
    return np.concatenate(ru), np.concatenate(rx), np.concatenate(nn)


def place_sample(x, u, pivot, J, k, rho, site, col):
    """Put one sample of window k at rho times the threshold: a u value (mtop grows as du^J) or an x value of column `col`
    (its max grows).  The sample sits in groups that are not the minimum of their sub-block, so the typical monomials the
    guard compares with do not move; the placement is checked against the restatement afterwards.  Returns its index."""
    N, C = x.shape
    ws = win_tiles(N) * SM_T
    st = min(win_tiles(N), 16) * SM_T
    fine = win_tiles(N) <= 16
    ru, rx, _ = guard_ratios(x, u, None, pivot, J, k, k + 1)
    du = np.abs(u - pivot[0])
    lo, hi = k * ws, min((k + 1) * ws, N)
    # group means of this window's rows (for the choice of a sample outside the minimal groups)
    loc = np.arange(lo, hi)
    lr = loc % st
    sbk = (loc - lo) // st
    gu = (lr % 256) // (4 if fine else 64) + sbk * 64
    gx = ((lr // (st // 4)) * 16 + lr % 16 if fine else lr // (st // 4)) + sbk * 64
    mono = du[lo:hi] ** J

    def argmin_group(key, vals):
        cnt = np.bincount(key)
        s = np.bincount(key, weights=vals)
        return int(np.argmin(np.where(cnt > 0, s / np.maximum(cnt, 1), np.inf)))

    bad_u = argmin_group(gu, mono)
    bad_x = {argmin_group(gx, mono * np.abs(x[lo:hi, c] - pivot[1 + c])) for c in range(C)}
    i = lo + next(j for j in range((hi - lo) // 2, hi - lo) if gu[j] != bad_u and gx[j] not in bad_x)
    if site == "u":
        a = max(ru[0], rx[0].max())                 # ratio per unit of mtop: max|du|^J of the bulk
        dumax = du[lo:hi].max()
        d = dumax * (rho / a) ** (1.0 / J)          # -> mtop = d^J, every ratio scales with it
        u[i] = pivot[0] + d
    else:
        dxmax = np.abs(x[lo:hi, col] - pivot[1 + col]).max()
        x[i, col] = pivot[1 + col] + dxmax * rho / rx[0, col]
    return i


@pytest.mark.parametrize("J", [1, 2, 4, 7])
@pytest.mark.parametrize("site", ["u", "x"])
@pytest.mark.parametrize("rho", [0.8, 1.25])
def test_threshold_both_sides(eng, orc, J, site, rho):
    """One sample at 0.8 (kept on the int8 kernel: the worst data it may keep) or 1.25 (sent to the FP64 kernel) times the
    guard's threshold, in u or in one column; a bounded bulk (uniform), so that the margins are the data's and not noise.
    The library counts exactly the windows the host restatement flags, and the result meets the oracle either way."""
    N, C, nrep, order = 5 * 4096 + 1500, 3, 64, J
    rng = np.random.default_rng(1000 + 10 * J + (site == "x"))
    pivot = np.array([100.0, 2.0, -1.0, 0.5])
    if site == "u":
        # |du| uniform in [0.8, 1] (x 3), lowered in the u row's group of row phases 0-3 mod 256 so that its mean of |du|^J is
        # half the others'; |dx| uniform in [0.9, 1.1] (x 0.4): the u row's statistic binds, the columns' stay below it
        mag = rng.uniform(0.8, 1.0, N)
        mag[np.arange(N) % 256 < 4] *= 0.5 ** (1.0 / J)
        u = pivot[0] + 3.0 * rng.choice([-1.0, 1.0], N) * mag
        x = pivot[1:][None, :] + 0.4 * rng.choice([-1.0, 1.0], (N, C)) * rng.uniform(0.9, 1.1, (N, C))
    else:
        tu = rng.uniform(-1.0, 1.0, N)
        u = pivot[0] + 3.0 * tu
        x = pivot[1:][None, :] + 0.4 * (0.5 * tu[:, None] + 0.5 * rng.uniform(-1.0, 1.0, (N, C)))
    xc, uc = x.copy(), u.copy()
    assert win_tiles(N) == 4
    k = 2
    i = place_sample(x, u, pivot, J, k, rho, site, 1)
    ru, rx, n = guard_ratios(x, u, None, pivot, J)
    r = np.maximum(ru, rx.max(axis=1))
    assert abs(r[k] / rho - 1.0) < 1e-9, (r[k], rho)
    others = np.delete(r, k)
    assert others.max() < 0.2, others
    want = int((r > 1.0).sum())
    assert want == (1 if rho > 1 else 0)
    # the statistic the case means to place: the u row's, or column 1's
    assert (ru[k] > 1.2 * rx[k].max()) if site == "u" else (rx[k, 1] > 1.2 * max(ru[k], np.delete(rx[k], 1).max())), (ru[k], rx[k])
    xd, ud, pd = (torch.as_tensor(a, device="cuda") for a in (x, u, pivot))
    s = eng.DeviceSampler(77 + J, nrep, N)
    got = eng.resample_vals(xd, ud, order, sampler=s, pivot=pd, path="int8")
    info = eng.resample_info()
    print(f"J {J}, {site}, {rho} theta: kernel {info['kernel']}, windows_fp64 {info['windows_fp64']} "
          f"(host: {want})")
    assert info["path"] == "int8" and info["kernel"] == "int8_fused", info
    assert info["windows_fp64"] == want, (info, want)
    freq = s.freq()
    reps = drew(freq, i)
    sc = scale(torch.as_tensor(xc, device="cuda"), torch.as_tensor(uc, device="cuda"), order + 1).cpu().numpy()
    e = truth_err(orc, got, xd, ud, order, freq, reps, sc=sc)
    print(f"oracle: max err {e:.3e} (bound {tol(order):.1e})")
    assert e < tol(order), e
    if rho < 1:
        # the realised error of the kept window against the guard's design bound 1e-13 n typ, typ = the typical monomial of
        # the statistic (u row, or the column with the sample), both as sums over samples: the top-power entry times the
        # replicate weight
        du = np.abs(u - pivot[0])[k * 4096:(k + 1) * 4096]
        mtop = du.max() ** J
        theta = I8_GUARD * math.sqrt(n[k])
        typ_u = mtop / (ru[k] * theta)
        typ_x = mtop * np.abs(x[k * 4096:(k + 1) * 4096, 1] - pivot[2]).max() / (rx[k, 1] * theta)
        for r_ in reps:
            t = orc.truth_cov(x, u, order, w=freq[r_].cpu().numpy().astype(np.float64))
            g_ = got[r_].cpu().numpy()
            W = float(freq[r_].sum())
            eu = abs(g_[0, 0, J] - t[0, 0, J]) * W / (1e-13 * n[k] * typ_u)
            ex = abs(g_[1, 1, J] - t[1, 1, J]) * W / (1e-13 * n[k] * typ_x)
            print(f"0.8 theta, replicate {r_}: top-power error / design bound: u row {eu:.3e}, column 1 {ex:.3e}")


def test_threshold_long_window(eng, orc):
    """N = 2^26: 256-tile windows of 16 sub-blocks -- the four-groups-per-sub-block rule of the north star's length.  One call
    holds a u sample at 1.25 theta (window 100) and an x sample at 0.8 theta (window 40): exactly one window is flagged;
    both the table-fed and the fused narrow kernel, bit for bit; the oracle on a replicate with and one without the flagged
    sample."""
    N, C, nrep, order, J = 1 << 26, 4, 8, 4, 4
    assert win_tiles(N) == 256
    g = torch.Generator(device="cuda").manual_seed(2026)
    pivot = np.array([50.0, 1.0, 2.0, 3.0, 4.0])
    tu = 2.0 * torch.rand(N, generator=g, dtype=torch.float64, device="cuda") - 1.0
    xd = torch.as_tensor(pivot[1:], device="cuda")[None, :] + 0.3 * (0.5 * tu[:, None] + (torch.rand(N, C, generator=g, dtype=torch.float64, device="cuda") - 0.5))
    ud = pivot[0] + 2.0 * tu
    del tu
    x, u = xd.cpu().numpy(), ud.cpu().numpy()
    xsc, usc = float(xd.std()), float(ud.std())
    i1 = place_sample(x, u, pivot, J, 100, 1.25, "u", 0)
    i2 = place_sample(x, u, pivot, J, 40, 0.8, "x", 2)
    ru, rx, _ = guard_ratios(x, u, None, pivot, J)
    r = np.maximum(ru, rx.max(axis=1))
    assert abs(r[100] / 1.25 - 1) < 1e-9 and abs(r[40] / 0.8 - 1) < 1e-9, (r[100], r[40])
    assert np.delete(r, [40, 100]).max() < 0.2
    want = int((r > 1).sum())
    assert want == 1
    ud[i1] = float(u[i1])
    xd[i2, 2] = float(x[i2, 2])
    pd = torch.as_tensor(pivot, device="cuda")
    s = eng.DeviceSampler(31, nrep, N)
    out = {}
    for path in ("int8_fused", "int8_table"):
        out[path] = eng.resample_vals(xd, ud, order, sampler=s, pivot=pd, path=path)
        info = eng.resample_info()
        print(f"N = 2^26: kernel {info['kernel']}, windows_fp64 {info['windows_fp64']} of {info['windows']} (host: {want})")
        assert info["path"] == "int8" and info["kernel"] == path and info["windows_fp64"] == want, info
    got = out["int8_fused"]
    assert torch.equal(out["int8_table"], got)
    # one replicate with and one without the flagged sample (the count rows one at a time: 0.5 GB each)
    f1 = [int(s.rows(r, r + 1).freq()[0, i1].item()) for r in range(nrep)]
    reps = [f1.index(0), next(r for r in range(nrep) if f1[r] > 0)]
    sc = np.empty((C, 2, J + 1))
    for b in range(J + 1):
        sc[:, 0, b] = usc ** b
        sc[:, 1, b] = xsc * usc ** b
    worst = 0.0
    for r in reps:
        fr = s.rows(r, r + 1).freq()[0].cpu().numpy().astype(np.float64)
        t = orc.truth_cov(x, u, order, w=fr)
        worst = max(worst, float((np.abs(got[r].cpu().numpy() - t) / (np.abs(t) + sc)).max()))
    print(f"N = 2^26 oracle: max err {worst:.3e} (replicates {reps})")
    assert worst < tol(order), worst


# ---------------------------------------------------------------------------------------------------------------------
# 3. pre-pass blocks and replicate slabs that carry guard flags and a fallback list
@pytest.mark.parametrize("nrep,kernel", [(64, "int8_fused"), (256, "int8_table")])
def test_prep_block_with_flagged_windows(txm, eng, nrep, kernel):
    """Two bootstraps through one data object with an outlier: the second reuses the block (flags and run list included),
    both carry the same count of flagged windows, and their bits equal a fresh call without any block."""
    from thermoextrap_amd.moments import DeviceDataArray

    N, C, order = 300_000, 32, 4
    x, u = data(N, C, 61, heavy=True)
    d = txm.DataCentralMomentsVals.from_vals(xv=DeviceDataArray(x, ("rec", "val")), uv=DeviceDataArray(u, ("rec",)),
                                             order=order, central=True)
    spec = {"nrep": nrep, "seed": 19, "device": True}
    with eng.forced_path("int8"):
        a = d.resample(spec).dxduave.device_values.clone()
        i1 = eng.resample_info()
        b = d.resample(spec).dxduave.device_values.clone()
        i2 = eng.resample_info()
        fresh = eng.resample_vals(x, u, order, sampler=eng.DeviceSampler(19, nrep, N))
        i3 = eng.resample_info()
    print(f"first {i1}, second {i2}, fresh {i3}")
    assert i1["kernel"] == i2["kernel"] == i3["kernel"] == kernel
    assert not i1["prep_reused"] and i2["prep_reused"] and not i3["prep_reused"]
    assert 2 <= i1["windows_fp64"] == i2["windows_fp64"] == i3["windows_fp64"] <= 4, (i1, i2, i3)
    assert torch.equal(a, b) and torch.equal(a, fresh)


def test_workspace_budget_slabs_with_flagged_windows(txm):
    """The workspace-budget slabs of engine.resample_vals on dirty data: the rows of the unslabbed call bit for bit, on the
    fused and the table-fed kernel, with and without a second matrix, one pre-pass block for all slabs."""
    from thermoextrap_amd import engine as eng

    N, C = 1_200_000, 32
    x, u = data(N, C, 71, heavy=True)
    y = 0.5 * x + 1.0
    y[N // 5, 3] += 4.0e4
    L = eng._L()
    for nrep, order, path, withy in ((1000, 4, None, False), (700, 6, "int8_table", True), (600, 3, "int8_fused", True),
                                     (520, 1, "int8_fused", False)):
        s = eng.DeviceSampler(78, nrep, N, rep0=5)
        kw = dict(sampler=s, path=path, y=y if withy else None)
        old = eng.WORKSPACE_BUDGET_BYTES
        try:
            eng.WORKSPACE_BUDGET_BYTES = 1 << 50
            whole = eng.resample_vals(x, u, order, **kw)
            iw = eng.resample_info()
            need = L.txm_resample_vals_ws_bytes_opts(N, C, nrep, order, eng._call_path(path), int(withy))
            eng.WORKSPACE_BUDGET_BYTES = need // 3
            assert eng._slab_size(L, N, C, nrep, order, eng._call_path(path), withy) < nrep
            prep = eng.ResamplePrep()
            parts = eng.resample_vals(x, u, order, prep=prep, **kw)
            ip = eng.resample_info()
        finally:
            eng.WORKSPACE_BUDGET_BYTES = old
        print(f"nrep {nrep}, order {order}, {path}, y {withy}: whole {iw}, last slab {ip}")
        assert iw["kernel"] == ip["kernel"] != "fp64" and iw["windows_fp64"] == ip["windows_fp64"] >= 2, (iw, ip)
        a, b = (whole, parts) if not withy else (whole[0], parts[0])
        assert torch.equal(a, b), (nrep, order, path)
        if withy:
            assert torch.equal(whole[1], parts[1]), (nrep, order, path)
        assert prep.misses == 1 and prep.hits >= 2, (prep.misses, prep.hits)
