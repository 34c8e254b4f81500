"""The lag sums of a state collection (txm_lag_rows_batched, txm_lag_sums_batched) and the collection-level timeseries
functions on the device.

The central contract is bits: row i of a batched call equals engine.lag_sums of that state and pair alone, whatever else
is in the batch.  The shapes are the smallest at which the batched kernels can differ from the single call: lengths around
the 16-sample tile, the 256-lag block and the 1008-sample stage, several chunks, and one state above 1008 * 512 records,
whose chunks have two stages (chunk length 2016) next to one-stage states and which sets grid.x.  One comparison is
independent of the single call: the long-double restatement of tests/test_timeseries_cpu.py, held to check_lag_sums' bound
1e-12 (1 + |mu_a| / sigma_a + |mu_b| / sigma_b) sum |dA| |dB|."""

import ctypes as ct

import numpy as np
import pytest
import torch

from test_timeseries_cpu import ref_centered, ref_lag_sum
from test_timeseries_gpu import ar1, correlated_state, series_of

pytestmark = pytest.mark.gpu

NS = [1, 3, 255, 257, 1007, 1008, 1009, 2017, 4099, 200_000, 600_000]
C = 2
NPAIRS = 2 * C + 1


@pytest.fixture(scope="module")
def eng(txm):
    from thermoextrap_amd import engine

    assert engine.LAG_STAGE == 1008 and engine.lag_chunks(600_000) == 298 and engine.lag_chunks(200_000) == 199
    return engine


class Batch:
    """Host and device copies of a list of states, their centres, the rows handle and a cache of single-call references."""

    def __init__(self, eng, host, xd=None, center=None):
        self.eng, self.host = eng, host
        self.u = [torch.as_tensor(u).cuda() for u, _ in host]
        if xd is None:
            xd = [torch.as_tensor(x).cuda() if x.shape[1] else None for _, x in host]
        self.x = xd
        self.center = [eng.lag_center(x, u) for x, u in zip(self.x, self.u)] if center is None else center
        self.handle = eng.lag_rows_batched(None if self.x[0] is None else self.x, self.u, self.center)
        self._ref = {}

    def single(self, s, p, t0, nlags):
        key = (s, p, t0, nlags)
        if key not in self._ref:
            self._ref[key] = self.eng.lag_sums(self.x[s], self.u[s], [p], t0, nlags, center=self.center[s])[0].clone()
        return self._ref[key]

    def check(self, items, t0, nlags):
        got = self.eng.lag_sums_batched(self.handle, items, t0, nlags)
        again = self.eng.lag_sums_batched(self.handle, items, t0, nlags)
        assert got.shape == (len(items), nlags) and torch.equal(got, again)          # two calls: the same bits
        for row, (s, p) in enumerate(items):
            assert torch.equal(got[row], self.single(s, p, t0, nlags)), (s, p, t0, nlags, len(self.host[s][0]))
        return got


@pytest.fixture(scope="module")
def ragged(eng):
    return Batch(eng, [correlated_state(n, C, 300 + i) for i, n in enumerate(NS)])


def all_items(ns, npairs):
    return [(s, p) for s in range(len(ns)) for p in range(npairs)]


def test_first_block_all_pairs_in_shuffled_order(ragged):
    assert ragged.handle.C == C and ragged.handle.ns.tolist() == NS
    items = all_items(NS, NPAIRS)
    order = np.random.default_rng(0).permutation(len(items))
    got = ragged.check([items[i] for i in order], 0, 256)
    for row, i in enumerate(order):
        n = NS[items[i][0]]
        if n < 256:
            assert (got[row, n:] == 0.0).all()                                         # lags beyond n: exact zeros
    assert (got[:, 0] != 0.0).sum() >= len(items) - NPAIRS                            # (n = 1: the centred series is zero)


@pytest.mark.parametrize("t0, nlags", [(256, 512), (1024, 1024)])
def test_pair_subsets_per_state_two_and_four_tiles(ragged, t0, nlags):
    """NT = 2 and 4; every state another subset of its pairs, one state cross pairs only, a state listed in two places."""
    items = []
    for s in range(len(NS)):
        sub = [(s + k) % NPAIRS for k in range(1 + s % 3)]
        if s == 9:
            sub = [C + 1, 2 * C]                                                      # cross pairs only
        items += [(s, p) for p in sub]
    items.append((10, 4))                                                             # the long state again, behind the others
    kinds = {s: {p > C for st, p in items if st == s} for s in range(len(NS))}
    assert kinds[9] == {True} and any(k == {False} for k in kinds.values()) and any(k == {True, False} for k in kinds.values())
    ragged.check(items, t0, nlags)
    ragged.check([(10, 0), (0, 0)], t0, nlags)                                        # auto pairs only: one instance launched
    ragged.check([(8, 3)], t0, nlags)                                                 # a single cross item


def test_block_past_the_short_states(ragged):
    """(3840, 512): every state up to 3840 records lies entirely below the block and must give exact zeros."""
    items = all_items(NS, NPAIRS)[::-1]
    got = ragged.check(items, 3840, 512)
    for row, (s, p) in enumerate(items):
        if NS[s] <= 3840:
            assert (got[row] == 0.0).all(), (s, p)
        else:
            assert (got[row, : min(512, NS[s] - 3840)] != 0.0).any()
            if NS[s] - 3840 < 512:
                assert (got[row, NS[s] - 3840:] == 0.0).all()


def test_energy_only_states(eng):
    ns = [5, 1009, 70_001]
    b = Batch(eng, [correlated_state(n, 0, 40 + i) for i, n in enumerate(ns)])
    assert b.handle.C == 0
    b.check([(2, 0), (0, 0), (1, 0)], 0, 256)
    b.check([(1, 0), (2, 0)], 512, 512)


def test_five_columns_row_pitch_and_an_unaligned_pointer(eng):
    """C = 5 as column slices of wider matrices (pitch 8 > C), the second state's x 8 bytes off a 16-byte boundary."""
    ns, Cw = [300, 2500, 70_001], 5
    host = [correlated_state(n, Cw, 60 + i) for i, n in enumerate(ns)]
    xd = []
    for i, (_, x) in enumerate(host):
        n = x.shape[0]
        buf = torch.zeros(n * 8 + 2, dtype=torch.float64, device="cuda")
        off = (buf.data_ptr() % 16) // 8                       # 0 here: the allocator aligns
        if i == 1:
            off = 1 - off
        view = buf[off:off + n * 8].view(n, 8)[:, :Cw]
        view.copy_(torch.as_tensor(x).cuda())
        assert view.stride() == (8, 1) and view.data_ptr() % 16 == (8 if i == 1 else 0)
        xd.append(view)
    tight = Batch(eng, host)
    b = Batch(eng, host, xd, tight.center)                      # (one set of centres: the layouts are compared bit for bit)
    items = all_items(ns, 2 * Cw + 1)
    g0 = b.check(items, 0, 256)
    assert torch.equal(g0, tight.check(items, 0, 256))         # the layout changes no bits
    b.check(items[::3], 256, 256)
    # states that differ in their pitch are copied to one tight layout: still the same bits
    mixed = eng.lag_rows_batched([xd[0], tight.x[1], xd[2]], b.u, b.center)
    assert torch.equal(eng.lag_sums_batched(mixed, items, 0, 256), g0)


def test_against_the_long_double_restatement(ragged):
    """Independent of the single call's kernel: three states, six lags, every pair, check_lag_sums' bound."""
    lags = [0, 1, 17, 255, 300, 1023]
    states = [NS.index(n) for n in (257, 2017, 200_000)]
    items = [(s, p) for s in states for p in range(NPAIRS)]
    blocks = {t: (t // 256 * 256, 256) for t in lags}
    got = {blk: ragged.eng.lag_sums_batched(ragged.handle, items, *blk).cpu().numpy() for blk in set(blocks.values())}
    worst = 0.0
    for row, (s, p) in enumerate(items):
        u, x = ragged.host[s]
        n = len(u)
        A, B = series_of(p, u, x)
        dA, dB = ref_centered(A, B)
        sa, sb = float(dA.std()), float(dB.std())
        mid = 1.0 + abs(float(np.mean(A))) / sa + abs(float(np.mean(A if B is None else B))) / sb
        aA, aB = np.abs(dA), np.abs(dB)
        for t in lags:
            ref = float(ref_lag_sum(dA, dB, t))
            bound = 1e-12 * mid * (float(np.dot(aA[: n - t], aB[t:])) if t < n else 0.0)
            val = got[blocks[t]][row, t - blocks[t][0]]
            err = abs(val - ref)
            if bound > 0:
                worst = max(worst, err / bound)
            assert err <= bound, (n, p, t, val, ref, err, bound)
    print(f"batched lag sums against long double: worst |hip - ref| / bound = {worst:.3e} (limit 1)")
    assert worst > 0.0


def test_buffers_are_not_overrun_and_slicing_changes_no_bits(ragged, eng, monkeypatch):
    from thermoextrap_amd import _lib

    L = eng._L()
    pick = [0, 6, 9, 10]                                                              # n = 1, 1009, 200 000, 600 000
    ns = np.ascontiguousarray([NS[s] for s in pick], dtype=np.int64)
    np_ns = ns.ctypes.data_as(ct.POINTER(ct.c_int64))
    S, BAND = len(pick), 4096
    tab = (_lib.LagState * S)(*[_lib.LagState(ragged.x[s].data_ptr(), ragged.u[s].data_ptr(), ragged.center[s].data_ptr(), NS[s])
                                for s in pick])
    nrows = L.txm_lag_rows_batched_bytes(np_ns, S, C)
    rows = torch.full((nrows + BAND,), 0xA5, dtype=torch.uint8, device="cuda")
    stream = ct.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.txm_lag_rows_batched(tab, S, C, C, ct.c_void_p(rows.data_ptr()), nrows, stream) == 0, _lib.last_error()
    items = [(i, p) for i in range(S) for p in range(NPAIRS)]
    itab = (_lib.LagItem * len(items))(*[_lib.LagItem(s, p) for s, p in items])
    for t0, nlags in ((0, 256), (1024, 1024)):
        nws = L.txm_lag_sums_batched_ws_bytes(np_ns, S, C, itab, len(items), nlags)
        assert nws == eng.lag_sums_batched_ws_bytes(ns, items, nlags)
        ws = torch.full((nws + BAND,), 0xA5, dtype=torch.uint8, device="cuda")
        out = torch.full((len(items) * nlags + BAND // 8,), float("nan"), dtype=torch.float64, device="cuda")
        rc = L.txm_lag_sums_batched(ct.c_void_p(rows.data_ptr()), nrows, np_ns, S, C, itab, len(items), t0, nlags,
                                    ct.c_void_p(out.data_ptr()), ct.c_void_p(ws.data_ptr()), nws, stream)
        assert rc == 0, _lib.last_error()
        torch.cuda.synchronize()
        assert (rows[nrows:] == 0xA5).all() and (ws[nws:] == 0xA5).all() and torch.isnan(out[len(items) * nlags:]).all()
        got = out[: len(items) * nlags].view(len(items), nlags)
        for row, (i, p) in enumerate(items):
            assert torch.equal(got[row], ragged.single(pick[i], p, t0, nlags))
    # the engine cuts the item list where the partials exceed the budget: >= 3 library calls, the same bits
    items = all_items(NS, NPAIRS)
    whole = ragged.check(items, 256, 256)
    budget = eng.lag_sums_batched_ws_bytes(NS, items, 256) // 4
    assert len(eng.lag_item_slices(NS, items, 256, budget)) >= 3
    calls = []
    real = L.txm_lag_sums_batched

    class Spy:
        def __getattr__(self, name):
            if name == "txm_lag_sums_batched":
                return lambda *a: (calls.append(a[6]), real(*a))[1]
            return getattr(L, name)

    monkeypatch.setattr(eng, "WORKSPACE_BUDGET_BYTES", budget)
    monkeypatch.setattr(eng, "_L", lambda: Spy())
    cut = eng.lag_sums_batched(ragged.handle, items, 256, 256)
    assert len(calls) >= 3 and sum(calls) == len(items)
    assert torch.equal(cut, whole)


# ---------------------------------------------------------------------------
# the public functions
# ---------------------------------------------------------------------------
PUB = [(phi, n) for phi in (0.0, 0.5, 0.9, 0.99) for n in (4099, 50_000, 200_000)]


@pytest.fixture(scope="module")
def pub():
    """Ragged AR(1) states, C = 2: u = AR(phi), both columns tied to u (the estimator is ill-conditioned for a pair whose
    covariance nearly vanishes: its C(t) is noise over a tiny sigma^2 and g comes out in the thousands).  At n = 4099,
    phi = 0.99 the scan runs past lag 1024: several lag blocks, the short state still active in the (1024, 1024) block."""
    out = []
    for i, (phi, n) in enumerate(PUB):
        u = 10.0 + ar1(phi, 700 + i, n)
        x = np.stack([0.6 * u + 0.8 * ar1(0.7, 800 + i, n) + 3.0, 0.3 * u + ar1(0.7, 900 + i, n) - 1.0], axis=1)
        out.append((u, x))
    return out


def same_ineff(a, b):
    return (a.g_u == b.g_u and a.g_max == b.g_max and a.stop_u == b.stop_u and np.array_equal(a.g_x, b.g_x)
            and np.array_equal(a.g_cross, b.g_cross) and np.array_equal(a.stop_x, b.stop_x) and np.array_equal(a.stop_cross, b.stop_cross)
            and a.stop_x.dtype == b.stop_x.dtype and a.g_x.shape == b.g_x.shape)


@pytest.fixture(scope="module")
def pub_single(txm, pub):
    return {fast: [txm.statistical_inefficiencies(u, x, fast=fast) for u, x in pub] for fast in (False, True)}


@pytest.mark.parametrize("fast", [False, True])
def test_inefficiencies_of_the_states_are_the_states_own(txm, pub, pub_single, fast):
    got = txm.statistical_inefficiencies_states([u for u, _ in pub], [x for _, x in pub], fast=fast)
    assert len(got) == len(pub) and all(isinstance(g, txm.timeseries.Inefficiencies) for g in got)
    for s, (a, b) in enumerate(zip(got, pub_single[fast])):
        assert same_ineff(a, b), (s, PUB[s], a, b)
    assert max(g.g_max for g in got) > 50 and min(g.g_max for g in got) < 10          # the grid spans short and long memories
    # device inputs, the energies alone, mintime and max_lag reach the scan
    ud = [torch.as_tensor(u).cuda() for u, _ in pub[:4]]
    e = txm.statistical_inefficiencies_states(ud, None, fast=fast, mintime=7)
    for s in range(4):
        one = txm.statistical_inefficiencies(ud[s], None, fast=fast, mintime=7)
        assert same_ineff(e[s], one) and e[s].g_x.shape == (0,)


def _values(o):
    return None if o is None else (o.tensor.cpu().numpy() if hasattr(o, "tensor") else np.asarray(o.values))


def _same_decorrelated(a, b):
    for k in range(3):
        va, vb = _values(a[k]), _values(b[k])
        assert (va is None) == (vb is None) and type(a[k]) is type(b[k])
        if va is not None:
            assert a[k].dims == b[k].dims and np.array_equal(va, vb)
    ia, ib = a[3], b[3]
    assert ia["g"] == ib["g"] and ia["n"] == ib["n"] and np.array_equal(ia["indices"], ib["indices"])
    assert (ia["inefficiencies"] is None) == (ib["inefficiencies"] is None)
    if ia["inefficiencies"] is not None:
        assert same_ineff(ia["inefficiencies"], ib["inefficiencies"])


@pytest.mark.parametrize("kind", ["host", "device"])
def test_decorrelate_states(txm, pub, kind):
    from thermoextrap_amd.moments import DeviceDataArray
    from thermoextrap_amd.xrlite import DataArray

    rng = np.random.default_rng(3)
    us, xs = [u for u, _ in pub], [x for _, x in pub]
    ws = [rng.uniform(0.5, 2.0, len(u)) for u in us]
    if kind == "device":
        us = [torch.as_tensor(u).cuda() for u in us]
        xs = [DeviceDataArray(torch.as_tensor(x).cuda(), ("rec", "val")) for x in xs]
        ws = [torch.as_tensor(w).cuda() for w in ws]
    S = len(us)
    want = DeviceDataArray if kind == "device" else DataArray
    # estimated g, with and without weights
    for w_list in (ws, None):
        got = txm.decorrelate_states(us, xs, w_list)
        assert len(got) == S
        for s in range(S):
            one = txm.decorrelate(us[s], xs[s], None if w_list is None else ws[s])
            _same_decorrelated(got[s], one)
            assert isinstance(got[s][0], want) and isinstance(got[s][1], want) and (got[s][2] is None) == (w_list is None)
            assert got[s][3]["inefficiencies"] is not None and 1 <= got[s][3]["n"] <= len(pub[s][0])
    # weights for some states only; keywords of the estimate; conservative
    some = [w if s % 2 else None for s, w in enumerate(ws)]
    got = txm.decorrelate_states(us, xs, some, conservative=True, fast=True, mintime=5)
    for s in range(S):
        _same_decorrelated(got[s], txm.decorrelate(us[s], xs[s], some[s], conservative=True, fast=True, mintime=5))
    # a list of given g, and one g for all
    gs = [1.0 + 0.75 * s for s in range(S)]
    got = txm.decorrelate_states(us, xs, ws, g=gs)
    for s in range(S):
        _same_decorrelated(got[s], txm.decorrelate(us[s], xs[s], ws[s], g=gs[s]))
        assert got[s][3]["inefficiencies"] is None
    got = txm.decorrelate_states(us, xs, g=7.5, conservative=True)
    for s in range(S):
        _same_decorrelated(got[s], txm.decorrelate(us[s], xs[s], g=7.5, conservative=True))
    with pytest.raises(TypeError):
        txm.decorrelate_states(us, xs, g=gs, fast=True)
    with pytest.raises(ValueError):
        txm.decorrelate_states(us, xs, g=gs[:-1])
    with pytest.raises(ValueError):
        txm.decorrelate_states(us, xs, ws[:-1])
    # the outputs feed from_vals unchanged
    uo, xo, _, _ = got[1]
    d = txm.DataCentralMomentsVals.from_vals(xv=xo, uv=uo, order=2, central=True)
    assert np.asarray(d.dxduave.values).shape[-2:] == (2, 3)


def test_block_lengths_feed_the_collection(txm, pub, pub_single):
    us, xs = [u for u, _ in pub], [x for _, x in pub]
    got = txm.block_lengths(us, xs)
    assert got == [txm.timeseries.block_length(u, x) for u, x in pub] and all(type(b) is int and b >= 1 for b in got)
    assert got == [max(1, int(np.ceil(10.0 * i.g_max))) for i in pub_single[False]]
    # derivs_cov(block=B) needs 2 B <= N: at n = 4099 and phi = 0.99 (g ~ 350 from so short a series) the default factor of
    # 10 asks for more than half the series, so the collection is fed with factor 2
    blocks = txm.block_lengths(us, xs, factor=2.0, fast=True)
    assert blocks == [txm.timeseries.block_length(u, x, factor=2.0, fast=True) for u, x in pub]
    assert all(2 * b <= len(u) for b, u in zip(blocks, us))
    DA = txm.DataArray

    def models():
        return [txm.beta.factory_extrapmodel(beta=1.0 + 0.1 * s, data=txm.DataCentralMomentsVals.from_vals(
            xv=DA(x, ("rec", "val")), uv=DA(u, ("rec",)), order=2, central=True)) for s, (u, x) in enumerate(pub)]

    cov = txm.StateCollection(models()).derivs_cov(block=blocks)
    cross = txm.StateCollection(models()).derivs_cross_cov(block=blocks)
    assert cov.shape[0] == cross.shape[0] == len(pub)
    for s, m in enumerate(models()):
        assert np.array_equal(np.asarray(cov.values)[s], np.asarray(m.derivs_cov(block=blocks[s]).values))
    assert np.isfinite(np.asarray(cross.values)).all()
    with pytest.raises(ValueError):
        txm.block_lengths(us, xs, factor=0.0)


def test_input_errors_name_the_state(txm, pub):
    us, xs = [u for u, _ in pub[:3]], [x.copy() for _, x in pub[:3]]
    xs[1][:, 1] = 2.5                                                                 # a constant column in state 1
    with pytest.raises(ValueError, match=r"x\[1\] of state 1\b"):
        txm.statistical_inefficiencies_states(us, xs)
    with pytest.raises(ValueError, match=r"x\[1\] of state 1\b"):
        txm.decorrelate_states(us, xs)
    with pytest.raises(ValueError, match=r"x\[1\] of state 1\b"):
        txm.block_lengths(us, xs)
    xs[1] = pub[1][1]
    with pytest.raises(ValueError, match=r"of state \d+ has not crossed zero by max_lag"):
        txm.statistical_inefficiencies_states(us, xs, max_lag=4)
    with pytest.raises(ValueError):
        txm.statistical_inefficiencies_states(us, xs[:2])                             # lists of unequal length
    with pytest.raises(ValueError):
        txm.statistical_inefficiencies_states(us, [xs[0], xs[1][:, :1], xs[2]])       # different column counts
    with pytest.raises(ValueError):
        txm.statistical_inefficiencies_states([], [])
    with pytest.raises(ValueError):
        txm.statistical_inefficiencies_states(us, [xs[0], xs[1][:-1], xs[2]])         # records of x and u differ
    with pytest.raises(TypeError):
        txm.statistical_inefficiencies_states([us[0], [1.0, 2.0, 3.0]], xs[:2])       # what _device_series refuses
    with pytest.raises(TypeError):
        txm.decorrelate_states(us, None)
