"""The collection-level timeseries functions without a device: the joint host scan against the per-state scan on numpy lag
sums (the restatement of tests/test_timeseries_cpu.py), the host logic of the batched C entry points (sizes, every refusal),
the struct mirrors, the item slicing of engine.lag_sums_batched and the lazy exports."""

import ctypes as ct
import re
from pathlib import Path

import numpy as np
import pytest

from test_timeseries_cpu import numpy_fetch

ROOT = Path(__file__).resolve().parent.parent
LENGTHS = [2, 3, 200, 257, 258, 700, 1500]
PHIS = [0.0, 0.9, 0.99]


def ar1(phi, seed, n):
    from scipy.signal import lfilter

    return lfilter([1.0], [1.0, -phi], np.random.default_rng(seed).standard_normal(n)) + 3.0


@pytest.fixture(scope="module")
def states():
    """One state per (phi, n): u = AR(phi), one column correlated with u; pairs 0 = u, 1 = x, 2 = (x, u).  The per-state
    numpy fetches are shared (and never changed) by the tests below."""
    out = []
    for i, phi in enumerate(PHIS):
        for j, n in enumerate(LENGTHS):
            u = ar1(phi, 100 * i + j, n)
            x = 0.5 * u + ar1(0.5, 1000 + 100 * i + j, n)
            out.append((n, numpy_fetch([(u, None), (x, None), (x, u)])))
    return out


def joint_fetch(states, calls):
    def fetch(items, t0, nlags):
        calls.append((list(items), t0, nlags))
        return np.concatenate([states[s][1]([p], t0, nlags) for s, p in items], axis=0)

    return fetch


@pytest.mark.parametrize("fast", [False, True])
@pytest.mark.parametrize("mintime", [3, 50, 300])
def test_joint_scan_equals_the_per_state_scan(states, fast, mintime):
    from thermoextrap_amd.timeseries import lag_blocks, scan_lag_sums, scan_lag_sums_states

    ns = [n for n, _ in states]
    calls = []
    got = scan_lag_sums_states(joint_fetch(states, calls), ns, [range(3)] * len(ns), fast=fast, mintime=mintime)
    assert len(got) == len(ns)
    stops, single = [], []
    for s, (n, f) in enumerate(states):
        mine = []

        def rec(pairs, t0, nl, f=f, mine=mine):
            mine.append((t0, nl, list(pairs)))
            return f(pairs, t0, nl)

        g, stop = scan_lag_sums(rec, n, range(3), fast=fast, mintime=mintime)
        assert np.array_equal(got[s][0], g) and np.array_equal(got[s][1], stop), (s, n)
        assert got[s][1].dtype == np.int64
        stops.append(stop)
        single.append(mine)
    # one fetch per block of the common sequence, none repeated
    blocks = [(t0, nl) for _, t0, nl in calls]
    assert blocks == list(lag_blocks(max(ns)))[: len(blocks)] and len(set(blocks)) == len(blocks)
    if mintime == 300:                                               # nothing stops before lag 300 but a series that runs out
        assert blocks[:2] == [(0, 256), (256, 256)]
    # block 0 holds every pair of every state, in state order
    assert calls[0][0] == [(s, p) for s in range(len(ns)) for p in range(3)]
    for items, t0, nl in calls[1:]:
        assert len(set(items)) == len(items)
        for s, p in items:
            assert t0 < ns[s] - 1                                    # lag_blocks(n_s)'s own rule
            assert stops[s][p] >= t0                                 # a stopped pair is absent from later blocks
    # every state sees in the joint fetches exactly the (block, pairs) its own scan fetches
    for s in range(len(ns)):
        joint = [(t0, nl, [p for st, p in items if st == s]) for items, t0, nl in calls]
        assert [j for j in joint if j[2]] == single[s], s
    second = calls[1][0] if len(calls) > 1 else []
    for s, n in enumerate(ns):
        mine = [it for it in second if it[0] == s]
        if n <= 257:
            assert not mine                                          # n = 257: t0 = 256 is not below n - 1
        if n == 258 and mintime == 300 and not fast:                 # present: it has not stopped, and lag 256 < n - 1
            assert len(mine) == 3 and all(stops[s] == 257)


def test_joint_scan_pair_subsets_and_errors(states):
    from thermoextrap_amd.timeseries import scan_lag_sums, scan_lag_sums_states

    ns = [n for n, _ in states]
    sub = [[2, 0] if s % 2 else [1] for s in range(len(ns))]
    got = scan_lag_sums_states(joint_fetch(states, []), ns, sub)
    for s, (n, f) in enumerate(states):
        g, stop = scan_lag_sums(f, n, sub[s])
        assert np.array_equal(got[s][0], g) and np.array_equal(got[s][1], stop)
    # max_lag: the longest phi = 0.99 state has not crossed zero by lag 5, and the error names it
    worst = max(range(len(ns)), key=lambda s: (scan_lag_sums(states[s][1], ns[s], [0])[1][0], s))
    lag = int(scan_lag_sums(states[worst][1], ns[worst], [0])[1][0])
    assert lag > 20
    others_ok = [s for s in range(len(ns)) if scan_lag_sums(states[s][1], ns[s], [0])[1][0] <= lag - 1]
    assert others_ok
    keep = others_ok + [worst]
    with pytest.raises(ValueError, match=rf"energy of state {len(keep) - 1}\b.*max_lag"):
        scan_lag_sums_states(joint_fetch([states[s] for s in keep], []), [ns[s] for s in keep], [[0]] * len(keep), max_lag=lag - 1,
                             names=[["energy"]] * len(keep))
    ok = scan_lag_sums_states(joint_fetch([states[s] for s in keep], []), [ns[s] for s in keep], [[0]] * len(keep), max_lag=lag)
    assert ok[-1][1][0] == lag
    # sigma^2 == 0 names the pair and the state
    const = (100, numpy_fetch([(np.full(100, 2.5), None)]))
    with pytest.raises(ValueError, match=r"sigma_AB\^2 = 0 for pair 0 of state 1\b"):
        scan_lag_sums_states(joint_fetch([states[2], const], []), [states[2][0], 100], [[0], [0]])
    with pytest.raises(ValueError):
        scan_lag_sums_states(joint_fetch(states, []), ns, [[0]])          # one pair list for many states


# ---------------------------------------------------------------------------
# the C ABI without a device
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from thermoextrap_amd import _build, _lib

    _build.build_library()
    return _lib.load()


def chunks(n):
    return -(-n // (1008 * max(1, -(-n // (1008 * 512)))))


def ldd(n):
    return -(-n // 16) * 16


def i64(vals):
    return (ct.c_int64 * len(vals))(*vals)


def items_of(pairs):
    from thermoextrap_amd import _lib

    return (_lib.LagItem * len(pairs))(*[_lib.LagItem(s, p) for s, p in pairs])


def test_bytes_functions_are_host_logic(lib):
    R, W = lib.txm_lag_rows_batched_bytes, lib.txm_lag_sums_batched_ws_bytes
    ns = [1, 3, 255, 1008, 1009, 600_000, 1_000_000]
    for C in (0, 2, 5):
        body = sum(8 * (1 + C) * ldd(n) for n in ns)
        got = R(i64(ns), len(ns), C)
        assert body <= got <= body + 64 * len(ns) + 256, (C, got, body)             # the head: <= 64 bytes per state + padding
    assert R(i64([1000]), 1, 2) - R(i64([1000]), 1, 1) == 8 * ldd(1000)
    for bad in ((None, 1, 2), (i64([5]), 0, 2), (i64([5] * 3), 65536, 2), (i64([5, 0]), 2, 2), (i64([5, (1 << 36) + 1]), 2, 2),
                (i64([5]), 1, -1), (i64([5]), 1, 16384)):
        assert R(*bad) == 0, bad
    assert R(i64([1 << 36]), 1, 0) > 0 and R(i64([5]), 1, 16383) > 0
    C = 2
    its = [(5, 0), (6, 4), (0, 1), (5, 3), (2, 2), (6, 0)]
    n_chunks = sum(chunks(ns[s]) for s, _ in its)
    assert chunks(600_000) == 298 and chunks(1_000_000) == 497 and chunks(1008) == 1 and chunks(1009) == 2
    w256, w512, w4096 = (W(i64(ns), len(ns), C, items_of(its), len(its), nl) for nl in (256, 512, 4096))
    assert w512 - w256 == 8 * 256 * n_chunks and w4096 - w256 == 8 * 3840 * n_chunks   # the partials: exactly 8 nlags sum chunks
    assert 0 <= w256 - 8 * 256 * n_chunks <= 16 * len(its) + 256                        # the item table
    one = W(i64(ns), len(ns), C, items_of([(6, 0)]), 1, 256)
    two = W(i64(ns), len(ns), C, items_of([(6, 0), (0, 0)]), 2, 256)
    assert two - one == 8 * 256 * 1                                                    # a short state costs its own chunks only
    ok = (i64(ns), len(ns), C, items_of(its), len(its), 256)
    assert W(*ok) > 0
    for k, v in ((0, None), (1, 0), (1, 65536), (2, -1), (2, 16384), (3, None), (4, 0), (4, 65536), (5, 0), (5, 255), (5, 300), (5, 8192)):
        bad = list(ok)
        bad[k] = v
        assert W(*bad) == 0, (k, v)
    assert W(i64(ns), len(ns), C, items_of([(7, 0)]), 1, 256) == 0 and W(i64(ns), len(ns), C, items_of([(-1, 0)]), 1, 256) == 0
    assert W(i64(ns), len(ns), C, items_of([(0, 5)]), 1, 256) == 0 and W(i64(ns), len(ns), C, items_of([(0, -1)]), 1, 256) == 0
    assert W(i64([0] + ns[1:]), len(ns), C, items_of(its), len(its), 256) == 0


def test_batched_validation_needs_no_device(lib):
    from thermoextrap_amd import _lib

    one = ct.c_void_p(4096)                                          # never dereferenced: validation comes first
    err = lib.txm_last_error
    ns = [1000, 5, 70_000]
    C = 3

    def st(x=4096, u=4096, center=4096, n=1000):
        return _lib.LagState(x, u, center, n)

    def rows_call(states=None, S=None, ldx=4, C=C, rows=one, nbytes=None):
        states = [st(n=n) for n in ns] if states is None else states
        S = len(states) if S is None else S
        tab = (_lib.LagState * max(len(states), 1))(*states) if states != "null" else None
        if nbytes is None:
            nbytes = lib.txm_lag_rows_batched_bytes(i64([s.n for s in states]), len(states), C) if states != "null" else 0
        return lib.txm_lag_rows_batched(tab, S, ldx, C, rows, nbytes, None)

    assert rows_call(states="null", S=1) == -1 and b"null" in err()
    assert rows_call(rows=None) == -1 and b"null" in err()
    assert rows_call(states=[st(u=None)]) == -1 and b"null" in err()
    assert rows_call(states=[st(center=None)]) == -1 and b"null" in err()
    assert rows_call(states=[st(), st(x=None)]) == -1 and b"null x of state 1" in err()
    assert rows_call(S=0) == -1 and b"S = 0" in err()
    assert rows_call(S=65536) == -1 and b"S = 65536" in err()
    assert rows_call(states=[st(n=0)], nbytes=4096) == -1 and b"n = 0" in err()
    assert rows_call(states=[st(), st(n=(1 << 36) + 1)], nbytes=4096) == -1 and b"of state 1" in err()
    assert rows_call(C=-1, nbytes=4096) == -1 and b"C = -1" in err()
    assert rows_call(C=16384, ldx=16384, nbytes=4096) == -1 and b"C = 16384" in err()
    assert rows_call(ldx=2) == -1 and b"pitch" in err()
    good = lib.txm_lag_rows_batched_bytes(i64(ns), 3, C)
    assert rows_call(nbytes=good - 8) == -1 and b"rows_bytes" in err()
    assert rows_call(nbytes=good + 8) == -1 and b"rows_bytes" in err()

    its = [(0, 0), (2, 6), (1, 3)]

    def sums_call(rows=one, nbytes=good, n=ns, S=3, C=C, items=its, n_items=None, t0=0, nlags=256, out=one, ws=one, nws=1 << 40):
        tab = items_of(items) if items is not None else None
        n_items = len(items) if n_items is None else n_items
        return lib.txm_lag_sums_batched(rows, nbytes, i64(n) if n is not None else None, S, C, tab, n_items, t0, nlags, out, ws,
                                        nws, None)

    for name in ("rows", "n", "items", "out", "ws"):
        assert sums_call(**{name: None}, **({"n_items": 3} if name == "items" else {})) == -1 and b"null" in err(), name
    assert sums_call(S=0) == -1 and b"S = 0" in err()
    assert sums_call(S=65536) == -1 and b"S = 65536" in err()
    assert sums_call(n=[1000, 0, 70_000]) == -1 and b"of state 1" in err()
    assert sums_call(n=[1000, 5, (1 << 36) + 1]) == -1 and b"of state 2" in err()
    assert sums_call(C=-1) == -1 and b"C = -1" in err()
    assert sums_call(C=16384) == -1 and b"C = 16384" in err()
    assert sums_call(n_items=0) == -1 and b"n_items = 0" in err()
    assert sums_call(n_items=65536) == -1 and b"n_items = 65536" in err()
    assert sums_call(items=[(0, 0), (3, 0)]) == -1 and b"state index 3 (item 1)" in err()
    assert sums_call(items=[(-1, 0)]) == -1 and b"state index -1" in err()
    assert sums_call(items=[(0, 7)]) == -1 and b"pair index 7" in err()               # 2 C = 6 is the last
    assert sums_call(items=[(0, 6), (0, -1)]) == -1 and b"pair index -1 (item 1)" in err()
    assert sums_call(t0=100) == -1 and b"t0" in err()
    assert sums_call(t0=-256) == -1 and b"t0" in err()
    for nl in (0, 255, 300, 4352, 8192):
        assert sums_call(nlags=nl) == -1 and b"nlags" in err(), nl
    assert sums_call(nbytes=good + 16) == -1 and b"rows_bytes" in err()
    assert sums_call(n=[1000, 5, 70_016]) == -1 and b"rows_bytes" in err()           # other states than the rows were made for
    need = lib.txm_lag_sums_batched_ws_bytes(i64(ns), 3, C, items_of(its), 3, 256)
    assert sums_call(nws=need - 1) == -3 and b"workspace" in err()
    assert sums_call(nws=16) == -3
    # x = NULL with C = 0 is legal: the rows call gets as far as the size check
    assert rows_call(states=[st(x=None)], C=0, ldx=0, nbytes=8) == -1 and b"rows_bytes" in err()


def test_struct_mirrors_match_the_header():
    from thermoextrap_amd import _lib

    text = (ROOT / "include" / "txmom.h").read_text()

    def fields(name):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        return [(m.group(1).strip(), m.group(2)) for m in re.finditer(r"([\w \*]+?)\b(\w+);", body)]

    fs = fields("txm_lag_state")
    assert [f[1] for f in fs] == [f[0] for f in _lib.LagState._fields_] == ["x", "u", "center", "n"]
    assert all("*" in f[0] for f in fs[:3]) and fs[3][0] == "int64_t"
    assert ct.sizeof(_lib.LagState) == 32 and [getattr(_lib.LagState, f).offset for f in ("x", "u", "center", "n")] == [0, 8, 16, 24]
    fi = fields("txm_lag_item")
    assert fi == [("int32_t", "state"), ("int32_t", "pair")] and [f[0] for f in _lib.LagItem._fields_] == ["state", "pair"]
    assert ct.sizeof(_lib.LagItem) == 8 and _lib.LagItem.state.offset == 0 and _lib.LagItem.pair.offset == 4
    assert all(ct.sizeof(t) == 4 for _, t in _lib.LagItem._fields_)


def test_lag_item_slices(lib):
    from thermoextrap_amd import engine

    ns = [1_000_000, 5, 600_000, 1008]
    assert [engine.lag_chunks(n) for n in ns] == [chunks(n) for n in ns] == [497, 1, 298, 1]
    items = [(s, p) for s in range(4) for p in range(5)]

    def need(part, nlags):
        return lib.txm_lag_sums_batched_ws_bytes(i64(ns), len(ns), 2, items_of(part), len(part), nlags)

    for nlags in (256, 1024):
        assert engine.lag_sums_batched_ws_bytes(ns, items, nlags) == need(items, nlags)     # the restatement is the library's
        assert engine.lag_item_slices(ns, items, nlags, need(items, nlags)) == [slice(0, len(items))]
        budget = need(items, nlags) // 3
        cuts = engine.lag_item_slices(ns, items, nlags, budget)
        assert len(cuts) >= 3
        assert [c.start for c in cuts] == [0] + [c.stop for c in cuts[:-1]] and cuts[-1].stop == len(items)   # a partition, in order
        for c in cuts:
            part = items[c]
            assert len(part) >= 1 and (need(part, nlags) <= budget or len(part) == 1)
            if c.stop < len(items):                                   # greedy: the next item would not have fitted
                assert need(items[c.start:c.stop + 1], nlags) > budget
    # an item that alone exceeds the budget is still one slice
    cuts = engine.lag_item_slices(ns, [(1, 0), (0, 0), (0, 1), (3, 0)], 256, 1000)
    assert cuts == [slice(0, 1), slice(1, 2), slice(2, 3), slice(3, 4)]
    # the cap of 65535 items per call, whatever the budget
    many = [(1, 0)] * 140_000
    cuts = engine.lag_item_slices(ns, many, 256, 1 << 50)
    assert cuts == [slice(0, 65535), slice(65535, 131070), slice(131070, 140_000)]
    assert engine.lag_item_slices(ns, [], 256, 1 << 30) == []


def test_lazy_exports():
    import thermoextrap_amd as txa

    for name in ("statistical_inefficiencies_states", "decorrelate_states", "block_lengths"):
        assert getattr(txa, name) is getattr(txa.timeseries, name) and callable(getattr(txa, name)) and name in txa.__all__
    assert callable(txa.timeseries.scan_lag_sums_states)
