"""The MBAR entry points plan and refuse as they did: every size and plan query of the txm_mbar*.hip files answers, over a
grid that holds every boundary the host code branches on, exactly what the library of the parent commit of the entry-point
preamble refactor answered, and every call with a single fault is refused with the parent's status and the parent's text,
byte for byte (tests/golden/mbar_entry_parent.npz).  The engine sizes workspaces from these queries and three entry points
derive their launch plan from the bytes they are handed, so "equal" is integer equality.  Host-only: no query touches a
device (the CU count is 256 without one, as on an MI355X), and every call is refused before its first HIP call -- the
pointers are made-up values that are never dereferenced.

The fixture is recorded from a checkout of the commit to compare against, with this file copied into its tests/:

    python tests/test_mbar_entry_cpu.py --record        # builds that checkout's library, writes its tests/golden/...
"""

import ctypes as ct
import itertools
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
FIXTURE = ROOT / "tests" / "golden" / "mbar_entry_parent.npz"
SIZE_MAX = ct.c_size_t(-1).value

# the boundaries the host code branches on (0, 65 / 0, 9 / 33: refused)
KS = [0, 1, 8, 9, 15, 16, 17, 32, 33, 64, 65]
CS = [1, 15, 16, 17, 255, 256, 512, 513, 65535, 65536]
NAS = [0, 1, 2, 3, 4, 5, 8, 9]
NBINS = [1, 15, 16, 255, 1023, 1024]
NMAX = [1, 255, 256, 16383, 16384, 10**6, 10**8]
NREPS = [1, 5, 1000, 1 << 24, (1 << 24) + 1]
LEVELS = [1, 3, 32, 33]
BLOCKS = ["below", "equal", "above", "pieces"]      # block < n, == n, > n, and > 4096 records (summed in pieces)


def _load():
    sys.path.insert(0, str(ROOT))
    from thermoextrap_amd import _build, _lib

    _build.build_library()
    return _lib.load()


def _ws_ladder(plan_call, width):
    """A plan query at ws_bytes = 0, the smallest plan's bytes - 1, those bytes, twice those bytes and SIZE_MAX:
    (status, plan words) of each.  A refused shape leaves the words at -1 and is asked at 0 five times."""
    p = (ct.c_int64 * width)(*([-1] * width))
    plan_call(0, p)
    least = max(int(p[width - 1 if width == 4 else 5]), 0)
    rows = []
    for b in (0, max(least - 1, 0), least, 2 * least, SIZE_MAX):
        p = (ct.c_int64 * width)(*([-1] * width))
        rows.append([plan_call(b, p)] + list(p))
    return rows


def _block_tables(K, kind):
    n = np.asarray([100 + 37 * s for s in range(max(K, 1))], dtype=np.int64)
    if kind == "pieces":
        n = n + 10000
    blk = {"below": np.full_like(n, 7), "equal": n.copy(), "above": n + 5, "pieces": np.full_like(n, 5000)}[kind]
    return n, blk


def record_plans(lib):
    r = {}
    shapes = list(itertools.product(KS, CS, NAS))
    r["ws"] = np.asarray([lib.txm_mbar_ws_bytes(*s) for s in shapes], np.uint64)
    r["cov_ws"] = np.asarray([lib.txm_mbar_cov_ws_bytes(*s) for s in shapes], np.uint64)
    r["boot_ws"] = np.asarray([[[lib.txm_mbar_boot_ws_bytes(K, C, na, nt, nrep) for nrep in NREPS] for nt in NMAX + [1 << 36]]
                               for K, C, na in shapes], np.uint64)
    r["cross_plan"] = np.asarray(
        [_ws_ladder(lambda b, p: lib.txm_mbar_cross_cov_plan(K, C, na, x, nm, b, p), 4)
         for (K, C, na), x, nm in itertools.product(shapes, (0, 1), NMAX)], np.int64)
    r["hist_plan"] = np.asarray(
        [_ws_ladder(lambda b, p: lib.txm_mbar_hist_plan(K, nb, na, nm, b, p), 4)
         for K, nb, na, nm in itertools.product(KS, NBINS, NAS, NMAX)], np.int64)
    ip = ct.POINTER(ct.c_int64)
    rows = []
    for (K, C, na), nl, kind in itertools.product(shapes, LEVELS, BLOCKS):
        n, blk = _block_tables(K, kind)
        rows.append(_ws_ladder(lambda b, p: lib.txm_mbar_block_cov_plan(n.ctypes.data_as(ip), blk.ctypes.data_as(ip), K, C, na,
                                                                        nl, b, p), 7))
    r["block_plan"] = np.asarray(rows, np.int64)
    return r


# ---- refusals -----------------------------------------------------------------------------------------------------------
P = 0x30000            # a made-up device pointer: never dereferenced, the call is refused first
K0, C0, N0 = 3, 4, 100


def _doubles(bad=None, value=float("inf")):
    d = (ct.c_double * 65)()
    if bad is not None:
        d[bad] = value
    return d


def _states(_lib, K=K0, **fault):
    """K states of N0 samples and pitch C0; fault: {"u": s} / {"x": s} null that pointer, {"n": s} n = 0, {"ldx": s} C0 - 1."""
    tab = (_lib.MbarState * max(K, 1))()
    for s in range(max(K, 1)):
        tab[s].x, tab[s].u, tab[s].n, tab[s].ldx_s = 0x10000, 0x20000, N0, C0
    for what, s in fault.items():
        if what == "u":
            tab[s].u = None
        elif what == "x":
            tab[s].x = None
        elif what == "n":
            tab[s].n = 0
        elif what == "ldx":
            tab[s].ldx_s = C0 - 1
    return tab


def _samplers(_lib, K=K0, **fault):
    tab = (_lib.MbarBootState * max(K, 1))()
    for s in range(max(K, 1)):
        tab[s].spec = _lib.SamplerSpec(seed=7, nrep=5, ndat=N0, nsamp=0, rep0=0)
        tab[s].counts = 0x50000
    for what, s in fault.items():
        if what == "counts":
            tab[s].counts = None
        elif what == "ndat":
            tab[s].spec.ndat = N0 + 1
        elif what == "nsamp":
            tab[s].spec.nsamp = N0 - 1
        elif what == "nrep":
            tab[s].spec.nrep = 6 if s else 0
        elif what == "rep0":
            tab[s].spec.rep0 = -1
    return tab


def _entry_points(lib, _lib):
    """name -> (call(**overrides), the names of its pointer arguments, the bytes its good call needs)."""
    ip = ct.POINTER(ct.c_int64)
    n64 = np.full(K0, N0, dtype=np.int64)

    unset = object()

    def least(fn, width, at):
        p = (ct.c_int64 * width)()
        fn(0, p)
        return int(p[at])

    def ev(tab=None, K=K0, a0=unset, g=unset, upiv=0.0, out=P, logD=P, ws=P, ws_bytes=SIZE_MAX, **_):
        return lib.txm_mbar_eval(_states(_lib, K) if tab is None else tab, K, _doubles() if a0 is unset else a0,
                                 _doubles() if g is unset else g, upiv, out, logD, ws, ws_bytes, None)

    def pr(tab=None, K=K0, C=C0, upiv=0.0, logD=P, al=unset, na=2, out=P, ws=P, ws_bytes=SIZE_MAX, **_):
        return lib.txm_mbar_predict(_states(_lib, K) if tab is None else tab, K, C, upiv, logD, _doubles() if al is unset else al,
                                    na, out, ws, ws_bytes, None)

    def cv(tab=None, K=K0, C=C0, upiv=0.0, a0=unset, g=unset, logD=P, al=unset, na=2, mean=P, out=P, lnw=P, ws=P,
           ws_bytes=SIZE_MAX, **_):
        return lib.txm_mbar_cov(_states(_lib, K) if tab is None else tab, K, C, upiv, _doubles() if a0 is unset else a0,
                                _doubles() if g is unset else g, logD, _doubles() if al is unset else al, na, mean, out, lnw, ws,
                                ws_bytes, None)

    def xc(tab=None, K=K0, C=C0, upiv=0.0, logD=P, al=unset, na=2, mean=P, lnw=P, cross=0, out=P, ws=P, ws_bytes=SIZE_MAX, **_):
        return lib.txm_mbar_cross_cov(_states(_lib, K) if tab is None else tab, K, C, upiv, logD,
                                      _doubles() if al is unset else al, na, mean, lnw, cross, out, ws, ws_bytes, None)

    def hh(tab=None, K=K0, nbins=4, upiv=0.0, a0=unset, g=unset, logD=P, al=unset, na=2, out=P, lnw=P, ws=P, ws_bytes=SIZE_MAX,
           bins=unset, **_):
        bt = (ct.c_void_p * max(K, 1))(*([0x40000] * max(K, 1))) if bins is unset else bins
        return lib.txm_mbar_hist(_states(_lib, K) if tab is None else tab, bt, K, nbins, upiv, _doubles() if a0 is unset else a0,
                                 _doubles() if g is unset else g, logD, _doubles() if al is unset else al, na, out, lnw, ws,
                                 ws_bytes, None)

    def mk(tab=None, K=K0, C=C0, upiv=0.0, a0=unset, g=unset, logD=P, al=unset, na=2, mean=P, lnw=P, block=unset, levels=3,
           gamma=P, nblocks=P, ws=P, ws_bytes=SIZE_MAX, **_):
        blk = np.full(max(K, 1), 7, dtype=np.int64).ctypes.data_as(ip) if block is unset else block
        return lib.txm_mbar_block_cov(_states(_lib, K) if tab is None else tab, K, C, upiv, _doubles() if a0 is unset else a0,
                                      _doubles() if g is unset else g, logD, _doubles() if al is unset else al, na, mean, lnw, blk,
                                      levels, gamma, nblocks, ws, ws_bytes, None)

    def be(tab=None, samp=unset, K=K0, a0=unset, g=P, active=None, n_active=5, upiv=0.0, out=P, ws=P, ws_bytes=SIZE_MAX, **_):
        return lib.txm_mbar_boot_eval(_states(_lib, K) if tab is None else tab, _samplers(_lib, K) if samp is unset else samp, K,
                                      _doubles() if a0 is unset else a0, g, active, n_active, upiv, out, ws, ws_bytes, None)

    def bp(tab=None, samp=unset, K=K0, C=C0, upiv=0.0, a0=unset, g=P, gref=unset, al=unset, na=2, out=P, ws=P, ws_bytes=SIZE_MAX,
           **_):
        return lib.txm_mbar_boot_predict(_states(_lib, K) if tab is None else tab, _samplers(_lib, K) if samp is unset else samp,
                                         K, C, upiv, _doubles() if a0 is unset else a0, g, _doubles() if gref is unset else gref,
                                         _doubles() if al is unset else al, na, out, ws, ws_bytes, None)

    blk7 = np.full(K0, 7, dtype=np.int64)
    return {
        "mbar_eval": (ev, ["a0", "g", "out", "ws"], lib.txm_mbar_ws_bytes(K0, 1, 1)),
        "mbar_predict": (pr, ["logD", "al", "out", "ws"], lib.txm_mbar_ws_bytes(K0, C0, 2)),
        "mbar_cov": (cv, ["a0", "g", "logD", "al", "mean", "out", "ws"], lib.txm_mbar_cov_ws_bytes(K0, C0, 2)),
        "mbar_cross_cov": (xc, ["logD", "al", "mean", "lnw", "out", "ws"],
                           least(lambda b, p: lib.txm_mbar_cross_cov_plan(K0, C0, 2, 0, N0, b, p), 4, 3)),
        "mbar_hist": (hh, ["a0", "g", "logD", "al", "out", "ws", "bins"],
                      least(lambda b, p: lib.txm_mbar_hist_plan(K0, 4, 2, N0, b, p), 4, 3)),
        "mbar_block_cov": (mk, ["a0", "g", "logD", "al", "mean", "lnw", "block", "gamma", "nblocks", "ws"],
                           least(lambda b, p: lib.txm_mbar_block_cov_plan(n64.ctypes.data_as(ip), blk7.ctypes.data_as(ip), K0, C0,
                                                                          2, 3, b, p), 7, 5)),
        "mbar_boot_eval": (be, ["samp", "a0", "g", "out", "ws"], lib.txm_mbar_boot_ws_bytes(K0, 1, 1, K0 * N0, 5)),
        "mbar_boot_predict": (bp, ["samp", "a0", "g", "gref", "al", "out", "ws"],
                              lib.txm_mbar_boot_ws_bytes(K0, C0, 2, K0 * N0, 5)),
    }


def faults(lib, _lib):
    """(entry point, fault name, call): one call per single fault.  An argument an entry point does not take is ignored
    by its wrapper, and such a call is not listed."""
    out = []
    for name, (call, pointers, need) in _entry_points(lib, _lib).items():
        boot, takes_x = name.startswith("mbar_boot"), name in ("mbar_predict", "mbar_cov", "mbar_cross_cov", "mbar_block_cov",
                                                                "mbar_boot_predict")
        takes_g = name in ("mbar_eval", "mbar_cov", "mbar_hist", "mbar_block_cov")
        takes_a0 = takes_g or boot
        takes_al = name not in ("mbar_eval", "mbar_boot_eval")

        def add(fault, **kw):
            out.append((name, fault, lambda call=call, kw=kw: call(**kw)))

        add("null table", tab=ct.POINTER(_lib.MbarState)())
        add("K = 0", K=0)
        add("K = 65", K=65)
        if takes_x:
            add("C = 0", C=0)
            if name in ("mbar_cross_cov", "mbar_block_cov"):          # (the others take up to 65535 columns)
                add("C = 256", C=256, tab=_wide(_lib, 256))
            add("C = 65536", C=65536, tab=_wide(_lib, 65536))
        for s in range(K0):
            add(f"state {s} null u", tab=_states(_lib, u=s))
            add(f"state {s} n = 0", tab=_states(_lib, n=s))
            if takes_x:
                add(f"state {s} null x", tab=_states(_lib, x=s))
                add(f"state {s} ldx_s < C", tab=_states(_lib, ldx=s))
            if name == "mbar_hist":
                bt = (ct.c_void_p * K0)(*([0x40000] * K0))
                bt[s] = None
                add(f"state {s} null bins", bins=bt)
            if boot:
                for what in ("counts", "ndat", "nsamp", "nrep", "rep0"):
                    add(f"state {s} sampler {what}", samp=_samplers(_lib, **{what: s}))
        for arg in pointers:
            add(f"null {arg}", **{arg: None})
        if takes_al:
            add("n_alpha = 0", na=0)
            add("n_alpha = 9", na=9)
            if name != "mbar_predict":                                # (txm_mbar_predict does not look at the targets)
                add("target 1 inf", al=_doubles(1))
                add("target 0 nan", al=_doubles(0, float("nan")))
        if takes_a0:
            add("alpha0 1 inf", a0=_doubles(1))
            add("alpha0 2 nan", a0=_doubles(2, float("nan")))
        if takes_g:
            add("g 1 inf", g=_doubles(1))
        if name == "mbar_boot_predict":
            add("gref 1 inf", gref=_doubles(1))
        add("pivot inf", upiv=float("inf"))
        add("pivot nan", upiv=float("nan"))
        if name == "mbar_cross_cov":
            add("cross_alpha = 2", cross=2)
        if name == "mbar_hist":
            add("nbins = 0", nbins=0)
            add("nbins = 1024", nbins=1024)
        if name == "mbar_block_cov":
            add("n_levels = 0", levels=0)
            add("n_levels = 33", levels=33)
            zero = np.asarray([7, 0, 7], dtype=np.int64)
            out.append((name, "block 1 = 0", lambda call=call, zero=zero: call(block=zero.ctypes.data_as(ct.POINTER(ct.c_int64)))))
        if name == "mbar_boot_eval":
            add("n_active = 0", n_active=0)
            add("n_active = 6", n_active=6)
        add("workspace one byte short", ws_bytes=need - 1)
        add("workspace of 16 bytes", ws_bytes=16)
    return out


def _wide(_lib, C):
    tab = _states(_lib)
    for s in range(K0):
        tab[s].ldx_s = C
    return tab


def record_refusals(lib):
    from thermoextrap_amd import _lib

    names, status, text = [], [], []
    for name, fault, call in faults(lib, _lib):
        rc = call()
        names.append(f"{name}: {fault}")
        status.append(rc)
        text.append(_lib.last_error() if rc != 0 else "")
    return {"refusal_name": np.asarray(names), "refusal_status": np.asarray(status, np.int32), "refusal_text": np.asarray(text)}


def record(lib):
    return {**record_plans(lib), **record_refusals(lib)}


@pytest.fixture(scope="module")
def answers():
    return record(_load())


@pytest.fixture(scope="module")
def parent():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def test_the_grid_holds_the_boundaries():
    assert KS == [0, 1, 8, 9, 15, 16, 17, 32, 33, 64, 65] and CS == [1, 15, 16, 17, 255, 256, 512, 513, 65535, 65536]
    assert NAS == [0, 1, 2, 3, 4, 5, 8, 9] and NBINS[:5] == [1, 15, 16, 255, 1023] and LEVELS == [1, 3, 32, 33]
    assert NMAX == [1, 255, 256, 16383, 16384, 10**6, 10**8]
    for K in (1, 17):
        for kind, rel in (("below", -1), ("equal", 0), ("above", 1)):
            n, blk = _block_tables(K, kind)
            assert np.all(np.sign(blk - n) == rel)


def test_every_plan_query_answers_what_the_parent_answered(answers, parent):
    assert sorted(answers) == sorted(parent)
    for k in sorted(k for k in parent if not k.startswith("refusal_")):
        assert answers[k].dtype == parent[k].dtype and answers[k].shape == parent[k].shape, k
        bad = np.argwhere(answers[k] != parent[k])
        assert bad.size == 0, (k, len(bad), bad[:5].tolist(), answers[k][tuple(bad[0])], parent[k][tuple(bad[0])])


def test_every_refusal_is_the_parents_status_and_text(answers, parent):
    assert answers["refusal_name"].tolist() == parent["refusal_name"].tolist()
    for name, rc, text, prc, ptext in zip(parent["refusal_name"].tolist(), answers["refusal_status"].tolist(),
                                          answers["refusal_text"].tolist(), parent["refusal_status"].tolist(),
                                          parent["refusal_text"].tolist()):
        assert (rc, text) == (prc, ptext), name


def test_the_recorded_answers_are_refusals_and_the_calibration_points(parent):
    """No recorded call got past the host checks (none reaches a HIP call), every entry point has its faults, and plan
    values written down independently of the recording: the MBAR workspace head is 64 * 32 + 2 * 64 * 8 + 256 bytes and a
    cross-covariance record of one target pair is 256 doubles."""
    assert np.all(parent["refusal_status"] != 0) and np.all(parent["refusal_text"] != "")
    assert set(parent["refusal_status"].tolist()) == {-1, -3}
    per = {}
    for n in parent["refusal_name"].tolist():
        per[n.split(":")[0]] = per.get(n.split(":")[0], 0) + 1
    assert sorted(per) == ["mbar_block_cov", "mbar_boot_eval", "mbar_boot_predict", "mbar_cov", "mbar_cross_cov", "mbar_eval",
                           "mbar_hist", "mbar_predict"] and min(per.values()) >= 18
    head = 64 * 32 + 2 * 64 * 8 + 256
    cases = list(itertools.product(itertools.product(KS, CS, NAS), (0, 1), NMAX))
    i = cases.index(((1, 1, 1), 0, 1))
    assert parent["cross_plan"][i, 2].tolist() == [0, 1, 1, 1, head + 256 * 8]          # exactly the smallest plan's bytes
    assert parent["cross_plan"][i, 1].tolist() == [-3, 1, 1, 0, head + 256 * 8]         # one byte short: refused, the size
    shapes = list(itertools.product(KS, CS, NAS))
    assert parent["ws"][shapes.index((0, 1, 1))] == 0 and parent["cov_ws"][shapes.index((65, 1, 1))] == 0


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit("usage: python tests/test_mbar_entry_cpu.py --record")
    res = record(_load())
    np.savez_compressed(FIXTURE, **res)
    print(f"wrote {FIXTURE} ({FIXTURE.stat().st_size} bytes, {sum(v.size for v in res.values())} answers)")
