"""Every entry point of include/txmom.h against the workspace and output sizes it declares.

The contract ("Workspace contract"): a call handed EXACTLY what its ``*_bytes`` query returns succeeds, whatever
the workspace holds on entry; it writes nothing outside the workspace and its outputs, and it writes every output element;
one byte less is refused before anything is launched.  ``engine.workspace`` never hands out less than 1 MiB and reuses
the buffer the previous call just filled, so neither a query that under-reports nor a partial-sum slot that nobody wrote
can show through the engine: here the calls go through ctypes with guard-banded buffers (tests/_bands.py).

``CONTRACTS`` has one row per size query of the header (tests/test_workspace_table_cpu.py checks that).  A row names
the query, the calls it sizes and a list of cases; per case:

  (a) workspace of exactly the queried size filled with NaN patterns, every output (and caller-owned side buffer) of exactly
      its size painted NaN / -1: status 0, every band intact, no output element still painted, every float finite;
  (b) the same call with a zeroed workspace gives ``array_equal`` outputs, and where ``engine`` wraps the call the engine's
      result for the same operands is ``array_equal`` too (the engine is held to the long-double references elsewhere);
  (c) the query minus one byte returns TXM_ERR_WORKSPACE, outputs keep their paint, the workspace keeps its fill, bands
      intact.  Two documented exceptions: a bootstrap call whose query includes the count table runs the kernel that
      draws in place when handed less than that (include/txmom.h, txm_resample_vals_ws_bytes_opts) -- there one byte less
      must give status 0, the fused kernel and the SAME bits, and one byte below the table-free query is refused; the
      rows buffer of txm_lag_rows_batched is checked with ``==``: both -1 and +1 are TXM_ERR_INVALID.

Every assertion is exact: equality, finiteness, a status code or an untouched byte pattern.
"""

from __future__ import annotations

import ctypes as ct
from collections import Counter
from typing import Callable, NamedTuple

import numpy as np
import pytest
import torch

from _bands import NAN_BITS, Banded

F64, I64, I32, U8 = torch.float64, torch.int64, torch.int32, torch.uint8
ERR_INVALID, ERR_WORKSPACE = -1, -3
PATH_AUTO, PATH_FP64, PATH_INT8, PATH_FUSED, PATH_TABLE, WITH_Y = -1, 0, 1, 2, 3, 0x100
PASSED: Counter = Counter()


def P(t):
    return ct.c_void_p(t.data_ptr()) if t is not None else None


def dp(a):
    return a.ctypes.data_as(ct.POINTER(ct.c_double))


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda")


def cdiv(a, b):
    return -(-a // b)


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


class Ctx:
    """The buffers of ONE run of a case: the target call's workspace (``short`` bytes below the query in run (c)), the
    workspaces of preparatory calls, outputs and caller-owned side buffers -- all guard-banded, all of exactly their size."""

    def __init__(self, fill: str, short: int = 0, target: str = "ws", ws_bytes: int | None = None):
        self.fill, self.short, self.target, self.ws_bytes = fill, short, target, ws_bytes
        self.bufs: dict[str, tuple] = {}
        self.compared: set[str] = set()

    def _add(self, name, b, kind, shape=None, mask=None, init=None):
        assert name not in self.bufs, name
        self.bufs[name] = (b, kind, shape, mask, init)
        return ct.c_void_p(b.ptr)

    def ws(self, nbytes: int):
        """The target call's workspace: (pointer, ws_bytes)."""
        assert nbytes > 0
        if self.ws_bytes is not None:
            nbytes = self.ws_bytes
        elif self.target == "ws":
            nbytes -= self.short
        b = Banded(nbytes, self.fill, dtype=U8)
        return self._add("ws", b, "ws"), nbytes

    def scratch(self, name: str, nbytes: int):
        """The workspace of a preparatory call: exact, never short."""
        assert nbytes > 0
        return self._add(name, Banded(nbytes, self.fill, dtype=U8), "scratch"), nbytes

    def side(self, name: str, nbytes: int, by_target: bool = True, delta: int = 0, compare: bool = False):
        """A caller-owned block with a layout of the library's own (pre-pass block, rows buffer): NaN patterns, exact size.
        ``compare``: its bytes are a result like an output's (the padding inside keeps the NaN pattern in every run)."""
        assert nbytes > 0
        if self.target == name:
            nbytes -= self.short
        nbytes += delta
        ptr = self._add(name, Banded(nbytes, "nan", dtype=U8), "side" if by_target else "aux_side")
        if compare:
            self.compared.add(name)
        return ptr, nbytes

    def out(self, name: str, shape, dtype=F64, mask=None, aux: bool = False, init=None):
        """An output of exactly ``shape`` painted NaN / -1.  ``mask`` (bool array): the elements the call must write, the
        others must keep their paint.  ``init``: an in/out operand, preloaded instead of painted.  ``aux``: written by a
        preparatory call, not by the target."""
        n = int(np.prod(shape))
        b = Banded(n * torch.empty((), dtype=dtype).element_size(), "value", dtype=dtype)
        if init is not None:
            b.view().copy_(init.reshape(-1))
        return self._add(name, b, "aux" if aux else "inout" if init is not None else "out", tuple(shape), mask, init)

    def verify_ok(self):
        torch.cuda.synchronize()
        for name, (b, kind, shape, mask, _) in self.bufs.items():
            assert b.check(), f"{name}: a band was written"
            if kind in ("out", "aux"):
                if mask is None:
                    assert b.unwritten() == 0, f"{name}: {b.unwritten()} of {b.view().numel()} elements left unwritten"
                else:
                    assert np.array_equal(b.painted().cpu().numpy(), ~np.asarray(mask).reshape(-1)), f"{name}: written set differs"
            if kind in ("out", "aux", "inout") and b.dtype.is_floating_point:
                v = b.view().cpu().numpy()
                if mask is not None:
                    v = v[np.asarray(mask).reshape(-1)]
                assert np.all(np.isfinite(v)), f"{name}: non-finite output"

    def results(self):
        res = {name: b.view().cpu().numpy().reshape(shape) for name, (b, kind, shape, _, _) in self.bufs.items()
               if kind in ("out", "aux", "inout")}
        res.update({name: self.bufs[name][0].payload.cpu().numpy() for name in self.compared})
        return res

    def verify_refused(self):
        torch.cuda.synchronize()
        for name, (b, kind, shape, _, init) in self.bufs.items():
            assert b.check(), f"{name}: a band was written by a refused call"
            if kind == "out":
                assert b.unwritten() == b.view().numel(), f"{name}: written by a refused call"
            elif kind == "inout":
                assert torch.equal(b.view(), init.reshape(-1)), f"{name}: changed by a refused call"
            elif kind in ("ws", "side"):
                assert b.holds_fill(), f"{name}: written by a refused call"


class Row(NamedTuple):
    query: str                       # the size query of include/txmom.h
    calls: tuple                     # the entry points it sizes
    cases: list                      # dicts with an "id"
    size: Callable                   # (L, case) -> bytes; host logic, runs without a GPU
    make: Callable                   # (L, eng, case) -> operands (device tensors, host arrays)
    run: Callable                    # (L, case, operands, ctx) -> status of the target call
    engine: Callable | None = None   # (eng, case, operands) -> {output name: tensor} through the engine wrapper
    path: Callable | None = None     # (L, case, operands, results of (a)) -> asserts the case takes the path it is named for
    short: str = "standard"          # "standard" / "none" (no ws_bytes argument) / "exact" (rows_bytes) / per case "table"


def lib():
    from thermoextrap_amd import _lib

    return _lib.load()


# ---- operands ---------------------------------------------------------------------------------------------------------
def xuw(N, C, weighted, seed, colmajor=False, pitch=None):
    """x (N, C) as a device view (tight, column-major, or the first C columns of rows of ``pitch`` doubles with NaN
    behind them), u, w (or None)."""
    r = np.random.default_rng(seed)
    x = r.normal(size=(N, C)) + 0.3
    u = r.normal(size=N)
    if colmajor:
        xd = dev(x.T.copy()).t()
    elif pitch is not None and pitch != C:
        wide = torch.full((N, pitch), float("nan"), dtype=F64, device="cuda")
        wide[:, :C] = dev(x)
        xd = wide[:, :C]
    else:
        xd = dev(x)
    return xd, dev(u), (dev(r.uniform(0.5, 1.5, N)) if weighted else None)


def ld(xd):
    """(ldx_s, ldx_c) of a 2-D device view."""
    N, C = xd.shape
    s0, s1 = xd.stride()
    if s1 == 1 or C == 1 and s0 != 1:
        return (s0 if N > 1 else max(C, 1)), 1
    return 1, s1


# ---- reductions -------------------------------------------------------------------------------------------------------
def reduce_cases():
    out = []
    for i, C in enumerate((1, 17, 33, 514)):
        for weighted in (False, True):
            for col in (False, True):
                call = "txm_reduce_vals" if (i + weighted + col) % 2 == 0 else "txm_reduce_vals_sums"
                out.append(dict(id=f"C{C}_{'w' if weighted else 'u'}_{'col' if col else 'row'}_N100_{call[4:]}", N=100, C=C,
                                order=3, weighted=weighted, col=col, call=call, capped=False))
                # the pivot estimate takes no workspace: its [1 + C] output in bands, no refusal to provoke
                call = "txm_reduce_vals_pivot_w" if weighted else "txm_reduce_vals_pivot"
                out.append(dict(id=f"C{C}_{'w' if weighted else 'u'}_{'col' if col else 'row'}_N100_{call[4:]}", N=100, C=C,
                                order=3, weighted=weighted, col=col, call=call, capped=False, short="none"))
    # pivot_w without weights is the unweighted estimate; more rows than the 1024 the estimate samples
    out.append(dict(id="C33_u_row_N5000_reduce_vals_pivot_w_null", N=5000, C=33, order=3, weighted=False, col=False,
                    call="txm_reduce_vals_pivot_w", capped=False, short="none"))
    out.append(dict(id="C17_w_col_N5000_reduce_vals_pivot_w", N=5000, C=17, order=3, weighted=True, col=True,
                    call="txm_reduce_vals_pivot_w", capped=False, short="none"))
    # the grid cap binds: more than 8 workgroups per CU of rows (txm_reduce.hip grid_x_for)
    out.append(dict(id="C33_w_row_grid_cap", N=70_001, C=33, order=8, weighted=True, col=False, call="txm_reduce_vals", capped=True))
    out.append(dict(id="C3_u_col_grid_cap", N=4_200_000, C=3, order=1, weighted=False, col=True, call="txm_reduce_vals", capped=True))
    return out


def reduce_make(L, eng, c):
    x, u, w = xuw(c["N"], c["C"], c["weighted"], 11 + c["C"], colmajor=c["col"])
    return dict(x=x, u=u, w=w, ld=ld(x), pivot=eng.reduce_pivot(x, u, w))


def reduce_run(L, c, o, ctx):
    N, C, order = c["N"], c["C"], c["order"]
    if c["call"] == "txm_reduce_vals_pivot":
        return L.txm_reduce_vals_pivot(P(o["x"]), *o["ld"], P(o["u"]), N, C, ctx.out("pivot", (1 + C,)), None)
    if c["call"] == "txm_reduce_vals_pivot_w":
        return L.txm_reduce_vals_pivot_w(P(o["x"]), *o["ld"], P(o["u"]), P(o["w"]), N, C, ctx.out("pivot", (1 + C,)), None)
    out = ctx.out("out", (C, 2, order + 1))
    ws, nb = ctx.ws(L.txm_reduce_vals_ws_bytes(N, C, order))
    if c["call"] == "txm_reduce_vals":
        return L.txm_reduce_vals(P(o["x"]), *o["ld"], P(o["u"]), P(o["w"]), N, C, order, out, ws, nb, None)
    return L.txm_reduce_vals_sums(P(o["x"]), *o["ld"], P(o["u"]), P(o["w"]), N, C, order, P(o["pivot"]), out, ws, nb, None)


def reduce_engine(eng, c, o):
    if "pivot" in c["call"]:
        return {"pivot": o["pivot"]}          # engine.reduce_pivot of the same operands (reduce_make)
    if c["call"] == "txm_reduce_vals":
        return {"out": eng.reduce_vals(o["x"], o["u"], c["order"], o["w"])}
    return {"out": eng.reduce_sums(o["x"], o["u"], c["order"], o["pivot"], o["w"])}


def reduce_path(L, c, o, res):
    """txm_reduce.hip: a row-major launch has 256 >> l2 rows per workgroup (l2 = log2 of the lanes a row takes), a
    column-major one 512; the grid wants ceil(rows / (4 rows per workgroup)) workgroups and is capped at 8 per CU."""
    N, C, col = c["N"], c.get("C", 1), c.get("col", "R" in c)      # (the 1-D reduction runs the column-major kernel)
    if "ld" in o:
        assert o["ld"] == ((1, N) if col else (C, 1))
    if col:
        rows_per = 512
    else:
        vec = 2 if C % 2 == 0 else 1
        l2 = 0
        while (1 << l2) < cdiv(C, vec) and l2 < 8:
            l2 += 1
        rows_per = 256 >> l2
    assert (cdiv(N, rows_per * 4) > 8 * cus()) == c.get("capped", N >= 70_001)


def push_cases():
    return [dict(id=f"C{C}_{'w' if w else 'u'}_{'col' if col else 'row'}", N=N, C=C, order=order, weighted=w, col=col)
            for N, C, order, w, col in ((100, 1, 3, False, False), (100, 33, 4, True, True), (70_001, 17, 2, True, False),
                                        (300, 514, 1, False, False))]


def push_make(L, eng, c):
    x0, u0, w0 = xuw(57, c["C"], c["weighted"], 5, colmajor=c["col"])
    x, u, w = xuw(c["N"], c["C"], c["weighted"], 6, colmajor=c["col"])
    return dict(x=x, u=u, w=w, ld=ld(x), state=eng.reduce_vals(x0, u0, c["order"], w0).contiguous())


def push_run(L, c, o, ctx):
    N, C, order = c["N"], c["C"], c["order"]
    st = ctx.out("state", (C, 2, order + 1), init=o["state"])
    ws, nb = ctx.ws(L.txm_push_vals_ws_bytes(N, C, order))
    return L.txm_push_vals(st, P(o["x"]), *o["ld"], P(o["u"]), P(o["w"]), N, C, order, ws, nb, None)


def r1d_make(L, eng, c):
    r = np.random.default_rng(21)
    return dict(u=dev(r.normal(size=(c["R"], c["N"]))), w=dev(r.uniform(0.5, 1.5, c["N"])) if c["weighted"] else None)


def r1d_run(L, c, o, ctx):
    N, R, M = c["N"], c["R"], c["M"]
    out = ctx.out("out", (R, M))
    ws, nb = ctx.ws(L.txm_reduce_vals_1d_ws_bytes(N, R, M))
    return L.txm_reduce_vals_1d(P(o["u"]), N, 1, P(o["w"]), N, R, M, out, ws, nb, None)


def rbatch_make(L, eng, c):
    ops = [xuw(c["N"], c["C"], c["weighted"], 30 + s) for s in range(c["S"])]
    tab, keep, S, N, C = eng._state_table([t[0] for t in ops], [t[1] for t in ops], [t[2] for t in ops] if c["weighted"] else None)
    return dict(ops=ops, tab=tab, keep=keep)


def rbatch_run(L, c, o, ctx):
    S, N, C, order = c["S"], c["N"], c["C"], c["order"]
    out = ctx.out("out", (S, C, 2, order + 1))
    ws, nb = ctx.ws(L.txm_reduce_vals_batched_ws_bytes(S, N, C, order))
    return L.txm_reduce_vals_batched(o["tab"], S, C, N, C, order, out, ws, nb, None)


def rbatch_engine(eng, c, o):
    ops = o["ops"]
    return {"out": eng.reduce_vals_batched([t[0] for t in ops], [t[1] for t in ops], c["order"],
                                           ws=[t[2] for t in ops] if c["weighted"] else None)}


# ---- sampler ----------------------------------------------------------------------------------------------------------
def spec_of(c, seed=777):
    from thermoextrap_amd._lib import SamplerSpec

    return SamplerSpec(seed=seed, nrep=c["nrep"], ndat=c["ndat"], nsamp=c.get("nsamp", 0), rep0=c.get("rep0", 0))


def i2f_make(L, eng, c):
    r = np.random.default_rng(3)
    return dict(idx=dev(r.integers(0, c["ndat"], size=(c["nrep"], c["nsamp"]), dtype=np.int64)))


def i2f_run(L, c, o, ctx):
    freq = ctx.out("freq", (c["nrep"], c["ndat"]), dtype=I64)
    ws, nb = ctx.ws(L.txm_indices_to_freq_ws_bytes())
    return L.txm_indices_to_freq(P(o["idx"]), c["nrep"], c["nsamp"], c["ndat"], freq, ws, nb, None)


def sampler_cases():
    return [dict(id=f"ndat{ndat}_nrep{nrep}_nsamp{nsamp}_rep0{rep0}", ndat=ndat, nrep=nrep, nsamp=nsamp, rep0=rep0)
            for ndat, nrep, nsamp, rep0 in ((1, 3, 0, 0), (1023, 3, 700, 5), (1025, 1024, 0, 0), (4097, 3, 5000, 1000),
                                            (4097, 1024, 0, 7), (1025, 3, 1025, 0))]


def counts_run(L, c, o, ctx):
    """txm_sampler_tile_counts (the launch is 1024 lanes wide below 1024 replicates, 256 from there), then the per-sample
    counts txm_sampler_freq regenerates from them."""
    spec = spec_of(c)
    nt = L.txm_sampler_ntiles(c["ndat"])
    counts = ctx.out("counts", (c["nrep"], nt), dtype=I32)
    ws, nb = ctx.ws(L.txm_sampler_counts_ws_bytes(ct.byref(spec)))
    rc = L.txm_sampler_tile_counts(ct.byref(spec), counts, ws, nb, None)
    if rc != 0:
        return rc
    freq = ctx.out("freq", (c["nrep"], c["ndat"]), dtype=I64)
    return L.txm_sampler_freq(ct.byref(spec), counts, freq, None)


def counts_engine(eng, c, o):
    sm = eng.DeviceSampler(777, c["nrep"], c["ndat"], nsamp=c["nsamp"], rep0=c["rep0"])
    return {"counts": sm.counts, "freq": sm.freq()}


def counts_path(L, c, o, res):
    nsamp = c["nsamp"] or c["ndat"]
    assert np.all(res["freq"].sum(axis=1) == nsamp) and res["freq"].min() >= 0
    assert np.all(res["counts"].astype(np.int64).sum(axis=1) == nsamp)


def table_make(L, eng, c):
    return dict(sm=eng.DeviceSampler(777, c["nrep"], c["ndat"], rep0=c["rep0"]))


def table_run(L, c, o, ctx):
    spec = o["sm"].spec
    nbytes = L.txm_sampler_count_table_bytes(c["ndat"], c["nreps"])
    assert nbytes == cdiv(c["nreps"], 128) * cdiv(c["ndat"], 1024) * 131072
    table = ctx.out("table", (nbytes,), dtype=U8)
    return L.txm_sampler_count_table(ct.byref(spec), P(o["sm"].counts), c["begin"], c["nreps"], table, None)


def table_path(L, c, o, res):
    """Every replicate of the slab holds its nsamp draws: the table's sum is the slab's draw count (padded replicates and
    the samples a slid last tile shares with its predecessor are written as zeros)."""
    real = min(c["nreps"], c["nrep"] - c["begin"])
    assert int(res["table"].astype(np.int64).sum()) == real * c["ndat"]


# ---- bootstrap --------------------------------------------------------------------------------------------------------
def rs_case(id, N, C, nrep, order, path, *, w=False, pitch=None, y=False, prep=False, freq=False, pivot=False, guard=False,
            kernel="path"):
    """``kernel``: the contraction kernel the case is named for ("path": the forced path itself; None: either int8 kernel,
    the library's choice under TXM_PATH_INT8)."""
    return dict(id=id, N=N, C=C, nrep=nrep, order=order, path=path, weighted=w, pitch=pitch, y=y, prep=prep, freq=freq,
                pivot=pivot, guard=guard, kernel=path if kernel == "path" else kernel)


RS_AUTO = [
    rs_case("fp64_N300_C3_nrep7_o0", 300, 3, 7, 0, PATH_AUTO, kernel=PATH_FP64),
    rs_case("fp64_N300_C16_nrep65_o1_w", 300, 16, 65, 1, PATH_AUTO, w=True, kernel=PATH_FP64),
    rs_case("fp64_N5000_C17_nrep130_o4", 5000, 17, 130, 4, PATH_AUTO, kernel=PATH_FP64),
    rs_case("fp64_N12325_C33_nrep65_o6_w_pivot", 12288 + 37, 33, 65, 6, PATH_AUTO, w=True, pivot=True, kernel=PATH_FP64),
    rs_case("fp64_freq_N5000_C3_nrep7_o4_w", 5000, 3, 7, 4, PATH_AUTO, w=True, freq=True, kernel=PATH_FP64),
]
RS_OPTS = [
    rs_case("fp64_N300_C3_nrep7_o1", 300, 3, 7, 1, PATH_FP64),
    rs_case("fp64_N5000_C17_nrep65_o8_w", 5000, 17, 65, 8, PATH_FP64, w=True),
    rs_case("fp64_N12325_C33_nrep130_o4", 12288 + 37, 33, 130, 4, PATH_FP64),
    rs_case("fp64_N5000_C16_nrep7_o0_pitch19", 5000, 16, 7, 0, PATH_FP64, pitch=19),
    rs_case("int8_N5000_C16_nrep65_o1", 5000, 16, 65, 1, PATH_INT8, kernel=None),
    rs_case("int8_N12325_C4_nrep130_o4_w", 12288 + 37, 4, 130, 4, PATH_INT8, w=True, kernel=None),
    rs_case("fused_N5000_C3_nrep7_o1", 5000, 3, 7, 1, PATH_FUSED),
    rs_case("fused_N12325_C33_nrep65_o6_w", 12288 + 37, 33, 65, 6, PATH_FUSED, w=True),
    rs_case("fused_N5000_C17_nrep130_o4", 5000, 17, 130, 4, PATH_FUSED),
    rs_case("fused_N5000_C33_nrep130_o0", 5000, 33, 130, 0, PATH_FUSED),
    rs_case("table_N5000_C16_nrep130_o1", 5000, 16, 130, 1, PATH_TABLE),
    rs_case("table_N12325_C33_nrep130_o4_w_pitch36", 12288 + 37, 33, 130, 4, PATH_TABLE, w=True, pitch=36),
    rs_case("table_N5000_C17_nrep65_o6_pitch20", 5000, 17, 65, 6, PATH_TABLE, pitch=20),
    rs_case("table_N5000_C33_nrep7_o0_pitch36", 5000, 33, 7, 0, PATH_TABLE, pitch=36),
    rs_case("guard_int8_N5000_C4_nrep65_o2", 5000, 4, 65, 2, PATH_INT8, guard=True, kernel=None),
    rs_case("guard_table_N12325_C33_nrep130_o1_pitch36", 12288 + 37, 33, 130, 1, PATH_TABLE, pitch=36, guard=True),
]
RS_Y = [
    rs_case("fp64_y_N300_C3_nrep7_o1", 300, 3, 7, 1, PATH_FP64, y=True),
    rs_case("fp64_y_N5000_C17_nrep65_o2_w", 5000, 17, 65, 2, PATH_FP64, w=True, y=True),
    rs_case("fused_y_N5000_C3_nrep65_o1", 5000, 3, 65, 1, PATH_FUSED, y=True),
    rs_case("fused_y_N12325_C33_nrep130_o4_w", 12288 + 37, 33, 130, 4, PATH_FUSED, w=True, y=True),
    rs_case("table_y_N5000_C33_nrep130_o1_pitch36", 5000, 33, 130, 1, PATH_TABLE, pitch=36, y=True),
]
RS_PREP = [
    rs_case("prep_fused_N5000_C3_nrep65_o1", 5000, 3, 65, 1, PATH_FUSED, prep=True),
    rs_case("prep_fused_N12325_C33_nrep130_o4_w", 12288 + 37, 33, 130, 4, PATH_FUSED, w=True, prep=True),
    rs_case("prep_table_N5000_C17_nrep130_o6_pitch20", 5000, 17, 130, 6, PATH_TABLE, pitch=20, prep=True),
    rs_case("prep_guard_int8_N5000_C4_nrep65_o2", 5000, 4, 65, 2, PATH_INT8, prep=True, guard=True, kernel=None),
]


def rs_aligned(c):
    """txm_resample_kernel's `aligned` for the case's operands: torch allocations are 256-byte aligned, so only the row
    pitch decides (even, at least C rounded up to 4)."""
    ldx = c["pitch"] or c["C"]
    return int(ldx % 2 == 0 and ldx >= cdiv(c["C"], 4) * 4)


def rs_kernel(L, c, path=None):
    return L.txm_resample_kernel(c["N"], c["C"], c["nrep"], c["order"], c["path"] if path is None else path, int(c["y"]),
                                 rs_aligned(c))


def rs_rides(L, c, path=None):
    """The call's kernel carries the second matrix as a row set of its own (no separate order-0 pass, no extra workspace)."""
    return bool(not c["freq"] and rs_kernel(L, c, path) & WITH_Y)


def rs_need(L, c, path=None):
    """What the call is handed: the query for its own path / has_y, plus the second matrix's extra workspace unless the
    call's kernel carries y."""
    n = L.txm_resample_vals_ws_bytes_opts(c["N"], c["C"], c["nrep"], c["order"], c["path"] if path is None else path, int(c["y"]))
    if path is None and c["path"] == PATH_AUTO and not c["y"]:
        assert n == L.txm_resample_vals_ws_bytes(c["N"], c["C"], c["nrep"], c["order"])
    return n + (L.txm_resample_y_ws_bytes(c["N"], c["C"], c["nrep"]) if c["y"] and not rs_rides(L, c, path) else 0)


def rs_floor(L, c):
    """What the call needs when it cannot have the count table: the table-free query, plus the second matrix's extra
    workspace unless the kernel it then runs (the one for operands the table kernel cannot take) carries y."""
    N, C, nrep, order = c["N"], c["C"], c["nrep"], c["order"]
    n = L.txm_resample_vals_ws_bytes_opts(N, C, nrep, order, PATH_FUSED, int(c["y"]))
    if c["y"] and (c["freq"] or not L.txm_resample_kernel(N, C, nrep, order, c["path"], 1, 0) & WITH_Y):
        n += L.txm_resample_y_ws_bytes(N, C, nrep)
    return n


def rs_make(L, eng, c):
    N, C, nrep = c["N"], c["C"], c["nrep"]
    x, u, w = xuw(N, C, c["weighted"], 40 + C + c["order"], pitch=c["pitch"])
    o = dict(x=x, u=u, w=w, y=None, freq=None, sm=None, pivot=None)
    if c["guard"]:      # one sample at +-1e150: the precision guard flags its window, the FP64 fallback blocks get written
        x[N // 3, 0] = 1e150
        x[2 * N // 3, C - 1] = -1e150
        o["pivot"] = dev(np.concatenate([[0.0], np.full(C, 0.3)]))    # (a pivot the outliers have no part in)
    if c["y"]:
        o["y"] = xuw(N, C, False, 90 + C, pitch=c["pitch"])[0]
    if c["freq"]:
        o["freq"] = dev(np.random.default_rng(8).multinomial(N, np.full(N, 1.0 / N), size=nrep).astype(np.int64))
    else:
        o["sm"] = eng.DeviceSampler(4321, nrep, N, rep0=3)
    if c["pivot"]:
        o["pivot"] = eng.reduce_pivot(x, u, w)
    return o


def rs_run(L, c, o, ctx):
    from thermoextrap_amd._lib import ResampleOpts

    N, C, nrep, order = c["N"], c["C"], c["nrep"], c["order"]
    out = ctx.out("out", (nrep, C, 2, order + 1))
    opts = ResampleOpts()
    opts.path = c["path"]
    opts.info = ctx.out("info", (4,), dtype=I64).value
    if c["y"]:
        opts.y, opts.ldy_s = o["y"].data_ptr(), o["y"].stride(0)
        opts.out_y = ctx.out("out_y", (nrep, C)).value
    if c["prep"]:
        pp, pn = ctx.side("prep", L.txm_resample_prep_bytes(N, C, nrep, order))
        opts.prep, opts.prep_bytes, opts.prep_valid = pp.value, pn, 0
    ws, nb = ctx.ws(rs_need(L, c))
    spec, counts = (None, None) if c["freq"] else (ct.byref(o["sm"].spec), P(o["sm"].counts))
    return L.txm_resample_vals(P(o["x"]), o["x"].stride(0), 1, P(o["u"]), P(o["w"]), N, C, order, nrep, P(o["freq"]), spec, counts,
                               P(o["pivot"]), out, None if (c["path"] == PATH_AUTO and not c["y"] and not c["prep"]) else ct.byref(opts),
                               ws, nb, None)


def rs_run_auto(L, c, o, ctx):
    """A call without options (opts_host NULL): no info words."""
    N, C, nrep, order = c["N"], c["C"], c["nrep"], c["order"]
    out = ctx.out("out", (nrep, C, 2, order + 1))
    ws, nb = ctx.ws(rs_need(L, c))
    spec, counts = (None, None) if c["freq"] else (ct.byref(o["sm"].spec), P(o["sm"].counts))
    return L.txm_resample_vals(P(o["x"]), o["x"].stride(0), 1, P(o["u"]), P(o["w"]), N, C, order, nrep, P(o["freq"]), spec, counts,
                               P(o["pivot"]), out, None, ws, nb, None)


_RS_NAMES = {PATH_AUTO: None, PATH_FP64: "fp64", PATH_INT8: "int8", PATH_FUSED: "int8_fused", PATH_TABLE: "int8_table"}


def rs_engine(eng, c, o):
    r = eng.resample_vals(o["x"], o["u"], c["order"], freq=o["freq"], sampler=o["sm"], w=o["w"], pivot=o["pivot"],
                          path=_RS_NAMES[c["path"]], y=o["y"])
    return {"out": r[0], "out_y": r[1]} if c["y"] else {"out": r}


def rs_path(L, c, o, res):
    """The kernel word the library reports for the shape, and the info words the call wrote: [0] path (1 = int8), [2]
    windows the guard sent to the FP64 kernel, [3] bit 1 the count-table kernel ran."""
    kern = PATH_FP64 if c["freq"] else rs_kernel(L, c) & 0xFF
    if c["kernel"] is not None:
        assert kern == c["kernel"], (kern, c["kernel"])
    else:
        assert kern in (PATH_FUSED, PATH_TABLE)
    assert c["N"] >= 1024 or kern == PATH_FP64
    if "info" in res:
        info = res["info"]
        assert info[0] == (0 if kern == PATH_FP64 else 1) and bool(info[3] & 2) == (kern == PATH_TABLE), info
        # the guard is data dependent (at orders >= 4 it flags a window or two of plain normal samples as well): the cases
        # named for it must take the fallback, the FP64 kernel never does, the others are free to
        assert info[2] > 0 or not c["guard"], info
        assert info[2] == 0 or kern != PATH_FP64, info
        if not c["guard"] and c["order"] <= 2:      # ... and up to order 2 they do not: the fallback blocks stay untouched
            assert info[2] == 0, info


def rs_table_short(L, c, o, row, res_a):
    """A call whose query includes the count table: one byte less runs the kernel that draws in place -- status 0, the SAME
    bits; one byte below the table-free query is refused."""
    need = rs_need(L, c)
    floor = rs_floor(L, c)
    assert floor < need
    ctx = Ctx("nan", ws_bytes=need - 1)
    assert row.run(L, c, o, ctx) == 0
    ctx.verify_ok()
    res = ctx.results()
    assert "info" not in res or not res["info"][3] & 2
    for name in ("out", "out_y"):
        assert name not in res_a or np.array_equal(res[name], res_a[name]), name
    ctx = Ctx("nan", ws_bytes=floor - 1)
    assert row.run(L, c, o, ctx) == ERR_WORKSPACE
    ctx.verify_refused()


def rsb_case(id, S, N, C, nrep, order, path, *, w=False, prep=False, freq=False, guard=False):
    return dict(id=id, S=S, N=N, C=C, nrep=nrep, order=order, path=path, weighted=w, prep=prep, freq=freq, guard=guard)


RSB = [
    rsb_case("fp64_S2_N300_C4_nrep7_o1", 2, 300, 4, 7, 1, PATH_AUTO),
    rsb_case("fp64_S5_N5000_C20_nrep65_o2_w", 5, 5000, 20, 65, 2, PATH_FP64, w=True),
    rsb_case("fp64_freq_S2_N1500_C4_nrep7_o3", 2, 1500, 4, 7, 3, PATH_AUTO, freq=True),
    rsb_case("int8_S2_N5000_C4_nrep65_o2", 2, 5000, 4, 65, 2, PATH_INT8),
    rsb_case("int8_S5_N12325_C4_nrep130_o4_w_guard", 5, 12288 + 37, 4, 130, 4, PATH_INT8, w=True, guard=True),
]
RSB_PREP = [
    rsb_case("prep_int8_S2_N5000_C4_nrep65_o2", 2, 5000, 4, 65, 2, PATH_INT8, prep=True),
    rsb_case("prep_int8_S5_N12325_C16_nrep130_o1_guard", 5, 12288 + 37, 16, 130, 1, PATH_INT8, prep=True, guard=True),
]


def rsb_make(L, eng, c):
    S, N, C, nrep = c["S"], c["N"], c["C"], c["nrep"]
    ops = [xuw(N, C, c["weighted"], 60 + s) for s in range(S)]
    if c["guard"]:      # one state with a guard-flagged window
        ops[1][0][N // 2, 1] = 1e150
    tab, keep, _, _, _ = eng._state_table([t[0] for t in ops], [t[1] for t in ops], [t[2] for t in ops] if c["weighted"] else None)
    o = dict(ops=ops, tab=tab, keep=keep, freq=None, sm=None)
    if c["freq"]:
        o["freq"] = dev(np.random.default_rng(9).multinomial(N, np.full(N, 1.0 / N), size=S * nrep).astype(np.int64))
    else:
        o["sm"] = eng.DeviceSampler(99, S * nrep, N, rep0=11)
    return o


def rsb_run(L, c, o, ctx):
    from thermoextrap_amd._lib import ResampleOpts

    S, N, C, nrep, order = c["S"], c["N"], c["C"], c["nrep"], c["order"]
    out = ctx.out("out", (S, nrep, C, 2, order + 1))
    opts = ResampleOpts()
    opts.path = c["path"]
    opts.info = ctx.out("info", (4,), dtype=I64).value
    if c["prep"]:
        pp, pn = ctx.side("prep", L.txm_resample_batched_prep_bytes(S, N, C, nrep, order))
        opts.prep, opts.prep_bytes, opts.prep_valid = pp.value, pn, 0
    ws, nb = ctx.ws(L.txm_resample_vals_batched_ws_bytes(S, N, C, nrep, order))
    spec, counts = (None, None) if c["freq"] else (ct.byref(o["sm"].spec), P(o["sm"].counts))
    if c["path"] == PATH_AUTO and not c["prep"]:     # the entry point without options
        del ctx.bufs["info"]
        return L.txm_resample_vals_batched(o["tab"], S, C, N, C, order, nrep, P(o["freq"]), spec, counts, out, ws, nb, None)
    return L.txm_resample_vals_batched_opts(o["tab"], S, C, N, C, order, nrep, P(o["freq"]), spec, counts, out, ct.byref(opts),
                                            ws, nb, None)


def rsb_engine(eng, c, o):
    ops = o["ops"]
    return {"out": eng.resample_vals_batched([t[0] for t in ops], [t[1] for t in ops], c["order"], nrep=c["nrep"], sampler=o["sm"],
                                             freq=o["freq"], ws=[t[2] for t in ops] if c["weighted"] else None,
                                             path=_RS_NAMES[c["path"]])}


def rsb_path(L, c, o, res):
    i8 = c["path"] == PATH_INT8
    assert (L.txm_resample_i8_supported(c["N"], c["C"], c["nrep"], c["order"]) == 1) or not i8
    assert L.txm_resample_batched_path(c["S"], c["N"], c["C"], c["nrep"], c["order"]) == PATH_FP64    # the rule leaves small N on FP64
    if "info" in res:
        assert res["info"][0] == int(i8) and (res["info"][2] > 0 or not c["guard"]) and (res["info"][2] == 0 or i8), res["info"]


def rdata_make(L, eng, c):
    r = np.random.default_rng(70)
    nrec, C, K = c["nrec"], c["C"], c["order"] + 1
    data = 0.1 * r.normal(size=(nrec, C, 2, K))
    data[:, :, 0, 0] = r.uniform(1.0, 5.0, size=(nrec, C))
    freq = None if c["nrep"] is None else dev(r.integers(0, 4, size=(c["nrep"], nrec), dtype=np.int64))
    return dict(data=dev(data), freq=freq)


def rdata_run(L, c, o, ctx):
    nrec, C, order, nrep = c["nrec"], c["C"], c["order"], c["nrep"] or 1
    out = ctx.out("out", (nrep, C, 2, order + 1))
    ws, nb = ctx.ws(L.txm_resample_data_ws_bytes(nrec, C, order))
    return L.txm_resample_data(P(o["data"]), P(o["freq"]), nrec, C, nrep, order, out, ws, nb, None)


# ---- perturbation -----------------------------------------------------------------------------------------------------
# perturb_kernel<NA, VEC, LPR_LOG2, FREQ> and perturb_cov's iid kernel: VEC 2 needs an even C, an even pitch and a 16-byte
# aligned x, LPR = 2^LPR_LOG2 lanes a row (at most 256, then column chunks).  Aligned even C: VEC 2 with 1 .. 256 lanes and
# two chunks (514); odd C: VEC 1 with 1, 4 .. 256 lanes and two chunks (257); C = 2 with an odd pitch, C = 4 and 16 one column
# into a wider tensor (misaligned x): VEC 1 with 2, 4 and 16 lanes -- all 18 (VEC, LPR_LOG2) pairs, both chunk counts.
PT_LAYOUTS = [(2, "aligned"), (4, "aligned"), (8, "aligned"), (16, "aligned"), (32, "aligned"), (64, "aligned"), (128, "aligned"),
              (256, "aligned"), (512, "aligned"), (514, "aligned"), (1, "aligned"), (2, "odd pitch"), (4, "misaligned"),
              (16, "misaligned"), (3, "aligned"), (5, "aligned"), (9, "aligned"), (17, "aligned"), (33, "aligned"), (65, "aligned"),
              (129, "aligned"), (257, "aligned")]


def pt_plan(C, layout):
    """(VEC, LPR_LOG2, column chunks) of pb_plan for a layout of PT_LAYOUTS (torch allocations are 256-byte aligned)."""
    vec = 2 if (C % 2 == 0 and layout == "aligned") else 1
    l2 = 0
    while (1 << l2) < cdiv(C, vec) and l2 < 8:
        l2 += 1
    return vec, l2, cdiv(C, (1 << l2) * vec)


assert {pt_plan(C, lay)[:2] for C, lay in PT_LAYOUTS} == {(v, l) for v in (1, 2) for l in range(9)}
assert {(pt_plan(C, lay)[0], pt_plan(C, lay)[2]) for C, lay in PT_LAYOUTS} == {(1, 1), (1, 2), (2, 1), (2, 2)}


def pt_cases():
    """Every (VEC, LPR_LOG2) pair and both chunk counts at n_alpha 1, 5, 8 (the instantiations the -1 byte calls of
    tests/test_perturb_gpu.py reach), each without and with bootstrap counts (FREQ); then shapes off that grid."""
    out = [dict(id=f"C{C}_{lay.replace(' ', '_')}_na{na}_{'freq3' if nrep else 'nofreq'}", N=3001, C=C, layout=lay, na=na, nrep=nrep)
           for C, lay in PT_LAYOUTS for na in (1, 5, 8) for nrep in (None, 3)]
    out += [dict(id=f"N{N}_C{C}_na{na}_nrep{nrep}_pitch{pitch}", N=N, C=C, na=na, nrep=nrep, pitch=pitch)
            for N, C, na, nrep, pitch in ((10, 3, 2, None, None), (1000, 2, 3, 4, None), (777, 8, 8, None, 9), (300, 130, 3, 9, 136),
                                          (70_001, 4, 7, None, None), (50_000, 32, 3, 9, None))]
    return out


def ptc_cases():
    """txm_perturb_cov: the iid kernel on every (VEC, LPR_LOG2) pair and both chunk counts at n_alpha 1 and 8 (where
    tests/test_perturb_cov_gpu.py makes its -1 byte calls), the blocked path of its shapes, sizes and the grid cap."""
    out = [dict(id=f"C{C}_{lay.replace(' ', '_')}_na{na}_iid", N=1537, C=C, layout=lay, na=na, block=1, levels=1)
           for C, lay in PT_LAYOUTS for na in (1, 8)]
    out += [dict(id=f"N{N}_C{C}_{lay.replace(' ', '_')}_na{na}_block{block}_l{levels}", N=N, C=C, layout=lay, na=na, block=block, levels=levels)
            for N, C, lay, na, block, levels in ((10, 3, "aligned", 2, 1, 1), (10, 3, "aligned", 2, 2, 2), (4099, 5, "aligned", 3, 7, 4),
                                                 (4099, 32, "aligned", 8, 64, 3), (4099, 6, "odd pitch", 2, 2, 2),
                                                 (4099, 514, "aligned", 2, 16, 2), (1, 32, "aligned", 3, 1, 1), (200_000, 1, "aligned", 8, 1, 1),
                                                 (70_001, 514, "aligned", 1, 1, 1), (70_001, 2, "aligned", 8, 1000, 3))]
    return out


def pt_place(N, C, layout, seed):
    """x (N, C) in a layout of PT_LAYOUTS, with NaN in what lies beyond the columns, and u."""
    x, u, _ = xuw(N, C, False, seed)
    if layout == "aligned":
        return x, u
    off = 0 if layout == "odd pitch" else 1
    wide = torch.full((N, C + (3 if layout == "odd pitch" else 2)), float("nan"), dtype=F64, device="cuda")
    wide[:, off:off + C] = x
    return wide[:, off:off + C], u


def pt_path(L, c, o, res):
    if "layout" in c:
        x = o["x"]
        vec = 2 if (c["C"] % 2 == 0 and x.stride(0) % 2 == 0 and x.data_ptr() % 16 == 0) else 1
        assert vec == pt_plan(c["C"], c["layout"])[0], (vec, c["layout"])


def pt_make(L, eng, c):
    if "layout" in c:
        x, u = pt_place(c["N"], c["C"], c["layout"], 80 + c["C"])
    else:
        x, u, _ = xuw(c["N"], c["C"], False, 80 + c["C"], pitch=c.get("pitch"))
    da = np.ascontiguousarray(0.05 * (np.arange(c["na"]) - (c["na"] - 1) / 2.0) + 0.01)
    freq = None
    if c.get("nrep"):
        freq = dev(np.random.default_rng(4).multinomial(c["N"], np.full(c["N"], 1.0 / c["N"]), size=c["nrep"]).astype(np.int64))
    return dict(x=x, u=u, da=da, freq=freq, mean=eng.perturb(x, u, da).contiguous())


def pt_run(L, c, o, ctx):
    N, C, na, nrep = c["N"], c["C"], c["na"], c.get("nrep") or 1
    out = ctx.out("out", (nrep, na, C))
    ws, nb = ctx.ws(L.txm_perturb_ws_bytes(N, C, na, nrep))
    return L.txm_perturb(P(o["x"]), o["x"].stride(0), P(o["u"]), N, C, dp(o["da"]), na, P(o["freq"]), nrep, out, ws, nb, None)


def ptc_run(L, c, o, ctx):
    N, C, na, block, nl = c["N"], c["C"], c["na"], c["block"], c["levels"]
    var, neff = ctx.out("var", (nl, na, C)), ctx.out("neff", (na,))
    lnq, vl = ctx.out("lnq", (na,)), ctx.out("var_lnq", (nl, na))
    ws, nb = ctx.ws(L.txm_perturb_cov_ws_bytes(N, C, na, block, nl))
    return L.txm_perturb_cov(P(o["x"]), o["x"].stride(0), P(o["u"]), N, C, dp(o["da"]), na, P(o["mean"]), block, nl, var, neff, lnq,
                             vl, ws, nb, None)


def ptc_engine(eng, c, o):
    r = eng.perturb_cov(o["x"], o["u"], o["da"], block=c["block"], n_levels=c["levels"])
    return {"var": r.var, "neff": r.neff, "lnq": r.lnq, "var_lnq": r.var_lnq}


# ---- MBAR -------------------------------------------------------------------------------------------------------------
def mbar_ns(K, big=1025):
    """Ragged states, one of a single sample."""
    base = [37, 1, 300, big, 64, 255, 257, 5]
    return [base[s % len(base)] + (s // len(base)) for s in range(K)]


def mbar_make(L, eng, c):
    K, C = c["K"], c["C"]
    ns = c.get("ns") or mbar_ns(K)
    r = np.random.default_rng(100 + K)
    a0 = np.ascontiguousarray(1.0 + 0.02 * np.arange(K))
    us = [dev(r.normal(size=n) + 0.1 * s) for s, n in enumerate(ns)]
    pitch = c.get("pitch")
    xs = [xuw(n, C, False, 200 + s, pitch=pitch)[0] for s, n in enumerate(ns)]
    upiv = eng.mbar_pivot(us)
    g = np.ascontiguousarray(np.log(np.asarray(ns, dtype=np.float64)) - a0 * upiv)
    g -= g.max()
    tab, keep, _, _ = eng._mbar_table(us, xs)
    logD = torch.empty(sum(ns), dtype=F64, device="cuda")
    eng.mbar_eval(us, a0, g, upiv, logD)
    na = c.get("na", 1)
    al = np.ascontiguousarray(a0[0] - 0.01 + 0.013 * np.arange(na))
    return dict(ns=ns, a0=a0, us=us, xs=xs, upiv=upiv, g=g, tab=tab, keep=keep, logD=logD, al=al)


def mbar_run(L, c, o, ctx):
    K, C, na, ntot = c["K"], c["C"], c["na"], sum(o["ns"])
    if c["call"] == "txm_mbar_eval":          # sized with (K, 1, 1), as the engine does
        out = ctx.out("out", (K + K * (K + 1) // 2 + 1,))
        logD = ctx.out("logD", (ntot,))
        ws, nb = ctx.ws(L.txm_mbar_ws_bytes(K, 1, 1))
        return L.txm_mbar_eval(o["tab"], K, dp(o["a0"]), dp(o["g"]), o["upiv"], out, logD, ws, nb, None)
    out = ctx.out("out", (na, C))
    ws, nb = ctx.ws(L.txm_mbar_ws_bytes(K, C, na))
    return L.txm_mbar_predict(o["tab"], K, C, o["upiv"], P(o["logD"]), dp(o["al"]), na, out, ws, nb, None)


def mbar_engine(eng, c, o):
    K = c["K"]
    if c["call"] == "txm_mbar_eval":
        logD = torch.empty(sum(o["ns"]), dtype=F64, device="cuda")
        S, H, obj = eng.mbar_eval(o["us"], o["a0"], o["g"], o["upiv"], logD)
        nh = K * (K + 1) // 2
        return {"logD": logD, "out": torch.as_tensor(np.concatenate([S, H[np.triu_indices(K)], [obj]]))}
    return {"out": eng.mbar_predict(o["xs"], o["us"], o["a0"], None, o["logD"], o["al"], upiv=o["upiv"])}


def mbar_cases():
    out = []
    for K, C, na in ((1, 1, 1), (8, 5, 3), (9, 70, 8), (33, 5, 1), (8, 1, 8), (33, 70, 3)):
        for call in ("txm_mbar_eval", "txm_mbar_predict"):
            out.append(dict(id=f"K{K}_C{C}_na{na}_{call[9:]}", K=K, C=C, na=na, call=call))
    return out


def mcov_make(L, eng, c):
    from test_mbar_oracle_cpu import cov_case

    a0, ns, us, xs, upiv, g, targets, logD, means, pitch = cov_case(c["name"])
    assert (len(ns), xs[0].shape[1], len(targets)) == (c["K"], c["C"], c["na"]) and pitch is None
    ud, xd = [dev(u) for u in us], [dev(x) for x in xs]
    tab, keep, _, _ = eng._mbar_table(ud, xd)
    a0 = np.ascontiguousarray(a0, dtype=np.float64)
    # the log-weights as engine.mbar_cov_sums forms them from a solution's free energies (the case's g up to a constant and
    # a rounding): the same words go to the ctypes call, so the two results can be compared bit for bit
    f = np.asarray(g, dtype=np.float64) - np.log(np.asarray(ns, dtype=np.float64)) + a0 * float(upiv)
    sol = eng.MbarSolution(f, dev(logD), float(upiv), 0, 0, 0.0)
    g, shift = eng.mbar_solution_g(np.asarray(ns, dtype=np.float64), a0, sol)
    return dict(tab=tab, keep=keep, ud=ud, xd=xd, sol=sol, shift=shift, a0=a0, g=np.ascontiguousarray(g),
                al=np.ascontiguousarray(targets, dtype=np.float64), logD=sol.logD, mean=dev(means), upiv=float(upiv))


def mcov_engine(eng, c, o):
    """engine.mbar_cov_sums splits the [n_alpha][1 + K + C (1 + K)] rows into Q, B, yy, b on the host and moves lnw to the
    gauge of the solution: recombined / redone here with the same operations."""
    Q, B, yy, b, lnw = eng.mbar_cov_sums(o["xd"], o["ud"], o["a0"], o["sol"], o["al"], o["mean"], with_lnw=True)
    rest = np.concatenate([yy[:, :, None], b], axis=2).reshape(c["na"], -1)
    assert np.array_equal(o["_res"]["lnw"] - o["al"] * o["upiv"] + o["shift"], lnw), "lnw: differs from the engine's result"
    return {"out": torch.as_tensor(np.concatenate([Q[:, None], B, rest], axis=1))}


def mcov_run(L, c, o, ctx):
    K, C, na = c["K"], c["C"], c["na"]
    out, lnw = ctx.out("out", (na, 1 + K + C * (1 + K))), ctx.out("lnw", (na,))
    ws, nb = ctx.ws(L.txm_mbar_cov_ws_bytes(K, C, na))
    return L.txm_mbar_cov(o["tab"], K, C, o["upiv"], dp(o["a0"]), dp(o["g"]), P(o["logD"]), dp(o["al"]), na, P(o["mean"]), out, lnw,
                          ws, nb, None)


BOOT_NREP = 5


def boot_cases():
    out = []
    for K, C, na, big, pitch, active, tpc in ((2, 1, 3, 1025, None, None, 1), (8, 5, 8, 40_000, 7, [4, 0, 2], 2),
                                              (12, 70, 3, 1025, None, None, 1), (64, 5, 8, 5000, None, [1, 3], 2),
                                              (12, 1, 8, 23_000, 3, None, 2)):
        for call in ("txm_mbar_boot_eval", "txm_mbar_boot_predict"):
            out.append(dict(id=f"K{K}_C{C}_na{na}_big{big}_tpc{tpc}_{call[14:]}", K=K, C=C, na=na, ns=mbar_ns(K, big), pitch=pitch,
                            active=active, call=call, nrep=BOOT_NREP, tpc=tpc))
    return out


def boot_size(L, c):
    ntot = sum(c["ns"])
    if c["call"] == "txm_mbar_boot_eval":     # sized with (K, 1, 1, ...), as the engine does
        return L.txm_mbar_boot_ws_bytes(c["K"], 1, 1, ntot, c["nrep"])
    return L.txm_mbar_boot_ws_bytes(c["K"], c["C"], c["na"], ntot, c["nrep"])


def boot_make(L, eng, c):
    o = mbar_make(L, eng, c)
    K, nrep = c["K"], c["nrep"]
    o["sm"] = [eng.DeviceSampler(9000 + K, nrep, n, rep0=s * nrep) for s, n in enumerate(o["ns"])]
    o["tab"], o["stab"], o["keep"], _, _, _ = eng._mbar_boot_tables(o["us"], o["sm"], o["xs"])
    r = np.random.default_rng(5)
    o["f"] = 0.01 * r.normal(size=(nrep, K))
    o["f"][:, 0] = 0.0
    b = np.log(np.asarray(o["ns"], dtype=np.float64)) - o["a0"] * o["upiv"]       # engine.mbar_bootstrap_predict's g and gref
    gg = b[None, :] + o["f"]
    o["gb"] = np.ascontiguousarray(gg - gg.max(axis=1, keepdims=True))
    o["gref"] = np.ascontiguousarray(b - b.max())
    o["gd"] = dev(o["gb"])
    o["active"] = None if c["active"] is None else dev(np.asarray(c["active"], dtype=np.int32))
    return o


def boot_run(L, c, o, ctx):
    K, C, na, nrep = c["K"], c["C"], c["na"], c["nrep"]
    ws, nb = ctx.ws(boot_size(L, c))
    if c["call"] == "txm_mbar_boot_eval":
        nv = K + K * (K + 1) // 2 + 1
        rows = list(range(nrep)) if c["active"] is None else c["active"]
        mask = np.zeros((nrep, nv), dtype=bool)
        mask[rows] = True
        out = ctx.out("out", (nrep, nv), mask=mask)
        return L.txm_mbar_boot_eval(o["tab"], o["stab"], K, dp(o["a0"]), P(o["gd"]), P(o["active"]), len(rows), o["upiv"], out, ws, nb,
                                    None)
    out = ctx.out("out", (nrep, na, C))
    return L.txm_mbar_boot_predict(o["tab"], o["stab"], K, C, o["upiv"], dp(o["a0"]), P(o["gd"]), dp(o["gref"]), dp(o["al"]), na, out,
                                   ws, nb, None)


def boot_engine(eng, c, o):
    K = c["K"]
    if c["call"] == "txm_mbar_boot_eval":
        S, H, obj = eng.mbar_boot_eval(o["us"], o["a0"], o["sm"], o["gb"], o["upiv"], active=c["active"])
        rows = list(range(c["nrep"])) if c["active"] is None else c["active"]
        full = np.full((c["nrep"], K + K * (K + 1) // 2 + 1), np.nan)
        iu = np.triu_indices(K)
        full[rows] = np.concatenate([S, H[:, iu[0], iu[1]], obj[:, None]], axis=1)
        return {"out": torch.as_tensor(full)}
    sol0 = eng.MbarSolution(np.zeros(K), o["logD"], o["upiv"], 0, 0, 0.0)
    return {"out": eng.mbar_bootstrap_predict(o["xs"], o["us"], o["a0"], o["sm"], o["f"], sol0, o["al"])}


def boot_path(L, c, o, res):
    """txm_mbar_boot: a state's sampler tiles are split over at most 256 / K chunks; the cases named big* have a state
    with more tiles than that, so its chunks hold more than one tile."""
    cap = max(1, 256 // c["K"])
    tpc = max(cdiv(cdiv(n, 1024), min(cdiv(n, 1024), cap)) for n in c["ns"])
    assert tpc == c["tpc"], (tpc, cap)
    if c["pitch"] is not None:
        assert all(o["tab"][s].ldx_s == c["pitch"] > c["C"] for s in range(c["K"]) if c["ns"][s] > 1)


# ---- lag sums ---------------------------------------------------------------------------------------------------------
def lag_make(L, eng, c):
    n, C = c["n"], c["C"]
    r = np.random.default_rng(300 + C)
    u = dev(r.normal(size=n))
    x = None
    if C:
        x = xuw(n, C, False, 301, pitch=c.get("pitch"))[0]
    center = dev(np.concatenate([[0.01], np.full(C, 0.3)]))
    return dict(x=x, u=u, center=center, idx=np.ascontiguousarray(c["idx"], dtype=np.int32))


def lag_run(L, c, o, ctx):
    n, C, nl = c["n"], c["C"], c["nlags"]
    idx = o["idx"]
    ip = idx.ctypes.data_as(ct.POINTER(ct.c_int32))
    ldx = o["x"].stride(0) if C else 0
    if c["call"] == "txm_lag_sums":
        out = ctx.out("out", (idx.size, nl))
        ws, nb = ctx.ws(L.txm_lag_sums_ws_bytes(n, C, idx.size, nl))
        return L.txm_lag_sums(P(o["x"]), ldx, P(o["u"]), n, C, P(o["center"]), ip, idx.size, c["t0"], nl, out, ws, nb, None)
    no = cdiv(n - 1, c["nskip"])
    out = ctx.out("out", (idx.size, no, nl))
    mean = ctx.out("mean", (idx.size, no)) if c["mean"] else None
    ws, nb = ctx.ws(L.txm_lag_origin_sums_ws_bytes(n, C, idx.size, c["nskip"], nl))
    return L.txm_lag_origin_sums(P(o["x"]), ldx, P(o["u"]), n, C, P(o["center"]), ip, idx.size, c["nskip"], c["t0"], nl, out, mean,
                                 ws, nb, None)


def lag_engine(eng, c, o):
    if c["call"] == "txm_lag_sums":
        return {"out": eng.lag_sums(o["x"], o["u"], o["idx"], c["t0"], c["nlags"], center=o["center"])}
    out, mean = eng.lag_origin_sums(o["x"], o["u"], o["idx"], c["nskip"], c["t0"], c["nlags"], center=o["center"])
    return {"out": out, "mean": mean} if c["mean"] else {"out": out}


def lag_path(L, c, o, res):
    """A chunk is 1008 ceil(n / (1008 * 512)) samples: n = 516097 is the first n whose chunks take two stages."""
    n = c["n"]
    assert cdiv(n, 1008 * 512) == (2 if "n516097" in c["id"] else 1)
    if c["t0"] >= n:
        assert not res["out"].any()       # every lag of the block lies past the series


LAG_CASES = [
    dict(id="n1_C0_256", call="txm_lag_sums", n=1, C=0, idx=[0], t0=0, nlags=256),
    dict(id="n1009_C33_512_pitch35", call="txm_lag_sums", n=1009, C=33, idx=[0, 33, 34, 66], t0=0, nlags=512, pitch=35),
    dict(id="n1009_C5_t0_past_n", call="txm_lag_sums", n=1009, C=5, idx=[0, 5, 10], t0=1024, nlags=256),
    dict(id="n516097_C5_1024", call="txm_lag_sums", n=516097, C=5, idx=[0, 3, 8], t0=256, nlags=1024),
]
LAGO_CASES = [
    dict(id="n300_C5_nskip1_256_mean", call="txm_lag_origin_sums", n=300, C=5, idx=[0, 2, 5], nskip=1, t0=0, nlags=256, mean=True),
    dict(id="n4000_C0_nskip1500_512_nomean", call="txm_lag_origin_sums", n=4000, C=0, idx=[0], nskip=1500, t0=0, nlags=512, mean=False),
    dict(id="n4000_C33_nskip1500_t0_past_n", call="txm_lag_origin_sums", n=4000, C=33, idx=[33, 0], nskip=1500, t0=4096, nlags=256,
         mean=True, pitch=40),
    dict(id="n516097_C1_nskip200000_1024", call="txm_lag_origin_sums", n=516097, C=1, idx=[1], nskip=200_000, t0=0, nlags=1024,
         mean=True),
]
LAGB_NS = [1, 3, 255, 257, 1007, 1008, 1009, 2017, 4099, 200_000, 600_000]    # the ragged states of test_timeseries_states_gpu.py
LAGB_C = 2


def lagb_ns_ptr(c):
    ns = np.ascontiguousarray(c["ns"], dtype=np.int64)
    return ns, ns.ctypes.data_as(ct.POINTER(ct.c_int64))


def lagb_items(c):
    from thermoextrap_amd._lib import LagItem

    items = [(s, p) for s in range(len(c["ns"])) for p in range(2 * c["C"] + 1)][::-1] if c.get("items") is None else c["items"]
    return items, (LagItem * len(items))(*[LagItem(s, p) for s, p in items])


def lagb_make(L, eng, c):
    from thermoextrap_amd._lib import LagState

    C = c["C"]
    r = np.random.default_rng(400)
    us = [dev(r.normal(size=n)) for n in c["ns"]]
    xs = [xuw(n, C, False, 401 + s, pitch=c.get("pitch"))[0] for s, n in enumerate(c["ns"])] if C else [None] * len(us)
    centers = [dev(np.concatenate([[0.01], np.full(C, 0.3)])) for _ in us]
    tab = (LagState * len(us))(*[LagState(x.data_ptr() if C else None, u.data_ptr(), m.data_ptr(), int(n))
                                 for x, u, m, n in zip(xs, us, centers, c["ns"])])
    return dict(us=us, xs=xs, centers=centers, tab=tab)


def lagb_rows_run(L, c, o, ctx, delta=0):
    ns, nsp = lagb_ns_ptr(c)
    S, C = len(ns), c["C"]
    rows, rb = ctx.side("rows", L.txm_lag_rows_batched_bytes(nsp, S, C), delta=delta, compare=True)
    return L.txm_lag_rows_batched(o["tab"], S, c.get("pitch") or C, C, rows, rb, None)


def lagb_sums_run(L, c, o, ctx):
    ns, nsp = lagb_ns_ptr(c)
    S, C, nl = len(ns), c["C"], c["nlags"]
    items, itab = lagb_items(c)
    rows, rb = ctx.side("rows", L.txm_lag_rows_batched_bytes(nsp, S, C), by_target=False)
    rc = L.txm_lag_rows_batched(o["tab"], S, c.get("pitch") or C, C, rows, rb, None)
    assert rc == 0
    out = ctx.out("out", (len(items), nl))
    ws, nb = ctx.ws(L.txm_lag_sums_batched_ws_bytes(nsp, S, C, itab, len(items), nl))
    return L.txm_lag_sums_batched(rows, rb, nsp, S, C, itab, len(items), c["t0"], nl, out, ws, nb, None)


def lagb_rows_engine(eng, c, o):
    return {"rows": eng.lag_rows_batched(o["xs"] if c["C"] else None, o["us"], o["centers"]).rows}


def lagb_engine(eng, c, o):
    h = eng.lag_rows_batched(o["xs"] if c["C"] else None, o["us"], o["centers"])
    return {"out": eng.lag_sums_batched(h, lagb_items(c)[0], c["t0"], c["nlags"])}


def lagb_rows_exact(L, c, o, row):
    """rows_bytes is checked with ==: one byte less and one byte more are both TXM_ERR_INVALID, nothing is written."""
    for delta in (-1, +1):
        ctx = Ctx("nan")
        assert lagb_rows_run(L, c, o, ctx, delta=delta) == ERR_INVALID
        ctx.verify_refused()


LAGB_CASES = [dict(id="ragged11_C2_256", ns=LAGB_NS, C=LAGB_C, t0=0, nlags=256),
              dict(id="ragged5_C0_512_t0_256", ns=LAGB_NS[4:9], C=0, t0=256, nlags=512),
              dict(id="ragged4_C3_pitch5_items", ns=[1009, 1, 2017, 16], C=3, pitch=5, t0=0, nlags=256,
                   items=[(2, 6), (0, 0), (3, 4), (2, 6), (1, 1)])]


# ---- delta-method covariance --------------------------------------------------------------------------------------------
def inf_coefs(lead, nf, nq, seed):
    r = np.random.default_rng(seed)
    return dev(0.3 * r.normal(size=(*lead, nf, nq))), dev(0.3 * r.normal(size=(*lead, nf, nq))), dev(np.full(lead, 0.3))


def inf_make(L, eng, c):
    x, u, w = xuw(c["N"], c["C"], c["weighted"], 500 + c["C"], colmajor=c.get("col", False), pitch=c.get("pitch"))
    a, b, cx = inf_coefs((c["C"],), c["nf"], c["nq"], 501)
    return dict(x=x, u=u, w=w, a=a, b=b, cx=cx, ld=ld(x))


def inf_layout(c, ldx_s, aligned=True):
    """The instantiation txm_influence_cov picks: the series kernel for one tight column, two columns per lane when C and
    the pitch are even, x is 16-byte aligned and n_q <= 6, one column per lane otherwise."""
    if c["C"] == 1 and ldx_s == 1:
        return "series"
    return "two" if c["C"] % 2 == 0 and ldx_s % 2 == 0 and aligned and c["nq"] <= 6 else "one"


def inf_run(L, c, o, ctx):
    N, C, nf, nq = c["N"], c["C"], c["nf"], c["nq"]
    call = c["call"]
    front = (P(o["x"]), o["ld"][0]) + ((o["ld"][1],) if call == "txm_influence_cov" else ()) + (P(o["u"]), P(o["w"]), N, C, nf, nq,
                                                                                                 0.01, P(o["cx"]), P(o["a"]), P(o["b"]))
    if call == "txm_influence_cov":
        cov, mean = ctx.out("cov", (C, nf, nf)), ctx.out("mean", (C, nf))
        ws, nb = ctx.ws(L.txm_influence_cov_ws_bytes(N, C, nq))
        return L.txm_influence_cov(*front, cov, mean, ws, nb, None)
    if call == "txm_influence_cross_cov":
        cov = ctx.out("cov", (C, nf, C, nf))
        ws, nb = ctx.ws(L.txm_influence_cross_cov_ws_bytes(N, C, nf, nq))
        return L.txm_influence_cross_cov(*front, cov, ws, nb, None)
    block, nl = c["block"], c["levels"]
    if call == "txm_influence_block_cov":
        cov, mean = ctx.out("cov", (nl, C, nf, nf)), ctx.out("mean", (C, nf))
        ws, nb = ctx.ws(L.txm_influence_block_cov_ws_bytes(N, C, nf, nq, block))
        return L.txm_influence_block_cov(*front, block, nl, cov, mean, ws, nb, None)
    cov, mean = ctx.out("cov", (nl, C, nf, C, nf)), ctx.out("mean", (C, nf))
    ws, nb = ctx.ws(L.txm_influence_block_cross_cov_ws_bytes(N, C, nf, nq, block, nl))
    return L.txm_influence_block_cross_cov(*front, block, nl, cov, mean, ws, nb, None)


def inf_engine(eng, c, o):
    if c["C"] == 1 and c["pitch"]:      # the engine hands a single column over as a tight series: another kernel, other bits
        return {}
    args =(o["x"], o["u"], o["a"], o["b"], 0.01, o["cx"])
    call = c["call"]
    if call == "txm_influence_cov":
        cov, mean = eng.influence_cov(*args, w=o["w"])
    elif call == "txm_influence_cross_cov":
        return {"cov": eng.influence_cross_cov(*args, w=o["w"])}
    elif call == "txm_influence_block_cov":
        cov, mean = eng.influence_block_cov(*args, c["block"], c["levels"], w=o["w"])
    else:
        cov, mean = eng.influence_block_cross_cov(*args, c["block"], c["levels"], w=o["w"])
    return {"cov": cov, "mean": mean}


def inf_path(L, c, o, res):
    if "layout" in c:
        assert inf_layout(c, o["ld"][0]) == c["layout"]
    if c.get("capped"):     # more than 8 workgroups of 256 rows per CU
        assert cdiv(c["N"], 256) > 8 * cus()


def inf_case(call, id, N, C, nf, nq, *, w=False, pitch=None, col=False, layout=None, capped=False, block=None, levels=None):
    d = dict(id=id, call=call, N=N, C=C, nf=nf, nq=nq, weighted=w, pitch=pitch, col=col, capped=capped, block=block, levels=levels)
    if layout:
        d["layout"] = layout
    return d


INF_CASES = [
    inf_case("txm_influence_cov", "series_N100_C1_nq1", 100, 1, 2, 1, layout="series"),
    inf_case("txm_influence_cov", "one_N1000_C33_nq9_w", 1000, 33, 3, 9, w=True, layout="one"),
    inf_case("txm_influence_cov", "two_N1000_C514_nq2", 1000, 514, 2, 2, layout="two"),
    inf_case("txm_influence_cov", "one_N777_C1_pitch3_nq9", 777, 1, 9, 9, pitch=3, layout="one"),
    inf_case("txm_influence_cov", "col_N1000_C33_nq1_w", 1000, 33, 2, 1, w=True, col=True),
    inf_case("txm_influence_cov", "two_N700001_C2_nq3_grid_cap", 700_001, 2, 2, 3, layout="two", capped=True),
]
INFB_CASES = [
    inf_case("txm_influence_block_cov", "N100_C1_nq1_block1", 100, 1, 2, 1, block=1, levels=1),
    inf_case("txm_influence_block_cov", "N1000_C33_nq9_w_block7_l3", 1000, 33, 3, 9, w=True, block=7, levels=3),
    inf_case("txm_influence_block_cov", "N5000_C514_nq2_block64_l2", 5000, 514, 2, 2, block=64, levels=2),
    inf_case("txm_influence_block_cov", "N700001_C2_nq3_block1000_l4_pitch4", 700_001, 2, 2, 3, pitch=4, block=1000, levels=4, capped=True),
]
INFX_CASES = [
    inf_case("txm_influence_cross_cov", "N100_C1_nq1", 100, 1, 2, 1),
    inf_case("txm_influence_cross_cov", "N1000_C33_nq9_w", 1000, 33, 3, 9, w=True),
    inf_case("txm_influence_cross_cov", "N3000_C100_nq2_pitch101", 3000, 100, 2, 2, pitch=101),
    inf_case("txm_influence_cross_cov", "N700001_C2_nq3_grid_cap", 700_001, 2, 2, 3, capped=True),
]
INFBX_CASES = [
    inf_case("txm_influence_block_cross_cov", "N100_C1_nq1_block1", 100, 1, 2, 1, block=1, levels=1),
    inf_case("txm_influence_block_cross_cov", "N1000_C33_nq9_w_block7_l3", 1000, 33, 3, 9, w=True, block=7, levels=3),
    inf_case("txm_influence_block_cross_cov", "N3000_C100_nq2_block64_l2", 3000, 100, 2, 2, block=64, levels=2),
    inf_case("txm_influence_block_cross_cov", "N700001_C2_nq3_block1000_l4", 700_001, 2, 2, 3, block=1000, levels=4, capped=True),
]


def infs_make(L, eng, c):
    from thermoextrap_amd._lib import InfState

    ops = [xuw(n, c["C"], c["weighted"], 600 + s, pitch=c.get("pitch")) for s, n in enumerate(c["ns"])]
    S = len(ops)
    a, b, cx = inf_coefs((S, c["C"]), c["nf"], c["nq"], 601)
    tab = (InfState * S)()
    for s, (x, u, w) in enumerate(ops):
        tab[s].x, tab[s].u, tab[s].n = x.data_ptr(), u.data_ptr(), c["ns"][s]
        tab[s].w = w.data_ptr() if w is not None else None
    return dict(ops=ops, a=a, b=b, cx=cx, tab=tab, cu=dev(np.full(S, 0.01)))


def infs_run(L, c, o, ctx):
    S, C, nf, nq, nmax = len(c["ns"]), c["C"], c["nf"], c["nq"], max(c["ns"])
    ldx = c.get("pitch") or C
    front = (o["tab"], S, ldx, C, nf, nq, P(o["cu"]), P(o["cx"]), P(o["a"]), P(o["b"]))
    if c["call"] == "txm_influence_cov_batched":
        cov, mean = ctx.out("cov", (S, C, nf, nf)), ctx.out("mean", (S, C, nf))
        ws, nb = ctx.ws(L.txm_influence_cov_batched_ws_bytes(S, nmax, C, nq))
        return L.txm_influence_cov_batched(*front, cov, mean, ws, nb, None)
    cov = ctx.out("cov", (S, C, nf, C, nf))
    ws, nb = ctx.ws(L.txm_influence_cross_cov_batched_ws_bytes(S, nmax, C, nf, nq))
    return L.txm_influence_cross_cov_batched(*front, cov, ws, nb, None)


def infs_engine(eng, c, o):
    xs, us = [t[0] for t in o["ops"]], [t[1] for t in o["ops"]]
    ws = [t[2] for t in o["ops"]] if c["weighted"] else None
    if c["call"] == "txm_influence_cov_batched":
        cov, mean = eng.influence_cov_batched(xs, us, o["a"], o["b"], o["cu"], o["cx"], ws=ws)
        return {"cov": cov, "mean": mean}
    return {"cov": eng.influence_cross_cov_batched(xs, us, o["a"], o["b"], o["cu"], o["cx"], ws=ws)}


def infs_path(L, c, o, res):
    """States of unequal length: the launch is as wide as the longest state's plan, wider than the shorter states' own."""
    assert cdiv(max(c["ns"]), 256) > cdiv(min(c["ns"]), 256)
    assert (cdiv(max(c["ns"]), 256) > 8 * cus()) == ("grid_cap" in c["id"])     # more than 8 workgroups of 256 rows per CU
    if "layout" in c:
        assert inf_layout(c, c.get("pitch") or c["C"]) == c["layout"]


def infs_cases(call):
    return [dict(id="series_S3_C1_nq1", call=call, ns=[100, 700, 1], C=1, nf=2, nq=1, weighted=False, layout="series"),
            dict(id="two_S3_C4_nq3_w", call=call, ns=[700, 100, 2017], C=4, nf=3, nq=3, weighted=True, layout="two"),
            dict(id="one_S4_C33_nq9_pitch35", call=call, ns=[1, 700, 100, 5000], C=33, nf=2, nq=9, weighted=False, pitch=35, layout="one"),
            dict(id="two_S2_C100_nq2_grid_cap", call=call, ns=[700_001, 300], C=100, nf=1, nq=2, weighted=False, layout="two")]


# ---- the table --------------------------------------------------------------------------------------------------------
def _sz(fn, *keys):
    return lambda L, c: getattr(L, fn)(*[c[k] for k in keys])


CONTRACTS = [
    Row("txm_reduce_vals_ws_bytes", ("txm_reduce_vals", "txm_reduce_vals_sums", "txm_reduce_vals_pivot", "txm_reduce_vals_pivot_w"), reduce_cases(), _sz("txm_reduce_vals_ws_bytes", "N", "C", "order"),
        reduce_make, reduce_run, reduce_engine, reduce_path),
    Row("txm_push_vals_ws_bytes", ("txm_push_vals",), push_cases(), _sz("txm_push_vals_ws_bytes", "N", "C", "order"), push_make, push_run,
        lambda eng, c, o: {"state": eng.push_vals(o["state"].clone(), o["x"], o["u"], o["w"])}, reduce_path),
    Row("txm_reduce_vals_1d_ws_bytes", ("txm_reduce_vals_1d",),
        [dict(id=f"N{N}_R{R}_M{M}_{'w' if w else 'u'}", N=N, R=R, M=M, weighted=w)
         for N, R, M, w in ((100, 1, 3, False), (5000, 3, 5, True), (4_200_000, 2, 9, False), (1, 5, 2, True))],
        _sz("txm_reduce_vals_1d_ws_bytes", "N", "R", "M"), r1d_make, r1d_run,
        lambda eng, c, o: {"out": eng.reduce_vals_1d(o["u"], c["M"] - 1, o["w"])}, reduce_path),
    Row("txm_reduce_vals_batched_ws_bytes", ("txm_reduce_vals_batched",),
        [dict(id=f"S{S}_N{N}_C{C}_{'w' if w else 'u'}", S=S, N=N, C=C, order=order, weighted=w)
         for S, N, C, order, w in ((3, 100, 1, 3, False), (3, 100, 33, 4, True), (3, 70_001, 17, 2, False), (3, 300, 514, 1, True))],
        _sz("txm_reduce_vals_batched_ws_bytes", "S", "N", "C", "order"), rbatch_make, rbatch_run, rbatch_engine, reduce_path),
    Row("txm_indices_to_freq_ws_bytes", ("txm_indices_to_freq",),
        [dict(id=f"ndat{ndat}_nrep{nrep}_nsamp{nsamp}", ndat=ndat, nrep=nrep, nsamp=nsamp)
         for ndat, nrep, nsamp in ((1, 3, 5), (1023, 3, 700), (1025, 1024, 300), (4097, 3, 5000))],
        lambda L, c: L.txm_indices_to_freq_ws_bytes(), i2f_make, i2f_run,
        lambda eng, c, o: {"freq": eng.indices_to_freq(o["idx"], c["ndat"])}),
    Row("txm_sampler_counts_ws_bytes", ("txm_sampler_tile_counts", "txm_sampler_freq"), sampler_cases(),
        lambda L, c: L.txm_sampler_counts_ws_bytes(ct.byref(spec_of(c))), lambda L, eng, c: {}, counts_run, counts_engine, counts_path),
    Row("txm_sampler_count_table_bytes", ("txm_sampler_count_table",),
        [dict(id=f"ndat{ndat}_nrep{nrep}_begin{begin}_nreps{nreps}_rep0{rep0}", ndat=ndat, nrep=nrep, begin=begin, nreps=nreps, rep0=rep0)
         for ndat, nrep, begin, nreps, rep0 in ((1024, 3, 0, 3, 0), (1025, 130, 128, 2, 9), (4097, 130, 0, 130, 0), (4097, 3, 0, 128, 4))],
        _sz("txm_sampler_count_table_bytes", "ndat", "nreps"), table_make, table_run, None, table_path, short="none"),
    Row("txm_resample_vals_ws_bytes", ("txm_resample_vals",), RS_AUTO, rs_need, rs_make, rs_run_auto, rs_engine, rs_path),
    Row("txm_resample_vals_ws_bytes_opts", ("txm_resample_vals",), RS_OPTS, rs_need, rs_make, rs_run, rs_engine, rs_path),
    Row("txm_resample_y_ws_bytes", ("txm_resample_vals",), RS_Y, rs_need, rs_make, rs_run, rs_engine, rs_path),
    Row("txm_resample_prep_bytes", ("txm_resample_vals",), RS_PREP, _sz("txm_resample_prep_bytes", "N", "C", "nrep", "order"), rs_make,
        rs_run, rs_engine, rs_path, short="prep"),
    Row("txm_resample_vals_batched_ws_bytes", ("txm_resample_vals_batched", "txm_resample_vals_batched_opts"), RSB,
        _sz("txm_resample_vals_batched_ws_bytes", "S", "N", "C", "nrep", "order"), rsb_make, rsb_run, rsb_engine, rsb_path),
    Row("txm_resample_batched_prep_bytes", ("txm_resample_vals_batched_opts",), RSB_PREP,
        _sz("txm_resample_batched_prep_bytes", "S", "N", "C", "nrep", "order"), rsb_make, rsb_run, rsb_engine, rsb_path, short="prep"),
    Row("txm_resample_data_ws_bytes", ("txm_resample_data",),
        [dict(id=f"nrec{nrec}_C{C}_nrep{nrep}", nrec=nrec, C=C, order=order, nrep=nrep)
         for nrec, C, order, nrep in ((1, 1, 3, 5), (257, 32, 3, 5), (257, 1, 8, None), (1, 32, 0, 3), (257, 3, 2, 70))],
        _sz("txm_resample_data_ws_bytes", "nrec", "C", "order"), rdata_make, rdata_run,
        lambda eng, c, o: {"out": eng.resample_data(o["data"], o["freq"], c["order"])}),
    Row("txm_perturb_ws_bytes", ("txm_perturb",),
        pt_cases(), lambda L, c: L.txm_perturb_ws_bytes(c["N"], c["C"], c["na"], c["nrep"] or 1), pt_make, pt_run,
        lambda eng, c, o: {"out": eng.perturb(o["x"], o["u"], o["da"], freq=o["freq"]).reshape(c["nrep"] or 1, c["na"], c["C"])},
        pt_path),
    Row("txm_perturb_cov_ws_bytes", ("txm_perturb_cov",),
        ptc_cases(), _sz("txm_perturb_cov_ws_bytes", "N", "C", "na", "block", "levels"), pt_make, ptc_run, ptc_engine, pt_path),
    Row("txm_mbar_ws_bytes", ("txm_mbar_eval", "txm_mbar_predict"), mbar_cases(),
        lambda L, c: L.txm_mbar_ws_bytes(c["K"], 1, 1) if c["call"] == "txm_mbar_eval" else L.txm_mbar_ws_bytes(c["K"], c["C"], c["na"]),
        mbar_make, mbar_run, mbar_engine),
    Row("txm_mbar_cov_ws_bytes", ("txm_mbar_cov",),
        [dict(id="K17_C1_na1", name="K17_C1_na1", K=17, C=1, na=1), dict(id="K16_C15_na8", name="K16_C15_na8", K=16, C=15, na=8)],
        _sz("txm_mbar_cov_ws_bytes", "K", "C", "na"), mcov_make, mcov_run, mcov_engine),
    Row("txm_mbar_boot_ws_bytes", ("txm_mbar_boot_eval", "txm_mbar_boot_predict"), boot_cases(), boot_size, boot_make, boot_run,
        boot_engine, boot_path),
    Row("txm_lag_sums_ws_bytes", ("txm_lag_sums",), LAG_CASES,
        lambda L, c: L.txm_lag_sums_ws_bytes(c["n"], c["C"], len(c["idx"]), c["nlags"]), lag_make, lag_run, lag_engine, lag_path),
    Row("txm_lag_origin_sums_ws_bytes", ("txm_lag_origin_sums",), LAGO_CASES,
        lambda L, c: L.txm_lag_origin_sums_ws_bytes(c["n"], c["C"], len(c["idx"]), c["nskip"], c["nlags"]), lag_make, lag_run,
        lag_engine, lag_path),
    Row("txm_lag_rows_batched_bytes", ("txm_lag_rows_batched",), LAGB_CASES,
        lambda L, c: L.txm_lag_rows_batched_bytes(lagb_ns_ptr(c)[1], len(c["ns"]), c["C"]), lagb_make, lagb_rows_run, lagb_rows_engine, None,
        short="exact"),
    Row("txm_lag_sums_batched_ws_bytes", ("txm_lag_sums_batched",), LAGB_CASES,
        lambda L, c: L.txm_lag_sums_batched_ws_bytes(lagb_ns_ptr(c)[1], len(c["ns"]), c["C"], lagb_items(c)[1], len(lagb_items(c)[0]),
                                                     c["nlags"]), lagb_make, lagb_sums_run, lagb_engine),
    Row("txm_influence_cov_ws_bytes", ("txm_influence_cov",), INF_CASES, _sz("txm_influence_cov_ws_bytes", "N", "C", "nq"), inf_make,
        inf_run, inf_engine, inf_path),
    Row("txm_influence_cov_batched_ws_bytes", ("txm_influence_cov_batched",), infs_cases("txm_influence_cov_batched"),
        lambda L, c: L.txm_influence_cov_batched_ws_bytes(len(c["ns"]), max(c["ns"]), c["C"], c["nq"]), infs_make, infs_run, infs_engine,
        infs_path),
    Row("txm_influence_block_cov_ws_bytes", ("txm_influence_block_cov",), INFB_CASES,
        _sz("txm_influence_block_cov_ws_bytes", "N", "C", "nf", "nq", "block"), inf_make, inf_run, inf_engine, inf_path),
    Row("txm_influence_cross_cov_ws_bytes", ("txm_influence_cross_cov",), INFX_CASES,
        _sz("txm_influence_cross_cov_ws_bytes", "N", "C", "nf", "nq"), inf_make, inf_run, inf_engine, inf_path),
    Row("txm_influence_block_cross_cov_ws_bytes", ("txm_influence_block_cross_cov",), INFBX_CASES,
        _sz("txm_influence_block_cross_cov_ws_bytes", "N", "C", "nf", "nq", "block", "levels"), inf_make, inf_run, inf_engine, inf_path),
    Row("txm_influence_cross_cov_batched_ws_bytes", ("txm_influence_cross_cov_batched",), infs_cases("txm_influence_cross_cov_batched")[:3],
        lambda L, c: L.txm_influence_cross_cov_batched_ws_bytes(len(c["ns"]), max(c["ns"]), c["C"], c["nf"], c["nq"]), infs_make, infs_run,
        infs_engine, infs_path),
]
ALL = [(row, case) for row in CONTRACTS for case in row.cases]
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(txm):
    from thermoextrap_amd import engine

    return engine


def _same(got, want, what):
    want = want.detach().cpu().numpy() if isinstance(want, torch.Tensor) else np.asarray(want)
    assert np.array_equal(got.reshape(-1), want.reshape(-1).astype(got.dtype), equal_nan=True), what


@pytest.mark.parametrize("row,case", ALL, ids=[f"{row.query[4:]}-{case['id']}" for row, case in ALL])
def test_contract(eng, row, case):
    from thermoextrap_amd import _lib

    L = lib()
    need = row.size(L, case)
    assert need > 0
    o = row.make(L, eng, case)
    short = case.get("short", row.short)
    target = "prep" if short == "prep" else "rows" if short == "exact" else "ws"
    done = []
    # (a) exact size, dirty workspace
    a = Ctx("nan")
    rc = row.run(L, case, o, a)
    assert rc == 0, (rc, _lib.last_error())
    a.verify_ok()
    res = o["_res"] = a.results()
    has_ws = "ws" in a.bufs
    done.append("exact size with a dirty workspace" if has_ws else "exact-size buffers")
    if row.path is not None:
        row.path(L, case, o, res)
    # (b) contents do not matter; the engine's result for the same operands
    b = Ctx("zero")
    assert row.run(L, case, o, b) == 0
    b.verify_ok()
    for name, v in b.results().items():
        _same(res[name], v, f"{name}: {'a zeroed workspace' if has_ws else 'a second call'} gives other bits")
    done.append("zeroed workspace" if has_ws else "second call")
    if row.engine is not None:
        got = row.engine(eng, case, o)
        for name, v in got.items():
            if a.bufs[name][1] == "side":     # a block with padding nobody writes: the words the call wrote, against the engine's
                wrote = res[name].view(np.int64) != NAN_BITS
                assert wrote.sum() >= (1 + case["C"]) * sum(case["ns"]), name      # at least every centred sample
                assert np.array_equal(res[name].view(np.int64)[wrote], v.cpu().numpy().view(np.int64)[wrote]), f"{name}: differs from the engine's"
            else:
                _same(res[name], v, f"{name}: differs from the engine's result")
        if got:
            done.append("engine")
    # (c) one byte short
    if row.run in (rs_run, rs_run_auto) and short == "standard" and rs_need(L, case) > rs_floor(L, case):
        rs_table_short(L, case, o, row, res)
        done.append("fallback below the count table, refusal below the table-free query")
    elif short == "exact":
        lagb_rows_exact(L, case, o, row)
        done.append("refusal one byte short and one byte long")
    elif short != "none":
        c = Ctx("nan", short=1, target=target)
        assert row.run(L, case, o, c) == ERR_WORKSPACE
        c.verify_refused()
        done.append("refusal one byte short")
    PASSED[row.query] += 1
    print(f"\n{row.query} [{case['id']}]: {need} bytes: {', '.join(done)} ok; passed so far in this row: "
          f"{PASSED[row.query]} of {len(row.cases)}")


def test_every_selected_case_passed(request):
    """The per-row pass counts, for the log -- and every case of the table that this session selected has passed (a run
    of the whole module: every case of every row)."""
    selected = Counter(item.callspec.params["row"].query for item in request.session.items
                       if getattr(item, "originalname", "") == "test_contract" and item.module.__name__ == __name__)
    for row in CONTRACTS:
        print(f"{row.query}: {PASSED[row.query]} of {len(row.cases)} cases passed ({selected[row.query]} selected)")
    assert all(PASSED[row.query] == selected[row.query] for row in CONTRACTS)


# ---- the engine asks for what it uses ---------------------------------------------------------------------------------
def _engine_calls(eng):
    """One small public call of every engine wrapper that takes a workspace: name -> thunk returning tensors / arrays."""
    L = lib()
    x, u, w = xuw(700, 4, True, 900)
    xs = [xuw(n, 4, True, 910 + s) for s, n in enumerate((300, 700, 1))]
    same = [xuw(1500, 4, True, 920 + s) for s in range(2)]
    a, b, cx = inf_coefs((4,), 3, 3, 930)
    aS, bS, cxS = inf_coefs((3, 4), 3, 3, 931)
    piv = eng.reduce_pivot(x, u, w)
    da = np.array([0.02, -0.03, 0.05])
    freq = dev(np.random.default_rng(1).multinomial(700, np.full(700, 1 / 700), size=5).astype(np.int64))
    idx = dev(np.random.default_rng(2).integers(0, 700, size=(5, 700), dtype=np.int64))
    sm = eng.DeviceSampler(5, 7, 700, rep0=2)
    smb = eng.DeviceSampler(6, 2 * 7, 1500)
    st0 = eng.reduce_vals(x[:100], u[:100], 3, w[:100]).contiguous()
    data = eng.resample_vals(x, u, 3, sampler=sm, w=w).contiguous()
    mo = mbar_make(L, eng, dict(K=3, C=4, na=3))
    bo = boot_make(L, eng, dict(K=3, C=4, na=3, nrep=5, ns=mbar_ns(3), active=None))
    sol = eng.MbarSolution(np.zeros(3), mo["logD"], mo["upiv"], 0, 0, 0.0)
    means = eng.mbar_predict(mo["xs"], mo["us"], mo["a0"], None, mo["logD"], mo["al"], upiv=mo["upiv"])
    center = dev(np.array([0.01, 0.3, 0.3, 0.3, 0.3]))
    lx, lu = [t[0] for t in xs], [t[1] for t in xs]
    lw = [t[2] for t in xs]
    return {
        "reduce_vals": lambda: eng.reduce_vals(x, u, 3, w),
        "reduce_sums": lambda: eng.reduce_sums(x, u, 3, piv, w),
        "push_vals": lambda: eng.push_vals(st0.clone(), x, u, w),
        "reduce_vals_1d": lambda: eng.reduce_vals_1d(u, 4, w),
        "indices_to_freq": lambda: eng.indices_to_freq(idx),
        "DeviceSampler.draw": lambda: eng.DeviceSampler(5, 7, 700, rep0=2).counts,
        "resample_vals": lambda: eng.resample_vals(x, u, 3, sampler=sm, w=w),
        "resample_vals_freq_y": lambda: eng.resample_vals(x, u, 2, freq=freq, w=w, y=x * 2.0),
        "resample_vals_int8_y": lambda: eng.resample_vals(same[0][0], same[0][1], 2, sampler=eng.DeviceSampler(7, 65, 1500), path="int8",
                                                          y=same[1][0]),
        "reduce_vals_batched": lambda: eng.reduce_vals_batched([t[0] for t in same], [t[1] for t in same], 3, ws=[t[2] for t in same]),
        "resample_vals_batched": lambda: eng.resample_vals_batched([t[0] for t in same], [t[1] for t in same], 2, nrep=7, sampler=smb),
        "resample_vals_batched_int8": lambda: eng.resample_vals_batched([t[0] for t in same], [t[1] for t in same], 2, nrep=7, sampler=smb,
                                                                        path="int8"),
        "resample_data": lambda: eng.resample_data(data, freq[:, :7].contiguous(), 3),
        "influence_cov": lambda: eng.influence_cov(x, u, a, b, 0.01, cx, w=w),
        "influence_cov_batched": lambda: eng.influence_cov_batched(lx, lu, aS, bS, [0.01] * 3, cxS, ws=lw),
        "influence_block_cov": lambda: eng.influence_block_cov(x, u, a, b, 0.01, cx, 7, 3, w=w),
        "influence_cross_cov": lambda: eng.influence_cross_cov(x, u, a, b, 0.01, cx, w=w),
        "influence_cross_cov_batched": lambda: eng.influence_cross_cov_batched(lx, lu, aS, bS, [0.01] * 3, cxS, ws=lw),
        "influence_block_cross_cov": lambda: eng.influence_block_cross_cov(x, u, a, b, 0.01, cx, 7, 3, w=w),
        "perturb": lambda: eng.perturb(x, u, da, freq=freq),
        "perturb_cov": lambda: tuple(eng.perturb_cov(x, u, da, block=7, n_levels=2)),
        "mbar_eval": lambda: eng.mbar_eval(mo["us"], mo["a0"], mo["g"], mo["upiv"]),
        "mbar_predict": lambda: eng.mbar_predict(mo["xs"], mo["us"], mo["a0"], None, mo["logD"], mo["al"], upiv=mo["upiv"]),
        "mbar_cov_sums": lambda: eng.mbar_cov_sums(mo["xs"], mo["us"], mo["a0"], sol, mo["al"], means, with_lnw=True),
        "mbar_boot_eval": lambda: eng.mbar_boot_eval(bo["us"], bo["a0"], bo["sm"], bo["gb"], bo["upiv"]),
        "mbar_bootstrap_predict": lambda: eng.mbar_bootstrap_predict(bo["xs"], bo["us"], bo["a0"], bo["sm"], bo["f"], sol, bo["al"]),
        "lag_sums": lambda: eng.lag_sums(x, u, [0, 2, 7], 0, 256, center=center),
        "lag_origin_sums": lambda: eng.lag_origin_sums(x, u, [0, 3], 100, 0, 256, center=center),
        "lag_sums_batched": lambda: eng.lag_sums_batched(eng.lag_rows_batched(lx, lu, [center] * 3), [(0, 0), (2, 1), (1, 8)], 0, 256),
    }


def _flat(r):
    if isinstance(r, torch.Tensor):
        return [r.detach().cpu().numpy()]
    if isinstance(r, (tuple, list)):
        return [v for t in r for v in _flat(t)]
    return [np.asarray(r)]


def test_engine_asks_for_what_it_uses(eng, monkeypatch):
    """Every engine wrapper that takes a workspace, with ``engine.workspace`` handing out a fresh guard-banded buffer of
    EXACTLY the bytes asked for, full of NaN patterns: no 1 MiB floor, no cache.  A wrapper that sizes with other arguments
    than it calls with gets TXM_ERR_WORKSPACE; each result equals the unpatched one bit for bit; every band is intact."""
    calls = _engine_calls(eng)
    plain = {name: _flat(fn()) for name, fn in calls.items()}
    torch.cuda.synchronize()
    handed: list[tuple[str, Banded]] = []
    current = [""]

    def exact(nbytes, tag="main"):
        b = Banded(int(nbytes), "nan", dtype=U8)
        handed.append((current[0], b))
        return b.payload

    monkeypatch.setattr(eng, "workspace", exact)
    for name, fn in calls.items():
        current[0] = name
        before = len(handed)
        got = _flat(fn())
        torch.cuda.synchronize()
        assert len(handed) > before, f"{name}: took no workspace"
        assert len(got) == len(plain[name])
        for g, p in zip(got, plain[name]):
            assert np.array_equal(g, p, equal_nan=True), f"{name}: differs from the unpatched result"
    for name, b in handed:
        assert b.check(), f"{name}: wrote outside the {b.nbytes} bytes it asked for"
    print(f"\nengine wrappers under an exact-size workspace: {len(calls)} calls, {len(handed)} workspaces, all bands intact")
