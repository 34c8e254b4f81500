"""Device-level calls into libtxmom: torch CUDA tensors in, torch CUDA tensors out.

Thin layer over the C ABI (include/txmom.h): allocates outputs and scratch with
torch, passes raw pointers and the current torch stream, checks status codes.
The labelled-array API that mirrors the reference sits on top (moments.py,
data.py); nothing here knows about dims or names.
"""

from __future__ import annotations

import contextlib
import ctypes as ct
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from ._lib import ResampleOpts, SamplerSpec, check
from ._mbar_host import (_MBAR_MAX_STEP, _MBAR_PINV_CUT, _sym_pinv, mbar_block_coef_mean, mbar_block_coef_sampled,  # noqa: F401
                         mbar_block_coef_target, mbar_block_covariance, mbar_block_variance, mbar_block_width, mbar_hist_covariance, mbar_hist_terms,
                         mbar_hist_variance, mbar_mean_covariance, mbar_mean_variance, mbar_newton, mbar_newton_batched,
                         mbar_overlap, mbar_reduced_pinv, mbar_solution_g, mbar_theta, mbar_unpack_h)
from ._operands import either_layout, resample_pitch_ok, rowmajor_layout  # noqa: F401

F64 = torch.float64
_last_info: dict[tuple[int, int], torch.Tensor] = {}
_ws_cache: dict[tuple[int, int, str], torch.Tensor] = {}


def _L():
    if not _lib.gpu_ready():
        _lib.require_gpu()
    return _lib.load()


def _stream():
    return ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return ct.c_void_p(t.data_ptr()) if t is not None else None


def workspace(nbytes: int, tag: str = "main") -> torch.Tensor:
    """Grow-only scratch buffer per (device, stream, tag): calls issued on different torch streams never
    share scratch, and a buffer is only ever used (and, when it grows, released) on the stream it was
    allocated on, which is what torch's caching allocator assumes."""
    key = (torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream, tag)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = None
        _ws_cache.pop(key, None)
        buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device="cuda")
        _ws_cache[key] = buf
    return buf


_const_cache: "dict" = {}


def const_tensor(values, dtype=F64) -> torch.Tensor:
    """A small constant (a pointer table, the 1 / n! factors, a callback's scalars) as a device tensor, uploaded ONCE per
    (values, dtype, device, stream) from pinned memory without blocking the host, then served from a cache.
    ``torch.tensor(list, device="cuda")`` is a pageable host-to-device copy: the host waits until everything queued on the stream
    before it has run -- in the middle of a step (between the bootstrap launch and the derivative evaluation) that serialises host
    and device and leaves the device idle while the host issues the step's small launches (config 5: 0.4 ms of a 6.2 ms step)."""
    key = (tuple(values), dtype, torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream)
    hit = _const_cache.get(key)
    if hit is None:
        if len(_const_cache) >= 512:          # (bounded: pointer tables of long-lived programs repeat; anything else is transient)
            _const_cache.pop(next(iter(_const_cache)))
        host = torch.tensor(list(values), dtype=dtype).pin_memory()
        hit = _const_cache[key] = (host.to("cuda", non_blocking=True), host)   # (the pinned source lives as long as the entry)
    return hit[0]


def to_device(a, dtype=F64) -> torch.Tensor:
    if isinstance(a, torch.Tensor):
        return a.to(device="cuda", dtype=dtype)
    return torch.as_tensor(np.asarray(a), dtype=dtype).to("cuda")


def _check_f64_cuda(t, name):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == F64):
        raise TypeError(f"{name} must be a float64 CUDA tensor")


# The layout rule of an entry point (_operands.py): "either" layout of reduce_vals; "rowmajor" with a pitch >= C;
# "rowmajor_pitch", the same within TXM_RESAMPLE_PITCH_OK; "tight": always a contiguous array (the batched entry points).
def _layout(x2, rule):
    """(copy, ls, lc) of the (N, C) tensor x2 under ``rule``: the one place that reads a tensor's strides to decide that."""
    N, C = x2.shape
    s0, s1 = x2.stride()
    if rule == "either":
        return either_layout(N, C, s0, s1)
    return (*rowmajor_layout(N, C, s0, s1, rule == "rowmajor_pitch"), 1)


def _place(x2, rule):
    """x2 (N, C) as the library takes it under ``rule``: (tensor, ls, lc) -- x2 itself, or its contiguous copy."""
    if rule == "tight":
        return (x2 if x2.is_contiguous() else x2.contiguous()), x2.shape[1], 1
    copy, ls, lc = _layout(x2, rule)
    return (x2.contiguous() if copy else x2), ls, lc


def _sample_vector(t, name, N):
    """u or w of N samples: checked, contiguous."""
    _check_f64_cuda(t, name)
    if t.shape != (N,):
        raise ValueError(f"{name} must have shape ({N},), got {tuple(t.shape)}")
    return t.contiguous()


def _operands(x, u, w, rule):
    """(x2, ls, lc, u, w, N, C, squeeze) for the sample-matrix entry points: x (N, C) or (N,) placed by ``rule``, u and
    w (N,)."""
    _check_f64_cuda(x, "x")
    squeeze = x.dim() == 1
    x2 = x.unsqueeze(1) if squeeze else x
    if x2.dim() != 2:
        raise ValueError("x must be (N,) or (N, C)")
    N, C = x2.shape
    u = _sample_vector(u, "u", N)
    if w is not None:
        w = _sample_vector(w, "w", N)
    x2, ls, lc = _place(x2, rule)
    return x2, ls, lc, u, w, N, C, squeeze


def _eight_per_pass(values):
    """(i0, chunk) over the targets, 8 per pass over the samples; every chunk a contiguous float64 array."""
    for i0 in range(0, len(values), 8):
        yield i0, np.ascontiguousarray(values[i0:i0 + 8])


def _info_words(cache):
    """The 4 int64 words a bootstrap call reports in, one buffer per (device, stream) in ``cache``."""
    key = (torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream)
    info = cache.get(key)
    if info is None:
        info = cache[key] = torch.zeros(4, dtype=torch.int64, device="cuda")
    return info


def _most_that_fit(need, hi, budget, unit=1):
    """The most of ``hi`` items whose ``need(n)`` bytes (growing with n) fit ``budget``: all of them when they fit or are
    no more than one group of ``unit``, else whole groups of ``unit`` -- at least one, fitting or not."""
    if need(hi) <= budget or hi <= unit:
        return hi
    lo, top = 1, (hi + unit - 1) // unit
    while lo < top:
        mid = (lo + top + 1) // 2
        if need(min(mid * unit, hi)) <= budget:
            lo = mid
        else:
            top = mid - 1
    return min(lo * unit, hi)


# ---------------------------------------------------------------------------
def reduce_vals(x: torch.Tensor, u: torch.Tensor, order: int, w: torch.Tensor | None = None) -> torch.Tensor:
    """x: (N, C) with either stride(1) == 1 or stride(0) == 1 (a transposed view
    of a (C, N) array), or (N,).  Returns (C, 2, K) (or (2, K))."""
    L = _L()
    x2, ls, lc, u, w, N, C, squeeze = _operands(x, u, w, "either")
    out = torch.empty((C, 2, order + 1), dtype=F64, device="cuda")
    nws = L.txm_reduce_vals_ws_bytes(N, C, order)
    ws = workspace(nws)
    check(
        L.txm_reduce_vals(_ptr(x2), ls, lc, _ptr(u), _ptr(w), N, C, order, _ptr(out), _ptr(ws), ws.numel(), _stream()),
        "txm_reduce_vals",
    )
    return out[0] if squeeze else out


def reduce_pivot(x: torch.Tensor, u: torch.Tensor, w: torch.Tensor | None = None) -> torch.Tensor:
    """The library's pivot estimate {pivot_u, pivot_x[...]} for a (shard of a) sample matrix: (1 + C,) -- strided means
    (txm_reduce_vals_pivot), with ``w`` the weighted estimate reduce_vals itself uses (txm_reduce_vals_pivot_w)."""
    L = _L()
    x2, ls, lc, u, w, N, C, _ = _operands(x, u, w, "either")
    piv = torch.empty(1 + C, dtype=F64, device="cuda")
    if w is None:
        check(L.txm_reduce_vals_pivot(_ptr(x2), ls, lc, _ptr(u), N, C, _ptr(piv), _stream()), "txm_reduce_vals_pivot")
    else:
        check(L.txm_reduce_vals_pivot_w(_ptr(x2), ls, lc, _ptr(u), _ptr(w), N, C, _ptr(piv), _stream()),
              "txm_reduce_vals_pivot_w")
    return piv


def reduce_sums(x: torch.Tensor, u: torch.Tensor, order: int, pivot: torch.Tensor, w: torch.Tensor | None = None) -> torch.Tensor:
    """Weight-scaled power sums of the samples about ``pivot``: (C, 2, K) -- sums about one pivot add like the samples
    (txm_reduce_vals_sums): shards of a sample-sharded reduce, chunks of a stream."""
    L = _L()
    x2, ls, lc, u, w, N, C, _ = _operands(x, u, w, "either")
    _check_f64_cuda(pivot, "pivot")
    pivot = pivot.contiguous()
    if pivot.numel() != 1 + C:
        raise ValueError("pivot must have 1 + C entries")
    out = torch.empty((C, 2, order + 1), dtype=F64, device="cuda")
    ws = workspace(L.txm_reduce_vals_ws_bytes(N, C, order))
    check(L.txm_reduce_vals_sums(_ptr(x2), ls, lc, _ptr(u), _ptr(w), N, C, order, _ptr(pivot), _ptr(out), _ptr(ws), ws.numel(),
                                 _stream()), "txm_reduce_vals_sums")
    return out


def sums_to_state(sums: torch.Tensor, pivot: torch.Tensor) -> torch.Tensor:
    """(n, C, 2, K) stacks of sums about ``pivot`` (or one (C, 2, K)) -> the cmomy state (C, 2, K) of all their samples,
    the stacks added in index order (txm_sums_to_state)."""
    L = _L()
    _check_f64_cuda(sums, "sums")
    s = sums.contiguous()
    if s.dim() == 3:
        s = s.unsqueeze(0)
    n, C, two, K = s.shape
    if two != 2 or pivot.numel() != 1 + C:
        raise ValueError("sums must be (n, C, 2, K) with a (1 + C,) pivot")
    out = torch.empty((C, 2, K), dtype=F64, device="cuda")
    check(L.txm_sums_to_state(_ptr(s), n, _ptr(pivot.contiguous()), C, K - 1, _ptr(out), _stream()), "txm_sums_to_state")
    return out


def push_vals(state: torch.Tensor, x: torch.Tensor, u: torch.Tensor, w: torch.Tensor | None = None) -> torch.Tensor:
    """Accumulate the samples (x, u[, w]) into ``state`` (C, 2, K) IN PLACE (cmomy push_vals; zeros = the empty
    accumulator) and return it (txm_push_vals)."""
    L = _L()
    _check_f64_cuda(state, "state")
    x2, ls, lc, u, w, N, C, squeeze = _operands(x, u, w, "either")
    st = state.unsqueeze(0) if (squeeze and state.dim() == 2) else state
    if st.dim() != 3 or st.shape[0] != C or st.shape[1] != 2 or not st.is_contiguous():
        raise ValueError(f"state must be a contiguous ({C}, 2, K) tensor, got {tuple(state.shape)}")
    order = st.shape[2] - 1
    ws = workspace(L.txm_push_vals_ws_bytes(N, C, order))
    check(L.txm_push_vals(_ptr(st), _ptr(x2), ls, lc, _ptr(u), _ptr(w), N, C, order, _ptr(ws), ws.numel(), _stream()),
          "txm_push_vals")
    return state


def reduce_vals_1d(u: torch.Tensor, mom: int, w: torch.Tensor | None = None) -> torch.Tensor:
    """u: (R, N) rows contiguous, or (N,).  Returns (R, mom+1) / (mom+1,)."""
    L = _L()
    _check_f64_cuda(u, "u")
    squeeze = u.dim() == 1
    u2 = u.unsqueeze(0) if squeeze else u
    if u2.stride(1) != 1:
        u2 = u2.contiguous()
    R, N = u2.shape
    if w is not None:
        _check_f64_cuda(w, "w")
        w = w.contiguous()
    M = mom + 1
    out = torch.empty((R, M), dtype=F64, device="cuda")
    ws = workspace(L.txm_reduce_vals_1d_ws_bytes(N, R, M))
    check(
        L.txm_reduce_vals_1d(_ptr(u2), u2.stride(0) if R > 1 else N, 1, _ptr(w), N, R, M, _ptr(out), _ptr(ws),
                             ws.numel(), _stream()),
        "txm_reduce_vals_1d",
    )
    return out[0] if squeeze else out


def indices_to_freq(indices: torch.Tensor, ndat: int | None = None) -> torch.Tensor:
    L = _L()
    idx = indices.to(device="cuda", dtype=torch.int64).contiguous()
    nrep, nsamp = idx.shape
    ndat = nsamp if ndat is None else int(ndat)
    freq = torch.empty((nrep, ndat), dtype=torch.int64, device="cuda")
    ws = workspace(L.txm_indices_to_freq_ws_bytes(), "indices")
    check(L.txm_indices_to_freq(_ptr(idx), nrep, nsamp, ndat, _ptr(freq), _ptr(ws), ws.numel(), _stream()),
          "txm_indices_to_freq")
    return freq


class DeviceSampler:
    """Counter-based exact multinomial sampler (include/txmom.h txm_sampler_*).

    Holds only the per-(replicate, tile) draw counts (uint32, nrep x ceil(ndat/1024));
    the per-sample counts are regenerated inside the bootstrap kernel.

    ``rep0``: row r of this sampler is replicate ``rep0 + r`` of the stream of ``seed`` -- a replicate's draws
    depend on (seed, stream replicate, tile) only, so ``DeviceSampler(seed, b - a, ndat, rep0=a)`` is rows
    ``a:b`` of ``DeviceSampler(seed, n, ndat)`` bit for bit.  That is how replicate slabs and state shards of a
    multi-GPU run reproduce the one-GPU result exactly (distributed.py).
    """

    def __init__(self, seed: int, nrep: int, ndat: int, nsamp: int = 0, rep0: int = 0):
        L = _L()
        self.spec = SamplerSpec(seed=0, nrep=int(nrep), ndat=int(ndat), nsamp=int(nsamp), rep0=int(rep0))
        self.ntiles = int(L.txm_sampler_ntiles(ndat))
        self.counts = torch.empty((nrep, self.ntiles), dtype=torch.int32, device="cuda")  # bit pattern of uint32
        self._nws = L.txm_sampler_counts_ws_bytes(ct.byref(self.spec))
        if self._nws == 0:
            raise _lib.TxmError(f"sampler spec rejected: {_lib.last_error()}")
        self.draw(seed)

    def draw(self, seed: int) -> "DeviceSampler":
        """(Re)draw the tile counts for a new seed, reusing the buffers."""
        L = _L()
        self.spec.seed = int(seed) & (2**64 - 1)
        ws = workspace(self._nws, "sampler")
        check(
            L.txm_sampler_tile_counts(ct.byref(self.spec), _ptr(self.counts), _ptr(ws), ws.numel(), _stream()),
            "txm_sampler_tile_counts",
        )
        return self

    @property
    def seed(self):
        return self.spec.seed

    @property
    def nrep(self):
        return self.spec.nrep

    @property
    def ndat(self):
        return self.spec.ndat

    @property
    def rep0(self):
        return self.spec.rep0

    def rows(self, a: int, b: int) -> "DeviceSampler":
        """Replicates [a, b) of this sampler as a sampler of their own (a view: the same count rows, stream offset rep0 + a)."""
        if not 0 <= a < b <= self.spec.nrep:
            raise ValueError(f"rows [{a}, {b}) outside [0, {self.spec.nrep})")
        v = object.__new__(DeviceSampler)
        v.spec = SamplerSpec(seed=self.spec.seed, nrep=b - a, ndat=self.spec.ndat, nsamp=self.spec.nsamp, rep0=self.spec.rep0 + a)
        v.ntiles, v.counts, v._nws = self.ntiles, self.counts[a:b], self._nws
        return v

    def freq(self) -> torch.Tensor:
        L = _L()
        out = torch.empty((self.spec.nrep, self.spec.ndat), dtype=torch.int64, device="cuda")
        check(L.txm_sampler_freq(ct.byref(self.spec), _ptr(self.counts), _ptr(out), _stream()), "txm_sampler_freq")
        return out


class ResamplePrep:
    """Persistent pre-pass block of the int8 bootstrap path for ONE set of sample arrays
    (txm_resample_opts.prep): pivot, per-window scale table, guard flags and the FP64 fallback list depend on
    (x, u, w, pivot, N, C, nrep, order) only, so a bootstrap loop over the same data computes them once.  The
    reference caches per data object the same way (data.py:285, 844-942).

    The key is built from the CALLER's tensors (storage pointer, torch version counter, shape, strides) -- not from the
    contiguous temporaries a call may have to make -- plus (N, C, order) and the KERNEL WORD of the call
    (txm_resample_kernel: fused / count-table kernel, and whether it carries a second matrix -- a block holds y's tables only
    then); the block keeps strong references to the tensors, so their storage cannot be recycled under the key; the
    temporaries themselves are kept here and reused with the tables.  An in-place edit of a sample array through torch,
    another shape, or a replicate count that the dispatch rule sends to another kernel therefore invalidates the block (the
    replicate slabs of one call and calls with other counts on the same kernel share it); so does ``new_like`` on the
    owning data object (a fresh cache).  What torch cannot see -- another library writing the
    samples through a raw pointer -- does not bump a version counter: call ``invalidate()`` after such a write (the C
    ABI has no such state: ``prep_valid`` there is the caller's own statement)."""

    def __init__(self):
        self.buf: torch.Tensor | None = None
        self.key = None
        self.refs = None     # the caller's tensors the key describes
        self.tensors = None  # what the kernels were given: (x2, u, w, pivot, y2), contiguous copies where needed
        self.hits = 0
        self.misses = 0

    def lookup(self, key):
        """The kernel operands of the last committed call if ``key`` still describes it, else None."""
        return self.tensors if (key is not None and self.key == key and self.buf is not None) else None

    def bind(self, key, nbytes: int) -> tuple[torch.Tensor, bool]:
        valid = self.key == key and self.buf is not None and self.buf.numel() >= nbytes
        if not valid:
            if self.buf is None or self.buf.numel() < nbytes:
                self.buf = torch.empty(int(nbytes), dtype=torch.uint8, device="cuda")
            self.key = None  # set by commit() once the call that fills the block has been issued
            self.refs = self.tensors = None
            self.misses += 1
        else:
            self.hits += 1
        return self.buf, valid

    def commit(self, key, refs=None, tensors=None):
        self.key = key
        self.refs, self.tensors = refs, tensors

    def invalidate(self):
        """Forget the tables (and the cached operand copies): the next call recomputes them.  Needed only after a write
        to the sample arrays that torch's version counters do not see."""
        self.key = None
        self.refs = self.tensors = None


def _tkey(t):
    return None if t is None else (t.data_ptr(), t._version, tuple(t.shape), tuple(t.stride()))


# Workspace of ONE library call of the device-sampler bootstrap (partial sums per scaling window, and the int8 path's count
# table: one byte per replicate and sample) grows with nrep -- 3.9 GB + 102 GB at N = 1e8, nrep = 1000; ten times that at
# nrep = 1e4.  resample_vals bounds it by bootstrapping the replicates in slabs of whole 128-replicate groups: rows [a, b) of
# a call equal the (b - a)-replicate call at rep0 = a BIT FOR BIT (txm_sampler_spec.rep0), so the slabs ARE the rows of the
# unslabbed result.  None: 45 % of the device's memory, at most 80 % of what is free at the first call.
WORKSPACE_BUDGET_BYTES: int | None = None
_budget_default: dict[int, int] = {}


def workspace_budget() -> int:
    if WORKSPACE_BUDGET_BYTES is not None:
        return int(WORKSPACE_BUDGET_BYTES)
    dev = torch.cuda.current_device()
    if dev not in _budget_default:
        free, total = torch.cuda.mem_get_info(dev)
        _budget_default[dev] = int(min(0.45 * total, 0.8 * free))
    return _budget_default[dev]


def _slab_size(L, N, C, nrep, order, path, has_y) -> int:
    """Replicates per library call: all of them when the call's workspace fits the budget, else the largest multiple of 128
    that does (at least 128)."""
    need = lambda n: L.txm_resample_vals_ws_bytes_opts(N, C, n, order, path, int(has_y)) + (L.txm_resample_y_ws_bytes(N, C, n) if has_y else 0)  # noqa: E731
    return _most_that_fit(need, nrep, workspace_budget(), unit=128)


def _call_path(path) -> int:
    """The kernel one device-sampler call takes: an explicit path, else the forced_path() context, else the
    library's shape rule (txm_resample_path, which honours txm_set_resample_path)."""
    eff = path if path is not None else _forced
    if eff in ("fp64", "int8", "int8_fused", "int8_table"):
        return _PATHS[eff]
    return -1


def _table_operands_ok(x2: torch.Tensor, ls: int, C: int, y: torch.Tensor | None) -> bool:
    """txm_resample_kernel's `aligned` for the operands a call will hand the library (the library's own statement of what the
    count-table kernel's DMA needs: txm_resample_operands_aligned).  A second matrix that resample_vals will have to copy
    (not row-major with unit column stride) is judged as the contiguous copy it becomes: pitch C, torch's 256-byte alignment."""
    L = _L()
    yp, ldy = None, 0
    if y is not None:
        y2 = y.unsqueeze(1) if y.dim() == 1 else y
        copy, ldy, _ = _layout(y2, "rowmajor_pitch") if y2.dim() == 2 else (True, C, 1)
        # (an address with torch's allocation alignment stands in for the copy's)
        yp = ct.c_void_p(256 if copy else y2.data_ptr())
    return L.txm_resample_operands_aligned(ct.c_void_p(x2.data_ptr()), ls, C, yp, ldy) == 1


def resample_vals(
    x: torch.Tensor,
    u: torch.Tensor,
    order: int,
    *,
    freq: torch.Tensor | None = None,
    sampler: DeviceSampler | None = None,
    w: torch.Tensor | None = None,
    pivot: torch.Tensor | None = None,
    out: torch.Tensor | None = None,
    path: str | None = None,
    prep: ResamplePrep | None = None,
    info: torch.Tensor | None = None,
    y: torch.Tensor | None = None,
    prep_src: tuple | None = None,
    _slab: int | None = None,
):
    """(nrep, C, 2, K) bootstrap states; x is (N, C) row-major (or (N,)).

    ``path``: "fp64" / "int8" for THIS call (None: the forced_path() context, else the library's rule).
    ``prep``: a ResamplePrep kept by the caller next to the data -- the int8 path's pre-pass is then computed once.
    ``prep_src``: the tensors the block's key should describe when x / u / w are themselves temporaries of the caller
    (default: the arguments as given, before any contiguous copy made here).
    ``info``: an int64 CUDA tensor of 4 words the library fills on the stream (path, windows, windows the guard
    sent to the FP64 kernel, tables reused) -- no synchronisation.
    ``y``: a second (N, C) sample matrix; returns ``(states, ymean)`` with ymean (nrep, C) = the per-replicate
    weighted mean of y on the same draw (VolumeDataCallback's <dx/dq>, reference volume.py:121-134)."""
    L = _L()
    # the key of a caller-held pre-pass block describes the CALLER's tensors; the copies made below are kept with it
    src = tuple(prep_src) if prep_src is not None else (x, u, w, pivot, y)
    # the kernels want (rec, val) row-major with a row pitch >= C that their 32-bit offsets hold (TXM_RESAMPLE_PITCH_OK)
    x2, ls, _, u, w, N, C, squeeze = _operands(x, u, w, "rowmajor_pitch")
    src_key = tuple(_tkey(t) for t in src)
    if (freq is None) == (sampler is None):
        raise ValueError("give exactly one of freq= or sampler=")
    if freq is not None:
        freq = freq.to(device="cuda", dtype=torch.int64).contiguous()
        if freq.dim() != 2 or freq.shape[1] != N:
            raise ValueError(f"freq must be (nrep, {N}), got {tuple(freq.shape)}")
        nrep = freq.shape[0]
        spec_p, counts_p = None, None
    else:
        if sampler.ndat != N:
            raise ValueError(f"sampler.ndat={sampler.ndat} must equal N={N}")
        nrep = sampler.nrep
        spec_p, counts_p = ct.byref(sampler.spec), _ptr(sampler.counts)
    if pivot is not None:
        _check_f64_cuda(pivot, "pivot")
        pivot = pivot.contiguous()
        if pivot.numel() != 1 + C:
            raise ValueError("pivot must have 1 + C entries")
    if out is None:
        out = torch.empty((nrep, C, 2, order + 1), dtype=F64, device="cuda")
    else:
        _check_f64_cuda(out, "out")
        if tuple(out.shape) != (nrep, C, 2, order + 1) or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous ({nrep}, {C}, 2, {order + 1}) tensor, got {tuple(out.shape)}")
    opts = ResampleOpts()
    opts.path = _slab if _slab is not None else _call_path(path)
    kern = -1
    if sampler is not None:
        # the contraction kernel this call runs (FP64 / int8 fused / int8 count table) and whether it carries y: decided ONCE,
        # for the whole call -- the rule looks at nrep, and neither a replicate slab nor a later call on the same pre-pass block
        # may fall on the other side of one of its thresholds (a block holds y's tables only when the kernel carries y)
        kern = L.txm_resample_kernel(N, C, nrep, order, opts.path, int(y is not None), int(_table_operands_ok(x2, ls, C, y)))
    if sampler is not None and _slab is None:
        slab = _slab_size(L, N, C, nrep, order, kern & 0xFF, y is not None)
        if slab < nrep:
            # replicate slabs: every slab is an ordinary call on its rows of the sampler with the whole call's kernel as its path
            ym = torch.empty((nrep, C), dtype=F64, device="cuda") if y is not None else None
            for a in range(0, nrep, slab):
                b = min(nrep, a + slab)
                r = resample_vals(x, u, order, sampler=sampler.rows(a, b), w=w, pivot=pivot, out=out[a:b], prep=prep,
                                  info=info, y=y, prep_src=prep_src if prep_src is not None else (x, u, w, pivot, y),
                                  _slab=kern & 0xFF)
                if y is not None:
                    ym[a:b] = r[1] if y.dim() > 1 else r[1][:, None]
            res = out[:, 0] if squeeze else out
            return (res, (ym[:, 0] if y.dim() == 1 else ym)) if y is not None else res
    ymean = y2 = None
    if y is not None:
        _check_f64_cuda(y, "y")
        y2 = y.unsqueeze(1) if y.dim() == 1 else y
        if tuple(y2.shape) != (N, C):
            raise ValueError(f"y must have the shape of x, ({N}, {C}); got {tuple(y2.shape)}")
        y2, ldy, _ = _place(y2, "rowmajor_pitch")
        ymean = torch.empty((nrep, C), dtype=F64, device="cuda")
        opts.y, opts.ldy_s, opts.out_y = y2.data_ptr(), ldy, ymean.data_ptr()
    key = None
    if prep is not None and freq is None:
        if (kern & 0xFF) != _PATHS["fp64"]:
            # the block holds pivot, window table, guard flags and fallback list of the caller's tensors -- and the second
            # matrix's tables exactly when the call's kernel carries y (txm_resample_kernel's WITH_Y bit; narrow tail groups
            # follow it too).  So the key is the kernel word, not nrep and not the path the caller asked for: the replicate
            # slabs of one call share the block, a call with another count shares it when the rule gives it the same kernel,
            # and gets a block of its own when it does not (order 4 with y: fused below two replicate groups, table above)
            key = (src_key, N, C, order, kern)
            kept = prep.lookup(key)
            if kept is not None:  # same caller tensors, unedited: the operands of the call that filled the block
                x2, u, w, pivot, y2 = kept   # (placed already: the rule passes them through and gives their pitch)
                x2, ls, _ = _place(x2, "rowmajor_pitch")
                if y2 is not None:
                    y2, opts.ldy_s, _ = _place(y2, "rowmajor_pitch")
                    opts.y = y2.data_ptr()
            buf, valid = prep.bind(key, L.txm_resample_prep_bytes(N, C, nrep, order))
            opts.prep, opts.prep_bytes, opts.prep_valid = buf.data_ptr(), buf.numel(), int(valid)
    if info is None:  # the words resample_info() reads back
        info = _info_words(_last_info)
    if not (info.is_cuda and info.dtype == torch.int64 and info.numel() >= 4 and info.is_contiguous()):
        raise TypeError("info must be a contiguous int64 CUDA tensor with >= 4 elements")
    opts.info = info.data_ptr()
    ws = workspace(L.txm_resample_vals_ws_bytes_opts(N, C, nrep, order, opts.path, int(y is not None))
                   + (L.txm_resample_y_ws_bytes(N, C, nrep) if y is not None else 0))
    check(
        L.txm_resample_vals(_ptr(x2), ls, 1, _ptr(u), _ptr(w), N, C, order, nrep, _ptr(freq), spec_p, counts_p,
                            _ptr(pivot), _ptr(out), ct.byref(opts), _ptr(ws), ws.numel(), _stream()),
        "txm_resample_vals",
    )
    if key is not None:
        prep.commit(key, refs=src, tensors=(x2, u, w, pivot, y2))
    res = out[:, 0] if squeeze else out
    if y is not None:
        return res, (ymean[:, 0] if y.dim() == 1 else ymean)
    return res


def _state_table(xs, us, ws):
    """Validate S state points of one shape and build the host pointer table of the batched entry points."""
    S = len(xs)
    if S < 1 or len(us) != S or (ws is not None and len(ws) != S):
        raise ValueError("need the same number (>= 1) of x, u (and w) tensors")
    x2 = []
    for x in xs:
        _check_f64_cuda(x, "x")
        x = x.unsqueeze(1) if x.dim() == 1 else x
        if x.dim() != 2:
            raise ValueError("every x must be (N,) or (N, C)")
        x2.append(_place(x, "tight")[0])   # (the table carries one pitch for all states: C)
    N, C = x2[0].shape
    if any(tuple(x.shape) != (N, C) for x in x2):
        raise ValueError("the batched path needs states of one shape (N, C)")
    u2 = [_sample_vector(u, "u", N) for u in us]
    w2 = None if ws is None else [_sample_vector(w, "w", N) for w in ws]
    tab = (_lib.StatePtrs * S)()
    for s in range(S):
        tab[s].x, tab[s].u = x2[s].data_ptr(), u2[s].data_ptr()
        tab[s].w = w2[s].data_ptr() if w2 is not None else None
    return tab, (x2, u2, w2), S, N, C


def reduce_vals_batched(xs, us, order: int, ws=None) -> torch.Tensor:
    """S state points of one shape in one launch per kernel (txm_reduce_vals_batched): (S, C, 2, K)."""
    L = _L()
    tab, keep, S, N, C = _state_table(xs, us, ws)
    out = torch.empty((S, C, 2, order + 1), dtype=F64, device="cuda")
    wsb = workspace(L.txm_reduce_vals_batched_ws_bytes(S, N, C, order))
    check(L.txm_reduce_vals_batched(tab, S, C, N, C, order, _ptr(out), _ptr(wsb), wsb.numel(), _stream()),
          "txm_reduce_vals_batched")
    del keep
    return out[:, 0] if xs[0].dim() == 1 else out


def resample_vals_batched(xs, us, order: int, *, nrep: int, sampler: DeviceSampler | None = None,
                          freq: torch.Tensor | None = None, ws=None, path: str | None = None,
                          prep: ResamplePrep | None = None) -> torch.Tensor:
    """Bootstrap of S state points of one shape in one launch per kernel (txm_resample_vals_batched_opts):
    (S, nrep, C, 2, K).  `sampler`: ONE DeviceSampler over S * nrep replicates of N samples (state s owns
    replicates s * nrep ...), or `freq`: (S * nrep, N) explicit counts.

    Narrow states (C <= 16) take the int8 path with the state on a grid axis of every kernel of it -- state s of the
    result is, bit for bit, the single call on state s with ``rep0 + s * nrep``.  ``path``: "fp64" / "int8" for THIS call
    (None: the forced_path() context, else the library's rule).  ``prep``: a ResamplePrep the caller keeps next to the
    collection -- the int8 path's pre-pass over the S states is then computed once (keyed on the callers' tensors)."""
    L = _L()
    src = (tuple(xs), tuple(us), None if ws is None else tuple(ws))
    tab, keep, S, N, C = _state_table(xs, us, ws)
    if (freq is None) == (sampler is None):
        raise ValueError("give exactly one of freq= or sampler=")
    spec_p = counts_p = None
    if freq is not None:
        freq = freq.to(device="cuda", dtype=torch.int64).contiguous()
        if tuple(freq.shape) != (S * nrep, N):
            raise ValueError(f"freq must be ({S * nrep}, {N}), got {tuple(freq.shape)}")
    else:
        if sampler.ndat != N or sampler.nrep != S * nrep:
            raise ValueError(f"the sampler must span {S} x {nrep} replicates of {N} samples")
        spec_p, counts_p = ct.byref(sampler.spec), _ptr(sampler.counts)
    out = torch.empty((S, nrep, C, 2, order + 1), dtype=F64, device="cuda")
    opts = _lib.ResampleOpts()
    opts.path = _call_path(path)
    key = None
    if prep is not None and freq is None:
        nb = L.txm_resample_batched_prep_bytes(S, N, C, nrep, order)
        # bind (and afterwards commit) the block only when THIS call runs the int8 path -- the library's own predicates, as the
        # single call does: a call that ran the FP64 kernel never fills the block, and a later int8 call would read it as valid
        takes_i8 = bool(nb) and (opts.path in (1, 2, 3) or (opts.path == -1 and L.txm_resample_batched_path(S, N, C, nrep, order) == 1))
        if takes_i8:
            key = (tuple(_tkey(t) for t in src[0]), tuple(_tkey(t) for t in src[1]),
                   None if src[2] is None else tuple(_tkey(t) for t in src[2]), S, N, C, nrep, order)
            kept = prep.lookup(key)
            if kept is not None:  # the operand copies of the call that filled the block
                tab, keep = kept
            buf, valid = prep.bind(key, nb)
            opts.prep, opts.prep_bytes, opts.prep_valid = buf.data_ptr(), buf.numel(), int(valid)
    opts.info = _info_words(_last_batched_info).data_ptr()  # the words batched_info() reads back
    wsb = workspace(L.txm_resample_vals_batched_ws_bytes(S, N, C, nrep, order))
    check(L.txm_resample_vals_batched_opts(tab, S, C, N, C, order, nrep, _ptr(freq), spec_p, counts_p, _ptr(out), ct.byref(opts),
                                           _ptr(wsb), wsb.numel(), _stream()), "txm_resample_vals_batched_opts")
    if key is not None:
        prep.commit(key, refs=src, tensors=(tab, keep))
    del keep
    return out[:, :, 0] if xs[0].dim() == 1 else out


_last_batched_info: dict = {}


def batched_info() -> dict:
    """What the last `resample_vals_batched` call on the current stream did (synchronises): {"path", "windows" (scaling
    windows x states), "windows_fp64" (how many of them the precision guard sent to the FP64 kernel), "prep_reused"}."""
    info = _last_batched_info.get((torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream))
    if info is None:
        return {}
    v = info.cpu().tolist()
    return {"path": "int8" if v[0] == 1 else "fp64", "windows": int(v[1]), "windows_fp64": int(v[2]), "prep_reused": bool(v[3] & 1)}


def resample_path(N: int, C: int, nrep: int, order: int) -> str:
    """Which kernel the device-sampler bootstrap takes for this shape: "fp64" or "int8" (inside a forced_path()
    context: that path wherever the int8 kernel supports the shape)."""
    L = _L()
    if _forced == "fp64":
        return "fp64"
    if _forced in ("int8", "int8_fused", "int8_table"):  # wherever the int8 kernel supports the shape: the library's own predicate
        return "int8" if L.txm_resample_i8_supported(int(N), int(C), int(nrep), int(order)) == 1 else "fp64"
    return "int8" if L.txm_resample_path(int(N), int(C), int(nrep), int(order)) == 1 else "fp64"


_PATHS = {None: -1, "auto": -1, "fp64": 0, "int8": 1, "int8_fused": 2, "int8_table": 3}
_forced: str | None = None


@contextlib.contextmanager
def forced_path(path: str | None):
    """Force the FP64 ("fp64") or the int8-sliced ("int8") bootstrap kernel wherever it applies, for the calls
    made inside the context; None / "auto" is the library's own choice.  The path travels with every call
    (txm_resample_opts.path): no process-global library state is touched.  For tests and benchmarks: the automatic
    choice plus the precision guard is what users get."""
    global _forced
    if path not in _PATHS:
        raise ValueError(f"path must be one of {sorted(k for k in _PATHS if k)} or None")
    _L()
    prev = _forced
    _forced = None if path == "auto" else path
    try:
        yield
    finally:
        _forced = prev


def resample_info(N: int | None = None, C: int | None = None, nrep: int | None = None, order: int | None = None) -> dict:
    """What the last `resample_vals` call on the current stream did: {"path", "windows", "windows_fp64",
    "prep_reused", "kernel"} -- "kernel": which contraction served the wide column groups ("int8_table" / "int8_fused" / "fp64"); "windows_fp64" counts the scaling windows (x column groups) that the precision guard of the
    int8 path handed to the FP64 kernel.  Reads the info words the library wrote on the stream
    (txm_resample_opts.info); synchronises.  The shape arguments are accepted for compatibility and ignored."""
    _L()
    info = _last_info.get((torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream))
    if info is None:
        raise RuntimeError("no resample_vals call has been made on this stream")
    v = info.cpu().tolist()
    return {"path": "int8" if v[0] == 1 else "fp64", "windows": int(v[1]), "windows_fp64": int(v[2]),
            "prep_reused": bool(v[3] & 1), "kernel": ("fp64" if v[0] != 1 else "int8_table" if v[3] & 2 else "int8_fused")}


def resample_data(data: torch.Tensor, freq: torch.Tensor | None, order: int) -> torch.Tensor:
    """data (nrec, C, 2, K); freq (nrep, nrec) or None (plain reduce) -> (nrep, C, 2, K)."""
    L = _L()
    _check_f64_cuda(data, "data")
    data = data.contiguous()
    nrec, C = data.shape[:2]
    if data.shape[2:] != (2, order + 1):
        raise ValueError("data must be (nrec, C, 2, order+1)")
    if freq is not None:
        freq = freq.to(device="cuda", dtype=torch.int64).contiguous()
        if freq.shape[1] != nrec:
            raise ValueError("freq must be (nrep, nrec)")
        nrep = freq.shape[0]
    else:
        nrep = 1
    out = torch.empty((nrep, C, 2, order + 1), dtype=F64, device="cuda")
    ws = workspace(L.txm_resample_data_ws_bytes(nrec, C, order))
    check(
        L.txm_resample_data(_ptr(data), _ptr(freq), nrec, C, nrep, order, _ptr(out), _ptr(ws), ws.numel(), _stream()),
        "txm_resample_data",
    )
    return out


def convert_cov(states: torch.Tensor, to_central: bool) -> torch.Tensor:
    L = _L()
    _check_f64_cuda(states, "states")
    s = states.contiguous()
    K = s.shape[-1]
    if s.shape[-2] != 2:
        raise ValueError("states must be (..., 2, K)")
    out = torch.empty_like(s)
    check(L.txm_convert_cov(_ptr(s), _ptr(out), s.numel() // (2 * K), K - 1, int(to_central), _stream()),
          "txm_convert_cov")
    return out


def convert_1d(states: torch.Tensor, to_central: bool) -> torch.Tensor:
    L = _L()
    _check_f64_cuda(states, "states")
    s = states.contiguous()
    M = s.shape[-1]
    out = torch.empty_like(s)
    check(L.txm_convert_1d(_ptr(s), _ptr(out), s.numel() // M, M, int(to_central), _stream()), "txm_convert_1d")
    return out


def cov_over_rep(vals: torch.Tensor) -> torch.Tensor:
    """vals (n_ord, nrep, nval) -> (nval, n_ord, n_ord), ddof = 1 (numpy.cov over replicates)."""
    L = _L()
    _check_f64_cuda(vals, "vals")
    v = vals.contiguous()
    n_ord, nrep, nval = v.shape
    out = torch.empty((nval, n_ord, n_ord), dtype=F64, device="cuda")
    check(L.txm_cov_over_rep(_ptr(v), n_ord, nrep, nval, _ptr(out), _stream()), "txm_cov_over_rep")
    return out


# ---- shared pieces of the six influence entry points ---------------------------------------------------------------------
CROSS_COV_MAX_COLUMNS = 255  # include/txmom.h (f-12): C + 1 logical columns in at most 16 tiles a side


def _influence_coefs(a, b, center_x, lead):
    """``(a, b, center_x, n_f, n_q)``, checked and contiguous: a, b ``(*lead, n_f, n_q)`` and center_x ``lead``, with
    ``lead = (C,)`` for one state -- the ``a.dim() != 3 or a.shape[0] != C`` check -- and ``(S, C)`` for a batch."""
    for t, name in ((a, "a"), (b, "b"), (center_x, "center_x")):
        _check_f64_cuda(t, name)
    if a.dim() != len(lead) + 2 or tuple(a.shape[:len(lead)]) != lead or b.shape != a.shape:
        raise ValueError(f"a and b must both have shape {str(lead)[:-1].rstrip(',')}, n_f, n_q), got {tuple(a.shape)} and "
                         f"{tuple(b.shape)}")
    if tuple(center_x.shape) != lead:
        raise ValueError(f"center_x must have shape {lead}, got {tuple(center_x.shape)}")
    return a.contiguous(), b.contiguous(), center_x.contiguous(), a.shape[-2], a.shape[-1]


def _check_cross_columns(fn, C, per=""):
    if C > CROSS_COV_MAX_COLUMNS:
        raise ValueError(f"{fn}: C = {C} columns, the limit is {CROSS_COV_MAX_COLUMNS} (the result has (C n_f)^2 entries{per})")


def _block_levels_args(block, n_levels):
    block, n_levels = int(block), int(n_levels)
    if block < 1 or not 1 <= n_levels <= 32:
        raise ValueError(f"need block >= 1 and 1 <= n_levels <= 32, got block={block}, n_levels={n_levels}")
    return block, n_levels


def _influence_states(xs, us, ws, rule):
    """``(ops, ws, S, C, pitches, tab)`` of a batched call: ``_operands`` of every state under ``rule`` (ws None when no
    state has weights), the set of the states' row pitches (one entry: one launch can serve them) and the filled
    ``_lib.InfState`` table."""
    S = len(xs)
    if S < 1 or len(us) != S or (ws is not None and len(ws) != S):
        raise ValueError("need the same number (>= 1) of x, u (and w) tensors")
    if ws is not None and any(w is None for w in ws) and not all(w is None for w in ws):
        raise ValueError("weights for all states or for none")
    if ws is not None and ws[0] is None:
        ws = None
    ops = [_operands(xs[s], us[s], None if ws is None else ws[s], rule) for s in range(S)]
    C = ops[0][6]
    if any(o[6] != C for o in ops):
        raise ValueError("every x must have the same number of columns")
    # (x2, ls, lc, u, w, N, C, squeeze) per state: a one-row state has no pitch of its own
    pitches = {o[1] for o in ops if o[5] > 1} or {ops[0][1]}
    tab = (_lib.InfState * S)()
    for s, (x2, _, _, u, w, N, _, _) in enumerate(ops):
        tab[s].x, tab[s].u, tab[s].n = x2.data_ptr(), u.data_ptr(), N
        tab[s].w = w.data_ptr() if w is not None else None
    return ops, ws, S, C, pitches, tab


def _center_u_device(center_u, S):
    cu_dev = center_u.contiguous() if isinstance(center_u, torch.Tensor) else to_device(np.asarray(center_u, dtype=np.float64))
    _check_f64_cuda(cu_dev, "center_u")
    if tuple(cu_dev.shape) != (S,):
        raise ValueError(f"center_u must hold {S} values, got shape {tuple(cu_dev.shape)}")
    return cu_dev


def _center_u_host(center_u):
    return center_u.cpu().numpy() if isinstance(center_u, torch.Tensor) else np.asarray(center_u, dtype=np.float64)


def influence_cov(x: torch.Tensor, u: torch.Tensor, a: torch.Tensor, b: torch.Tensor, center_u: float,
                  center_x: torch.Tensor, w: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """Delta-method covariance of n_f estimates per column from their influence polynomials (txm_influence_cov):
    ``psi_k = sum_q (a[c, k, q] + b[c, k, q] dx) du^q`` with ``dx = x[:, c] - center_x[c]``, ``du = u - center_u``.
    x: (N, C) in either layout of reduce_vals, or (N,); a, b: (C, n_f, n_q); center_x: (C,).
    Returns ``(cov [C, n_f, n_f], mean [C, n_f])`` on the device: ``sum w^2 psi_i psi_j / (sum w)^2`` and
    ``sum w psi_k / sum w``.  One pass over x."""
    L = _L()
    x2, ls, lc, u, w, N, C, _ = _operands(x, u, w, "either")
    a, b, center_x, n_f, n_q = _influence_coefs(a, b, center_x, (C,))
    cov = torch.empty((C, n_f, n_f), dtype=F64, device="cuda")
    mean = torch.empty((C, n_f), dtype=F64, device="cuda")
    ws = workspace(L.txm_influence_cov_ws_bytes(N, C, n_q))
    check(
        L.txm_influence_cov(_ptr(x2), ls, lc, _ptr(u), _ptr(w), N, C, n_f, n_q, float(center_u), _ptr(center_x), _ptr(a),
                            _ptr(b), _ptr(cov), _ptr(mean), _ptr(ws), ws.numel(), _stream()),
        "txm_influence_cov",
    )
    return cov, mean


def influence_cov_batched(xs, us, a: torch.Tensor, b: torch.Tensor, center_u, center_x: torch.Tensor,
                          ws=None) -> tuple[torch.Tensor, torch.Tensor]:
    """``influence_cov`` of S independent states in ONE launch per kernel (txm_influence_cov_batched): state s of the
    result is, bit for bit, ``influence_cov(xs[s], us[s], a[s], b[s], center_u[s], center_x[s], w=ws[s])``.
    xs[s]: (n_s, C) or (n_s,), us[s] (and ws[s]): (n_s,) -- the sample count may differ from state to state; a, b:
    (S, C, n_f, n_q); center_u: S host floats or an (S,) tensor; center_x: (S, C).
    Returns ``(cov [S, C, n_f, n_f], mean [S, C, n_f])`` on the device.

    The one launch needs every x row-major with one pitch (a single series each when C == 1) and all x alike in 16-byte
    alignment; otherwise the single call would pick another kernel for some state, and this loops over ``influence_cov``
    so that the promise above holds."""
    L = _L()
    ops, ws, S, C, pitches, tab = _influence_states(xs, us, ws, "either")
    a, b, center_x, n_f, n_q = _influence_coefs(a, b, center_x, (S, C))
    cu_dev = _center_u_device(center_u, S)
    one_launch = (all(o[2] == 1 for o in ops) and len(pitches) == 1
                  and len({o[0].data_ptr() & 15 == 0 for o in ops}) == 1)
    if not one_launch:
        cu_host = _center_u_host(center_u)
        parts = [influence_cov(xs[s], us[s], a[s], b[s], float(cu_host[s]), center_x[s], w=None if ws is None else ws[s])
                 for s in range(S)]
        return torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts])

    cov = torch.empty((S, C, n_f, n_f), dtype=F64, device="cuda")
    mean = torch.empty((S, C, n_f), dtype=F64, device="cuda")
    wsb = workspace(L.txm_influence_cov_batched_ws_bytes(S, max(o[5] for o in ops), C, n_q))
    check(
        L.txm_influence_cov_batched(tab, S, pitches.pop(), C, n_f, n_q, _ptr(cu_dev), _ptr(center_x), _ptr(a), _ptr(b),
                                    _ptr(cov), _ptr(mean), _ptr(wsb), wsb.numel(), _stream()),
        "txm_influence_cov_batched",
    )
    del ops
    return cov, mean


def block_levels(n: int, block: int) -> tuple[np.ndarray, np.ndarray]:
    """The levels of a blocking curve over ``n`` records from block length ``block``: ``(block_lengths, n_blocks)``
    with ``block_lengths[l] = block * 2**l`` and ``n_blocks[l] = ceil(n / block_lengths[l])`` -- a last short block is
    kept -- for every level that still has at least two blocks (at most 32).  Host logic."""
    n, block = int(n), int(block)
    if block < 1 or 2 * block > n:
        raise ValueError(f"block must satisfy 1 <= block and 2 * block <= N = {n} (at least two blocks), got {block}")
    lengths, counts = [], []
    b = block
    while -(-n // b) >= 2 and len(lengths) < 32:
        lengths.append(b)
        counts.append(-(-n // b))
        b *= 2
    return np.asarray(lengths, dtype=np.int64), np.asarray(counts, dtype=np.int64)


def influence_block_cov(x: torch.Tensor, u: torch.Tensor, a: torch.Tensor, b: torch.Tensor, center_u: float,
                        center_x: torch.Tensor, block: int, n_levels: int = 1,
                        w: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """Blocked (batch-means) delta-method covariance for a correlated series (txm_influence_block_cov): with psi_k as in
    ``influence_cov`` and p = w / sum w, ``cov[l, c] = sum_j z_j z_j'`` over the sums ``z_j = sum_{n in block j} p_n psi(n)``
    of the contiguous blocks of ``block * 2**l`` rows (a last short block is kept; no nb / (nb - 1) factor, so
    ``block=1`` is ``influence_cov``'s result).  x: (N, C) or (N,), copied to row-major if it is not; a, b:
    (C, n_f, n_q); center_x: (C,).  Returns ``(cov [n_levels, C, n_f, n_f], mean [C, n_f])`` on the device from one
    pass over x."""
    L = _L()
    x2, ls, _, u, w, N, C, _ = _operands(x, u, w, "rowmajor")
    a, b, center_x, n_f, n_q = _influence_coefs(a, b, center_x, (C,))
    block, n_levels = _block_levels_args(block, n_levels)
    cov = torch.empty((n_levels, C, n_f, n_f), dtype=F64, device="cuda")
    mean = torch.empty((C, n_f), dtype=F64, device="cuda")
    ws = workspace(L.txm_influence_block_cov_ws_bytes(N, C, n_f, n_q, block))
    check(
        L.txm_influence_block_cov(_ptr(x2), ls, _ptr(u), _ptr(w), N, C, n_f, n_q, float(center_u), _ptr(center_x), _ptr(a),
                                  _ptr(b), block, n_levels, _ptr(cov), _ptr(mean), _ptr(ws), ws.numel(), _stream()),
        "txm_influence_block_cov",
    )
    return cov, mean


def influence_cross_cov(x: torch.Tensor, u: torch.Tensor, a: torch.Tensor, b: torch.Tensor, center_u: float,
                        center_x: torch.Tensor, w: torch.Tensor | None = None) -> torch.Tensor:
    """Delta-method covariance ACROSS the columns (txm_influence_cross_cov): with psi_k(n, c) as in ``influence_cov`` and
    p = w / sum w, ``cov[c, i, c', j] = sum_n p_n^2 psi_i(n, c) psi_j(n, c')`` -- every block of the (C n_f)^2 matrix,
    bitwise symmetric, from one pass over x on the FP64 matrix pipe.  x: (N, C) or (N,), copied to row-major if it is
    not; a, b: (C, n_f, n_q); center_x: (C,); C <= 255.  Returns ``cov [C, n_f, C, n_f]`` on the device.  Independent
    samples are assumed; ``influence_block_cross_cov`` is the blocked form for a correlated series."""
    L = _L()
    x2, ls, _, u, w, N, C, _ = _operands(x, u, w, "rowmajor")
    a, b, center_x, n_f, n_q = _influence_coefs(a, b, center_x, (C,))
    _check_cross_columns("influence_cross_cov", C)
    cov = torch.empty((C, n_f, C, n_f), dtype=F64, device="cuda")
    ws = workspace(L.txm_influence_cross_cov_ws_bytes(N, C, n_f, n_q))
    check(
        L.txm_influence_cross_cov(_ptr(x2), ls, _ptr(u), _ptr(w), N, C, n_f, n_q, float(center_u), _ptr(center_x), _ptr(a),
                                  _ptr(b), _ptr(cov), _ptr(ws), ws.numel(), _stream()),
        "txm_influence_cross_cov",
    )
    return cov


def influence_cross_cov_batched(xs, us, a: torch.Tensor, b: torch.Tensor, center_u, center_x: torch.Tensor,
                                ws=None) -> torch.Tensor:
    """``influence_cross_cov`` of S independent states in ONE launch per kernel (txm_influence_cross_cov_batched).
    xs[s]: (n_s, C) or (n_s,), us[s] (and ws[s]): (n_s,) -- the sample count may differ from state to state; a, b:
    (S, C, n_f, n_q); center_u: S host floats or an (S,) tensor; center_x: (S, C); C <= 255.
    Returns ``cov [S, C, n_f, C, n_f]`` on the device, every ``cov[s]`` bitwise symmetric as a (C n_f)^2 matrix.

    The batch has a plan of its own (include/txmom.h (f-14)): the states share the device, each with at most
    ``q = max(1, 8 CUs // (tile pairs * S))`` sample workgroups.  State s equals
    ``influence_cross_cov(xs[s], us[s], a[s], b[s], center_u[s], center_x[s], w=ws[s])`` bit for bit when
    ``ceil(n_s / 256) <= q``; a state the budget binds has the same sums in another order, within the same rounding bound.

    The one launch needs every x row-major with one pitch; otherwise this loops over ``influence_cross_cov`` and stacks.
    Pointer alignment does not matter (the kernel reads 8 bytes at a time)."""
    L = _L()
    ops, ws, S, C, pitches, tab = _influence_states(xs, us, ws, "rowmajor")
    a, b, center_x, n_f, n_q = _influence_coefs(a, b, center_x, (S, C))
    _check_cross_columns("influence_cross_cov_batched", C, " per state")
    cu_dev = _center_u_device(center_u, S)
    as_given = all(not _layout(x.unsqueeze(1) if x.dim() == 1 else x, "rowmajor")[0] for x in xs)
    if not (as_given and len(pitches) == 1):
        cu_host = _center_u_host(center_u)
        return torch.stack([influence_cross_cov(xs[s], us[s], a[s], b[s], float(cu_host[s]), center_x[s],
                                                w=None if ws is None else ws[s]) for s in range(S)])

    cov = torch.empty((S, C, n_f, C, n_f), dtype=F64, device="cuda")
    wsb = workspace(L.txm_influence_cross_cov_batched_ws_bytes(S, max(o[5] for o in ops), C, n_f, n_q))
    check(
        L.txm_influence_cross_cov_batched(tab, S, pitches.pop(), C, n_f, n_q, _ptr(cu_dev), _ptr(center_x), _ptr(a), _ptr(b),
                                          _ptr(cov), _ptr(wsb), wsb.numel(), _stream()),
        "txm_influence_cross_cov_batched",
    )
    del ops
    return cov


def influence_block_cross_cov(x: torch.Tensor, u: torch.Tensor, a: torch.Tensor, b: torch.Tensor, center_u: float,
                              center_x: torch.Tensor, block: int, n_levels: int = 1,
                              w: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """Blocked (batch-means) delta-method covariance ACROSS the columns for a correlated series
    (txm_influence_block_cross_cov): with the block sums ``z_j[c, k] = sum_{n in block j} p_n psi_k(n, c)`` of
    ``influence_block_cov``, ``cov[l, c, i, c', j'] = sum_j z_j[c, i] z_j[c', j']`` over the contiguous blocks of
    ``block * 2**l`` rows (a last short block is kept; no nb / (nb - 1) factor, so ``block=1`` is ``influence_cross_cov``'s
    result and the blocks ``c == c'`` are ``influence_block_cov``'s, up to rounding) -- every level bitwise symmetric as
    a (C n_f)^2 matrix.  One pass over x (``influence_block_cov``'s own), then a Gram over the block sums on the FP64
    matrix pipe per level.  x: (N, C) or (N,), copied to row-major if it is not; a, b: (C, n_f, n_q); center_x: (C,);
    C <= 255.  Returns ``(cov [n_levels, C, n_f, C, n_f], mean [C, n_f])`` on the device.  Not covered: a batched
    (many-state) form, overlapping batch means."""
    L = _L()
    x2, ls, _, u, w, N, C, _ = _operands(x, u, w, "rowmajor")
    a, b, center_x, n_f, n_q = _influence_coefs(a, b, center_x, (C,))
    _check_cross_columns("influence_block_cross_cov", C, " a level")
    block, n_levels = _block_levels_args(block, n_levels)
    cov = torch.empty((n_levels, C, n_f, C, n_f), dtype=F64, device="cuda")
    mean = torch.empty((C, n_f), dtype=F64, device="cuda")
    ws = workspace(L.txm_influence_block_cross_cov_ws_bytes(N, C, n_f, n_q, block, n_levels))
    check(
        L.txm_influence_block_cross_cov(_ptr(x2), ls, _ptr(u), _ptr(w), N, C, n_f, n_q, float(center_u), _ptr(center_x),
                                        _ptr(a), _ptr(b), block, n_levels, _ptr(cov), _ptr(mean), _ptr(ws), ws.numel(),
                                        _stream()),
        "txm_influence_block_cross_cov",
    )
    return cov, mean


TAYLOR_MODES ={"sum": 0, "cumsum": 1, "terms": 2}


def predict_taylor(derivs: torch.Tensor, dalphas, mode: str = "sum") -> torch.Tensor:
    """Taylor series of a derivative table (n_ord, ...) at every dalpha: (n_alpha, ...) for ``mode="sum"``,
    (n_alpha, n_ord, ...) partial sums (``"cumsum"``) or terms (``"terms"``) -- ExtrapModel.predict in one launch."""
    L = _L()
    _check_f64_cuda(derivs, "derivs")
    if mode not in TAYLOR_MODES:
        raise ValueError(f"mode must be one of {sorted(TAYLOR_MODES)}")
    d = derivs.contiguous()
    n_ord = d.shape[0]
    if not 1 <= n_ord <= 16:
        raise ValueError("predict_taylor: 1 <= n_ord <= 16")
    M = d[0].numel()
    da = to_device(np.atleast_1d(np.asarray(dalphas, dtype=np.float64)).ravel())
    na = da.numel()
    if na < 1 or M < 1:
        raise ValueError("predict_taylor: empty input")
    shape = (na, *d.shape[1:]) if mode == "sum" else (na, n_ord, *d.shape[1:])
    out = torch.empty(shape, dtype=F64, device="cuda")
    # the kernel carries alpha on a 16-bit grid axis: more than 65535 alpha values go in slices (same launch shape)
    step = 65535
    for a0 in range(0, na, step):
        a1 = min(na, a0 + step)
        check(L.txm_predict_taylor(_ptr(d), n_ord, M, _ptr(da[a0:a1]), a1 - a0, TAYLOR_MODES[mode], _ptr(out[a0:a1]),
                                   _stream()), "txm_predict_taylor")
    return out


def perturb(x: torch.Tensor, u: torch.Tensor, dalphas, freq: torch.Tensor | None = None) -> torch.Tensor:
    """Exponentially reweighted averages for each dalpha: (n_alpha, C), or
    (nrep, n_alpha, C) with bootstrap counts ``freq`` (nrep, N).  x: (N, C) row-major or (N,)."""
    L = _L()
    x2, ls, _, u, _, N, C, squeeze = _operands(x, u, None, "rowmajor")
    da = np.atleast_1d(np.asarray(dalphas, dtype=np.float64))
    nrep = 1
    if freq is not None:
        freq = freq.to(device="cuda", dtype=torch.int64).contiguous()
        if freq.dim() != 2 or freq.shape[1] != N:
            raise ValueError(f"freq must be (nrep, {N}), got {tuple(freq.shape)}")
        nrep = freq.shape[0]
    outs = []
    for _, chunk in _eight_per_pass(da):
        na = len(chunk)
        out = torch.empty((nrep, na, C), dtype=F64, device="cuda")
        ws = workspace(L.txm_perturb_ws_bytes(N, C, na, nrep))
        check(
            L.txm_perturb(_ptr(x2), ls, _ptr(u), N, C,
                          chunk.ctypes.data_as(ct.POINTER(ct.c_double)), na, _ptr(freq), nrep, _ptr(out), _ptr(ws),
                          ws.numel(), _stream()),
            "txm_perturb",
        )
        outs.append(out)
    res = torch.cat(outs, dim=1)
    if freq is None:
        res = res[0]
    return res[..., 0] if squeeze else res


class PerturbCov(NamedTuple):
    """What ``perturb_cov`` returns, all on the device: ``mean`` (n_alpha, C) is ``perturb``'s output, ``var``
    (n_levels, n_alpha, C) its delta-method variance per level, ``neff`` (n_alpha,) Kish's effective sample number,
    ``lnq`` (n_alpha,) ``ln <e^{-dalpha u}>`` and ``var_lnq`` (n_levels, n_alpha) its variance.  The C axis is dropped for
    1-D x."""

    mean: torch.Tensor
    var: torch.Tensor
    neff: torch.Tensor
    lnq: torch.Tensor
    var_lnq: torch.Tensor


def perturb_cov(x: torch.Tensor, u: torch.Tensor, dalphas, block: int = 1, n_levels: int = 1) -> PerturbCov:
    """Delta-method (infinitesimal-jackknife) variance of ``perturb``'s averages (txm_perturb_cov): with
    ``p_na = w_na / sum_n w_na`` the normalised weights ``e^{-dalpha_a u_n}``, ``var[l, a, c] = sum_j z_j^2`` over the
    sums ``z_j = sum_{n in block j} p_na (x_nc - mean_ac)`` of the contiguous blocks of ``block * 2**l`` rows (a last
    short block is kept; no nb / (nb - 1) factor; ``block=1, n_levels=1`` is the iid ``sum_n p_n^2 (x_n - m)^2``),
    ``neff = (sum w)^2 / sum w^2``, ``lnq = ln <e^{-dalpha u}>`` and ``var_lnq[l, a] = sum_j (sum_{n in j} p_na -
    n_j / N)^2``.  ``perturb`` gives the means, then one more pass over the samples per 8 dalphas.  x: (N, C) row-major
    or (N,)."""
    L = _L()
    block, n_levels = _block_levels_args(block, n_levels)
    x2, ls, _, u, _, N, C, squeeze = _operands(x, u, None, "rowmajor")
    da = np.atleast_1d(np.asarray(dalphas, dtype=np.float64))
    mean = perturb(x2, u, da)                                                              # (n_alpha, C)
    parts = []
    for i0, chunk in _eight_per_pass(da):
        na = len(chunk)
        var = torch.empty((n_levels, na, C), dtype=F64, device="cuda")
        neff = torch.empty(na, dtype=F64, device="cuda")
        lnq = torch.empty(na, dtype=F64, device="cuda")
        var_lnq = torch.empty((n_levels, na), dtype=F64, device="cuda")
        ws = workspace(L.txm_perturb_cov_ws_bytes(N, C, na, block, n_levels))
        check(
            L.txm_perturb_cov(_ptr(x2), ls, _ptr(u), N, C, chunk.ctypes.data_as(ct.POINTER(ct.c_double)), na,
                              _ptr(mean[i0:i0 + na]), block, n_levels, _ptr(var), _ptr(neff), _ptr(lnq), _ptr(var_lnq),
                              _ptr(ws), ws.numel(), _stream()),
            "txm_perturb_cov",
        )
        parts.append((var, neff, lnq, var_lnq))
    var = torch.cat([p[0] for p in parts], dim=1)
    if squeeze:
        mean, var = mean[..., 0], var[..., 0]
    return PerturbCov(mean, var, torch.cat([p[1] for p in parts]), torch.cat([p[2] for p in parts]),
                      torch.cat([p[3] for p in parts], dim=1))


# ---------------------------------------------------------------------------
# MBAR (MBARModel; reference models.py:1049-1111, which wraps pymbar)
# ---------------------------------------------------------------------------
class MbarSolution(NamedTuple):
    """What ``mbar_solve`` returns: the free energies ``f`` (gauge f_0 = 0), the device buffer ``logD`` of the pooled
    samples' log-denominators stored by the last evaluation, the pivot ``upiv`` it was computed with (``mbar_predict``
    must use the same one), and how the solve went."""

    f: np.ndarray
    logD: torch.Tensor
    upiv: float
    iterations: int
    evaluations: int
    gradient: float


def _mbar_table(us, xs=None):
    """The host table of txm_mbar_state entries for K states (x may be omitted for the evaluation), the tensors it
    points into (keep them alive over the call), the per-state sample counts and C."""
    K = len(us)
    if not 1 <= K <= 64:
        raise ValueError(f"MBAR needs 1 <= K <= 64 states, got {K}")
    if xs is not None and len(xs) != K:
        raise ValueError("need one x per u")
    u2, x2, ldx, ns, C = [], [], [], [], 1
    for s in range(K):
        u = us[s]
        _check_f64_cuda(u, "u")
        if u.dim() != 1 or u.shape[0] < 1:
            raise ValueError("every u must be (n,) with n >= 1")
        u2.append(u.contiguous())
        ns.append(u.shape[0])
        if xs is not None:
            x = xs[s]
            _check_f64_cuda(x, "x")
            x = x.unsqueeze(1) if x.dim() == 1 else x
            if x.dim() != 2 or x.shape[0] != u.shape[0]:
                raise ValueError(f"x of state {s} must be ({u.shape[0]},) or ({u.shape[0]}, C)")
            x, ls, _ = _place(x, "rowmajor")
            if s == 0:
                C = x.shape[1]
            elif x.shape[1] != C:
                raise ValueError("every state's x must have the same number of columns")
            x2.append(x)
            ldx.append(ls)
    tab = (_lib.MbarState * K)()
    for s in range(K):
        tab[s].u = u2[s].data_ptr()
        tab[s].n = ns[s]
        if xs is not None:
            tab[s].x = x2[s].data_ptr()
            tab[s].ldx_s = ldx[s]
    return tab, (u2, x2), np.asarray(ns, dtype=np.float64), C


def _mbar_alpha0(alpha0, K):
    """alpha0 as a contiguous float64 (K,)."""
    a0 = np.ascontiguousarray(np.asarray(alpha0, dtype=np.float64).reshape(-1))
    if a0.shape != (K,):
        raise ValueError("need one alpha0 per state")
    return a0


def _mbar_b(us, alpha0, upiv):
    """(ns, a0, b): the states' sample counts, alpha0 as (K,) and b = ln N - alpha0 upiv, the log-weights at f = 0."""
    a0 = _mbar_alpha0(alpha0, len(us))
    ns = np.array([u.shape[0] for u in us], dtype=np.float64)
    return ns, a0, np.log(ns) - a0 * upiv


MBAR_CROSS_MAX_TARGETS = 8    # txm_mbar_cross_cov with cross_alpha: one call, MB_MAXA targets
MBAR_CROSS_MAX_COLUMNS = 255  # txm_mbar_cross_cov, txm_mbar_block_cov: C + 1 logical columns in at most 16 tiles a side


class _MbarTargetCall(NamedTuple):
    """What a pass over the targets at a solution starts from (``_mbar_target_call``)."""

    tab: object        # the host table of txm_mbar_state entries
    keep: object       # the tensors it points into: alive until the results are on the host
    K: int
    C: int
    ns: np.ndarray     # samples per state
    a0: np.ndarray     # (K,), contiguous
    g: np.ndarray      # (K,), contiguous: the solution's shifted log-weights (mbar_solution_g)
    c: float           # their shift: sol.logD is the true log-denominator + c
    al: np.ndarray     # the targets, flat


def _mbar_target_call(us, xs, alpha0, sol, alphas, means=None, *, wide=None, many=None) -> _MbarTargetCall:
    """The checked operands of mbar_cov_sums, mbar_cross_cov_sums, mbar_block_gamma and mbar_hist_sums (``xs=None``).
    ``means``: checked to be (n_alpha, C) float64 CUDA.  ``wide`` / ``many``: the caller's refusal of more than 255
    columns / more than 8 targets (a text with one ``{}``); None: no limit."""
    tab, keep, ns, C = _mbar_table(us, xs)
    K = len(us)
    a0 = _mbar_alpha0(alpha0, K)
    g, c = mbar_solution_g(ns, a0, sol)
    al = np.atleast_1d(np.asarray(alphas, dtype=np.float64)).reshape(-1)
    if wide is not None and C > MBAR_CROSS_MAX_COLUMNS:
        raise ValueError(wide.format(C))
    if many is not None and len(al) > MBAR_CROSS_MAX_TARGETS:
        raise ValueError(many.format(len(al)))
    if means is not None:
        _check_f64_cuda(means, "means")
        if means.shape != (len(al), C):
            raise ValueError(f"means must be ({len(al)}, {C}), got {tuple(means.shape)}")
    if sol.logD.shape != (int(ns.sum()),):
        raise ValueError("sol.logD must hold one value per pooled sample")
    return _MbarTargetCall(tab, keep, K, C, ns, a0, np.ascontiguousarray(g), c, al)


def _mbar_cov_passes(t: _MbarTargetCall, sol, means):
    """txm_mbar_cov per 8 targets, launched: yields (chunk, mean, out, lnw, ws, nbytes) of each pass -- the targets, their
    rows of ``means``, the pass's device output [n][1 + K + C (1 + K)] and ln sum_n w_an, its workspace (tag "mbar_cov")
    and the bytes of the size query.  A second pass of the caller's goes onto the same stream inside the loop, fed lnw on
    the device: nothing waits on the host in between."""
    L = _L()
    dp = ct.POINTER(ct.c_double)
    K, C = t.K, t.C
    for i0, chunk in _eight_per_pass(t.al):
        na = len(chunk)
        mean = means[i0:i0 + na].contiguous()
        out = torch.empty((na, 1 + K + C * (1 + K)), dtype=F64, device="cuda")
        lnw = torch.empty(na, dtype=F64, device="cuda")
        nbytes = L.txm_mbar_cov_ws_bytes(K, C, na)
        ws = workspace(nbytes, tag="mbar_cov")
        check(L.txm_mbar_cov(t.tab, K, C, float(sol.upiv), t.a0.ctypes.data_as(dp), t.g.ctypes.data_as(dp), _ptr(sol.logD),
                             chunk.ctypes.data_as(dp), na, _ptr(mean), _ptr(out), _ptr(lnw), _ptr(ws), nbytes,
                             _stream()), "txm_mbar_cov")
        yield chunk, mean, out, lnw, ws, nbytes


def _mbar_cov_rows(t: _MbarTargetCall, outs):
    """(Q, B, yy, b) on the host from the passes' ``out`` rows: per target Q, B_k, then (yy_c, b_kc) per column."""
    v = torch.cat(outs, dim=0).cpu().numpy()
    rest = v[:, 1 + t.K:].reshape(len(t.al), t.C, 1 + t.K)
    return v[:, 0].copy(), v[:, 1:1 + t.K].copy(), rest[:, :, 0].copy(), rest[:, :, 1:].copy()


def _mbar_true_lnw(t: _MbarTargetCall, sol, lnws) -> np.ndarray:
    """ln sum_n e^{-alpha u_n - logD_n} with the true log-denominators from the kernels' lnw: their exponents are
    -alpha (u - upiv) - (logD + c), so the sum is e^{-alpha upiv + c} times theirs."""
    return torch.cat(lnws).cpu().numpy() - t.al * sol.upiv + t.c


def mbar_pivot(us) -> float:
    """The pivot the MBAR kernels subtract from u: the pooled mean (torch's sum, a deterministic reduction)."""
    tot = sum(float(u.sum()) for u in us)
    return tot / sum(u.shape[0] for u in us)


def mbar_eval(us, alpha0, g, upiv: float, logD: torch.Tensor | None = None):
    """One device evaluation pass (txm_mbar_eval) at the shifted log-weights ``g``: (S (K,), H (K, K) symmetric, objective),
    copied to the host; ``logD`` (float64 CUDA, pooled length) receives the per-sample log-denominators."""
    L = _L()
    tab, keep, ns, _ = _mbar_table(us)
    K = len(us)
    a0 = np.ascontiguousarray(alpha0, dtype=np.float64)
    gg = np.ascontiguousarray(g, dtype=np.float64)
    if a0.shape != (K,) or gg.shape != (K,):
        raise ValueError("alpha0 and g need one entry per state")
    if logD is not None:
        _check_f64_cuda(logD, "logD")
        if logD.shape != (int(ns.sum()),) or not logD.is_contiguous():
            raise ValueError("logD must be a contiguous (sum n,) tensor")
    nh = K * (K + 1) // 2
    out = torch.empty(K + nh + 1, dtype=F64, device="cuda")
    ws = workspace(L.txm_mbar_ws_bytes(K, 1, 1), tag="mbar")
    dp = ct.POINTER(ct.c_double)
    check(L.txm_mbar_eval(tab, K, a0.ctypes.data_as(dp), gg.ctypes.data_as(dp), float(upiv), _ptr(out), _ptr(logD), _ptr(ws),
                          ws.numel(), _stream()), "txm_mbar_eval")
    v = out.cpu().numpy()
    del keep
    return v[:K].copy(), mbar_unpack_h(v[K:K + nh], K), float(v[K + nh])


def mbar_initial_f(us, alpha0) -> np.ndarray:
    """Starting free energies by thermodynamic integration over the states sorted by alpha0 (df/dalpha = <u>, trapezoid
    between neighbours), gauge f_0 = 0: close enough that no state's weights underflow, even without overlap."""
    a0 = np.asarray(alpha0, dtype=np.float64)
    means = np.array([float(u.mean()) for u in us])
    order = np.argsort(a0, kind="stable")
    f = np.zeros(len(a0))
    for i in range(1, len(order)):
        p, q = order[i - 1], order[i]
        f[q] = f[p] + (a0[q] - a0[p]) * 0.5 * (means[p] + means[q])
    return f - f[0]


def mbar_solve(us, alpha0, *, tol: float = 1e-12, max_iter: int = 100) -> MbarSolution:
    """MBAR free energies of K states (1 <= K <= 64) from their reduced potentials alpha0_k u_n over the pooled samples
    (u: one float64 CUDA tensor per state, any lengths).  Damped Newton (``mbar_newton``), one device evaluation pass
    (``mbar_eval``) per step: the host waits for each pass -- acceptable because a model solves once and caches the
    result.  Every pass also stores the pooled log-denominators, so the buffer returned is the solution's."""
    upiv = mbar_pivot(us)
    ns, a0, b = _mbar_b(us, alpha0, upiv)
    logD = torch.empty(int(ns.sum()), dtype=F64, device="cuda")

    def evaluate(g):
        return mbar_eval(us, a0, g, upiv, logD)

    f, _, it, n_eval, err = mbar_newton(evaluate, ns, b, f0=mbar_initial_f(us, a0), tol=tol, max_iter=max_iter)
    return MbarSolution(f, logD, upiv, it, n_eval, err)


def mbar_predict(xs, us, alpha0, f, logD, alphas, *, upiv: float | None = None) -> torch.Tensor:
    """MBAR averages of x at each target alpha: (n_alpha, C), from the log-denominators ``logD`` that ``mbar_solve`` stored
    (``upiv``: the pivot it used, ``MbarSolution.upiv``; by default the pooled mean, which is what the solve takes).  With
    ``logD=None`` one evaluation pass at ``f`` computes them first.  Targets go 8 per pass over the samples."""
    L = _L()
    tab, keep, ns, C = _mbar_table(us, xs)
    K = len(us)
    if upiv is None:
        upiv = mbar_pivot(us)
    if logD is None:
        a0 = np.asarray(alpha0, dtype=np.float64).reshape(-1)
        g = np.log(ns) + np.asarray(f, dtype=np.float64) - a0 * upiv      # (summed in this order: not _mbar_b's b + f)
        logD = torch.empty(int(ns.sum()), dtype=F64, device="cuda")
        mbar_eval(us, a0, g - g.max(), upiv, logD)
    _check_f64_cuda(logD, "logD")
    if logD.shape != (int(ns.sum()),):
        raise ValueError("logD must hold one value per pooled sample")
    al = np.atleast_1d(np.asarray(alphas, dtype=np.float64)).reshape(-1)
    outs = []
    for _, chunk in _eight_per_pass(al):
        na = len(chunk)
        out = torch.empty((na, C), dtype=F64, device="cuda")
        ws = workspace(L.txm_mbar_ws_bytes(K, C, na), tag="mbar")
        check(L.txm_mbar_predict(tab, K, C, float(upiv), _ptr(logD), chunk.ctypes.data_as(ct.POINTER(ct.c_double)), na,
                                 _ptr(out), _ptr(ws), ws.numel(), _stream()), "txm_mbar_predict")
        outs.append(out)
    res = torch.cat(outs, dim=0)
    del keep
    return res


# ---------------------------------------------------------------------------
# MBAR's asymptotic covariance (Shirts & Chodera 2008, eq. 8 and appendix D; include/txmom.h txm_mbar_cov).
# Theta = W^T (I_N - W N W^T)^+ W over the columns W_nk = p_kn / N_k of the sampled states and W_na of the targets needs
# only the Gram matrix G = W^T W: the sampled block is H / (N_j N_k) of one evaluation pass at the solution, the target
# blocks are the sums of txm_mbar_cov.
# ---------------------------------------------------------------------------

def mbar_gram(us, alpha0, sol: MbarSolution) -> np.ndarray:
    """G_jk = sum_n W_nj W_nk of the sampled states: one ``mbar_eval`` at the solution's g, H_jk / (N_j N_k)."""
    ns = np.array([u.shape[0] for u in us], dtype=np.float64)
    g, _ = mbar_solution_g(ns, alpha0, sol)
    _, H, _ = mbar_eval(us, np.asarray(alpha0, dtype=np.float64).reshape(-1), g, sol.upiv)
    return H / np.outer(ns, ns)


def mbar_cov_sums(xs, us, alpha0, sol: MbarSolution, alphas, means, *, with_lnw: bool = False):
    """The target sums of the asymptotic covariance (txm_mbar_cov), 8 targets per pass over the samples, on the host:
    Q (n_alpha,) = sum_n W_na^2, B (n_alpha, K) = sum_n W_nk W_na, yy (n_alpha, C) = sum_n W_na^2 (x_nc - mean_ac)^2 and
    b (n_alpha, C, K) = sum_n W_nk W_na (x_nc - mean_ac).  ``means``: (n_alpha, C) float64 CUDA, ``mbar_predict``'s output
    for the same targets.  ``with_lnw``: also ln sum_n e^{-alpha u_n - logD_n} (n_alpha,) with the true log-denominators
    (the solve's pivot and shift taken out): minus the target's free energy in the gauge of ``sol.f``."""
    t = _mbar_target_call(us, xs, alpha0, sol, alphas, means)
    outs, lnws = [], []
    for _, _, out, lnw, _, _ in _mbar_cov_passes(t, sol, means):
        outs.append(out)
        lnws.append(lnw)
    sums = _mbar_cov_rows(t, outs)
    return (*sums, _mbar_true_lnw(t, sol, lnws)) if with_lnw else sums


def mbar_cross_cov_sums(xs, us, alpha0, sol: MbarSolution, alphas, means, *, cross_alpha: bool = False):
    """The sums of the asymptotic covariance ACROSS columns (txm_mbar_cross_cov), on the host: the Gram matrix
    sum_n W_na W_na' d_nac d_na'c' (d_nac = x_nc - mean_ac) and ``mbar_cov_sums``' b (n_alpha, C, K).  The Gram is
    (n_alpha, C, C), a' = a, or with ``cross_alpha`` (n_alpha, C, n_alpha, C), at most 8 targets.  Per 8 targets a
    txm_mbar_cov pass, then the Gram pass in the same workspace on the same stream, fed the first's ln sum_n w_an on the
    device: nothing waits on the host between them.  At most 255 columns."""
    L = _L()
    t = _mbar_target_call(us, xs, alpha0, sol, alphas, means,
                          wide="the covariance across columns takes at most 255 columns, got {}",
                          many="the covariance across targets takes at most 8 targets, got {}" if cross_alpha else None)
    K, C, n = t.K, t.C, len(t.al)
    outs, grams = [], []
    for chunk, mean, out, lnw, ws, nbytes in _mbar_cov_passes(t, sol, means):
        na = len(chunk)
        gram = torch.empty((na * C, na * C) if cross_alpha else (na, C, C), dtype=F64, device="cuda")
        # (the query's bytes, not the cached buffer's: the plan, and with it the bits, depend on nothing else)
        check(L.txm_mbar_cross_cov(t.tab, K, C, float(sol.upiv), _ptr(sol.logD), chunk.ctypes.data_as(ct.POINTER(ct.c_double)),
                                   na, _ptr(mean), _ptr(lnw), int(bool(cross_alpha)), _ptr(gram), _ptr(ws), nbytes, _stream()),
              "txm_mbar_cross_cov")
        outs.append(out)
        grams.append(gram)
    b = _mbar_cov_rows(t, outs)[3]
    G = torch.cat(grams, dim=0).cpu().numpy()
    return (G.reshape(n, C, n, C) if cross_alpha else G), b


HIST_MAX_BINS = 1023    # txm_mbar_hist: nbins + 1 columns in at most 64 tiles of 16
_SIZE_MAX = ct.c_size_t(-1).value


class MbarBlockGamma(NamedTuple):
    """What ``mbar_block_gamma`` returns, on the host.  Targets go 8 per slab; slab i holds the targets 8 i .. 8 i + 7 and
    has its own Gram matrix (its leading K x K block, the sampled states', is the same in every slab)."""

    gamma: list            # per slab (n_levels, M_i, M_i), M_i = K + n_i (C + 1): Gamma of every level
    nblocks: np.ndarray    # (n_levels, K) int64: the blocks of every state at every level
    b: np.ndarray          # (n_alpha, C, K): mbar_cov_sums' b
    B: np.ndarray          # (n_alpha, K): mbar_cov_sums' B
    lnw: np.ndarray        # (n_alpha,): mbar_cov_sums' lnw (with_lnw=True)

    def slabs(self):
        """(gamma, b, B) of every slab: its Gram matrices and its targets' rows of ``b`` and ``B`` (the slab width is
        ``_eight_per_pass``'s)."""
        for gamma, (i0, chunk) in zip(self.gamma, _eight_per_pass(self.lnw)):
            yield gamma, self.b[i0:i0 + len(chunk)], self.B[i0:i0 + len(chunk)]


def mbar_block_lengths(block, ns) -> np.ndarray:
    """``block`` of the blocked MBAR error bars as int64 (K,): an int serves every state, a sequence gives each state its
    own (what ``timeseries.block_lengths`` returns)."""
    K = len(ns)
    if isinstance(block, (str, bytes, bool)) or (np.ndim(block) == 0 and not isinstance(block, (int, np.integer))):
        raise TypeError(f"block must be an int or one int per state, got {block!r}")
    vals = [block] * K if np.ndim(block) == 0 else list(block)
    if len(vals) != K:
        raise ValueError(f"block must be an int or hold one entry per state: len(block)={len(vals)}, {K} states")
    for v in vals:
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise TypeError(f"block must be an int or one int per state, got {v!r}")
        if v < 1:
            raise ValueError(f"block must be >= 1, got {v}")
    return np.ascontiguousarray(vals, dtype=np.int64)


def mbar_block_levels(ns, block) -> tuple[np.ndarray, np.ndarray]:
    """The levels of a blocking curve of the pooled states: ``(factors, n_blocks)`` with ``factors[l] = 2**l`` (level l
    cuts state s into blocks of ``block[s] * 2**l`` records) and ``n_blocks[l][s] = ceil(ceil(n_s / block[s]) / 2**l)``,
    for every level at which some state still has at least two blocks (at least one level)."""
    blk = mbar_block_lengths(block, ns)
    nb0 = -(-np.asarray(ns, dtype=np.int64) // np.minimum(blk, np.asarray(ns, dtype=np.int64)))
    counts, l = [], 0
    while l < 32:
        c = (nb0 + (1 << l) - 1) >> l
        if l > 0 and c.max() < 2:
            break
        counts.append(c)
        l += 1
    return 2 ** np.arange(len(counts), dtype=np.int64), np.asarray(counts, dtype=np.int64)


def mbar_block_gamma(xs, us, alpha0, sol: MbarSolution, alphas, means, block, n_levels: int = 1) -> MbarBlockGamma:
    """The Gram matrices behind the blocked (batch-means) MBAR error bars (txm_mbar_block_cov) with the sums the
    coefficient vectors need, on the host.  Per 8 targets a txm_mbar_cov pass (b, B and, on the device, ln sum_n w_an),
    then the block pass on the same stream, fed the first's lnw and ``means`` on the device: nothing waits on the host
    between them.  ``block``: an int or one int per state; ``n_levels``: Gamma for blocks of block * 2**l, l < n_levels.
    At most 255 columns."""
    L = _L()
    n_levels = int(n_levels)
    if not 1 <= n_levels <= 32:
        raise ValueError(f"n_levels must be in [1, 32], got {n_levels}")
    t = _mbar_target_call(us, xs, alpha0, sol, alphas, means, wide="the blocked MBAR error bars take at most 255 columns, got {}")
    K, C = t.K, t.C
    blk = mbar_block_lengths(block, t.ns)
    n64 = np.ascontiguousarray(t.ns, dtype=np.int64)
    dp, ip = ct.POINTER(ct.c_double), ct.POINTER(ct.c_int64)
    outs, lnws, gammas = [], [], []
    nblocks = torch.empty((n_levels, K), dtype=torch.int64, device="cuda")
    for chunk, mean, out, lnw, _, _ in _mbar_cov_passes(t, sol, means):
        na = len(chunk)
        M = mbar_block_width(K, na, C)
        gamma = torch.empty((n_levels, M, M), dtype=F64, device="cuda")
        plan = (ct.c_int64 * 7)()
        check(L.txm_mbar_block_cov_plan(n64.ctypes.data_as(ip), blk.ctypes.data_as(ip), K, C, na, n_levels, _SIZE_MAX, plan),
              "txm_mbar_block_cov_plan")
        bbytes = int(plan[5])
        wsb = workspace(bbytes, tag="mbar_block")
        # (the plan's bytes, not the cached buffer's: the plan, and with it the bits, depend on nothing else)
        check(L.txm_mbar_block_cov(t.tab, K, C, float(sol.upiv), t.a0.ctypes.data_as(dp), t.g.ctypes.data_as(dp), _ptr(sol.logD),
                                   chunk.ctypes.data_as(dp), na, _ptr(mean), _ptr(lnw), blk.ctypes.data_as(ip), n_levels,
                                   _ptr(gamma), _ptr(nblocks), _ptr(wsb), bbytes, _stream()), "txm_mbar_block_cov")
        outs.append(out)
        lnws.append(lnw)
        gammas.append(gamma)
    _, B, _, b = _mbar_cov_rows(t, outs)
    gam = [g.cpu().numpy() for g in gammas]
    return MbarBlockGamma(gam, nblocks.cpu().numpy(), b, B, _mbar_true_lnw(t, sol, lnws))


def bin_index(values, edges) -> torch.Tensor:
    """The int32 bin index of every value under ``numpy.histogram``'s rule for the increasing ``edges`` (float64,
    nbins + 1 of them): bin i holds edges[i] <= v < edges[i + 1], the last bin also v == edges[-1]; values below, above
    and NaN map to -1.  ``torch.bucketize`` on the device ``values`` lives on."""
    v = values if isinstance(values, torch.Tensor) else torch.as_tensor(np.asarray(values))
    v = v.to(F64)
    e = torch.as_tensor(np.ascontiguousarray(edges, dtype=np.float64), device=v.device)
    if e.dim() != 1 or e.shape[0] < 2 or not bool((e[1:] > e[:-1]).all()):
        raise ValueError("edges must be 1-D and increasing, at least two of them")
    nb = e.shape[0] - 1
    idx = torch.bucketize(v, e, right=True) - 1          # edges[idx] <= v < edges[idx + 1]; nb for v >= edges[-1]
    idx = torch.where(v == e[-1], torch.full_like(idx, nb - 1), idx)
    idx = torch.where((idx < 0) | (idx >= nb) | torch.isnan(v), torch.full_like(idx, -1), idx)
    return idx.to(torch.int32)


def mbar_hist_sums(bins, us, alpha0, sol: MbarSolution, alphas, nbins: int):
    """The class sums of reweighted histograms and of their covariance (txm_mbar_hist), 8 targets per pass over the
    samples, on the host.  ``bins``: one int32 CUDA tensor per state, the bin index of every sample; an index outside
    [0, nbins) puts the sample into the class ``nbins`` ("outside the range").  Returns (H, S, T, Q, B, lnw):
    H (n_alpha, nbins + 1) = sum_n W_na 1_b, S (n_alpha, nbins + 1) = sum_n W_na^2 1_b,
    T (n_alpha, K, nbins + 1) = sum_n W_nk W_na 1_b, Q (n_alpha,) = sum_b S_ab, B (n_alpha, K) = sum_b T_kab and
    lnw (n_alpha,) = ln sum_n e^{-alpha u_n - logD_n} as ``mbar_cov_sums`` gives it."""
    L = _L()
    nbins = int(nbins)
    if not 1 <= nbins <= HIST_MAX_BINS:
        raise ValueError(f"a histogram takes 1 <= nbins <= {HIST_MAX_BINS} bins, got {nbins}")
    t = _mbar_target_call(us, None, alpha0, sol, alphas)
    K, ns = t.K, t.ns
    if len(bins) != K:
        raise ValueError("need one tensor of bin indices per state")
    b2 = []
    for s, b in enumerate(bins):
        if not (isinstance(b, torch.Tensor) and b.is_cuda and b.dtype == torch.int32):
            raise TypeError("bins must be int32 CUDA tensors")
        if b.shape != (int(ns[s]),):
            raise ValueError(f"bins of state {s} must be ({int(ns[s])},), got {tuple(b.shape)}")
        b2.append(b.contiguous())
    btab = (ct.c_void_p * K)(*[b.data_ptr() for b in b2])
    dp = ct.POINTER(ct.c_double)
    outs, lnws = [], []
    for _, chunk in _eight_per_pass(t.al):
        na = len(chunk)
        plan = (ct.c_int64 * 4)()
        check(L.txm_mbar_hist_plan(K, nbins, na, int(ns.max()), _SIZE_MAX, plan), "txm_mbar_hist_plan")
        nbytes = int(plan[3])
        out = torch.empty((na, K + 2, nbins + 1), dtype=F64, device="cuda")
        lnw = torch.empty(na, dtype=F64, device="cuda")
        ws = workspace(nbytes, tag="mbar_hist")
        # (the plan's bytes, not the cached buffer's: the plan, and with it the bits, depend on nothing else)
        check(L.txm_mbar_hist(t.tab, btab, K, nbins, float(sol.upiv), t.a0.ctypes.data_as(dp), t.g.ctypes.data_as(dp),
                              _ptr(sol.logD), chunk.ctypes.data_as(dp), na, _ptr(out), _ptr(lnw), _ptr(ws), nbytes,
                              _stream()), "txm_mbar_hist")
        outs.append(out)
        lnws.append(lnw)
    v = torch.cat(outs, dim=0).cpu().numpy()
    lnw = _mbar_true_lnw(t, sol, lnws)
    del b2
    T, H, S = v[:, :K, :].copy(), v[:, K, :].copy(), v[:, K + 1, :].copy()
    return H, S, T, S.sum(axis=-1), T.sum(axis=-1), lnw


# ---------------------------------------------------------------------------
# MBAR bootstrap (MBARModel.bootstrap; include/txmom.h section (f-6)).  The reference stops at
# models.py:1109-1111 (MBARModel.resample raises): replicate r is the weighted MBAR with the multinomial counts of
# row r of every state's DeviceSampler, solved for all replicates at once from the point solution.
# ---------------------------------------------------------------------------
def _mbar_boot_tables(us, samplers, xs=None):
    """The two host tables of the bootstrap entry points (txm_mbar_state, txm_mbar_boot_state), what they point into,
    the per-state sample counts, C and nrep."""
    tab, keep, ns, C = _mbar_table(us, xs)
    K = len(us)
    if len(samplers) != K:
        raise ValueError("need one sampler per state")
    nrep = int(samplers[0].nrep)
    stab = (_lib.MbarBootState * K)()
    counts = []
    for s, sm in enumerate(samplers):
        if not isinstance(sm, DeviceSampler):
            raise TypeError(f"state {s}: the MBAR bootstrap needs a DeviceSampler, got {type(sm).__name__}")
        if sm.ndat != us[s].shape[0] or sm.spec.nsamp not in (0, sm.ndat):
            raise ValueError(f"state {s}: the sampler draws {sm.spec.nsamp or sm.ndat} of {sm.ndat}, the state has {us[s].shape[0]} samples")
        if sm.nrep != nrep:
            raise ValueError(f"state {s}: sampler nrep = {sm.nrep} differs from state 0's {nrep}")
        c = sm.counts.contiguous()
        counts.append(c)
        stab[s].spec = SamplerSpec(seed=sm.spec.seed, nrep=sm.spec.nrep, ndat=sm.spec.ndat, nsamp=sm.spec.nsamp, rep0=sm.spec.rep0)
        stab[s].counts = c.data_ptr()
    return tab, stab, (keep, counts), ns, C, nrep


def _mbar_boot_slab(K: int, C: int, n_alpha: int, ntot: int, nrep: int) -> int:
    """Replicates per library call: all of them when the call's workspace fits ``workspace_budget()``, else the most
    that do (at least one).  Rows of a slab equal the rows of the unslabbed call bit for bit (DeviceSampler.rows)."""
    L = _L()
    need = lambda n: L.txm_mbar_boot_ws_bytes(K, C, n_alpha, ntot, n)  # noqa: E731  (grows with n)
    return _most_that_fit(need, nrep, workspace_budget())


def mbar_boot_eval(us, alpha0, samplers, g, upiv: float, active=None):
    """One batched weighted evaluation pass (txm_mbar_boot_eval) at the log-weights ``g`` (nrep, K) of the replicates
    ``active`` (row indices; None: all): (S (R, K), H (R, K, K) symmetric, objective (R,)) of those rows, on the host."""
    L = _L()
    tab, stab, keep, ns, _, nrep = _mbar_boot_tables(us, samplers)
    K = len(us)
    a0 = np.ascontiguousarray(alpha0, dtype=np.float64)
    gg = np.ascontiguousarray(g, dtype=np.float64)
    if a0.shape != (K,) or gg.shape != (nrep, K):
        raise ValueError("alpha0 needs one entry per state and g one row of them per replicate")
    rows = np.arange(nrep) if active is None else np.asarray(active, dtype=np.int64).reshape(-1)
    if len(rows) < 1 or rows.min() < 0 or rows.max() >= nrep or len(np.unique(rows)) != len(rows):
        raise ValueError(f"active must list distinct rows of [0, {nrep})")
    nh = K * (K + 1) // 2
    nv = K + nh + 1
    gd = torch.as_tensor(gg).to("cuda")
    ad = None if active is None else torch.as_tensor(rows.astype(np.int32)).to("cuda")
    out = torch.zeros((nrep, nv), dtype=F64, device="cuda")
    ws = workspace(L.txm_mbar_boot_ws_bytes(K, 1, 1, int(ns.sum()), nrep), tag="mbar_boot")
    check(L.txm_mbar_boot_eval(tab, stab, K, a0.ctypes.data_as(ct.POINTER(ct.c_double)), _ptr(gd), _ptr(ad), len(rows),
                               float(upiv), _ptr(out), _ptr(ws), ws.numel(), _stream()), "txm_mbar_boot_eval")
    v = out.cpu().numpy()[rows]
    del keep
    return v[:, :K].copy(), mbar_unpack_h(v[:, K:K + nh], K), v[:, K + nh].copy()


def mbar_bootstrap_solve(us, alpha0, samplers, sol0: MbarSolution, *, tol: float = 1e-12, max_iter: int = 100) -> np.ndarray:
    """Free energies of every bootstrap replicate, (nrep, K) on the host, gauge f[:, 0] = 0: replicate r is the MBAR
    of the pooled samples weighted by row r of each state's sampler, solved by ``mbar_newton_batched`` from the point
    solution ``sol0`` (``mbar_solve`` of the same states; its pivot is reused).  Replicates go in slabs whose
    workspace fits ``workspace_budget()``; a slab's rows are the rows of the unslabbed call bit for bit."""
    K = len(us)
    upiv = float(sol0.upiv)
    ns, a0, b = _mbar_b(us, alpha0, upiv)
    if len(samplers) != K:
        raise ValueError("need one sampler per state")
    nrep = int(samplers[0].nrep)
    f0 = np.asarray(sol0.f, dtype=np.float64)
    slab = _mbar_boot_slab(K, 1, 1, int(ns.sum()), nrep)
    out = np.empty((nrep, K))
    for r0 in range(0, nrep, slab):
        r1 = min(r0 + slab, nrep)
        sub = list(samplers) if (r0, r1) == (0, nrep) else [sm.rows(r0, r1) for sm in samplers]

        def evaluate(g, active, sub=sub):
            return mbar_boot_eval(us, a0, sub, g, upiv, None if len(active) == g.shape[0] else active)

        out[r0:r1] = mbar_newton_batched(evaluate, ns, b, np.tile(f0, (r1 - r0, 1)), tol=tol, max_iter=max_iter)[0]
    return out


def mbar_bootstrap_predict(xs, us, alpha0, samplers, f, sol0: MbarSolution, alphas) -> torch.Tensor:
    """MBAR averages of x of every bootstrap replicate at each target: (nrep, n_alpha, C), from the replicates' free
    energies ``f`` (nrep, K) of ``mbar_bootstrap_solve``.  logD is recomputed from f inside the kernel; the exponents
    are shifted by a bound taken from the point solution ``sol0`` (txm_mbar_boot_predict).  Targets go 8 per pass,
    replicates in slabs under ``workspace_budget()``."""
    L = _L()
    tab, _, keep, ns, C, nrep = _mbar_boot_tables(us, samplers, xs)
    K = len(us)
    a0 = np.ascontiguousarray(np.asarray(alpha0, dtype=np.float64).reshape(-1))
    f = np.asarray(f, dtype=np.float64)
    if a0.shape != (K,) or f.shape != (nrep, K):
        raise ValueError("alpha0 needs one entry per state and f one row of them per replicate")
    upiv = float(sol0.upiv)
    b = np.log(ns) - a0 * upiv
    g = b[None, :] + f
    g = np.ascontiguousarray(g - g.max(axis=1, keepdims=True))
    gref = b + np.asarray(sol0.f, dtype=np.float64)
    gref = np.ascontiguousarray(gref - gref.max())
    al = np.atleast_1d(np.asarray(alphas, dtype=np.float64)).reshape(-1)
    ntot = int(ns.sum())
    slab = _mbar_boot_slab(K, C, min(8, len(al)), ntot, nrep)
    dp = ct.POINTER(ct.c_double)
    res = torch.empty((nrep, len(al), C), dtype=F64, device="cuda")
    for r0 in range(0, nrep, slab):
        r1 = min(r0 + slab, nrep)
        sub = list(samplers) if (r0, r1) == (0, nrep) else [sm.rows(r0, r1) for sm in samplers]
        _, stab, keep2, _, _, _ = _mbar_boot_tables(us, sub)
        gd = torch.as_tensor(g[r0:r1]).to("cuda")
        for i0, chunk in _eight_per_pass(al):
            na = len(chunk)
            out = torch.empty((r1 - r0, na, C), dtype=F64, device="cuda")
            ws = workspace(L.txm_mbar_boot_ws_bytes(K, C, na, ntot, r1 - r0), tag="mbar_boot")
            check(L.txm_mbar_boot_predict(tab, stab, K, C, upiv, a0.ctypes.data_as(dp), _ptr(gd), gref.ctypes.data_as(dp),
                                          chunk.ctypes.data_as(dp), na, _ptr(out), _ptr(ws), ws.numel(), _stream()),
                  "txm_mbar_boot_predict")
            res[r0:r1, i0:i0 + na] = out
        del keep2
    del keep
    return res


# ---------------------------------------------------------------------------
# lag sums (timeseries.py; the reference takes pymbar.timeseries.statistical_inefficiency: gpr_active/active_utils.py:244-269)
# ---------------------------------------------------------------------------
LAG_BLOCK = 256        # t0 and nlags of a call are multiples of it
LAG_MAX_LAGS = 4096    # lags per call
LAG_STAGE = 1008       # samples per staged piece of a chunk; a chunk is LAG_STAGE * ceil(n / (LAG_STAGE * 512)) samples


def lag_center(x: torch.Tensor | None, u: torch.Tensor) -> torch.Tensor:
    """The means the lag sums are centred with, (1 + C,): <u>, <x_0> .. <x_{C-1}> -- from the package's own reduction."""
    if x is None or x.shape[1] == 0:
        return reduce_vals_1d(u, 1)[1:2].contiguous()
    st = reduce_vals(x, u, 1)
    return torch.cat([st[0, 0, 1:2], st[:, 1, 0]]).contiguous()


def _lag_series_args(x, u):
    """(x2, u, N, C, row pitch) as txm_lag_sums and txm_lag_origin_sums take them."""
    _check_f64_cuda(u, "u")
    if u.dim() != 1:
        raise ValueError("u must be (N,)")
    N = u.shape[0]
    u = u.contiguous()
    C, ls, x2 = 0, 0, None
    if x is not None:
        _check_f64_cuda(x, "x")
        x2 = x.unsqueeze(1) if x.dim() == 1 else x
        if x2.dim() != 2 or x2.shape[0] != N:
            raise ValueError(f"x must be ({N},) or ({N}, C), got {tuple(x.shape)}")
        C = x2.shape[1]
        if C == 0:
            x2 = None
        else:
            x2, ls, _ = _place(x2, "rowmajor")
    return x2, u, N, C, ls


def lag_sums(x: torch.Tensor | None, u: torch.Tensor, pairs, t0: int, nlags: int, center: torch.Tensor | None = None) -> torch.Tensor:
    """R(t) = sum_i (da_i db_{i+t} + db_i da_{i+t}) of the centred series, t = t0 .. t0 + nlags - 1, for every pair of
    ``pairs``: index 0 is (u, u), 1 + c is (x_c, x_c), 1 + C + c is (x_c, u).  x: (N, C) row-major (any row pitch), (N,)
    or None; u: (N,).  Returns (len(pairs), nlags); lags >= N are 0.  Bitwise reproducible, and independent of how the
    lags are cut into 256-aligned calls."""
    L = _L()
    x2, u, N, C, ls = _lag_series_args(x, u)
    if center is None:
        center = lag_center(x2, u)
    _check_f64_cuda(center, "center")
    if center.shape != (1 + C,):
        raise ValueError(f"center must have shape ({1 + C},), got {tuple(center.shape)}")
    center = center.contiguous()
    pl = np.ascontiguousarray(np.atleast_1d(np.asarray(pairs)).astype(np.int32))
    if pl.ndim != 1 or pl.size == 0:
        raise ValueError("pairs must be a non-empty list of pair indices")
    out = torch.empty((pl.size, int(nlags)), dtype=F64, device="cuda")
    nws = L.txm_lag_sums_ws_bytes(N, C, pl.size, int(nlags))
    ws = workspace(nws, tag="lag")
    check(L.txm_lag_sums(_ptr(x2), ls, _ptr(u), N, C, _ptr(center), pl.ctypes.data_as(ct.POINTER(ct.c_int32)), pl.size,
                         int(t0), int(nlags), _ptr(out), _ptr(ws), ws.numel(), _stream()), "txm_lag_sums")
    return out


LAG_MAX_ORIGINS = 4096  # origins per call of lag_origin_sums (txm_lagsum.hip: LG_MAX_ORIGINS)


def lag_origin_center(x: torch.Tensor | None, u: torch.Tensor) -> torch.Tensor:
    """The default pivots of ``lag_origin_sums``, (1 + C,): the mean of the SECOND HALF of each series."""
    h = u.shape[0] // 2
    return lag_center(None if x is None else (x.unsqueeze(1) if x.dim() == 1 else x)[h:], u[h:])


def lag_origin_sums(x: torch.Tensor | None, u: torch.Tensor, series, nskip: int, t0: int, nlags: int,
                    center: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """The auto lag sums of every suffix: for each series of ``series`` (0 is u, 1 + c is x_c) and each origin
    j * nskip in range(0, N - 1, nskip), R_j(t) = 2 sum_i (a_i - m_j)(a_{i+t} - m_j) over the suffix a[j nskip:] centred
    with its own mean m_j, t = t0 .. t0 + nlags - 1 (multiples of 256; lags beyond the suffix give 0).  Returns
    (R (len(series), n_origins, nlags), suffix means (len(series), n_origins)) from one pass over the samples.

    ``center`` (1 + C,) is the pivot the series are centred on once; R_j is expanded around it (txmom.h, (f-8)).  None:
    the mean of the second half of each series -- the origins that matter lie past the transient, so their
    delta_j = m_j - pivot nearly vanishes and R_j is not a difference of large terms.

    When the workspace for ``nlags`` exceeds ``workspace_budget()`` the call is made in shorter lag blocks; the bits do
    not depend on that (nor on how the caller cuts the lags into 256-aligned calls), and two runs give the same bits."""
    L = _L()
    x2, u, N, C, ls = _lag_series_args(x, u)
    if center is None:
        center = lag_origin_center(x2, u)
    _check_f64_cuda(center, "center")
    if center.shape != (1 + C,):
        raise ValueError(f"center must have shape ({1 + C},), got {tuple(center.shape)}")
    center = center.contiguous()
    sl = np.ascontiguousarray(np.atleast_1d(np.asarray(series)).astype(np.int32))
    if sl.ndim != 1 or sl.size == 0:
        raise ValueError("series must be a non-empty list of series indices")
    nskip, t0, nlags = int(nskip), int(t0), int(nlags)
    no = -(-(N - 1) // nskip) if N >= 2 and nskip >= 1 else 0   # len(range(0, N - 1, nskip))
    from .timeseries import pick_nskip

    pick_nskip(N, nskip)          # (ValueError before anything of n_origins x nlags is allocated)
    step = nlags
    if nlags >= 2 * LAG_BLOCK and L.txm_lag_origin_sums_ws_bytes(N, C, sl.size, nskip, nlags) > workspace_budget():
        step = LAG_BLOCK
        for cand in (2048, 1024, 512):
            if cand < nlags and nlags % cand == 0 and L.txm_lag_origin_sums_ws_bytes(N, C, sl.size, nskip, cand) <= workspace_budget():
                step = cand
                break
    out = torch.empty((sl.size, no, nlags), dtype=F64, device="cuda")
    mean = torch.empty((sl.size, no), dtype=F64, device="cuda")
    ws = workspace(L.txm_lag_origin_sums_ws_bytes(N, C, sl.size, nskip, step), tag="lag")
    sp = sl.ctypes.data_as(ct.POINTER(ct.c_int32))
    for off in range(0, nlags, step):
        part = out if step == nlags else torch.empty((sl.size, no, step), dtype=F64, device="cuda")
        check(L.txm_lag_origin_sums(_ptr(x2), ls, _ptr(u), N, C, _ptr(center), sp, sl.size, nskip, t0 + off, step, _ptr(part),
                                    _ptr(mean), _ptr(ws), ws.numel(), _stream()), "txm_lag_origin_sums")
        if part is not out:
            out[:, :, off:off + step] = part
    return out, mean


# ---------------------------------------------------------------------------
# lag sums of a state collection (timeseries.statistical_inefficiencies_states): the centred rows of all states from one
# launch, kept over the lag blocks of a scan; every (state, pair) of a block from one launch set
# ---------------------------------------------------------------------------
LAG_MAX_ITEMS = 65535  # (state, pair) items per library call (the item rides grid.y)


def lag_chunks(n: int) -> int:
    """The number of sample chunks the lag kernels cut a series of n records into (txm_lagsum.hip: lg_chunk_len)."""
    n = int(n)
    return -(-n // (LAG_STAGE * max(1, -(-n // (LAG_STAGE * 512)))))


def lag_sums_batched_ws_bytes(ns, items, nlags: int) -> int:
    """txm_lag_sums_batched_ws_bytes restated on the host: the item table (16 bytes per item, padded to 256) and one
    partial per (item, chunk of its state, lag)."""
    return -(-16 * len(items) // 256) * 256 + 8 * int(nlags) * sum(lag_chunks(ns[s]) for s, _ in items)


def lag_item_slices(ns, items, nlags: int, budget: int) -> list[slice]:
    """The cuts of ``items`` [(state, pair), ...] into library calls: consecutive runs, each as long as its workspace
    (``lag_sums_batched_ws_bytes``) fits ``budget`` and it has at most 65535 items -- at least one item, fitting or not."""
    out, a, chunks = [], 0, 0
    per = 8 * int(nlags)
    for i, (s, _) in enumerate(items):
        c = lag_chunks(ns[s])
        k = i - a + 1
        if i > a and (k > LAG_MAX_ITEMS or -(-16 * k // 256) * 256 + per * (chunks + c) > budget):
            out.append(slice(a, i))
            a, chunks = i, 0
        chunks += c
    if len(items) > a:
        out.append(slice(a, len(items)))
    return out


class LagRows(NamedTuple):
    """What ``lag_rows_batched`` returns and ``lag_sums_batched`` takes: the rows buffer of txm_lag_rows_batched, the record
    counts it was made with, the column count and the centres (S tensors of (1 + C,))."""

    rows: torch.Tensor
    ns: np.ndarray
    C: int
    centers: list


def lag_rows_batched(xs, us, centers=None) -> LagRows:
    """The centred, transposed series of S states from ONE launch, for any number of ``lag_sums_batched`` calls.  xs: S
    tensors (n_s, C) sharing C (None, or a list of None, for the energies alone), us: S tensors (n_s,).  ``centers``: S
    tensors (1 + C,); None takes ``lag_center`` of every state -- S small reductions, and the very means ``lag_sums``
    takes, so that every lag sum equals the single-state call's bit for bit."""
    L = _L()
    S = len(us)
    if S == 0:
        raise ValueError("no states")
    xs = [None] * S if xs is None else list(xs)
    if len(xs) != S:
        raise ValueError(f"{len(xs)} sample matrices for {S} energy series")
    args = [_lag_series_args(x, u) for x, u in zip(xs, us)]
    C = args[0][3]
    if any(a[3] != C for a in args):
        raise ValueError(f"the states differ in their column count: {sorted({a[3] for a in args})}")
    x2s = [a[0] for a in args]
    ls = 0
    if C:                                            # one row pitch for the launch (a single row has none of its own)
        pitches = {a[4] for a in args if a[2] > 1}
        ls = pitches.pop() if len(pitches) == 1 else C
        if pitches:
            x2s = [x2.contiguous() for x2 in x2s]
    u2s = [a[1] for a in args]
    if centers is None:
        centers = [lag_center(None if x is None else (x.unsqueeze(1) if x.dim() == 1 else x), u) for x, u in zip(xs, u2s)]
    centers = list(centers)
    if len(centers) != S:
        raise ValueError(f"{len(centers)} centres for {S} states")
    for c in centers:
        _check_f64_cuda(c, "center")
        if c.shape != (1 + C,):
            raise ValueError(f"center must have shape ({1 + C},), got {tuple(c.shape)}")
    centers = [c.contiguous() for c in centers]
    ns = np.ascontiguousarray([a[2] for a in args], dtype=np.int64)
    tab = (_lib.LagState * S)(*[_lib.LagState(x2.data_ptr() if C else None, u.data_ptr(), c.data_ptr(), int(n))
                                for x2, u, c, n in zip(x2s, u2s, centers, ns)])
    nbytes = L.txm_lag_rows_batched_bytes(ns.ctypes.data_as(ct.POINTER(ct.c_int64)), S, C)
    if nbytes == 0:
        raise ValueError(f"lag_rows_batched: {S} states of {C} columns and {int(ns.min())} .. {int(ns.max())} records are out of range")
    rows = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    check(L.txm_lag_rows_batched(tab, S, ls, C, _ptr(rows), nbytes, _stream()), "txm_lag_rows_batched")
    return LagRows(rows, ns, C, centers)


def lag_sums_batched(handle: LagRows, items, t0: int, nlags: int) -> torch.Tensor:
    """R(t), t = t0 .. t0 + nlags - 1, of every (state, pair) of ``items`` (pair as in ``lag_sums``; any order, any subset)
    from the rows of ``lag_rows_batched``: (len(items), nlags), row i bit for bit ``lag_sums`` of that state and pair
    with the handle's centre.  The item list is cut into several library calls where the partials (one per item, chunk
    and lag) would exceed ``workspace_budget()``, and at 65535 items; the cuts change no bits."""
    L = _L()
    items = [(int(s), int(p)) for s, p in items]
    if not items:
        raise ValueError("items must be a non-empty list of (state, pair)")
    S, C, ns = len(handle.ns), handle.C, handle.ns
    for s, p in items:
        if not (0 <= s < S and 0 <= p <= 2 * C):
            raise ValueError(f"item ({s}, {p}) outside {S} states x pairs [0, {2 * C}]")
    t0, nlags = int(t0), int(nlags)
    out = torch.empty((len(items), nlags), dtype=F64, device="cuda")
    np_ns = ns.ctypes.data_as(ct.POINTER(ct.c_int64))
    for sl in lag_item_slices(ns, items, nlags, workspace_budget()):
        part = items[sl]
        tab = (_lib.LagItem * len(part))(*[_lib.LagItem(s, p) for s, p in part])
        nws = L.txm_lag_sums_batched_ws_bytes(np_ns, S, C, tab, len(part), nlags)
        ws = workspace(nws, tag="lag")
        check(L.txm_lag_sums_batched(_ptr(handle.rows), handle.rows.numel(), np_ns, S, C, tab, len(part), t0, nlags,
                                     _ptr(out[sl.start:sl.stop]), _ptr(ws), ws.numel(), _stream()), "txm_lag_sums_batched")
    return out
