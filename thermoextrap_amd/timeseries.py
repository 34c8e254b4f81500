"""Statistical inefficiency and decorrelation of simulation time series on the device.

The reference decorrelates before it builds a state (gpr_active/active_utils.py:244-269, ``DataWrapper.get_data``):
``pymbar.timeseries.statistical_inefficiency`` of every observable column, of the potential energy and of every (column,
energy) pair, the largest of them as g, ``subsample_correlated_data`` with it, and only then
``DataCentralMomentsVals.from_vals``.  This module is that half of pymbar for samples that live in HBM:

  statistical_inefficiency, normalized_fluctuation_correlation_function, subsample_correlated_data
      pymbar.timeseries' functions of the same names (unweighted series);
  statistical_inefficiencies(uv, xv)   all 2C + 1 pairs of a state through one set of launches;
  decorrelate(uv, xv, w)               what get_data lines 253-269 do, the gather on the device.

The estimator.  dA = A - mean(A), dB = B - mean(B) (B = A when omitted), sigma^2 = mean(dA dB) (0 raises ValueError),

    R(t) = sum_{n=0}^{N-1-t} (dA_n dB_{n+t} + dB_n dA_{n+t}),   C(t) = R(t) / (2 (N - t) sigma^2),   sigma^2 = R(0) / (2 N)

    g = 1; t = 1; inc = 1
    while t < N - 1:
        if C(t) <= 0 and t > mintime: break
        g += 2 C(t) (1 - t / N) inc;  t += inc;  if fast: inc += 1
    return max(g, 1)

The lag sums R(t) are the device work (engine.lag_sums -> txm_lag_sums, the FP64 matrix pipe on Toeplitz slices); the loop
over t runs on the host over blocks of lags -- 256, 256, 512, 1024, ... lags, each block doubling the covered range, at most
4096 lags per call, one device-to-host copy of [pairs][lags] doubles per block.  Pairs that have stopped are dropped from
the next call's list; the scan ends when every pair has stopped or t reaches N - 1.  R(t) has the same bits in whichever
block it is computed, so g does not depend on the schedule.  There is no CPU path: every function that takes series needs
the device (``require_gpu``), as everywhere in this package.
"""

from __future__ import annotations

import math
from typing import Callable, NamedTuple

import numpy as np

LAG_BLOCK = 256
LAG_MAX_LAGS = 4096


class Inefficiencies(NamedTuple):
    """What ``statistical_inefficiencies`` returns.  ``stop_*``: the lag at which the loop of each pair ended -- the first
    visited t > mintime with C(t) <= 0, or the first visited t >= N - 1 when the series ran out before that."""

    g_u: float
    g_x: np.ndarray        # (C,)  (x_c, x_c)
    g_cross: np.ndarray    # (C,)  (x_c, u)
    g_max: float
    stop_u: int
    stop_x: np.ndarray     # (C,) int64
    stop_cross: np.ndarray # (C,) int64


def lag_blocks(n: int):
    """The host scan's lag blocks (t0, nlags): (0, 256), (256, 256), (512, 512), (1024, 1024), ... -- each doubles the
    covered range, capped at 4096 lags per call -- while t0 < n - 1 (block 0 always: it holds sigma^2)."""
    t0, nl = 0, LAG_BLOCK
    while True:
        yield t0, nl
        t0 += nl
        nl = min(t0, LAG_MAX_LAGS)
        if t0 >= n - 1:
            return


def scan_lag_sums(fetch: Callable[[list, int, int], np.ndarray], n: int, pair_ids, *, fast: bool = False, mintime: int = 3,
                  max_lag: int | None = None, names=None):
    """The loop for g over blocks of lag sums.  ``fetch(pairs, t0, nlags)`` returns R(t0 .. t0 + nlags - 1) of the listed
    pairs as a (len(pairs), nlags) float64 array (the device call, or numpy in the CPU tests).  Returns (g, stop) arrays in
    the order of ``pair_ids``.  Raises ValueError when a pair has sigma^2 == 0, or has not stopped by ``max_lag``."""
    pair_ids = [int(p) for p in pair_ids]
    m = len(pair_ids)
    names = list(names) if names is not None else [f"pair {p}" for p in pair_ids]
    g = np.ones(m)
    t = np.ones(m, dtype=np.int64)
    inc = np.ones(m, dtype=np.int64)
    sig2 = np.zeros(m)
    active = list(range(m))
    for t0, nl in lag_blocks(n):
        if not active:
            break
        R = np.asarray(fetch([pair_ids[k] for k in active], t0, nl), dtype=np.float64)
        if R.shape != (len(active), nl):
            raise ValueError(f"fetch returned {R.shape}, expected {(len(active), nl)}")
        still = []
        for row, k in enumerate(active):
            if t0 == 0:
                sig2[k] = R[row, 0] / (2.0 * n)
                if sig2[k] == 0.0:
                    raise ValueError(f"sample covariance sigma_AB^2 = 0 for {names[k]}: cannot compute the statistical inefficiency")
            tk, ik, gk, done = int(t[k]), int(inc[k]), g[k], False
            while tk < t0 + nl:
                if tk >= n - 1:
                    done = True
                    break
                if max_lag is not None and tk > max_lag:
                    raise ValueError(f"the correlation function of {names[k]} has not crossed zero by max_lag = {max_lag}")
                c = R[row, tk - t0] / (2.0 * (n - tk) * sig2[k])
                if c <= 0.0 and tk > mintime:
                    done = True
                    break
                gk += 2.0 * c * (1.0 - tk / n) * ik
                tk += ik
                if fast:
                    ik += 1
            t[k], inc[k], g[k] = tk, ik, gk
            if not done and tk < n - 1:
                still.append(k)
        active = still
    return np.maximum(g, 1.0), t


def subsample_correlated_data(A_t, g: float | None = None, fast: bool = False, conservative: bool = False) -> np.ndarray:
    """Indices of an uncorrelated subsample (pymbar.timeseries.subsample_correlated_data).  T = len(A_t), or A_t itself when
    it is an int; g defaults to statistical_inefficiency(A_t, fast=fast).  conservative: range(0, T, ceil(g)); otherwise
    t = round(n g) for n = 0, 1, ... while t < T, an index equal to its predecessor dropped (round: half to even)."""
    if isinstance(A_t, (int, np.integer)):
        T = int(A_t)
    else:
        T = len(A_t)
        if g is None:
            g = statistical_inefficiency(A_t, fast=fast)
    if g is None:
        raise ValueError("g is required when A_t is a length")
    g = float(g)
    if not (g > 0.0) or not math.isfinite(g):
        raise ValueError(f"g = {g} must be positive and finite")
    if T <= 0:
        return np.zeros(0, dtype=np.int64)
    if conservative:
        return np.arange(0, T, int(math.ceil(g)), dtype=np.int64)
    m = int(math.ceil(T / g)) + 2                       # n g < T + 1/2 for every kept n
    t = np.rint(np.arange(m, dtype=np.float64) * g)
    t = t[: int(np.searchsorted(t, T, side="left"))].astype(np.int64)   # non-decreasing: the kept ones are a prefix
    keep = np.ones(t.size, dtype=bool)
    keep[1:] = t[1:] != t[:-1]
    return t[keep]


# ---------------------------------------------------------------------------
# device side
# ---------------------------------------------------------------------------
def _device_series(a, ndim: int, name: str):
    """A float64 CUDA tensor of the given rank from a numpy array, a device tensor, an xrlite.DataArray or a
    DeviceDataArray; (tensor, kind) with kind "host" or "device" (what ``decorrelate`` hands back)."""
    import torch

    from . import engine
    from .moments import DeviceDataArray
    from .xrlite import is_labelled, as_labelled

    if isinstance(a, DeviceDataArray):
        t, kind = a.tensor, "device"
    elif isinstance(a, torch.Tensor):
        t, kind = a.to(device="cuda", dtype=torch.float64), "device"
    elif isinstance(a, np.ndarray):
        t, kind = engine.to_device(a), "host"
    elif is_labelled(a):
        t, kind = engine.to_device(np.asarray(as_labelled(a).values)), "host"
    else:
        raise TypeError(f"{name}: expected a numpy array, a device tensor or a DataArray, got {type(a).__name__}")
    if t.dim() != ndim:
        raise ValueError(f"{name} must have {ndim} dimension(s) ({'rec' if ndim == 1 else 'rec, val'}), got shape {tuple(t.shape)}")
    return t, kind


def _pair_names(C: int):
    return ["u"] + [f"x[{c}]" for c in range(C)] + [f"(x[{c}], u)" for c in range(C)]


def _fetcher(x, u):
    from . import engine

    center = engine.lag_center(x, u)

    def fetch(pairs, t0, nlags):
        return engine.lag_sums(x, u, pairs, t0, nlags, center=center).cpu().numpy()

    return fetch


def _prepare(uv, xv):
    from ._lib import require_gpu

    require_gpu()
    u, ku = _device_series(uv, 1, "uv")
    x, kx = (None, ku) if xv is None else _device_series(xv, 2, "xv")
    if x is not None and x.shape[0] != u.shape[0]:
        raise ValueError(f"xv has {x.shape[0]} records, uv {u.shape[0]}")
    return u, x, ("device" if "device" in (ku, kx) else "host")


def statistical_inefficiencies(uv, xv, *, fast: bool = False, mintime: int = 3, max_lag: int | None = None) -> Inefficiencies:
    """g of the energy series uv (rec), of every column of xv (rec, val) and of every (column, energy) pair: all 2C + 1
    pairs in one set of launches per lag block."""
    u, x, _ = _prepare(uv, xv)
    C = 0 if x is None else x.shape[1]
    n = u.shape[0]
    g, stop = scan_lag_sums(_fetcher(x, u), n, range(2 * C + 1), fast=fast, mintime=mintime, max_lag=max_lag,
                            names=_pair_names(C))
    return Inefficiencies(float(g[0]), g[1:1 + C].copy(), g[1 + C:].copy(), float(g.max()), int(stop[0]),
                          stop[1:1 + C].copy(), stop[1 + C:].copy())


def _one_pair(A_n, B_n):
    """(x, u, pair index, n) of pymbar's (A_n, B_n): the auto pair of A, or the cross pair (A, B)."""
    if B_n is None:
        u, _, _ = _prepare(A_n, None)
        return None, u, 0
    from ._lib import require_gpu

    require_gpu()
    a, _ = _device_series(A_n, 1, "A_n")
    b, _ = _device_series(B_n, 1, "B_n")
    if a.shape != b.shape:
        raise ValueError(f"A_n and B_n differ in length: {a.shape[0]} and {b.shape[0]}")
    return a.unsqueeze(1).contiguous(), b, 2


def statistical_inefficiency(A_n, B_n=None, fast: bool = False, mintime: int = 3, *, max_lag: int | None = None) -> float:
    """pymbar.timeseries.statistical_inefficiency for one series or one pair of series (max_lag None: pymbar's behaviour;
    an int: ValueError if the correlation function has not crossed zero by then)."""
    x, u, p = _one_pair(A_n, B_n)
    g, _ = scan_lag_sums(_fetcher(x, u), u.shape[0], [p], fast=fast, mintime=mintime, max_lag=max_lag,
                         names=["A_n" if B_n is None else "(A_n, B_n)"])
    return float(g[0])


def normalized_fluctuation_correlation_function(A_n, B_n=None, *, N_max: int, norm: bool = True) -> np.ndarray:
    """R(t) / (2 (N - t)) for t = 0 .. N_max, divided by sigma^2 if ``norm``.  N_max is required (pymbar's None means all
    N lags, which is O(N^2)) and must be below N."""
    x, u, p = _one_pair(A_n, B_n)
    n = u.shape[0]
    N_max = int(N_max)
    if not 0 <= N_max < n:
        raise ValueError(f"N_max = {N_max} outside [0, N - 1 = {n - 1}]")
    fetch = _fetcher(x, u)
    need = N_max + 1
    parts, t0 = [], 0
    while t0 < need:
        nl = min(LAG_MAX_LAGS, -(-(need - t0) // LAG_BLOCK) * LAG_BLOCK)
        parts.append(fetch([p], t0, nl)[0])
        t0 += nl
    R = np.concatenate(parts)[:need]
    sig2 = R[0] / (2.0 * n)
    if norm and sig2 == 0.0:
        raise ValueError("sample covariance sigma_AB^2 = 0: cannot normalise the correlation function")
    c = R / (2.0 * (n - np.arange(need, dtype=np.float64)))
    return c / sig2 if norm else c


def decorrelate(uv, xv, w=None, *, g: float | None = None, conservative: bool = False, **kw):
    """Subsample (uv, xv, w) to uncorrelated records as DataWrapper.get_data does (gpr_active/active_utils.py:253-269):
    g = the largest statistical inefficiency over the energy, every observable column and every (column, energy) pair
    (or the given g), indices = subsample_correlated_data(N, g), the gather on the device.  Returns (uv, xv, w, info): the
    subsampled arrays with dims (rec) / (rec, val) -- ``DeviceDataArray`` when an input lived on the device, ``DataArray``
    otherwise; both feed ``from_vals`` unchanged -- and info = {"g", "indices", "n", "inefficiencies"}.  Further keywords
    (fast, mintime, max_lag) go to ``statistical_inefficiencies``."""
    import torch

    from .moments import DeviceDataArray
    from .xrlite import DataArray

    u, x, kind = _prepare(uv, xv)
    if x is None:
        raise TypeError("xv is required")
    wt = None
    if w is not None:
        wt, kw_kind = _device_series(w, 1, "w")
        if wt.shape != u.shape:
            raise ValueError(f"w has {wt.shape[0]} records, uv {u.shape[0]}")
    ineff = None
    if g is None:
        ineff = statistical_inefficiencies(u, x, **kw)
        g = ineff.g_max
    elif kw:
        raise TypeError(f"keywords {sorted(kw)} only apply when g is estimated")
    idx = subsample_correlated_data(u.shape[0], g, conservative=conservative)
    di = torch.as_tensor(idx).to("cuda")
    outs = [u.index_select(0, di), x.index_select(0, di), None if wt is None else wt.index_select(0, di)]
    dims = [("rec",), ("rec", "val"), ("rec",)]
    if kind == "device":
        outs = [None if t is None else DeviceDataArray(t, d) for t, d in zip(outs, dims)]
    else:
        outs = [None if t is None else DataArray(t.cpu().numpy(), d) for t, d in zip(outs, dims)]
    info = {"g": float(g), "indices": idx, "n": int(idx.size), "inefficiencies": ineff}
    return outs[0], outs[1], outs[2], info
