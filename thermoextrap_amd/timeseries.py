"""Statistical inefficiency and decorrelation of simulation time series on the device.

The reference decorrelates before it builds a state (gpr_active/active_utils.py:244-269, ``DataWrapper.get_data``):
``pymbar.timeseries.statistical_inefficiency`` of every observable column, of the potential energy and of every (column,
energy) pair, the largest of them as g, ``subsample_correlated_data`` with it, and only then
``DataCentralMomentsVals.from_vals``.  This module is that half of pymbar for samples that live in HBM:

  statistical_inefficiency, normalized_fluctuation_correlation_function, subsample_correlated_data
      pymbar.timeseries' functions of the same names (unweighted series);
  statistical_inefficiencies(uv, xv)   all 2C + 1 pairs of a state through one set of launches;
  decorrelate(uv, xv, w)               what get_data lines 253-269 do, the gather on the device;
  detect_equilibration                 pymbar.timeseries' function of that name: where the initial transient ends;
  detect_equilibrations(uv, xv)        the same for the energy and every observable column in one set of launches;
  equilibrate(uv, xv, w)               drops the transient on the device; its output feeds decorrelate unchanged.
  statistical_inefficiencies_states, decorrelate_states, block_lengths
      the same for a COLLECTION of states (lists of uv, xv; one column count, any record counts): the centred series of all
      states made once and kept over the scan, one set of launches and one copy per lag block for every state
      (engine.lag_rows_batched, lag_sums_batched -> txm_lag_rows_batched, txm_lag_sums_batched); every result equals the
      single-state function's in every field.

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

Equilibration (Chodera 2016).  For the origins t0 in range(0, T - 1, nskip): g(t0) = statistical_inefficiency(A[t0:]) (the
estimator above on the suffix, centred with the suffix's own mean; a suffix of zero variance gives g = T - t0 + 1),
Neff(t0) = (T - t0 + 1) / g(t0); the answer is the origin of the largest Neff (the first on a tie); a series of zero variance
gives (0, 1, 1).  The lag sums of EVERY origin come from one pass over the samples per lag block (engine.lag_origin_sums ->
txm_lag_origin_sums: per-segment partials, a suffix scan over the segments), not from one scan per origin; the host runs the
loop above once per (series, origin) over one fetch of [series][origins][lags] per block.
"""

from __future__ import annotations

import math
from typing import Callable, NamedTuple

import numpy as np

LAG_BLOCK = 256
LAG_MAX_LAGS = 4096


class Equilibration(NamedTuple):
    """What ``detect_equilibrations`` returns, series 0 the energy and 1 + c column c.  ``t0_max``: the largest detected
    origin -- the conservative choice, as ``decorrelate`` takes the largest g."""

    t0: np.ndarray         # (1 + C,) int64: the origin of the largest Neff
    g: np.ndarray          # (1 + C,)  g of the series from there on
    neff: np.ndarray       # (1 + C,)  (T - t0 + 1) / g
    t0_max: int
    origins: np.ndarray    # (1 + C, n_origins) int64: the origins tested, range(0, T - 1, nskip)
    g_t: np.ndarray        # (1 + C, n_origins)
    neff_t: np.ndarray     # (1 + C, n_origins)


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


def _scan_block(R, t0: int, nl: int, n: int, sig2, tk: int, ik: int, gk, fast: bool, mintime: int, max_lag, name):
    """The loop for g of one series of length n over one block R = R(t0 .. t0 + nl - 1) of its lag sums, from the state
    (t, inc, g) the previous block left.  Returns (t, inc, g, done): done when the loop has ended inside this block."""
    while tk < t0 + nl:
        if tk >= n - 1:
            return tk, ik, gk, True
        if max_lag is not None and tk > max_lag:
            raise ValueError(f"the correlation function of {name} has not crossed zero by max_lag = {max_lag}")
        c = R[tk - t0] / (2.0 * (n - tk) * sig2)
        if c <= 0.0 and tk > mintime:
            return tk, ik, gk, True
        gk += 2.0 * c * (1.0 - tk / n) * ik
        tk += ik
        if fast:
            ik += 1
    return tk, ik, gk, False


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
            tk, ik, gk, done = _scan_block(R[row], t0, nl, n, sig2[k], int(t[k]), int(inc[k]), g[k], fast, mintime, max_lag, names[k])
            t[k], inc[k], g[k] = tk, ik, gk
            if not done and tk < n - 1:
                still.append(k)
        active = still
    return np.maximum(g, 1.0), t


def origin_count(T: int, nskip: int) -> int:
    """len(range(0, T - 1, nskip))."""
    return -(-(int(T) - 1) // int(nskip)) if T >= 2 else 0


def pick_nskip(T: int, nskip: int | None = None, max_origins: int = 512) -> int:
    """The origin step of ``detect_equilibration``: the given one, or (None) the smallest that gives at most ``max_origins``
    origins.  ValueError for a series of fewer than 2 records and for a step that needs more origins than one device call
    takes (engine.LAG_MAX_ORIGINS = 4096)."""
    from .engine import LAG_MAX_ORIGINS as most

    T = int(T)
    if T < 2:
        raise ValueError(f"a series of {T} record(s) has no origin to test")
    if nskip is None:
        if not 1 <= int(max_origins) <= most:
            raise ValueError(f"max_origins = {max_origins} outside [1, {most}]")
        return max(1, -(-(T - 1) // int(max_origins)))
    nskip = int(nskip)
    if nskip < 1:
        raise ValueError(f"nskip = {nskip} < 1")
    if origin_count(T, nskip) > most:
        raise ValueError(f"nskip = {nskip} gives {origin_count(T, nskip)} origins for T = {T}, more than {most} per call: "
                         f"the smallest legal nskip is {-(-(T - 1) // most)}")
    return nskip


def _expansion_bound(R0: float, M: int, delta: float) -> float:
    """1e-12 * 2 (sqrt(Q) + sqrt(M) |delta|)^2 with Q = R0 / 2 + M delta^2: what R_j(0) of a pivot expansion is good to."""
    q = max(0.5 * R0 + M * delta * delta, 0.0)
    return 2e-12 * (math.sqrt(q) + math.sqrt(M) * abs(delta)) ** 2


def scan_origin_lag_sums(fetch: Callable[[list, int, int], np.ndarray], n: int, nskip: int, series_ids, *, fast: bool = True,
                         mintime: int = 3):
    """``scan_lag_sums`` for every suffix of every listed series.  ``fetch(series, t0, nlags)`` returns R_j(t0 .. t0 + nlags - 1)
    of the suffixes A[j nskip:] as a (len(series), n_origins, nlags) float64 array (the device call, or numpy in the CPU
    tests).  Each (series, origin) runs the loop for g with its own length M = n - j nskip; a suffix with sigma^2 == 0 takes
    g = M + 1 (pymbar's fallback in detect_equilibration).  A series leaves the fetch list when all its origins have stopped.

    A fetch that expands R_j around a pivot (the device: R = 2 [Q - delta X + (M - t) delta^2]) gets a constant suffix away
    from the pivot to zero only up to rounding.  Such a fetch returns (R, delta) on the block t0 == 0, delta
    (len(series), n_origins) the suffix means minus the pivot, and sigma^2 counts as 0 when |R_j(0)| is within the
    expansion's own rounding bound 1e-12 * 2 sum (|d| + |delta|)^2 <= 1e-12 * 2 (sqrt(Q_j(0)) + sqrt(M) |delta|)^2, with
    Q_j(0) = R_j(0) / 2 + M delta^2 (the bound the device is tested to).  With delta == 0 that is R_j(0) == 0.

    Returns (g, stop, zero): (len(series_ids), n_origins) arrays; ``zero`` marks the fallback."""
    series_ids = [int(p) for p in series_ids]
    m, no = len(series_ids), origin_count(n, nskip)
    M = n - nskip * np.arange(no, dtype=np.int64)
    g = np.ones((m, no))
    t = np.ones((m, no), dtype=np.int64)
    inc = np.ones((m, no), dtype=np.int64)
    sig2 = np.zeros((m, no))
    zero = np.zeros((m, no), dtype=bool)
    live = [[j for j in range(no)] for _ in range(m)]      # the origins of each series whose loop has not ended
    for t0, nl in lag_blocks(n):
        active = [k for k in range(m) if live[k]]
        if not active:
            break
        R = fetch([series_ids[k] for k in active], t0, nl)
        delta = None
        if isinstance(R, tuple):
            R, delta = R
        R = np.asarray(R, dtype=np.float64)
        if R.shape != (len(active), no, nl):
            raise ValueError(f"fetch returned {R.shape}, expected {(len(active), no, nl)}")
        for row, k in enumerate(active):
            still = []
            for j in live[k]:
                Mj = int(M[j])
                if t0 == 0:
                    sig2[k, j] = R[row, j, 0] / (2.0 * Mj)
                    if abs(R[row, j, 0]) <= _expansion_bound(R[row, j, 0], Mj, 0.0 if delta is None else delta[row][j]):
                        g[k, j], zero[k, j] = Mj + 1.0, True
                        continue
                tk, ik, gk, done = _scan_block(R[row, j], t0, nl, Mj, sig2[k, j], int(t[k, j]), int(inc[k, j]), g[k, j], fast,
                                               mintime, None, None)
                t[k, j], inc[k, j], g[k, j] = tk, ik, gk
                if not done and tk < Mj - 1:
                    still.append(j)
            live[k] = still
    return np.where(zero, g, np.maximum(g, 1.0)), t, zero


def pick_origin(M, g, zero):
    """(index, g, Neff) of the origin with the largest Neff = (M + 1) / g, the first on a tie, and the Neff of every origin;
    a series whose first suffix -- the whole series -- has zero variance gives (0, 1.0, 1.0)."""
    neff = (np.asarray(M, dtype=np.float64) + 1.0) / g
    if zero[0]:
        return 0, 1.0, 1.0, neff
    j = int(np.argmax(neff))
    return j, float(g[j]), float(neff[j]), neff


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


def block_length(uv, xv, factor: float = 10.0, **kw) -> int:
    """A block length for the blocked error bars (``ExtrapModel.derivs_cov(block=...)``): ``ceil(factor * g_max)`` with
    g_max the largest statistical inefficiency of ``statistical_inefficiencies(uv, xv, **kw)``.

    For an AR(1)-like series the relative bias of batch means is about ``-g / (2 B)``, so the default factor of 10 leaves
    about -5 % on the variance (-2.5 % on the standard deviation).  g_max is taken over the raw observables, while what
    the error bar of the k-th derivative needs is the g of its own influence series, which differs with the order: treat
    the result as a starting point and CHECK it with ``ExtrapModel.blocking_curve`` -- the variance must have levelled
    off at the chosen block length."""
    if not factor > 0:
        raise ValueError(f"factor must be positive, got {factor}")
    return max(1, int(math.ceil(float(factor) * statistical_inefficiencies(uv, xv, **kw).g_max)))


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


def detect_equilibrations(uv, xv, *, fast: bool = True, nskip: int | None = None, mintime: int = 3,
                          max_origins: int = 512) -> Equilibration:
    """``detect_equilibration`` of the energy series uv (rec) and of every column of xv (rec, val; may be None): the 1 + C
    auto series through one set of launches per lag block.  See ``detect_equilibration`` for nskip and max_origins."""
    from . import engine

    u, x, _ = _prepare(uv, xv)
    C = 0 if x is None else x.shape[1]
    n = u.shape[0]
    nskip = pick_nskip(n, nskip, max_origins)
    center = engine.lag_origin_center(x, u)

    def fetch(series, t0, nlags):
        R, mean = engine.lag_origin_sums(x, u, series, nskip, t0, nlags, center=center)
        if t0 == 0:
            return R.cpu().numpy(), (mean - center[list(series)][:, None]).cpu().numpy()
        return R.cpu().numpy()

    g_t, _, zero = scan_origin_lag_sums(fetch, n, nskip, range(1 + C), fast=fast, mintime=mintime)
    origins = nskip * np.arange(g_t.shape[1], dtype=np.int64)
    picks = [pick_origin(n - origins, g_t[s], zero[s]) for s in range(1 + C)]
    t0 = np.array([origins[p[0]] for p in picks], dtype=np.int64)
    return Equilibration(t0, np.array([p[1] for p in picks]), np.array([p[2] for p in picks]), int(t0.max()),
                         np.tile(origins, (1 + C, 1)), g_t, np.stack([p[3] for p in picks]))


def detect_equilibration(A_t, fast: bool = True, nskip: int | None = None, *, mintime: int = 3, max_origins: int = 512):
    """pymbar.timeseries.detect_equilibration: (t, g, Neff_max) -- the origin t in range(0, T - 1, nskip) from which the
    series has the most uncorrelated samples, its statistical inefficiency from there on, and that number of samples.
    nskip None picks the smallest step that gives at most ``max_origins`` origins (pymbar's default of 1 tests every record,
    which is O(T^2) there and T origins here); an explicit nskip that needs more than 4096 origins raises ValueError."""
    e = detect_equilibrations(A_t, None, fast=fast, nskip=nskip, mintime=mintime, max_origins=max_origins)
    return int(e.t0[0]), float(e.g[0]), float(e.neff[0])


def equilibrate(uv, xv, w=None, *, t0: int | None = None, **kw):
    """Drop the initial transient of (uv, xv, w) on the device: the first ``t0`` records, by default
    ``detect_equilibrations(uv, xv, **kw).t0_max``.  Returns (uv, xv, w, info) of the kinds and dims ``decorrelate`` returns --
    they feed ``decorrelate`` and then ``from_vals`` unchanged -- and info = {"t0", "n", "equilibration"}."""
    from .moments import DeviceDataArray
    from .xrlite import DataArray

    u, x, kind = _prepare(uv, xv)
    if x is None:
        raise TypeError("xv is required")
    wt = None
    if w is not None:
        wt, _ = _device_series(w, 1, "w")
        if wt.shape != u.shape:
            raise ValueError(f"w has {wt.shape[0]} records, uv {u.shape[0]}")
    eq = None
    if t0 is None:
        eq = detect_equilibrations(u, x, **kw)
        t0 = eq.t0_max
    elif kw:
        raise TypeError(f"keywords {sorted(kw)} only apply when t0 is detected")
    t0 = int(t0)
    if not 0 <= t0 < u.shape[0]:
        raise ValueError(f"t0 = {t0} outside [0, {u.shape[0] - 1}]")
    outs = [u[t0:].contiguous(), x[t0:].contiguous(), None if wt is None else wt[t0:].contiguous()]
    dims = [("rec",), ("rec", "val"), ("rec",)]
    if kind == "device":
        outs = [None if a is None else DeviceDataArray(a, d) for a, d in zip(outs, dims)]
    else:
        outs = [None if a is None else DataArray(a.cpu().numpy(), d) for a, d in zip(outs, dims)]
    info = {"t0": t0, "n": int(u.shape[0] - t0), "equilibration": eq}
    return outs[0], outs[1], outs[2], info


# ---------------------------------------------------------------------------
# a collection of states: the same estimator, every state's lag sums from one set of launches per lag block
# ---------------------------------------------------------------------------
def scan_lag_sums_states(fetch: Callable[[list, int, int], np.ndarray], ns, pair_ids_per_state, *, fast: bool = False,
                         mintime: int = 3, max_lag: int | None = None, names=None):
    """``scan_lag_sums`` for S states at once.  ``fetch(items, t0, nlags)`` returns R(t0 .. t0 + nlags - 1) of the listed
    (state, pair) items as a (len(items), nlags) float64 array.  The common block sequence (0, 256), (256, 256), (512, 512),
    ... is walked once, ONE fetch per block over every pair that is still active; a state takes part in a block only if
    it is block 0 or t0 < n_s - 1 (``lag_blocks(n_s)``'s own rule), so each state sees exactly the blocks, and its pairs
    exactly the loop, of ``scan_lag_sums(fetch_s, n_s, pair_ids_s)``.  Returns a list of (g, stop) per state, in the order
    of that state's pair ids.  ``names``: per state the names of its pairs; the ValueErrors (sigma^2 == 0, ``max_lag``)
    name the pair and the state."""
    ns = [int(n) for n in ns]
    S = len(ns)
    pids = [[int(p) for p in ps] for ps in pair_ids_per_state]
    if len(pids) != S:
        raise ValueError(f"{len(pids)} pair lists for {S} states")
    names = [None] * S if names is None else list(names)
    if len(names) != S:
        raise ValueError(f"{len(names)} name lists for {S} states")
    names = [[f"{nm} of state {s}" for nm in (nl if nl is not None else [f"pair {p}" for p in pids[s]])] for s, nl in enumerate(names)]
    g = [np.ones(len(p)) for p in pids]
    t = [np.ones(len(p), dtype=np.int64) for p in pids]
    inc = [np.ones(len(p), dtype=np.int64) for p in pids]
    sig2 = [np.zeros(len(p)) for p in pids]
    active = [list(range(len(p))) for p in pids]
    t0, nl = 0, LAG_BLOCK
    while True:
        states = [s for s in range(S) if active[s] and (t0 == 0 or t0 < ns[s] - 1)]
        if not states:
            break
        items = [(s, pids[s][k]) for s in states for k in active[s]]
        R = np.asarray(fetch(items, t0, nl), dtype=np.float64)
        if R.shape != (len(items), nl):
            raise ValueError(f"fetch returned {R.shape}, expected {(len(items), nl)}")
        row = 0
        for s in states:
            n, still = ns[s], []
            for k in active[s]:
                if t0 == 0:
                    sig2[s][k] = R[row, 0] / (2.0 * n)
                    if sig2[s][k] == 0.0:
                        raise ValueError(f"sample covariance sigma_AB^2 = 0 for {names[s][k]}: cannot compute the statistical inefficiency")
                tk, ik, gk, done = _scan_block(R[row], t0, nl, n, sig2[s][k], int(t[s][k]), int(inc[s][k]), g[s][k], fast, mintime,
                                               max_lag, names[s][k])
                t[s][k], inc[s][k], g[s][k] = tk, ik, gk
                if not done and tk < n - 1:
                    still.append(k)
                row += 1
            active[s] = still
        t0 += nl
        nl = min(t0, LAG_MAX_LAGS)
    return [(np.maximum(g[s], 1.0), t[s]) for s in range(S)]


def _prepare_states(uvs, xvs):
    """[(u, x, kind)] of ``_prepare`` per state; ValueError for an empty collection, lists of unequal length and states that
    differ in their column count."""
    uvs = list(uvs)
    xvs = [None] * len(uvs) if xvs is None else list(xvs)
    if not uvs:
        raise ValueError("no states")
    if len(xvs) != len(uvs):
        raise ValueError(f"{len(uvs)} energy series and {len(xvs)} observable arrays")
    st = [_prepare(uv, xv) for uv, xv in zip(uvs, xvs)]
    cols = [0 if x is None else x.shape[1] for _, x, _ in st]
    if len(set(cols)) > 1:
        raise ValueError(f"the states differ in their column count: {cols}")
    return st, cols[0]


def _inefficiencies_states(st, C, fast, mintime, max_lag):
    from . import engine

    S = len(st)
    rows = engine.lag_rows_batched(None if C == 0 else [x for _, x, _ in st], [u for u, _, _ in st])

    def fetch(items, t0, nlags):
        return engine.lag_sums_batched(rows, items, t0, nlags).cpu().numpy()

    res = scan_lag_sums_states(fetch, [u.shape[0] for u, _, _ in st], [range(2 * C + 1)] * S, fast=fast, mintime=mintime,
                               max_lag=max_lag, names=[_pair_names(C)] * S)
    return [Inefficiencies(float(g[0]), g[1:1 + C].copy(), g[1 + C:].copy(), float(g.max()), int(stop[0]),
                           stop[1:1 + C].copy(), stop[1 + C:].copy()) for g, stop in res]


def statistical_inefficiencies_states(uvs, xvs, *, fast: bool = False, mintime: int = 3, max_lag: int | None = None) -> list:
    """``statistical_inefficiencies`` of every state of a collection: uvs a list of energy series (rec), xvs a list of
    (rec, val) arrays sharing the column count (None: the energies alone); the record counts may differ.  The centred series
    of all states are made once (one launch) and kept for the whole scan; every lag block is one set of launches and one
    device-to-host copy for all states.  Element s equals ``statistical_inefficiencies(uvs[s], xvs[s], ...)`` in every
    field: the lag sums and the means have the same bits and the host loop is the same loop."""
    st, C = _prepare_states(uvs, xvs)
    return _inefficiencies_states(st, C, fast, mintime, max_lag)


def block_lengths(uvs, xvs, factor: float = 10.0, **kw) -> list:
    """``block_length`` of every state of a collection, from one ``statistical_inefficiencies_states``: what
    ``StateCollection.derivs_cov(block=[...])`` and ``derivs_cross_cov(block=[...])`` take."""
    if not factor > 0:
        raise ValueError(f"factor must be positive, got {factor}")
    return [max(1, int(math.ceil(float(factor) * i.g_max))) for i in statistical_inefficiencies_states(uvs, xvs, **kw)]


def decorrelate_states(uvs, xvs, ws=None, *, g=None, conservative: bool = False, **kw) -> list:
    """``decorrelate`` of every state of a collection: a list of (uv, xv, w, info) of the kinds and dims ``decorrelate``
    returns.  ``g``: None (estimated for all states by ``statistical_inefficiencies_states``; further keywords go there), one
    number for every state, or one number per state.  The gather is one ``index_select`` per state."""
    import torch

    from .moments import DeviceDataArray
    from .xrlite import DataArray

    if xvs is None:
        raise TypeError("xvs is required")
    st, C = _prepare_states(uvs, xvs)
    S = len(st)
    ws = [None] * S if ws is None else list(ws)
    if len(ws) != S:
        raise ValueError(f"{S} states and {len(ws)} weight arrays")
    wts = []
    for (u, _, _), w in zip(st, ws):
        wt = None
        if w is not None:
            wt, _ = _device_series(w, 1, "w")
            if wt.shape != u.shape:
                raise ValueError(f"w has {wt.shape[0]} records, uv {u.shape[0]}")
        wts.append(wt)
    ineffs = [None] * S
    if g is None:
        ineffs = _inefficiencies_states(st, C, kw.pop("fast", False), kw.pop("mintime", 3), kw.pop("max_lag", None))
        if kw:
            raise TypeError(f"unexpected keywords {sorted(kw)}")
        gs = [i.g_max for i in ineffs]
    else:
        if kw:
            raise TypeError(f"keywords {sorted(kw)} only apply when g is estimated")
        gs = [float(g)] * S if np.ndim(g) == 0 else [float(v) for v in g]
        if len(gs) != S:
            raise ValueError(f"{S} states and {len(gs)} values of g")
    out = []
    dims = [("rec",), ("rec", "val"), ("rec",)]
    for (u, x, kind), wt, gk, ineff in zip(st, wts, gs, ineffs):
        idx = subsample_correlated_data(u.shape[0], gk, conservative=conservative)
        di = torch.as_tensor(idx).to("cuda")
        arrs = [u.index_select(0, di), x.index_select(0, di), None if wt is None else wt.index_select(0, di)]
        if kind == "device":
            arrs = [None if a is None else DeviceDataArray(a, d) for a, d in zip(arrs, dims)]
        else:
            arrs = [None if a is None else DataArray(a.cpu().numpy(), d) for a, d in zip(arrs, dims)]
        out.append((arrs[0], arrs[1], arrs[2], {"g": float(gk), "indices": idx, "n": int(idx.size), "inefficiencies": ineff}))
    return out
