"""Extrapolation models: the thermoextrap.models API for the derivative /
Taylor-series part of the path (reference models.py:290-576, 580-671).

``Derivatives.derivs(data)`` does not call lambdified Python functions through
one xarray ``isel`` per symbol occurrence (reference models.py:371): the
derivative polynomials (symbolic.py) are compiled once into a table and
evaluated for every (replicate, value) element by one libtxmom kernel
(txm_eval_poly), reading the moment states where the reduction kernels left
them in HBM.  ``minus_log=True`` is a second table (the -log chain rule) run on
the first one's output.
"""

from __future__ import annotations

import ctypes as ct
import math
from collections.abc import Mapping
from functools import lru_cache
from typing import NamedTuple

import numpy as np
import torch

from . import _delta, _lib, engine
from . import symbolic as S
from ._delta import check_block_type as _check_block_type
from .data import AbstractData, _Params, xrwrap_alpha
from .moments import IndexSampler
from .xrlite import DataArray, concat, is_dataset, is_labelled

__all__ = ["Derivatives", "ExtrapModel", "ExtrapWeightedModel", "InterpModel", "InterpModelPiecewise", "MBARModel",
           "PerturbModel", "PiecewiseMixin", "StateCollection", "SymDerivBase", "taylor_series_norm", "xr_weights_minkowski"]


class SymDerivBase(S.DerivSeries):
    """Recursive derivative expressions ``self[n] = d^n func / d alpha^n``
    (name of the reference's class, models.py:103-150).  Items are
    :class:`thermoextrap_amd.symbolic.Poly`; ``expr(n)`` gives sympy."""

    def __init__(self, func, args=None, expand=True, post_func=None, rule=S.beta_rule):
        super().__init__(func, rule=rule, post_func=post_func)
        self.func = self._items[0]
        self.args = args
        self.expand = expand

    def expr(self, order):
        return S.to_sympy(self[order])


class _ExprView:
    """``derivatives.exprs[i]`` -> sympy expression of order i."""

    def __init__(self, series):
        self._series = series

    def __getitem__(self, i):
        return S.to_sympy(self._series[i])


# ---------------------------------------------------------------------------
# device table plumbing
# ---------------------------------------------------------------------------
class _DeviceTable:
    """A compiled txm_poly_table living in HBM."""

    def __init__(self, table: dict, atom_specs: list[tuple[int, int, int, int]]):
        L = _lib.load()
        self.n_funcs = len(table["func_flags"])
        atoms = (_lib.Atom * max(len(atom_specs), 1))()
        for i, (src, off, s_rep, s_val) in enumerate(atom_specs):
            atoms[i] = _lib.Atom(src=src, pad=0, offset=off, s_rep=s_rep, s_val=s_val)
        raw = np.frombuffer(bytes(atoms), dtype=np.uint8).copy()
        self.atoms = torch.from_numpy(raw).cuda()

        def i32(a):
            return torch.tensor(a if len(a) else [0], dtype=torch.int32, device="cuda")

        self.func_term0 = i32(table["func_term0"])
        self.func_flags = i32(table["func_flags"])
        self.coef = torch.tensor(table["coef"] if table["coef"] else [0.0], dtype=torch.float64, device="cuda")
        self.term_fac0 = i32(table["term_fac0"])
        self.fac_atom = i32(table["fac_atom"])
        self.fac_pow = i32(table["fac_pow"])
        self.struct = _lib.PolyTable(
            n_funcs=self.n_funcs, n_atoms=len(atom_specs), n_terms=len(table["coef"]),
            n_factors=len(table["fac_atom"]), log_atom=table["log_atom"], pad=0,
            atoms=self.atoms.data_ptr(), func_term0=self.func_term0.data_ptr(),
            func_flags=self.func_flags.data_ptr(), coef=self.coef.data_ptr(),
            term_fac0=self.term_fac0.data_ptr(), fac_atom=self.fac_atom.data_ptr(),
            fac_pow=self.fac_pow.data_ptr(),
        )
        self._L = L

    def run(self, srcs: list[torch.Tensor], nrep: int, nval: int) -> torch.Tensor:
        # (the pointer table from a cache / a pinned non-blocking upload: no host wait in the middle of a step -- engine.const_tensor)
        ptrs = engine.const_tensor([t.data_ptr() for t in srcs], torch.int64)
        out = torch.empty((self.n_funcs, nrep, nval), dtype=torch.float64, device="cuda")
        _lib.check(
            self._L.txm_eval_poly(ct.byref(self.struct), ct.c_void_p(ptrs.data_ptr()), len(srcs), nrep, nval,
                                  ct.c_void_p(out.data_ptr()),
                                  ct.c_void_p(torch.cuda.current_stream().cuda_stream)),
            "txm_eval_poly",
        )
        return out


_STATE_KINDS = frozenset({"du", "u", "dxdu", "xu", "x1", "umean"})


@lru_cache(16)
def _minus_log_series():
    return S.DerivSeries(S.Poly.atom(("X", 0)), rule=S.chain_rule, post_func="minus_log")


class _HostSource:
    """What ``predict`` / the GP input need to know about a derivative array that was evaluated on the host (the layout
    words of data.DerivSource, without a device state behind them)."""

    def __init__(self, out_dims, out_shape, coords, lead_dim):
        self.out_dims, self.out_shape, self.coords = list(out_dims), list(out_shape), coords
        has_lead = lead_dim is not None and bool(out_dims) and out_dims[0] == lead_dim
        self.nrep = int(out_shape[0]) if has_lead else 1
        rest = out_shape[1:] if has_lead else out_shape
        self.nval = int(np.prod(rest)) if len(rest) else 1


class _SympyFuncs:
    """``Derivatives.from_sympy(exprs, args)``: ``self[i]`` is the lambdified ``exprs[i]`` exactly as the reference's
    ``Lambdify`` builds it (models.py:241-243), ``self.series[i]`` its translation into a polynomial table for the device
    evaluator -- raising NotImplementedError for an expression that is not a Laurent polynomial (+ one ``-log``) in the
    indexed symbols, in which case ``Derivatives.derivs`` evaluates the lambdified functions on the host."""

    def __init__(self, exprs, args):
        self.exprs, self.args = exprs, tuple(args)
        self._funcs: dict = {}
        self.series = _SympySeries(exprs)

    def __getitem__(self, order):
        if order not in self._funcs:
            import sympy as sp

            self._funcs[order] = sp.lambdify(self.args, self.exprs[order])
        return self._funcs[order]


class _SympySeries:
    def __init__(self, exprs):
        self._exprs = exprs
        self._items: dict = {}

    def __getitem__(self, order):
        if order not in self._items:
            self._items[order] = S.poly_from_expr(self._exprs[order])
        return self._items[order]


def _arg_names(args):
    """names of the symbol families of ``args``: strings as they are, sympy ``Symbol`` / ``IndexedBase`` by name."""
    if args is None:
        return None
    return tuple(a if isinstance(a, str) else str(getattr(a, "name", getattr(a, "label", a))) for a in args)


def _defining_class(obj, name):
    for klass in type(obj).__mro__:
        if name in vars(klass):
            return klass
    return None


class Derivatives(_Params):
    """Derivatives of an average to a given order (reference models.py:290-421).

    Parameters
    ----------
    funcs : sequence of callable -- or of polynomials
        ``funcs[i](*args)`` gives the i-th derivative (the reference's contract, models.py:296-300: any object with
        ``__getitem__``, e.g. the ``VolumeDerivFuncs`` class of examples/usage/basic/Customized_Derivatives.ipynb).
        The built-in factories pass a series of :class:`thermoextrap_amd.symbolic.Poly` instead, which is evaluated by
        ONE table kernel from the moment states in HBM (txm_eval_poly).
    exprs : sequence of sympy expressions, optional
    args : sequence of str or sympy symbols, optional
        the symbol families, in the order the functions take them (central: x1, du, dxdu; raw: u, xu; callbacks
        append their own).

    Which route ``derivs(data)`` takes:

    * polynomial series + a data object whose callback is the default one or supplies ``device_sources`` (the two
      built-in callbacks): the device table;
    * plain callables, or a callback that (re)defines ``derivs_args`` without a matching ``device_sources``, or an
      expression the table cannot hold: ``funcs[i](*data.derivs_args)`` on the host selectors, as the reference does
      (models.py:357-383).  A callback's ``derivs_args`` is never ignored.
    """

    _fields = ("funcs", "exprs", "args")

    def __init__(self, funcs=None, *, exprs=None, args=None, series=None):
        if funcs is None:
            funcs = series
        if funcs is None:
            raise TypeError("Derivatives needs funcs (callables, or a polynomial series)")
        self.funcs = funcs
        self.args = args
        # the polynomial series behind the functions, when there is one: from_sympy's translation, or the functions ARE polynomials
        self.series = funcs.series if isinstance(funcs, _SympyFuncs) else (funcs if self._looks_like_poly_series(funcs) else None)
        self.exprs = exprs if exprs is not None else (_ExprView(self.series) if self.series is not None else None)
        self._tables: dict = {}

    @staticmethod
    def _looks_like_poly_series(funcs) -> bool:
        try:
            return isinstance(funcs[0], S.Poly)
        except Exception:  # noqa: BLE001 -- a user's funcs object may refuse order 0 however it likes
            return False

    # ---- routes ---------------------------------------------------------------------------------------------------
    def _device_route(self, data) -> bool:
        """True when the device table can serve ``data`` (see the class docstring)."""
        if self.series is None:
            return False
        meta = getattr(data, "meta", None)
        if meta is None:
            return True
        from .data import DataCallback, DataCallbackABC

        args_cls = _defining_class(meta, "derivs_args")
        if args_cls in (DataCallback, DataCallbackABC, None):
            return True          # nothing appended to the data object's own selectors
        hook_cls = _defining_class(meta, "device_sources")
        if hook_cls is None:
            return False         # a callback with its own derivs_args and no device view of them
        # a subclass that overrides derivs_args BELOW the class that supplies device_sources changed the arguments
        # without telling the device hook: honour the arguments
        mro = type(meta).__mro__
        return mro.index(args_cls) >= mro.index(hook_cls)

    def _table_for(self, src, order, extra_resolve=None) -> _DeviceTable:
        key = (order, src.central, src.x_is_u, src.nrep, src.ndrv, src.nval, src.K)
        # tables that reference callback-owned buffers are rebuilt per call (tiny)
        if extra_resolve is not None or key not in self._tables:
            table = S.compile_table(self.series[i] for i in range(order + 1))
            specs = []
            for a in table["atoms"]:
                if extra_resolve is not None and a[0] in extra_resolve:
                    specs.append(extra_resolve[a[0]](a))
                    continue
                kind = a[0]
                n = a[1] if len(a) > 1 and a[1] is not None else 0
                d = a[2] if len(a) > 2 and a[2] is not None else 0
                if kind == "x1":
                    d, n = (a[1] or 0), 0
                if kind not in _STATE_KINDS:
                    # a symbol the moment state does not hold and no device hook supplied: the host route decides
                    # (the callback's derivs_args may carry it)
                    raise S.NotRepresentable(f"symbol family {kind!r} has no device source")
                off, s_rep, s_val = src.resolve(kind, n, d)
                specs.append((0, off, s_rep, s_val))
            built = _DeviceTable(table, specs)
            if extra_resolve is not None:
                return built
            self._tables[key] = built
        return self._tables[key]

    def derivs(self, data=None, order=None, args=None, minus_log=False, order_dim="order", concat_kws=None,
               norm=False, _device=False):
        """Derivatives for orders ``range(order + 1)`` as one array with leading
        ``order_dim`` (or a list when ``order_dim is None``)."""
        if data is None:
            if args is None:
                raise ValueError("must specify args or data")
            return self._derivs_from_args(args, order, minus_log, order_dim, norm)
        if order is None:
            order = data.order
        if order is None:
            raise ValueError("must specify order or data")

        vals = src = None
        if self._device_route(data):
            try:
                vals, src = self._derivs_device(data, order)
            except S.NotRepresentable:
                vals = None      # from_sympy expression outside the table's algebra: the lambdified functions serve
        if vals is None:
            return self._derivs_host(data, order, minus_log, order_dim, norm, _device)
        if minus_log:
            ml = _minus_log_series()
            key = ("mlog", order, src.nrep, src.nval)
            if key not in self._tables:
                t = S.compile_table(ml[i] for i in range(order + 1))
                stride = src.nrep * src.nval
                specs = [(0, a[1] * stride, src.nval, 1) for a in t["atoms"]]
                self._tables[key] = _DeviceTable(t, specs)
            vals = self._tables[key].run([vals], src.nrep, src.nval)
        if norm:
            fac = engine.const_tensor([1.0 / math.factorial(i) for i in range(order + 1)], torch.float64)
            vals = vals * fac[:, None, None]
        if _device:
            return vals, src
        host = vals.cpu().numpy().reshape(order + 1, *src.out_shape)
        if order_dim is None:
            outs = []
            for i in range(order + 1):
                o = DataArray(host[i], tuple(src.out_dims))
                o._inherit(src.coords)
                outs.append(o)
            return outs
        out = DataArray(host, (order_dim, *src.out_dims))
        out._inherit(src.coords)
        return out

    def _derivs_device(self, data, order):
        src = data._derivs_source()
        srcs = [src.tensor]
        extra = None
        hook = getattr(data.meta, "device_sources", None)
        if hook is not None:
            extra = hook(data=data, src=src, srcs=srcs)
        table = self._table_for(src, order, extra)
        return table.run(srcs, src.nrep, src.nval), src  # (order+1, nrep, nval)

    def _derivs_host(self, data, order, minus_log, order_dim, norm, _device):
        """``funcs[i](*data.derivs_args)`` (reference models.py:357-383).  The arguments are the data object's host
        selectors -- slices of the moment states the reduction kernels produced -- plus whatever the callback appends."""
        dargs = tuple(data.derivs_args)
        if self.series is not None and not callable(self._first_func()):
            out = self._derivs_from_args(dargs, order, minus_log, None, norm)
        else:
            out = [self.funcs[i](*dargs) for i in range(order + 1)]
            if minus_log:
                ml = _minus_log_series()
                X = list(out)
                out = [S.eval_host(ml[i], lambda a: X[a[1]]) for i in range(order + 1)]
            if norm:
                out = [x / math.factorial(i) for i, x in enumerate(out)]
        if _device or order_dim is not None:
            lab = [o if is_labelled(o) else DataArray(np.asarray(o, dtype=float), ()) for o in out]
            ref = max(lab, key=lambda o: len(o.dims))
            lab = [o if o.dims == ref.dims else (o + 0.0 * ref).transpose(*ref.dims) for o in lab]
        if _device:
            lead = getattr(data, "_lead_dim", lambda: None)()
            if lead is None and getattr(data, "rec_dim", None) in ref.dims:
                lead = data.rec_dim
            if lead in ref.dims and ref.dims[0] != lead:
                lab = [o.transpose(lead, *[d for d in ref.dims if d != lead]) for o in lab]
                ref = lab[0]
            host = np.stack([np.asarray(o.values, dtype=np.float64) for o in lab])
            src = _HostSource(ref.dims, list(ref.shape), dict(ref._coords), lead if lead in ref.dims else None)
            return engine.to_device(host.reshape(order + 1, src.nrep, src.nval)), src
        if order_dim is None:
            return out
        return concat(lab, order_dim)

    def _first_func(self):
        try:
            return self.funcs[0]
        except Exception:  # noqa: BLE001
            return None

    def _derivs_from_args(self, args, order, minus_log, order_dim, norm):
        """``derivs(args=...)`` without a data object (reference models.py:357-383: ``funcs[i](*args)``): the caller's
        arrays are not moment states in HBM, so the polynomials are evaluated where the arguments live -- on the host,
        with the arguments' own arithmetic (numpy / labelled arrays).  Same tables as the device path."""
        if order is None:
            raise ValueError("must specify order or data")
        if self.series is None or callable(self._first_func()):
            out = [self.funcs[i](*args) for i in range(order + 1)]
        else:
            if self.args is None:
                raise ValueError("this Derivatives object does not name its arguments (args=None)")
            resolve = S.resolve_from_args(_arg_names(self.args), tuple(args))
            out = [S.eval_host(self.series[i], resolve) for i in range(order + 1)]
        if minus_log:
            ml = _minus_log_series()
            X = list(out)
            out = [S.eval_host(ml[i], lambda a: X[a[1]]) for i in range(order + 1)]
        if norm:
            out = [x / math.factorial(i) for i, x in enumerate(out)]
        if order_dim is None:
            return out
        if all(is_labelled(o) for o in out):
            return concat(out, order_dim)
        return np.stack([np.asarray(o, dtype=float) for o in np.broadcast_arrays(*[np.asarray(o) for o in out])])

    def coefs(self, data=None, args=None, order=None, minus_log=False, order_dim="order"):
        """Taylor coefficients: ``derivs(..., norm=True)``."""
        return self.derivs(data=data, args=args, order=order, minus_log=minus_log, order_dim=order_dim, norm=True)

    @classmethod
    def from_series(cls, series, args):
        return cls(series, args=args)

    @classmethod
    def from_sympy(cls, exprs, args):
        """From sympy expressions over the reference's symbols -- ``IndexedBase`` families ``du[n]``, ``dxdu[n]`` /
        ``dxdu[n, d]``, ``u[n]``, ``xu[n]`` / ``xu[n, d]``, ``x1[d]`` and the plain symbols ``x1``, ``u`` (reference
        models.py:404-421, beta.py:46-240).  ``exprs[i]`` is the i-th derivative, ``args`` the symbols in the order the
        data object's ``derivs_args`` supplies them.  Expressions that are Laurent polynomials in those symbols (plus at
        most one ``-log(symbol)``) are compiled into the device table; anything else is lambdified and evaluated on the
        host selectors exactly as the reference does."""
        return cls(_SympyFuncs(exprs, args), exprs=exprs, args=args)


@lru_cache(10)
def taylor_series_norm(order, order_dim="order"):
    """``taylor_series_coefficients = derivs * taylor_series_norm``."""
    out = np.array([1 / math.factorial(i) for i in range(order + 1)])
    if order_dim is not None:
        out = DataArray(out, order_dim)
    return out


class ExtrapModel(_Params):
    """Taylor-series extrapolation about ``alpha0`` (reference models.py:433-576)."""

    _fields = ("alpha0", "data", "derivatives", "order", "minus_log", "alpha_name")

    def __init__(self, alpha0, data, derivatives, order=None, *, minus_log=False, alpha_name="alpha"):
        if not isinstance(data, AbstractData):
            raise TypeError("data must be a data object")
        if not isinstance(derivatives, Derivatives):
            raise TypeError("derivatives must be a Derivatives object")
        self.alpha0 = float(alpha0)
        self.data = data
        self.derivatives = derivatives
        self.order = data.order if order is None else order
        self.minus_log = bool(minus_log) if minus_log is not None else False
        self.alpha_name = str(alpha_name)
        self._cache: dict = {}

    def _derivs(self, order, order_dim, minus_log):
        key = (order, order_dim, minus_log)
        if key not in self._cache:
            self._cache[key] = self.derivatives.derivs(data=self.data, order=order, norm=False,
                                                       minus_log=minus_log, order_dim=order_dim)
        return self._cache[key]

    def derivs(self, order=None, order_dim="order", minus_log=None, norm=False):
        if minus_log is None:
            minus_log = self.minus_log
        if order is None:
            order = self.order
        out = self._derivs(order=order, order_dim=order_dim, minus_log=minus_log)
        if norm:
            out = out * taylor_series_norm(order, order_dim)
        return self._ds(out)

    def _ds(self, out):
        """Results of Dataset-valued observables go back out as a Dataset (the kernels saw one stacked matrix)."""
        f = getattr(self.data, "as_dataset_result", None)
        if f is None or isinstance(out, list):
            return out
        return f(out)

    def coefs(self, order=None, order_dim="order", minus_log=None):
        return self.derivs(order=order, order_dim=order_dim, minus_log=minus_log, norm=True)

    def __call__(self, *args, **kwargs):
        return self.predict(*args, **kwargs)

    def predict(self, alpha, order=None, order_dim="order", cumsum=False, no_sum=False, minus_log=None,
                alpha_name=None, dalpha_coords="dalpha", alpha0_coords=True, fused=True):
        """Taylor series at ``alpha``: sum_k coefs[k] * (alpha - alpha0)^k  (reference models.py:479-565).

        ``fused`` (default): derivative table -> 1/k! -> dalpha^k -> sum / cumsum over the order in ONE launch over
        (alpha, rep, val) on the device table (txm_predict_taylor), one copy back.  ``fused=False`` forms the same
        labelled expression on the host from ``coefs`` like the reference does."""
        if order is None:
            order = self.order
        if alpha_name is None:
            alpha_name = self.alpha_name
        if minus_log is None:
            minus_log = self.minus_log
        alpha = xrwrap_alpha(alpha, name=alpha_name)
        dalpha = alpha - self.alpha0
        if fused and order_dim is not None:
            key = ("device", order, minus_log)
            if key not in self._cache:
                self._cache[key] = self.derivatives.derivs(data=self.data, order=order, norm=False,
                                                           minus_log=minus_log, _device=True)
            vals, src = self._cache[key]
            mode = "terms" if no_sum else ("cumsum" if cumsum else "sum")
            res = engine.predict_taylor(vals, dalpha.values, mode).cpu().numpy()
            if mode == "sum":
                out = DataArray(res.reshape((*dalpha.shape, *src.out_shape)), (*dalpha.dims, *src.out_dims))
            else:
                out = DataArray(res.reshape((*dalpha.shape, order + 1, *src.out_shape)),
                                (*dalpha.dims, order_dim, *src.out_dims))
            out._inherit(dalpha._coords)
            out._inherit(src.coords)
        else:
            coefs = self._derivs(order=order, order_dim=order_dim, minus_log=minus_log) * taylor_series_norm(order, order_dim)
            p = DataArray(np.arange(order + 1), order_dim)
            prefac = dalpha**p
            out = prefac * coefs
        coords = {}
        if dalpha_coords is not None:
            coords[dalpha_coords] = dalpha
        if alpha0_coords:
            if not isinstance(alpha0_coords, str):
                alpha0_coords = alpha_name + "0"
            coords[alpha0_coords] = self.alpha0
        out = out.assign_coords(coords)
        if fused and order_dim is not None:
            return self._ds(out)
        if no_sum:
            return self._ds(out)
        if cumsum:
            return self._ds(out.cumsum(order_dim))
        return self._ds(out.sum(order_dim))

    # ---- delta-method error bars -----------------------------------------------------------------------
    def _delta_operands(self, device_state=False):
        """(x [N, C], u [N], w [N] or None, central state [C, 2, K] on the host, derivative source) for ``derivs_cov`` --
        or NotImplementedError naming what this model is that the one-pass formula does not cover.
        ``device_state``: leave the central state on the device (a collection copies all its states' at once)."""
        from . import moments as cm
        from .data import DataCallback, DataCentralMoments, DataCentralMomentsVals, DataValuesBase

        data, what = self.data, "derivs_cov / predict_with_error (delta-method error bars)"
        if isinstance(data, DataCentralMoments):
            raise NotImplementedError(f"{what}: DataCentralMoments holds reduced moments only -- there are no samples to pass "
                                      "over; build the model on DataCentralMomentsVals")
        if isinstance(data, DataValuesBase):
            raise NotImplementedError(f"{what}: DataValues / DataValuesCentral are not supported; build the model on "
                                      "DataCentralMomentsVals")
        if not isinstance(data, DataCentralMomentsVals):
            raise NotImplementedError(f"{what}: unsupported data object {type(data).__name__}")
        if data.xalpha:
            raise NotImplementedError(f"{what}: observables that depend on alpha (xalpha / deriv_dim) are not supported")
        if data.x_is_u:
            raise NotImplementedError(f"{what}: x_is_u data is not supported")
        if data.rec_dim in data.dxduave.val_dims:
            raise NotImplementedError(f"{what}: this model holds resampled data; take the error bars of the model it was "
                                      "resampled from")
        if type(data.meta) is not DataCallback:
            raise NotImplementedError(f"{what}: data callbacks (volume, lnPi) are not supported")
        if self.derivatives.series is None:
            raise NotImplementedError(f"{what}: the Derivatives object was built from plain callables; the influence "
                                      "functions need the polynomial series (beta.factory_derivatives, from_sympy)")
        src = data._derivs_source()
        state = data.dxduave if data.dxduave.val_dims == tuple(src.out_dims) else data.dxduave.transpose(
            *src.out_dims, *data.dxduave.mom_dims)
        xt, xdims = cm._dev_and_dims(data.xv)
        ut, udims = cm._dev_and_dims(data.uv)
        if tuple(udims) != (data.rec_dim,) or set(xdims) != {data.rec_dim, *src.out_dims}:
            raise NotImplementedError(f"{what}: uv must be 1-D along {data.rec_dim!r} and xv ({data.rec_dim!r}, values...)")
        N = xt.shape[xdims.index(data.rec_dim)]
        x2 = xt.permute([xdims.index(d) for d in (data.rec_dim, *src.out_dims)]).reshape(N, -1)
        wt = None
        if data.weight is not None:
            wt = cm._dev_and_dims(data.weight)[0] if (is_labelled(data.weight) or isinstance(data.weight, cm.DeviceDataArray)) \
                else engine.to_device(np.asarray(data.weight))
            if wt.shape != (N,):
                raise NotImplementedError(f"{what}: weight must be 1-D along {data.rec_dim!r}")
        K = state.device_values.shape[-1]
        sd = state.device_values.reshape(-1, 2, K)
        return x2, ut, wt, (sd if device_state else sd.cpu().numpy()), src

    def _delta_coefs(self, st, order, minus_log):
        """(a, b [C, order + 1, order + 1], <u>, <x> [C]) on the host: the influence polynomials of ``derivs(order)`` from
        the central state ``st`` [C, 2, K] (symbolic.influence_coefs)."""
        if order > st.shape[-1] - 1:
            raise ValueError(f"order {order} requested, but the data object only holds moments to order {st.shape[-1] - 1}")
        # the central state: [c][0][1] = <u>, [c][1][0] = <x_c>, [c][0][j] = <du^j>, [c][1][j] = <dx_c du^j>
        um, xm = float(st[0, 0, 1]), st[:, 1, 0]
        mom = S.influence_moments(xm, um, [0.0, 0.0] + [float(st[0, 0, j]) for j in range(2, order + 1)],
                                  [0.0] + [st[:, 1, j] for j in range(1, order + 1)])
        a, b = S.influence_coefs(self.derivatives.series, order, mom, minus_log=minus_log)
        return np.ascontiguousarray(a), np.ascontiguousarray(b), um, xm

    def _derivs_cov_device(self, order, minus_log, block=None):
        """``(cov [n_out, order + 1, order + 1] on the device, source)`` of ``derivs_cov`` (``_delta.extrap_table``): the
        iid entry ``("dcov", ...)``, or with a ``block`` the blocked estimator's, cached under a key of its
        own."""
        return _delta.extrap_table(self, order, minus_log, False, block)[:2]

    def _blocked_cov_device(self, order, minus_log, block, curve):
        """``(cov, source, block_lengths, n_blocks)`` of the blocked estimator: cov at ``block`` alone, or
        with ``curve`` [level, ...] for every level of ``engine.block_levels``."""
        return _delta.extrap_table(self, order, minus_log, False, _check_block_type(block), curve)

    @staticmethod
    def _derivs_cov_labelled(host, src, order, norm):
        """The host copy of a ``_derivs_cov_device`` table (n_out, order + 1, order + 1) as ``derivs_cov`` returns it."""
        if norm:
            f = _delta.taylor_norm(order)
            host = host * f[None, :, None] * f[None, None, :]
        out = DataArray(np.ascontiguousarray(np.moveaxis(host, 0, -1)).reshape(order + 1, order + 1, *src.out_shape),
                        ("order", "order_2", *src.out_dims))
        out._inherit(src.coords)
        return out

    def derivs_cov(self, order=None, norm=False, minus_log=None, block=None):
        """Delta-method (infinitesimal-jackknife) covariance of ``derivs(order)``: dims ``(order, order_2, *val_dims)``.

        ``V_ij = sum_n p_n^2 psi_i(n) psi_j(n)`` with ``p_n`` the normalised sample weights and ``psi_k(n)`` the empirical
        influence of sample n on the k-th derivative (symbolic.influence_coefs), from ONE pass over the samples
        (txm_influence_cov) -- no replicates, no sampling noise.  It is the first-order term of what the multinomial
        bootstrap (``resample``) estimates and, like it, assumes INDEPENDENT samples: decorrelate a time series first
        (``timeseries.decorrelate``).  It does not replace ``resample`` where the replicates themselves are wanted.
        ``norm=True`` carries the ``1 / (i! j!)`` factors of ``derivs(norm=True)``.

        Supported: beta-extrapolation models of ``x_ave`` (central or raw, ``minus_log`` on or off, weights) over
        ``DataCentralMomentsVals``; anything else raises NotImplementedError.

        ``block=B`` (an int, ``1 <= B`` and ``2 B <= N``) is for a CORRELATED series kept whole: the records are cut
        into contiguous blocks of B (a last short one is kept) and ``V_ij = sum_b z_bi z_bj`` with
        ``z_bk = sum_{n in b} p_n psi_k(n)`` -- batch means over the derivative's own influence series, one pass
        (txm_influence_block_cov), every record used.  B must exceed the correlation time: for an AR(1)-like series of
        statistical inefficiency g the relative bias is about ``-g / (2 B)`` (``timeseries.block_length``), and
        ``blocking_curve`` shows whether V has levelled off.  No ``nb / (nb - 1)`` factor is applied (``block=1`` is the
        iid result; the relative bias ``-1 / nb`` can be corrected with ``blocking_curve``'s block counts).  A non-integer
        block raises TypeError, one outside the range ValueError; ``block=None`` is the iid path, untouched."""
        if minus_log is None:
            minus_log = self.minus_log
        if order is None:
            order = self.order
        cov, src = self._derivs_cov_device(order, bool(minus_log), block)
        return self._ds(self._derivs_cov_labelled(cov.cpu().numpy(), src, order, norm))     # (n_out, order + 1, order + 1)

    def blocking_curve(self, block, order=None, norm=False, minus_log=None):
        """The blocking curve of Flyvbjerg & Petersen (1989) for ``derivs_cov``: ``(V, block_lengths, n_blocks)`` with
        ``V[l] = derivs_cov(block=block * 2**l)`` (dims ``(level, order, order_2, *val_dims)``), ``block_lengths[l] =
        block * 2**l`` and ``n_blocks[l] = ceil(N / block_lengths[l])``, for every level that still has at least two
        blocks.  ONE kernel call: block sums are additive, so each level merges the pairs of the level below.  Where
        the diagonal of V stops growing with the block length the blocks are longer than the correlation time; the
        last levels are noisy (relative standard deviation about ``sqrt(2 / (n_blocks - 1))``) and biased by
        ``-1 / n_blocks``."""
        if minus_log is None:
            minus_log = self.minus_log
        if order is None:
            order = self.order
        out, lengths, counts = _delta.blocking_levels(self._blocked_cov_device(order, bool(minus_log), block, curve=True),
                                                      lambda host, src: self._derivs_cov_labelled(host, src, order, norm))
        return self._ds(out), lengths, counts

    def predict_with_error(self, alpha, order=None, minus_log=None, alpha_name=None, block=None):
        """``(prediction, std)``: ``predict(alpha)`` and its delta-method standard deviation ``sqrt(t' V t)``,
        ``t_k = (alpha - alpha0)^k / k!``, ``V = derivs_cov(order, block=block)`` (named after
        ``MBARModel.predict_with_error``; the assumptions of ``derivs_cov`` apply: first order, and independent samples
        unless a ``block`` longer than the correlation time is given)."""
        if order is None:
            order = self.order
        if minus_log is None:
            minus_log = self.minus_log
        cov, src = self._derivs_cov_device(order, bool(minus_log), block)
        pred = self.predict(alpha, order=order, minus_log=minus_log, alpha_name=alpha_name)
        dalpha = xrwrap_alpha(alpha, name=alpha_name or self.alpha_name) - self.alpha0
        t = _delta.taylor_vectors(dalpha, order)                                              # (n_alpha, order + 1)
        var = np.einsum("ai,cij,aj->ac", t, cov.cpu().numpy(), t)
        return pred, self._ds(_delta.label_std(var, dalpha, src))

    # ---- the same across the observable columns ---------------------------------------------------------
    def _derivs_cross_cov_device(self, order, minus_log, block=None):
        """``(cov [n_out, order + 1, n_out, order + 1] on the device, source)`` from ONE ``engine.influence_cross_cov``,
        cached under a key of its own: the per-column entry ``("dcov", ...)`` is neither read nor written.  With a
        ``block`` it is the blocked estimator's (``_blocked_cross_cov_device``)."""
        return _delta.extrap_table(self, order, minus_log, True, block)[:2]

    def _blocked_cross_cov_device(self, order, minus_log, block, curve):
        """``(cov, source, block_lengths, n_blocks)`` of the blocked cross estimator: cov at ``block`` alone,
        or with ``curve`` [level, ...] for every level of ``engine.block_levels``."""
        return _delta.extrap_table(self, order, minus_log, True, _check_block_type(block), curve)

    _cross_labels = staticmethod(_delta.cross_labels)

    @classmethod
    def _derivs_cross_cov_labelled(cls, host, src, order, norm):
        """The host copy of a ``_derivs_cross_cov_device`` table (n_out, order + 1, n_out, order + 1) as
        ``derivs_cross_cov`` returns it."""
        host = host.transpose(1, 3, 0, 2)                                                    # (order, order_2, c, c')
        if norm:
            f = _delta.taylor_norm(order)
            host = host * f[:, None, None, None] * f[None, :, None, None]
        out = DataArray(np.ascontiguousarray(host).reshape(order + 1, order + 1, *src.out_shape, *src.out_shape),
                        ("order", "order_2", *src.out_dims, *[d + "_2" for d in src.out_dims]))
        return cls._cross_labels(out, src)

    def derivs_cross_cov(self, order=None, norm=False, minus_log=None, block=None):
        """Delta-method covariance of ``derivs(order)`` ACROSS the observable columns: dims
        ``(order, order_2, *val_dims, *[d + "_2" for d in val_dims])`` with

            ``V[i, j, c, c'] = sum_n p_n^2 psi_i(n, c) psi_j(n, c')``

        -- the off-diagonal blocks ``Cov(d_i of column c, d_j of column c')`` that ``derivs_cov`` does not hold and that
        any quantity combining columns needs: an integral over the bins of a profile, a sum of tensor components, a
        ratio of two observables.  The columns share one energy series and one set of samples, so these blocks are
        large.  ONE pass over the samples (txm_influence_cross_cov, Gram matrices on the FP64 matrix pipe) -- no
        replicates, no sampling noise.  The blocks ``c == c'`` are ``derivs_cov(order)`` up to rounding (another order of
        summation), and the result is exactly symmetric under ``(i, c) <-> (j, c')``.  ``norm=True`` carries the
        ``1 / (i! j!)`` factors of ``derivs(norm=True)``; ``minus_log`` acts per column as in ``derivs_cov``.

        The assumptions and the supported models are those of ``derivs_cov`` (first order, INDEPENDENT samples; anything
        else raises the same NotImplementedError), with at most 255 observable columns (ValueError beyond).  State
        collections and the multi-state models: ``StateCollection.derivs_cross_cov``; out of scope: ``gpr_input``.  A
        Dataset-valued observable comes back as
        ONE array over its stacked variable dimension -- the blocks between two variables have no place in a Dataset.

        ``block=B`` (an int, ``1 <= B`` and ``2 B <= N``) is for a CORRELATED series kept whole, as in ``derivs_cov``:
        ``V[i, j, c, c'] = sum_b z_bi(c) z_bj(c')`` with ``z_bk(c) = sum_{n in b} p_n psi_k(n, c)`` over the contiguous
        blocks of B records (a last short one is kept) -- batch means, every record used, one pass over the samples and
        a Gram over the block sums on the FP64 matrix pipe (txm_influence_block_cross_cov).  B must exceed the
        correlation time (``cross_blocking_curve`` shows whether V has levelled off); no ``nb / (nb - 1)`` factor is
        applied, so ``block=1`` is the iid result and the blocks ``c == c'`` are ``derivs_cov(block=B)``, both up to
        rounding.  A non-integer block raises TypeError, one outside the range ValueError; ``block=None`` is the iid
        path, untouched."""
        if minus_log is None:
            minus_log = self.minus_log
        if order is None:
            order = self.order
        cov, src = self._derivs_cross_cov_device(order, bool(minus_log), block)
        return self._derivs_cross_cov_labelled(cov.cpu().numpy(), src, order, norm)

    def cross_blocking_curve(self, block, order=None, norm=False, minus_log=None):
        """The blocking curve of ``derivs_cross_cov``: ``(V, block_lengths, n_blocks)`` with
        ``V[l] = derivs_cross_cov(block=block * 2**l)`` (dims ``(level, order, order_2, *val_dims, *val_dims_2)``, the
        level coordinates as in ``blocking_curve``), ``block_lengths[l] = block * 2**l`` and
        ``n_blocks[l] = ceil(N / block_lengths[l])``, for every level that still has at least two blocks.  ONE engine
        call: each level merges the pairs of the block sums of the level below and runs the Gram again.  V holds
        ``levels * (C * (order + 1))**2`` doubles (C the number of observable columns): 10 levels of 255 columns at
        order 4 are 130 MB -- take ``blocking_curve`` where the diagonal blocks are enough."""
        if minus_log is None:
            minus_log = self.minus_log
        if order is None:
            order = self.order
        return _delta.blocking_levels(self._blocked_cross_cov_device(order, bool(minus_log), block, curve=True),
                                      lambda host, src: self._derivs_cross_cov_labelled(host, src, order, norm))

    def predict_cov(self, alpha, order=None, minus_log=None, alpha_name=None, block=None):
        """``(prediction, cov)``: ``predict(alpha)`` and the delta-method covariance of the predicted columns,
        ``cov[alpha, c, c'] = sum_ij t_i t_j V[i, j, c, c']`` with ``t_k = (alpha - alpha0)^k / k!`` and
        ``V = derivs_cross_cov(order)``; cov has dims ``(*alpha dims, *val_dims, *[d + "_2" for d in val_dims])``.  Its
        diagonal ``c == c'`` is the square of ``predict_with_error``'s std; the rest is what the error bar of a sum, an
        integral or a ratio of predicted columns needs.  Assumptions, supported models and limits: ``derivs_cross_cov``;
        ``block=B`` takes ``V = derivs_cross_cov(order, block=B)`` for a correlated series (the prediction is the same)."""
        if order is None:
            order = self.order
        if minus_log is None:
            minus_log = self.minus_log
        cov, src = self._derivs_cross_cov_device(order, bool(minus_log), block)
        pred = self.predict(alpha, order=order, minus_log=minus_log, alpha_name=alpha_name)
        dalpha = xrwrap_alpha(alpha, name=alpha_name or self.alpha_name) - self.alpha0
        t = _delta.taylor_vectors(dalpha, order)                                              # (n_alpha, order + 1)
        pc = np.einsum("ai,cidj,aj->acd", t, cov.cpu().numpy(), t)
        return pred, _delta.label_cov(pc, dalpha, src)

    def resample(self, sampler, **kws):
        """New model on resampled data."""
        return self.new_like(order=self.order, alpha0=self.alpha0, derivatives=self.derivatives,
                             data=self.data.resample(sampler=sampler, **kws), minus_log=self.minus_log,
                             alpha_name=self.alpha_name)


class StateCollection(_Params):
    """Sequence of models (reference models.py:580-724)."""

    _fields = ("states", "kws")

    def __init__(self, states, kws=None):
        self.states = states
        self.kws = dict(kws or {})
        self._cache: dict = {}
        self._batch = None  # set by a batched resample: the (S, nrep, ...) tensor all states' replicate states view

    def __call__(self, *args, **kwargs):
        return self.predict(*args, **kwargs)

    def __len__(self):
        return len(self.states)

    def __getitem__(self, idx):
        return self.states[idx]

    @property
    def alpha_name(self):
        return getattr(self[0], "alpha_name", "alpha")

    # ---- batched path: S states of one shape in one set of launches ----------------------
    def _batch_eligible(self, min_states: int = 2):
        """The states' shared (N, column shape) when every state is an ExtrapModel over sample data
        (DataCentralMomentsVals) of one shape / order / layout with the default callback, else None.
        A single state is worth the batched launch only as a SHARD of a collection (min_states=1): it must run the
        kernels -- and so give the bits -- the unsharded collection's launch gives it."""
        from .data import DataCallback, DataCentralMomentsVals

        if len(self) < min_states:
            return None
        key = None
        for st in self.states:
            d = getattr(st, "data", None)
            if not isinstance(st, ExtrapModel) or type(d) is not DataCentralMomentsVals or type(d.meta) is not DataCallback:
                return None
            if getattr(st.derivatives, "series", None) is None:
                return None          # plain callables (Derivatives(funcs)): evaluated state by state on the host, as the reference does
            if d.x_is_u or d.xv.dims[0] != d.rec_dim or d.uv.dims != (d.rec_dim,):
                return None
            k = (tuple(d.xv.shape), tuple(d.xv.dims), d.order, d.weight is None, d.central, d.deriv_dim,
                 d.xmom_dim, d.umom_dim, st.order, st.minus_log, id(st.derivatives))
            if key is None:
                key = k
            elif k != key:
                return None
        return key

    # ---- delta-method error bars of all states from one set of launches ---------------------------------
    def _delta_batch_eligible(self):
        """The states' shared key when every state is an ExtrapModel over DataCentralMomentsVals with one column shape /
        order / central / minus_log / derivatives object, all weighted or none -- and ANY number of samples per state
        (txm_influence_cov_batched takes a count per state; ``_batch_eligible`` asks for one N).  Else None: the caller
        loops.  Whether ``ExtrapModel._delta_operands`` accepts the states shows when their operands are gathered: on
        either path a state it refuses raises its NotImplementedError through the collection."""
        from .data import DataCentralMomentsVals

        key = None
        for st in self.states:
            d = getattr(st, "data", None)
            if not isinstance(st, ExtrapModel) or type(d) is not DataCentralMomentsVals:
                return None
            try:
                rec = d.xv.dims.index(d.rec_dim)
                cols = tuple(n for i, n in enumerate(d.xv.shape) if i != rec)
                dims = tuple(n for i, n in enumerate(d.xv.dims) if i != rec)
            except (AttributeError, ValueError):
                return None
            k = (cols, dims, d.order, d.weight is None, d.central, st.order, st.minus_log, id(st.derivatives))
            if key is None:
                key = k
            elif k != key:
                return None
        return key

    def _blocks_per_state(self, block):
        """``block`` of the blocked error bars as one entry per state (None: the iid path): an int serves every state, a
        sequence gives each state its own -- states have different correlation times."""
        if block is None:
            return None
        if isinstance(block, (str, bytes)) or not hasattr(block, "__len__"):
            return [_check_block_type(block)] * len(self)
        if len(block) != len(self):
            raise ValueError(f"block must be an int or hold one entry per state: len(block)={len(block)}, {len(self)} states")
        return [_check_block_type(b) for b in block]

    def _derivs_cov_fill(self, order=None, minus_log=None, block=None):
        """Fill every state's ``("dcov", order, minus_log)`` cache -- what ``ExtrapModel._derivs_cov_device`` computes,
        bit for bit -- and return ``(cov [S, n_out, order + 1, order + 1] on the device, sources, order)``.
        Eligible states (``_delta_batch_eligible``): ONE copy of the stacked central states to the host, the
        per-state coefficient algebra there, ONE ``engine.influence_cov_batched`` (``_delta.states_tables``, which says
        why the algebra runs state by state).  Otherwise a loop over the states.

        With ``block`` (``_blocks_per_state``) the states are looped on the single blocked entry point, each with its own
        block length; the iid caches are neither read nor written."""
        sts = self.states
        blocks = self._blocks_per_state(block)
        if blocks is None and self._delta_batch_eligible() is not None:
            o = sts[0].order if order is None else order
            ml = bool(sts[0].minus_log if minus_log is None else minus_log)
            key = ("dcov", o, ml)
            todo = [st for st in sts if key not in st._cache]
            if todo and o <= todo[0].data.order:
                cov, srcs = _delta.states_tables(todo, o, ml, cross=False)
                for s, st in enumerate(todo):
                    st._cache[key] = (cov[s], srcs[s])
                if len(todo) == len(sts):
                    return cov, srcs, o
            parts = [st._derivs_cov_device(o, ml) for st in sts]
            return torch.stack([p_[0] for p_ in parts]), [p_[1] for p_ in parts], o
        parts, orders = [], []
        for s, st in enumerate(sts):
            if not hasattr(st, "_derivs_cov_device"):
                raise NotImplementedError(f"derivs_cov / predict_with_error (delta-method error bars): unsupported state "
                                          f"{type(st).__name__}")
            o = st.order if order is None else order
            ml = bool(st.minus_log if minus_log is None else minus_log)
            parts.append(st._derivs_cov_device(o, ml) if blocks is None else st._derivs_cov_device(o, ml, blocks[s]))
            orders.append(o)
        same = len(set(orders)) == 1 and len({tuple(p_[0].shape) for p_ in parts}) == 1
        return (torch.stack([p_[0] for p_ in parts]) if same else None), [p_[1] for p_ in parts], orders[0]

    def derivs_cov(self, order=None, norm=False, minus_log=None, block=None):
        """Every state's ``derivs_cov`` joined along the states: bit for bit
        ``map_concat(lambda m: m.derivs_cov(order, norm, minus_log))``.  The states are independent simulations, so the
        covariance of anything linear in their derivatives is block diagonal in these per-state blocks.

        States that share a column shape, order and derivatives object -- with ANY number of samples each, as
        ``timeseries.decorrelate`` leaves them -- are served by one launch per kernel (txm_influence_cov_batched) after one
        copy of their moments to the host; other collections loop.  Either way every state's own ``derivs_cov()`` is
        answered from its cache afterwards.  Assumptions: those of ``ExtrapModel.derivs_cov``.

        ``block`` (an int for all states, or one entry per state) gives the blocked error bars of correlated series
        (``ExtrapModel.derivs_cov(block=...)``): the states are looped on the single blocked entry point; ``block=None``
        leaves the path above untouched."""
        cov, srcs, o = self._derivs_cov_fill(order, minus_log, block)
        if cov is None:
            if block is None:
                return self.map_concat(lambda m: m.derivs_cov(order=order, norm=norm, minus_log=minus_log))
            blocks = self._blocks_per_state(block)
            out = [m.derivs_cov(order=order, norm=norm, minus_log=minus_log, block=blocks[s]) for s, m in enumerate(self.states)]
        else:
            host = cov.cpu().numpy()
            out = [st._ds(ExtrapModel._derivs_cov_labelled(host[s], srcs[s], o, norm)) for s, st in enumerate(self.states)]
        if is_labelled(out[0]):
            out = concat(out, dim=DataArray(np.asarray(self.alpha0), self.alpha_name))
        return out

    def _state_covs(self, order, minus_log, block=None):
        """Host copies of the states' delta-method covariances, [S][n_out, order + 1, order + 1], and their sources."""
        cov, srcs, _ = self._derivs_cov_fill(order, minus_log, block)
        if cov is None:
            blocks = self._blocks_per_state(block) or [None] * len(self)
            return [st._derivs_cov_device(order, bool(st.minus_log if minus_log is None else minus_log), blocks[s])[0].cpu().numpy()
                    for s, st in enumerate(self.states)], srcs
        return list(cov.cpu().numpy()), srcs

    # ---- the same across the observable columns ---------------------------------------------------------
    def _state_cross_covs(self, order=None, minus_log=None, block=None):
        """``(covs, sources, orders)``: per state the host copy of its cross-column delta-method covariance
        [n_out, order + 1, n_out, order + 1] (``ExtrapModel._derivs_cross_cov_device``).

        Eligible states (``_delta_batch_eligible``, at most 255 columns, no ``block``): ONE copy of the stacked central
        states to the host, the per-state coefficient algebra of ``_delta_coefs`` there, ONE
        ``engine.influence_cross_cov_batched``.  The result is cached ON THE COLLECTION under
        ``("dxcov_states", order, minus_log)``: the batch runs under a plan of its own, so a state with more samples than
        its share of the device need not have the bits of its own call, and the states' ``("dxcov", ...)`` entries are
        neither read nor written -- what a state's own ``derivs_cross_cov()`` returns does not depend on what was called
        before it.  Other collections, and every call with ``block`` (``_blocks_per_state``), loop over the states."""
        sts = self.states
        blocks = self._blocks_per_state(block)
        elig = self._delta_batch_eligible() if blocks is None else None
        if elig is not None and int(np.prod(elig[0], dtype=np.int64)) <= engine.CROSS_COV_MAX_COLUMNS:
            o = sts[0].order if order is None else order
            ml = bool(sts[0].minus_log if minus_log is None else minus_log)
            key = ("dxcov_states", o, ml)
            if key not in self._cache:
                cov, srcs = _delta.states_tables(sts, o, ml, cross=True)
                self._cache[key] = (cov.cpu().numpy(), srcs)
            host, srcs = self._cache[key]
            return list(host), srcs, [o] * len(sts)
        covs, srcs, orders = [], [], []
        for s, st in enumerate(sts):
            if not hasattr(st, "_derivs_cross_cov_device"):
                raise NotImplementedError(f"derivs_cross_cov / predict_cov (delta-method covariance across columns): "
                                          f"unsupported state {type(st).__name__}")
            o = st.order if order is None else order
            ml = bool(st.minus_log if minus_log is None else minus_log)
            cov, src = st._derivs_cross_cov_device(o, ml, None if blocks is None else blocks[s])
            covs.append(cov.cpu().numpy())
            srcs.append(src)
            orders.append(o)
        return covs, srcs, orders

    def derivs_cross_cov(self, order=None, norm=False, minus_log=None, block=None):
        """Every state's ``ExtrapModel.derivs_cross_cov`` -- dims ``(order, order_2, *val_dims, *val_dims_2)`` -- joined
        along the states, as ``derivs_cov`` joins its arrays.  The states are independent simulations: there are no blocks
        between two states, and the covariance of anything linear in the states' derivatives is block diagonal in these.

        States that share a column shape (at most 255 columns), order and derivatives object -- with ANY number of samples
        each -- are served by one launch per kernel (txm_influence_cross_cov_batched) after one copy of their moments to
        the host, and the result is cached on the collection.  A state's slice equals its own ``derivs_cross_cov()`` bit
        for bit unless it has more samples than its share of the device (``256 * (8 CUs // (tile pairs * states))``);
        then the same sums are added in another order, within the same rounding bound.  The states' own caches are not
        touched.  Other collections loop over the states.

        Assumptions: first order; independent states; independent samples within a state unless ``block`` is given (an
        int for all states, or one entry per state: ``ExtrapModel.derivs_cross_cov(block=...)``, looped over the states).
        A state that ``derivs_cov`` refuses raises its NotImplementedError, more than 255 columns ValueError."""
        covs, srcs, orders = self._state_cross_covs(order, minus_log, block)
        out = [ExtrapModel._derivs_cross_cov_labelled(covs[s], srcs[s], orders[s], norm) for s in range(len(self))]
        return concat(out, dim=DataArray(np.asarray(self.alpha0), self.alpha_name))

    # states per launch of the batched path: the sampler table is [S * nrep][ntiles] and the grid carries the state on z
    _BATCH_MAX_REPS = 1 << 22
    _BATCH_MAX_WS = 8 << 30   # bytes of library workspace per batched launch

    def _resample_batched(self, spec: Mapping, rep_dim=None, state0: int = 0):
        """One sampler over S * nrep replicates, one bootstrap launch, per-state views of the result.

        With the device sampler, state s of THIS collection draws replicates ``(state0 + s) * nrep ...`` of the
        stream of ``spec["seed"]`` (plus ``spec["rep0"]``): a sub-collection ``states[a:b]`` resampled with
        ``state0=a`` reproduces rows ``a:b`` of the whole collection's result bit for bit -- what
        ``resample(sharded=True)`` relies on."""
        from . import engine, moments as cm

        d0 = self.states[0].data
        S, N = len(self), len(d0)
        nrep = int(spec["nrep"])
        nsamp = spec.get("nsamp")
        if rep_dim is None:
            rep_dim = spec.get("rep_dim", "rep")
        def gather():
            xs, us, ws = [], [], []
            for st in self.states:
                xt, _ = cm._dev_and_dims(st.data.xv)
                ut, _ = cm._dev_and_dims(st.data.uv)
                xs.append(xt.reshape(N, -1))
                us.append(ut)
                if st.data.weight is not None:
                    w = st.data.weight
                    ws.append(cm._dev_and_dims(w)[0] if (is_labelled(w) or isinstance(w, cm.DeviceDataArray))
                              else engine.to_device(np.asarray(w)))
            return xs, us, ws

        use_device = spec.get("device")
        if use_device is None:
            # the serial loop's rule, per state (reference draws below that size): the batched call must not change
            # which draws a seeded {"nrep", "rng"} spec gets
            use_device = nrep * (nsamp or N) > cm.EXPLICIT_SAMPLER_MAX
        if use_device:
            seed = spec.get("seed")
            if seed is None:
                seed = int(cm.validate_rng(spec.get("rng")).integers(0, 2**63 - 1))
            rep0 = int(spec.get("rep0", 0)) + int(state0) * nrep
            ns = 0 if (nsamp is None or nsamp == N) else int(nsamp)
            # groups of states whose S_g * nrep replicates fit one sampler table / launch ...
            per = max(1, min(S, self._BATCH_MAX_REPS // max(nrep, 1)))
            # ... and whose workspace stays bounded: on the int8 path every state has its own per-window partial-sum slots
            # and fallback buffers (75 MB per state at config 5's shape -- a thousand states would ask for 75 GB at once)
            C_all = int(cm._dev_and_dims(d0.xv)[0].reshape(N, -1).shape[1])
            ws1 = int(engine._L().txm_resample_vals_batched_ws_bytes(1, N, C_all, nrep, d0.order))
            per = max(1, min(per, self._BATCH_MAX_WS // max(ws1, 1)))
            # the tile counts first: their kernel (0.2 - 0.4 ms for 64 x 100 replicates) runs while the host walks the states
            # for their tensors, keys and checks -- a step starts on an idle device (the previous one ended in a copy to the host)
            # (the first group's: further groups -- collections beyond _BATCH_MAX_REPS replicates -- draw theirs in turn, one table alive at a time)
            smp0 = engine.DeviceSampler(seed, min(S, per) * nrep, N, ns, rep0=rep0)
            xs, us, ws = gather()
            parts = []
            for a in range(0, S, per):
                b = min(S, a + per)
                smp = smp0 if a == 0 else engine.DeviceSampler(seed, (b - a) * nrep, N, ns, rep0=rep0 + a * nrep)
                smp0 = None
                # the int8 path's pre-pass block of this group of states lives with the group's first data object (the
                # reference caches per data object: data.py:285); its key is the whole group's tensors, so another
                # collection that merely starts with the same state recomputes it
                dcache = getattr(self.states[a].data, "_cache", None)
                prep = None
                if dcache is not None:
                    prep = dcache.get("resample_prep_batched")
                    if prep is None:
                        prep = dcache["resample_prep_batched"] = engine.ResamplePrep()
                parts.append(engine.resample_vals_batched(xs[a:b], us[a:b], d0.order, nrep=nrep, sampler=smp,
                                                          ws=ws[a:b] if ws else None, prep=prep))
            big = parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)
        else:
            if spec.get("rep0") or state0:
                raise ValueError("rep0 / state shards address the device sampler's stream: pass device=True in the spec")
            # the reference's draws, state after state from the same generator (what the serial loop consumes)
            # -- in groups of states whose index / frequency tables stay within EXPLICIT_SAMPLER_MAX elements per launch
            # (the rule above is per state: a collection just under it would otherwise build S such tables at once)
            xs, us, ws = gather()
            rng = cm.validate_rng(spec.get("rng"))
            per = max(1, min(S, cm.EXPLICIT_SAMPLER_MAX // max(nrep * (nsamp or N), 1)))
            parts = []
            for a in range(0, S, per):
                b = min(S, a + per)
                idx = np.concatenate([rng.choice(N, size=(nrep, nsamp or N), replace=True) for _ in range(a, b)])
                freq = engine.indices_to_freq(torch.as_tensor(idx).cuda(), N)
                del idx
                parts.append(engine.resample_vals_batched(xs[a:b], us[a:b], d0.order, nrep=nrep, freq=freq,
                                                          ws=ws[a:b] if ws else None))
                del freq
            big = parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)
        cshape = tuple(d0.xv.shape[1:])
        K = d0.order + 1
        big = big.reshape(S, nrep, *cshape, 2, K)
        dims = (rep_dim, *d0.xv.dims[1:], d0.xmom_dim, d0.umom_dim)
        states = []
        for s, st in enumerate(self.states):
            dx = cm.CentralMomentsData(big[s], mom_ndim=2, dims=dims)
            data = st.data.new_like(dxduave=dx, rec_dim=rep_dim, meta=st.data.meta)
            states.append(st.new_like(order=st.order, alpha0=st.alpha0, derivatives=st.derivatives, data=data,
                                      minus_log=st.minus_log, alpha_name=st.alpha_name))
        out = type(self)(states=tuple(states), kws=self.kws)
        out._batch = {"big": big, "nrep": nrep, "rep_dim": rep_dim}
        return out

    def resample(self, sampler, batched=None, **kws):
        """Resample every state; a single sampler spec is reused (each state
        draws its own sample from a mapping), or give one sampler per state.

        ``batched`` (extension): None -- when every state is an ExtrapModel over sample data of one shape and the
        sampler is a ``{"nrep": n, ...}`` mapping, all states are bootstrapped by ONE launch per kernel
        (txm_resample_vals_batched) instead of the reference's serial loop (models.py:635-641); False keeps
        the loop; True insists.  With the device sampler the states draw independent replicate streams of one
        seed; with numpy draws the generator is consumed state after state exactly as the loop does.
        ``sharded=True`` (extension) splits the states over the ranks of an initialised torch.distributed
        group (thermoextrap_amd.distributed.sharded_states) and all-gathers the replicate states."""
        sharded = kws.pop("sharded", False)
        state0 = kws.pop("state0", 0)
        is_spec = isinstance(sampler, Mapping) and "nrep" in sampler and "indices" not in sampler and "freq" not in sampler
        if sharded:
            return self._resample_sharded(sampler, batched=batched, **kws)
        # (a shard of a collection -- state0 given, or batched=True -- takes the batched launch even with one state)
        if batched is not False and is_spec and not kws and self._batch_eligible(1 if (state0 or batched) else 2) is not None:
            return self._resample_batched(sampler, state0=state0)
        if batched is True:
            raise ValueError("batched=True needs ExtrapModel states over DataCentralMomentsVals of one shape and a "
                             '{"nrep": n} sampler mapping')
        if state0:
            # the serial loop on the device stream: state s draws replicates (state0 + s) * nrep ... like the batched path
            if not (is_spec and sampler.get("device") and sampler.get("seed") is not None):
                raise ValueError('state0 needs a {"nrep", "seed", "device": True} sampler mapping')
            nrep, r0 = int(sampler["nrep"]), int(sampler.get("rep0", 0))
            sampler = [{**sampler, "rep0": r0 + (state0 + i) * nrep} for i in range(len(self))]
        elif is_spec and sampler.get("device") and sampler.get("seed") is not None:
            # one seed for the collection: independent replicate ranges per state, the same as the batched path
            nrep, r0 = int(sampler["nrep"]), int(sampler.get("rep0", 0))
            sampler = [{**sampler, "rep0": r0 + i * nrep} for i in range(len(self))]
        if isinstance(sampler, (np.ndarray, IndexSampler, Mapping)) or is_labelled(sampler):
            sampler = [sampler] * len(self)
        elif len(sampler) != len(self):
            raise ValueError(f"len(sampler)={len(sampler)} must equal len(self)={len(self)}")
        return type(self)(states=tuple(st.resample(sampler=sm, **kws) for st, sm in zip(self.states, sampler)),
                          kws=self.kws)

    def _resample_sharded(self, sampler, batched=None, **kws):
        """State-point sharding over torch.distributed ranks: rank r bootstraps its contiguous share of the states
        (batched when eligible), the replicate states are all-gathered (one collective of a few MB) and every
        rank returns the full collection.

        The result equals the unsharded ``resample(sampler)`` BIT FOR BIT: the spec must name the device stream
        (``{"nrep": n, "seed": s, "device": True}``) and state ``i`` of the collection draws stream replicates
        ``i * nrep ...`` on whichever rank owns it (txm_sampler_spec.rep0).  A spec without a seed gets one drawn
        on rank 0 and broadcast; numpy draws (``device=False``) cannot be sharded consistently and are refused.
        (The reference runs this loop serially with independent draws per state: models.py:614-641.)"""
        from . import distributed as D, moments as cm

        rank, w = D.world()
        is_spec = isinstance(sampler, Mapping) and "nrep" in sampler and "indices" not in sampler and "freq" not in sampler
        if not is_spec:
            raise ValueError('sharded=True needs a {"nrep": n, ...} sampler mapping (one stream for the whole collection)')
        if sampler.get("device") is False:
            raise ValueError("sharded=True draws from the device sampler stream; device=False (numpy draws) cannot be "
                             "split over ranks consistently")
        spec = {**sampler, "device": True}
        if spec.get("seed") is None:
            seed0 = int(cm.validate_rng(spec.get("rng")).integers(0, 2**63 - 1)) if rank == 0 else 0
            spec["seed"] = D.broadcast_int(seed0)
        mine = D.shard_range(len(self), rank, w)
        if len(mine) == 0:
            raise ValueError("more ranks than states: give every rank at least one state")
        if batched is None and not kws and self._batch_eligible() is not None:
            batched = True  # every shard on the batched kernels, also a rank that holds one state
        sub = type(self)(states=tuple(self.states[i] for i in mine), kws=self.kws).resample(
            spec, batched=batched, state0=mine[0], **kws)
        slabs = torch.stack([st.data.dxduave.device_values for st in sub.states])
        full = D.all_gather_slabs(slabs, D.shard_counts(len(self), w))
        states = []
        for s, st in enumerate(self.states):
            ref = sub.states[0].data
            dx = cm.CentralMomentsData(full[s], mom_ndim=2, dims=ref.dxduave.dims)
            data = st.data.new_like(dxduave=dx, rec_dim=ref.rec_dim, meta=st.data.meta)
            states.append(st.new_like(order=st.order, alpha0=st.alpha0, derivatives=st.derivatives, data=data,
                                      minus_log=st.minus_log, alpha_name=st.alpha_name))
        out = type(self)(states=tuple(states), kws=self.kws)
        if self._batch_eligible() is not None:
            out._batch = {"big": full, "nrep": full.shape[1], "rep_dim": ref.rec_dim}
        return out

    def map(self, func, *args, **kwargs):
        if isinstance(func, str):
            return [getattr(s, func)(*args, **kwargs) for s in self]
        return [func(s, *args, **kwargs) for s in self]

    def _derivs_batched(self, order=None, order_dim="order", minus_log=None, norm=False, _device=False):
        """derivs/coefs of every state of a batched resample in ONE evaluation: the replicate states sit in one
        (S, nrep, ...) tensor, so (state, rep) is the evaluator's replicate axis; one launch, one D2H copy."""
        from . import moments as cm

        b = self._batch
        st0 = self.states[0]
        big = b["big"]
        S, nrep = big.shape[0], big.shape[1]
        flat = big.reshape(S * nrep, *big.shape[2:])
        d0 = st0.data
        data = d0.new_like(dxduave=cm.CentralMomentsData(flat, mom_ndim=2, dims=d0.dxduave.dims))
        if minus_log is None:
            minus_log = st0.minus_log
        if order is None:
            order = st0.order
        vals, src = st0.derivatives.derivs(data=data, order=order, norm=norm, minus_log=minus_log, _device=True)
        vals = vals.reshape(order + 1, S, nrep, -1)
        if _device:
            return vals, src
        host = vals.permute(1, 0, 2, 3).cpu().numpy().reshape(S, order + 1, nrep, *src.out_shape[1:])
        out = DataArray(host, (self.alpha_name, order_dim, *src.out_dims))
        out._inherit(src.coords)
        return out.assign_coords({self.alpha_name: np.asarray(self.alpha0)})

    def map_concat(self, func, concat_dim=None, concat_kws=None, *args, **kwargs):
        if (func in ("derivs", "coefs") and getattr(self, "_batch", None) is not None and concat_dim is None
                and not args and not concat_kws and set(kwargs) <= {"order", "order_dim", "minus_log", "norm"}
                and kwargs.get("order_dim", "order") is not None):
            kw = dict(kwargs)
            if func == "coefs":
                kw["norm"] = True
            return self._derivs_batched(**kw)
        out = self.map(func, *args, **kwargs)
        if is_labelled(out[0]):
            if concat_dim is None:
                concat_dim = DataArray(np.asarray(self.alpha0), self.alpha_name)
            out = concat(out, dim=concat_dim, **(concat_kws or {}))
        return out

    def append(self, states, sort=True, key=None, **kws):
        new_states = list(self.states) + list(states)
        if sort:
            new_states = sorted(new_states, key=key or (lambda x: x.alpha0), **kws)
        return type(self)(new_states, kws=self.kws)

    @property
    def order(self):
        return min(m.order for m in self)

    @property
    def alpha0(self):
        return [m.alpha0 for m in self]


class PerturbModel(_Params):
    """Exponential reweighting to another alpha (reference models.py:1009-1047):

        <x>(alpha) = sum_i x_i e^{-(alpha-alpha0) u_i} / sum_i e^{-(alpha-alpha0) u_i}

    evaluated for all requested alphas in one pass over the samples
    (txm_perturb).  ``data`` must be a values-holding object (``DataValues``)."""

    _fields = ("alpha0", "data", "alpha_name")

    def __init__(self, alpha0, data, alpha_name="alpha"):
        if not isinstance(data, AbstractData):
            raise TypeError("data must be a data object")
        self.alpha0 = float(alpha0)
        self.data = data
        self.alpha_name = "alpha" if alpha_name is None else alpha_name

    def predict(self, alpha, alpha_name=None):
        from .moments import _dev_and_dims

        if alpha_name is None:
            alpha_name = self.alpha_name
        alpha = xrwrap_alpha(alpha, name=alpha_name)
        dalpha = np.atleast_1d(np.asarray(alpha.values, dtype=float) - self.alpha0)
        data = self.data
        rec = data.rec_dim
        res = getattr(data, "_resampled", None)
        if res is not None:
            buv, bxv, sampler, rep_dim = res
        else:
            buv, bxv, sampler, rep_dim = data._uv if hasattr(data, "_uv") else data.uv, \
                data._xv if hasattr(data, "_xv") else data.xv, None, None
        ut, udims = _dev_and_dims(buv)
        xt, xdims = _dev_and_dims(bxv)
        if udims != (rec,):
            raise NotImplementedError("uv must be 1-D along the record dim")
        others = [d for d in xdims if d != rec]
        x2 = xt.movedim(xdims.index(rec), 0)
        cshape = list(x2.shape[1:])
        x2 = x2.reshape(x2.shape[0], -1) if x2.dim() > 1 else x2
        freq = sampler.freq_device() if sampler is not None else None
        out = engine.perturb(x2, ut, dalpha, freq=freq)  # (na, C) | (nrep, na, C) | 1-D x: (na,) | (nrep, na)
        vals = out.cpu().numpy()
        if sampler is not None:
            vals = np.moveaxis(vals, 0, 1)  # (na, nrep, ...)
            vals = vals.reshape(len(dalpha), sampler.nrep, *cshape)
            dims = [alpha_name, rep_dim, *others]
        else:
            vals = vals.reshape(len(dalpha), *cshape)
            dims = [alpha_name, *others]
        if alpha.ndim == 0:
            vals, dims = vals[0], dims[1:]
            return DataArray(vals, dims, coords={alpha_name: alpha.values})
        return DataArray(vals, dims, coords={alpha_name: alpha.values})

    def __call__(self, *args, **kwargs):
        return self.predict(*args, **kwargs)

    def resample(self, sampler, **kws):
        return type(self)(alpha0=self.alpha0, data=self.data.resample(sampler=sampler, **kws),
                          alpha_name=self.alpha_name)

    # ---- delta-method error bars, effective samples, free energies --------------------------------------
    def _refuse_resampled(self, what):
        if getattr(self.data, "_resampled", None) is not None:
            raise NotImplementedError(f"{what}: this PerturbModel holds resampled data; take the error bars of the "
                                      "PerturbModel it was resampled from")

    def _perturb_cov(self, what, alpha, alpha_name, block, n_levels=1):
        """``(engine.PerturbCov, alpha, alpha_name, other dims, their shape)`` of one ``engine.perturb_cov`` on the
        operands ``predict`` passes to ``engine.perturb`` -- or NotImplementedError for a resampled model."""
        from .moments import _dev_and_dims

        self._refuse_resampled(what)
        data = self.data
        if alpha_name is None:
            alpha_name = self.alpha_name
        alpha = xrwrap_alpha(alpha, name=alpha_name)
        dalpha = np.atleast_1d(np.asarray(alpha.values, dtype=float) - self.alpha0)
        rec = data.rec_dim
        ut, udims = _dev_and_dims(data._uv if hasattr(data, "_uv") else data.uv)
        xt, xdims = _dev_and_dims(data._xv if hasattr(data, "_xv") else data.xv)
        if udims != (rec,):
            raise NotImplementedError("uv must be 1-D along the record dim")
        others = [d for d in xdims if d != rec]
        x2 = xt.movedim(xdims.index(rec), 0)
        cshape = list(x2.shape[1:])
        x2 = x2.reshape(x2.shape[0], -1) if x2.dim() > 1 else x2
        block = 1 if block is None else _check_block_type(block)
        res = engine.perturb_cov(x2, ut, dalpha, block=block, n_levels=n_levels)
        return res, alpha, alpha_name, others, cshape

    @staticmethod
    def _alpha_labelled(vals, alpha, alpha_name, dims=()):
        """vals (n_alpha, ...) with ``predict``'s labelling: the alpha axis dropped for a scalar alpha."""
        if alpha.ndim == 0:
            return DataArray(vals[0], list(dims), coords={alpha_name: alpha.values})
        return DataArray(vals, [alpha_name, *dims], coords={alpha_name: alpha.values})

    def predict_with_error(self, alpha, alpha_name=None, block=None):
        """``(value, std)``: ``predict(alpha)`` bit for bit and its delta-method (infinitesimal-jackknife) standard
        deviation, both with ``predict``'s dims: ``std^2 = sum_n p_n^2 (x_n - <x>(alpha))^2`` with ``p_n`` the normalised
        weights ``e^{-(alpha - alpha0) u_n}`` -- one more pass over the samples per 8 alphas (txm_perturb_cov), no
        replicates, no sampling noise.

        Assumptions: first order (what the multinomial bootstrap ``resample`` estimates, without its noise); INDEPENDENT
        samples unless ``block`` is given; no 1 / n_eff correction.  The bar is unreliable once ``effective_samples`` is
        small: exponential reweighting degrades silently when the target leaves the sampled energies, and that method
        is how to see it.  ``block=B`` (an int; ``None`` means 1) is for a CORRELATED series kept whole: the records are
        cut into contiguous blocks of B (a last short one is kept) and ``std^2 = sum_b (sum_{n in b} p_n (x_n - <x>))^2``
        -- batch means, B beyond the correlation time (``timeseries.block_length`` proposes one, ``blocking_curve`` shows
        whether the variance has levelled off).  A resampled model raises NotImplementedError."""
        res, alpha, alpha_name, others, cshape = self._perturb_cov("predict_with_error (delta-method error bars)", alpha,
                                                                   alpha_name, block)
        na = len(res.neff)
        val = res.mean.cpu().numpy().reshape(na, *cshape)
        std = np.sqrt(np.maximum(res.var[0].cpu().numpy(), 0.0)).reshape(na, *cshape)
        return self._alpha_labelled(val, alpha, alpha_name, others), self._alpha_labelled(std, alpha, alpha_name, others)

    def effective_samples(self, alpha, alpha_name=None):
        """Kish's effective sample number at every alpha, ``(sum_n w_n)^2 / sum_n w_n^2`` with
        ``w_n = e^{-(alpha - alpha0) u_n}``: N at ``alpha0``, towards 1 when a few samples carry the average (then
        neither the prediction nor its error bar means much)."""
        res, alpha, alpha_name, _, _ = self._perturb_cov("effective_samples", alpha, alpha_name, None)
        return self._alpha_labelled(res.neff.cpu().numpy(), alpha, alpha_name)

    def free_energy(self, alpha, alpha_name=None, block=None):
        """``(f, df)`` relative to ``alpha0`` (``MBARModel.free_energy(alpha)``'s convention; the Zwanzig / EXP estimator,
        MBAR with one state): ``f = -ln <e^{-(alpha - alpha0) u}>`` and its delta-method standard deviation
        ``df^2 = sum_n (p_n - 1 / N)^2 = 1 / n_eff - 1 / N``, or with ``block=B`` the batch-means form
        ``sum_b (sum_{n in b} p_n - n_b / N)^2`` for a correlated series.  The assumptions of ``predict_with_error``
        apply."""
        res, alpha, alpha_name, _, _ = self._perturb_cov("free_energy", alpha, alpha_name, block)
        f = -res.lnq.cpu().numpy()
        df = np.sqrt(np.maximum(res.var_lnq[0].cpu().numpy(), 0.0))
        return self._alpha_labelled(f, alpha, alpha_name), self._alpha_labelled(df, alpha, alpha_name)

    def blocking_curve(self, alpha, block, alpha_name=None):
        """The blocking curve of Flyvbjerg & Petersen (1989) for ``predict_with_error``: ``(var, block_lengths, n_blocks)``
        with ``var[l] = predict_with_error(alpha, block=block * 2**l)[1] ** 2`` (dims ``(level, alpha, *val_dims)``),
        ``block_lengths[l] = block * 2**l`` and ``n_blocks[l] = ceil(N / block_lengths[l])``, for every level that still
        has at least two blocks.  ONE kernel call per 8 alphas: block sums are additive, so each level merges the pairs
        of the level below.  Where var stops growing with the block length the blocks are longer than the correlation
        time; the last levels are noisy (relative standard deviation about ``sqrt(2 / (n_blocks - 1))``) and biased by
        ``-1 / n_blocks``."""
        from .moments import _dev_and_dims

        block = _check_block_type(block)
        self._refuse_resampled("blocking_curve")
        data = self.data
        ut, _ = _dev_and_dims(data._uv if hasattr(data, "_uv") else data.uv)
        lengths, counts = engine.block_levels(int(ut.shape[0]), block)
        res, alpha, alpha_name, others, cshape = self._perturb_cov("blocking_curve", alpha, alpha_name, block,
                                                                   n_levels=len(lengths))
        host = res.var.cpu().numpy()
        na = host.shape[1]
        out = concat([self._alpha_labelled(host[l].reshape(na, *cshape), alpha, alpha_name, others)
                      for l in range(host.shape[0])], dim=DataArray(lengths.copy(), "level"))
        return out, lengths.copy(), counts.copy()


# ---------------------------------------------------------------------------
# Multi-state models (reference models.py:710-1007).  Host algebra on top of
# ExtrapModel.derivs / predict, which are where the device work happens.
# ---------------------------------------------------------------------------
def _alpha_seq(alpha):
    try:
        return list(iter(alpha))
    except TypeError:
        return [alpha]


def xr_weights_minkowski(deltas, m=20, dim="state"):
    """Minkowski-like weights ``1 - d^m / sum_dim d^m`` (reference models.py:726-728)."""
    dm = deltas**m
    return 1.0 - dm / dm.sum(dim)


class PiecewiseMixin:
    """Pick the two states that bracket (or are nearest to) an alpha
    (reference models.py:731-761).  States must be in ascending ``alpha0`` order."""

    def _check_alpha(self, alpha, bounded=False) -> None:
        if not bounded:
            return
        lo, hi = self[0].alpha0, self[-1].alpha0
        for a in _alpha_seq(alpha):
            if a < lo or a > hi:
                raise ValueError(f"{a} outside of bounds [{lo}, {hi}]")

    def _indices_between_alpha(self, alpha):
        i = int(np.searchsorted(np.asarray(self.alpha0), alpha, side="right")) - 1
        i = min(max(i, 0), len(self) - 2)
        return [i, i + 1]

    def _indices_nearest_alpha(self, alpha):
        dist = np.abs(np.asarray(self.alpha0) - alpha)
        return [int(i) for i in np.argsort(dist)[:2]]

    def _indices_alpha(self, alpha, method):
        if method is None or method == "between":
            return self._indices_between_alpha(alpha)
        if method == "nearest":
            return self._indices_nearest_alpha(alpha)
        raise ValueError(f"unknown method {method}")

    def _states_alpha(self, alpha, method):
        return [self[i] for i in self._indices_alpha(alpha, method)]

    def _per_alpha(self, alpha, alpha_name, one):
        """Evaluate ``one(a)`` for each scalar alpha and join along ``alpha_name``."""
        seq = [float(a) for a in _alpha_seq(alpha)]
        outs = [one(a) for a in seq]
        if np.ndim(alpha) == 0:
            return outs[0]
        return concat(outs, dim=DataArray(np.asarray(seq), alpha_name))


class ExtrapWeightedModel(StateCollection, PiecewiseMixin):
    """Two Taylor series, one from each side, blended with Minkowski weights on
    the distance to each reference state (reference models.py:764-858)."""

    def predict(self, alpha, order=None, order_dim="order", cumsum=False, minus_log=None, alpha_name=None,
                method=None, bounded=False):
        self._check_alpha(alpha, bounded)
        if order is None:
            order = self.order
        if alpha_name is None:
            alpha_name = self.alpha_name
        if len(self) != 2:
            if np.ndim(np.asarray(alpha)) > 0:
                return self._per_alpha(alpha, alpha_name, lambda a: self.predict(
                    a, order=order, order_dim=order_dim, cumsum=cumsum, minus_log=minus_log,
                    alpha_name=alpha_name, method=method))
            pair = self._states_alpha(alpha, method)
        else:
            pair = list(self.states)
        alpha = xrwrap_alpha(alpha, name=alpha_name)
        preds = [m.predict(alpha, order=order, order_dim=order_dim, cumsum=cumsum, minus_log=minus_log,
                           alpha_name=alpha_name, dalpha_coords=None, alpha0_coords=False) for m in pair]
        dist = concat([abs(alpha - m.alpha0) for m in pair], dim="state")
        w = xr_weights_minkowski(dist, dim="state")
        num = sum(p * w.isel(state=i) for i, p in enumerate(preds))
        return num / w.sum("state")

    def predict_with_error(self, alpha, order=None, minus_log=None, alpha_name=None, method=None, bounded=False, block=None):
        """``(predict(alpha, ...), std)``: the blended prediction, bit for bit ``predict``'s, and its delta-method
        standard deviation.  The blend is ``sum_i w_i T_i(alpha) / sum_i w_i`` over the two states ``predict`` picks
        (``method``, ``bounded`` as there), with the Minkowski weights ``w_i`` a function of alpha alone, so

            var = sum_i (w_i / sum w)^2 t_i' V_i t_i,    t_ik = (alpha - alpha0_i)^k / k!,  V_i = states[i].derivs_cov(order)

        Assumptions: independent samples within a state (``ExtrapModel.derivs_cov``), independent states (no cross
        terms), first order.  All states' ``V_i`` come from one launch per kernel (``StateCollection.derivs_cov``); a state
        that ``derivs_cov`` refuses raises its NotImplementedError.  ``block`` (an int, or one entry per state): the
        blocked ``V_i`` of correlated series (``StateCollection.derivs_cov``)."""
        self._check_alpha(alpha, bounded)
        if order is None:
            order = self.order
        if alpha_name is None:
            alpha_name = self.alpha_name
        covs, srcs = self._state_covs(order, minus_log, block)         # (first: an unsupported state says so)
        pred = self.predict(alpha, order=order, minus_log=minus_log, alpha_name=alpha_name, method=method, bounded=bounded)
        al = xrwrap_alpha(alpha, name=alpha_name)
        var = _delta.minkowski_contract(self, al, order, method, covs, "i,cij,j->c")
        return pred, self[0]._ds(_delta.label_std(var, al, srcs[0]))

    def predict_cov(self, alpha, order=None, minus_log=None, alpha_name=None, method=None, bounded=False, block=None):
        """``(predict(alpha, ...), cov)``: the blended prediction, bit for bit ``predict``'s, and the delta-method
        covariance of the predicted columns, dims ``(*alpha dims, *val_dims, *[d + "_2" for d in val_dims])``:

            cov[alpha, c, c'] = sum_i (w_i / sum w)^2 t_i' V_i[:, :, c, c'] t_i,    V_i = states[i].derivs_cross_cov(order)

        with ``predict_with_error``'s weights and ``t``; its squared std is the diagonal ``c == c'`` up to rounding.  All
        ``V_i`` come from one launch per kernel (``StateCollection.derivs_cross_cov``).  Assumptions: first order;
        independent states; independent samples within a state unless ``block`` is given (an int, or one entry per
        state)."""
        self._check_alpha(alpha, bounded)
        if order is None:
            order = self.order
        if alpha_name is None:
            alpha_name = self.alpha_name
        covs, srcs, _ = self._state_cross_covs(order, minus_log, block)      # (first: an unsupported state says so)
        pred = self.predict(alpha, order=order, minus_log=minus_log, alpha_name=alpha_name, method=method, bounded=bounded)
        al = xrwrap_alpha(alpha, name=alpha_name)
        return pred, _delta.label_cov(_delta.minkowski_contract(self, al, order, method, covs, "i,cidj,j->cd"), al, srcs[0])


class InterpModel(StateCollection):
    """One polynomial through the value and the first ``order`` derivatives at
    every state (Hermite interpolation; reference models.py:861-946)."""

    def _hermite_inverse(self, order):
        key = ("hermite", order)
        if key not in self._cache:
            npoly = len(self) * (order + 1)
            p = np.arange(npoly)
            rows = []
            for a0 in self.alpha0:
                for j in range(order + 1):
                    # d^j/da^j a^p = p!/(p-j)! a^(p-j), zero below the diagonal
                    fall = np.array([math.perm(int(q), j) if q >= j else 0 for q in p], dtype=float)
                    powr = np.where(p >= j, np.power(float(a0), np.maximum(p - j, 0)), 0.0)
                    rows.append(fall * powr)
            self._cache[key] = np.linalg.inv(np.array(rows))
        return self._cache[key]

    def coefs(self, order=None, order_dim="porder", minus_log=None):
        if order is None:
            order = self.order
        inv = self._hermite_inverse(order)                       # [porder, state*(order+1)]
        ds = [m.derivs(order, norm=False, minus_log=minus_log, order_dim="order") for m in self.states]
        first = ds[0]
        rest = [d for d in first.dims if d != "order"]
        stacked = np.concatenate([d.transpose("order", *rest).values for d in ds], axis=0)
        vals = np.tensordot(inv, stacked, axes=(1, 0))
        out = DataArray(vals, (order_dim, *rest), None, first.name)
        out._inherit({k: v for k, v in first._coords.items() if "order" not in v[0]})
        return out

    def predict(self, alpha, order=None, order_dim="porder", minus_log=None, alpha_name=None):
        if order is None:
            order = self.order
        if alpha_name is None:
            alpha_name = self.alpha_name
        coefs = self.coefs(order=order, order_dim=order_dim, minus_log=minus_log)
        alpha = xrwrap_alpha(alpha, name=alpha_name)
        p = DataArray(np.arange(coefs.sizes[order_dim]), order_dim)
        return ((alpha**p) * coefs).sum(order_dim)

    def _predict_std(self, alpha, order, minus_log, alpha_name, block=None):
        """Delta-method standard deviation of ``predict(alpha)`` (see ``predict_with_error``)."""
        covs, srcs = self._state_covs(order, minus_log, block)              # [S][n_out, order + 1, order + 1]
        al = xrwrap_alpha(alpha, name=alpha_name)
        var = _delta.hermite_contract(self._hermite_inverse(order), al, order, covs, "ai,cij,aj->ac")
        return self[0]._ds(_delta.label_std(var, al, srcs[0]))

    def predict_with_error(self, alpha, order=None, minus_log=None, alpha_name=None, block=None):
        """``(predict(alpha), std)``: the interpolation, bit for bit ``predict``'s, and its delta-method standard
        deviation.  ``predict`` is linear in the states' un-normalised derivatives D (stacked state by state):
        ``g(alpha)' D`` with ``g = (alpha^p) . hermite_inverse``, so

            var = sum_s g_s' V_s g_s,      V_s = states[s].derivs_cov(order)

        Assumptions: independent samples within a state (``ExtrapModel.derivs_cov``: decorrelate time series first),
        independent states (the covariance of D is block diagonal), first order.  All ``V_s`` come from one launch per
        kernel (``StateCollection.derivs_cov``); a state that ``derivs_cov`` refuses raises its NotImplementedError.
        ``block`` (an int, or one entry per state): the blocked ``V_s`` of correlated series kept whole."""
        if order is None:
            order = self.order
        if alpha_name is None:
            alpha_name = self.alpha_name
        std = self._predict_std(alpha, order, minus_log, alpha_name, block)    # (first: an unsupported state says so)
        return self.predict(alpha, order=order, minus_log=minus_log, alpha_name=alpha_name), std

    def _predict_cov_from(self, alpha, order, alpha_name, covs, src):
        """``cov[alpha, c, c'] = sum_s g_s' V_s[:, :, c, c'] g_s`` with the ``g`` of ``_predict_std`` and the states'
        covariances handed in: ``covs[s]`` [n_out, order + 1, n_out, order + 1] on the host, one per state of THIS model
        in order.  Labelled ``(*alpha dims, *val_dims, *val_dims_2)``."""
        if len(covs) != len(self):
            raise ValueError(f"{len(covs)} covariances for {len(self)} states")
        al = xrwrap_alpha(alpha, name=alpha_name)
        return _delta.label_cov(_delta.hermite_contract(self._hermite_inverse(order), al, order, covs, "ai,cidj,aj->acd"), al, src)

    def predict_cov(self, alpha, order=None, minus_log=None, alpha_name=None, block=None):
        """``(predict(alpha), cov)``: the interpolation, bit for bit ``predict``'s, and the delta-method covariance of the
        predicted columns, dims ``(*alpha dims, *val_dims, *[d + "_2" for d in val_dims])``:

            cov[alpha, c, c'] = sum_s g_s' V_s[:, :, c, c'] g_s,     V_s = states[s].derivs_cross_cov(order)

        with ``g = (alpha^p) . hermite_inverse`` as in ``predict_with_error``, whose squared std is the diagonal
        ``c == c'`` up to rounding.  All ``V_s`` come from one launch per kernel (``StateCollection.derivs_cross_cov``).
        Assumptions: first order; independent states; independent samples within a state unless ``block`` is given (an
        int, or one entry per state: the blocked ``V_s`` of correlated series kept whole)."""
        if order is None:
            order = self.order
        if alpha_name is None:
            alpha_name = self.alpha_name
        covs, srcs, _ = self._state_cross_covs(order, minus_log, block)      # (first: an unsupported state says so)
        pred = self.predict(alpha, order=order, minus_log=minus_log, alpha_name=alpha_name)
        return pred, self._predict_cov_from(alpha, order, alpha_name, covs, srcs[0])


class InterpModelPiecewise(StateCollection, PiecewiseMixin):
    """Two-state Hermite interpolation chosen per alpha (reference models.py:949-1006)."""

    def single_interpmodel(self, *state_indices):
        key = ("pair", tuple(int(i) for i in state_indices))
        if key not in self._cache:
            i, j = key[1]
            self._cache[key] = InterpModel([self[i], self[j]])
        return self._cache[key]

    def predict(self, alpha, order=None, order_dim="porder", minus_log=None, alpha_name=None, method=None,
                bounded=False):
        self._check_alpha(alpha, bounded)
        if alpha_name is None:
            alpha_name = self.alpha_name
        kws = dict(order=order, order_dim=order_dim, minus_log=minus_log, alpha_name=alpha_name)
        if len(self) == 2:
            return self.single_interpmodel(0, 1).predict(alpha, **kws)
        seq = [float(a) for a in _alpha_seq(alpha)]
        outs = [self.single_interpmodel(*self._indices_alpha(a, method)).predict(a, **kws) for a in seq]
        if len(outs) == 1:
            return outs[0]
        return concat(outs, dim=DataArray(np.asarray(seq), alpha_name))

    def predict_with_error(self, alpha, order=None, minus_log=None, alpha_name=None, method=None, bounded=False, block=None):
        """``(predict(alpha, ...), std)``: for every alpha the two-state ``InterpModel`` that ``predict`` chooses
        (``method``, ``bounded`` as there) and that model's ``predict_with_error`` -- its assumptions apply: independent
        samples within a state, independent states, first order.  The covariances of ALL states are taken first, in one
        launch per kernel, so the pairs find them in their states' caches.  ``block`` (an int, or one entry per state):
        the blocked covariances of correlated series; a pair takes its two states' entries."""
        self._check_alpha(alpha, bounded)
        blocks = self._blocks_per_state(block)
        self._derivs_cov_fill(order, minus_log, block)                  # (first: an unsupported state says so)
        pred = self.predict(alpha, order=order, minus_log=minus_log, alpha_name=alpha_name, method=method, bounded=bounded)
        if alpha_name is None:
            alpha_name = self.alpha_name

        def std_of(idx, a):
            pair = self.single_interpmodel(*idx)
            return pair._predict_std(a, pair.order if order is None else order, minus_log, alpha_name,
                                     None if blocks is None else [blocks[int(i)] for i in idx])

        return pred, _delta.per_alpha_pairs(self, alpha, alpha_name, method, std_of)

    def predict_cov(self, alpha, order=None, minus_log=None, alpha_name=None, method=None, bounded=False, block=None):
        """``(predict(alpha, ...), cov)``: for every alpha the two-state ``InterpModel`` that ``predict`` chooses
        (``method``, ``bounded`` as there) and ``InterpModel.predict_cov``'s contraction over that pair's two
        ``V_s = states[s].derivs_cross_cov(order)``; cov has dims ``(*alpha dims, *val_dims, *val_dims_2)``.  The
        covariances of ALL states are taken once, at collection level (one launch per kernel), and handed to the pairs;
        the pair models' caches hold no covariance.  Assumptions: first order; independent states; independent samples
        within a state unless ``block`` is given (an int, or one entry per state)."""
        self._check_alpha(alpha, bounded)
        if order is None:
            order = self.order
        covs, srcs, _ = self._state_cross_covs(order, minus_log, block)      # (first: an unsupported state says so)
        pred = self.predict(alpha, order=order, minus_log=minus_log, alpha_name=alpha_name, method=method, bounded=bounded)
        if alpha_name is None:
            alpha_name = self.alpha_name

        def cov_of(idx, a):
            pair = self.single_interpmodel(*idx)
            return pair._predict_cov_from(a, order, alpha_name, [covs[int(i)] for i in idx], srcs[0])

        return pred, _delta.per_alpha_pairs(self, alpha, alpha_name, method, cov_of)


def _std(var):
    """The standard deviation of a variance that rounding may have left slightly negative."""
    return np.sqrt(np.clip(var, 0.0, None))


def _along_alpha(value, error, name, avals):
    """(value, error) as two DataArrays along the alpha dim ``name``."""
    coords = {name: avals}
    return DataArray(value, (name,), coords=coords), DataArray(error, (name,), coords=coords)


class MBAROverlap(NamedTuple):
    """What ``MBARModel.overlap`` returns: the K x K overlap ``matrix``, its ``eigenvalues`` (descending) and the
    ``scalar`` 1 - the second largest eigenvalue."""

    matrix: np.ndarray
    eigenvalues: np.ndarray
    scalar: float


class MBARHistogram:
    """What ``MBARModel.histogram`` returns.  ``p`` and ``std`` (dims (alpha, "bin")): the reweighted probability of every
    bin and its asymptotic standard deviation; ``cov`` (dims (alpha, "bin", "bin_2"), or None): the covariance between the
    bins; ``outside`` (dims (alpha,)): the weight of the samples outside the range; ``edges`` (nbins + 1); ``n_eff``
    (dims (alpha,)): Kish's effective sample number 1 / sum_n W_na^2.  The "bin" coordinate holds the bin centres."""

    def __init__(self, p, std, cov, outside, edges, n_eff, avals, alpha_name):
        self.edges = np.asarray(edges, dtype=np.float64)
        self.alpha_name = alpha_name
        centres = 0.5 * (self.edges[:-1] + self.edges[1:])
        coords = {alpha_name: avals, "bin": centres}
        self.p = DataArray(p, (alpha_name, "bin"), coords=coords)
        self.std = DataArray(std, (alpha_name, "bin"), coords=coords)
        self.cov = None if cov is None else DataArray(cov, (alpha_name, "bin", "bin_2"), coords={**coords, "bin_2": centres})
        self.outside = DataArray(outside, (alpha_name,), coords={alpha_name: avals})
        self.n_eff = DataArray(n_eff, (alpha_name,), coords={alpha_name: avals})

    def density(self):
        """(p / width, std / width): the probability density of every bin and its standard deviation."""
        w = np.diff(self.edges)
        return self.p / w, self.std / w

    def free_energy(self, reference=None):
        """(F, dF), dims (alpha, "bin"): the free-energy profile F = -ln p and its first-order standard deviation.
        ``reference=None``: dF = std / p.  ``reference`` a bin index, or ``"max"`` (every target's most probable bin): F
        relative to that bin and dF^2 = v_b / p_b^2 + v_r / p_r^2 - 2 c_br / (p_b p_r) from ``cov`` (dF = 0 at the
        reference).  Empty bins give F = +inf and dF = nan."""
        p, std = np.asarray(self.p.values, dtype=np.float64), np.asarray(self.std.values, dtype=np.float64)
        na, nb = p.shape
        with np.errstate(divide="ignore", invalid="ignore"):
            F = -np.log(p)
            if reference is None:
                dF = np.where(p > 0, std / p, np.nan)
            else:
                if self.cov is None:
                    raise ValueError("free_energy(reference=...) needs the covariance between the bins: histogram(..., cov=True)")
                if isinstance(reference, str):
                    if reference != "max":
                        raise ValueError(f'reference = {reference!r}: a bin index or "max"')
                    r = np.argmax(p, axis=1)
                else:
                    r = np.full(na, range(nb)[int(reference)])
                rows = np.arange(na)
                c = np.asarray(self.cov.values, dtype=np.float64)
                v = np.einsum("abb->ab", c)
                pr, vr, cbr = p[rows, r][:, None], v[rows, r][:, None], c[rows, :, r]
                var = v / (p * p) + vr / (pr * pr) - 2.0 * cbr / (p * pr)
                dF = np.where((p > 0) & (pr > 0), _std(var), np.nan)
                dF[rows, r] = np.where(pr[:, 0] > 0, 0.0, np.nan)
                F = F - F[rows, r][:, None]
        return (DataArray(F, self.p.dims, coords=self.p.coords), DataArray(dF, self.p.dims, coords=self.p.coords))


class MBARModel(StateCollection):
    """MBAR over the pooled samples of every state (reference models.py:1049-1111, which hands u_kn = alpha0_k u_n to
    pymbar):  <x>(alpha) = sum_n x_n e^{-alpha u_n - logD_n} / sum_n e^{-alpha u_n - logD_n}  with
    logD_n = ln sum_k N_k e^{f_k - alpha0_k u_n} and the free energies f solved once per model (engine.mbar_solve: damped
    Newton, one device pass per step) and cached with the device buffer of logD.  States hold sample values
    (``DataValues`` / ``DataCentralMomentsVals``, any mix, any sample counts); their weights are not used, as in the
    reference, which reads only ``uv`` and ``xv``."""

    def __init__(self, states, kws=None):
        super().__init__(states, kws)
        self._samples_host()

    def _samples_host(self):
        """[(uv, xv, rec_dim)] per state, checked: sample values, not resampled, a DataArray observable, one shape."""
        from .data import DataCentralMomentsVals, DataValuesBase

        out = []
        for i, m in enumerate(self.states):
            d = getattr(m, "data", None)
            if isinstance(d, DataValuesBase):
                if d._resampled is not None:
                    raise NotImplementedError(f"state {i}: MBARModel of resampled data")
                uv, xv = d._uv, d._xv
            elif isinstance(d, DataCentralMomentsVals):
                if d.ds_layout is not None or is_dataset(d.xv):
                    raise NotImplementedError(f"state {i}: MBARModel of xr.Dataset observables")
                if d.rec_dim not in d.uv.dims:
                    raise NotImplementedError(f"state {i}: MBARModel of resampled data")
                uv, xv = d.uv, d.xv
            else:
                raise TypeError(f"state {i}: MBARModel needs the sample values of every state (DataValues or "
                                f"DataCentralMomentsVals), got {type(d).__name__}")
            rec = d.rec_dim
            if tuple(uv.dims) != (rec,):
                raise NotImplementedError(f"state {i}: uv must be 1-D along the record dim {rec!r}, got {tuple(uv.dims)}")
            out.append((uv, xv, rec))
        shapes = [tuple((dm, n) for dm, n in zip(xv.dims, xv.shape) if dm != rec) for _, xv, rec in out]
        for i, sh in enumerate(shapes):
            if sh != shapes[0]:
                raise ValueError(f"the states' xv differ beyond the record dim: state 0 {shapes[0]}, state {i} {sh}")
        return out

    def _samples(self):
        """Device tensors (u per state, x per state as (n, C)), the output dims after alpha and their shape."""
        if "samples" not in self._cache:
            from .moments import _dev_and_dims

            us, xs = [], []
            for uv, xv, rec in self._samples_host():
                ut, _ = _dev_and_dims(uv)
                xt, xdims = _dev_and_dims(xv)
                x2 = xt.movedim(xdims.index(rec), 0)
                us.append(ut)
                xs.append(x2.reshape(x2.shape[0], -1))
            _, xv, rec = self._samples_host()[0]
            others = [dm for dm in xv.dims if dm != rec]
            cshape = [n for dm, n in zip(xv.dims, xv.shape) if dm != rec]
            self._cache["samples"] = (us, xs, others, cshape)
        return self._cache["samples"]

    def _solution(self) -> "engine.MbarSolution":
        if "mbar" not in self._cache:
            us, _, _, _ = self._samples()
            self._cache["mbar"] = engine.mbar_solve(us, self.alpha0)
        return self._cache["mbar"]

    def predict(self, alpha, alpha_name=None):
        """<x> at every alpha: dims (alpha_name, *the non-record dims of xv); a scalar alpha keeps a length-1 alpha dim
        (the reference's expand_dims, models.py:1085-1086)."""
        avals, alpha_name = self._alpha_values(alpha, alpha_name)
        _, _, others, cshape = self._samples()
        vals = self._means(avals)[1].cpu().numpy().reshape(len(avals), *cshape)
        return DataArray(vals, (alpha_name, *others), coords={alpha_name: avals})

    def _means(self, avals, first_column=False):
        """(xs, means): ``engine.mbar_predict`` at the cached solution, on the device, and the observables it averaged;
        ``first_column``: the first observable column only (the free energies need no x)."""
        us, xs, _, _ = self._samples()
        sol = self._solution()
        if first_column:
            xs = [x[:, :1] for x in xs]
        return xs, engine.mbar_predict(xs, us, self.alpha0, sol.f, sol.logD, avals, upiv=sol.upiv)

    # ---- the estimator's asymptotic covariance (Shirts & Chodera 2008, eq. 8 and appendix D) --------------------------
    # It assumes independent samples: decorrelate first (timeseries.statistical_inefficiencies).
    def _counts(self) -> np.ndarray:
        us, _, _, _ = self._samples()
        return np.array([u.shape[0] for u in us], dtype=np.float64)

    def _gram(self) -> np.ndarray:
        """G_jk = sum_n W_nj W_nk of the sampled states: one evaluation pass at the solution, cached."""
        if "mbar_gram" not in self._cache:
            us, _, _, _ = self._samples()
            self._cache["mbar_gram"] = engine.mbar_gram(us, self.alpha0, self._solution())
        return self._cache["mbar_gram"]

    def _reduced_pinv(self) -> np.ndarray:
        if "mbar_pinv" not in self._cache:
            self._cache["mbar_pinv"] = engine.mbar_reduced_pinv(self._gram(), self._counts())
        return self._cache["mbar_pinv"]

    def _alpha_values(self, alpha, alpha_name):
        """(values, name) of the targets: a float 1-D array (a scalar alpha becomes length 1) and the alpha dim."""
        if alpha_name is None:
            alpha_name = self.alpha_name
        alpha = xrwrap_alpha(alpha, name=alpha_name)
        avals = np.atleast_1d(np.asarray(alpha.values, dtype=float))
        if avals.ndim != 1:
            raise ValueError("alpha must be a scalar or 1-D")
        return avals, alpha_name

    def derivs_cov(self, order=None, norm=False, minus_log=None, block=None):
        raise NotImplementedError("derivs_cov (delta-method error bars of the states' derivatives): MBARModel predicts "
                                  "from the pooled samples, not from derivatives; its error bars are predict_with_error")

    def derivs_cross_cov(self, order=None, norm=False, minus_log=None, block=None):
        raise NotImplementedError("derivs_cross_cov (delta-method covariance of the states' derivatives across columns): "
                                  "MBARModel predicts from the pooled samples, not from derivatives; its error bars are "
                                  "predict_with_error")

    def predict_cov(self, alpha, alpha_name=None, **kws):
        raise NotImplementedError("predict_cov (delta-method covariance of the states' derivatives across columns): "
                                  "MBARModel predicts from the pooled samples, not from derivatives; its error bars are "
                                  "predict_with_error")

    # ---- blocked (batch-means) error bars for CORRELATED series kept whole ------------------------------
    # Every influence of an MBAR estimate is linear in the row t_n of txm_mbar_block_cov; its block sums are centred per
    # state (one stationary series per state, independent states) and var = l^T Gamma l.  First order; B beyond the
    # correlation time (timeseries.block_lengths proposes one per state, blocking_curve shows whether the variance has
    # levelled off); no nb / (nb - 1) factor; a state with a single block contributes exactly zero.  block=1 is the
    # per-state-centred sandwich estimator: it agrees with the Theta form asymptotically, not to rounding.
    def _block_gamma(self, avals, block, n_levels=1, first_column=False):
        """(means on the device, engine.MbarBlockGamma, C) of the targets; ``first_column``: the first observable column
        only (the free energies need no x)."""
        us, xs, _, _ = self._samples()
        C = 1 if first_column else int(xs[0].shape[1])
        if C > engine.MBAR_CROSS_MAX_COLUMNS:
            raise ValueError(f"the blocked MBAR error bars (block=...) take at most 255 observable columns, got {C}")
        xs, means = self._means(avals, first_column)
        return means, engine.mbar_block_gamma(xs, us, self.alpha0, self._solution(), avals, means, block, n_levels=n_levels), C

    def _block_mean_variance(self, res, C):
        """(n_levels, n_alpha, C): l^T Gamma l of every average, slab by slab."""
        Gs, N, pinv = self._gram(), self._counts(), self._reduced_pinv()
        out = []
        for gam, b, _ in res.slabs():
            L = engine.mbar_block_coef_mean(Gs, N, b, pinv=pinv)
            out.append(engine.mbar_block_variance(gam, L).reshape(gam.shape[0], -1, C))
        return np.concatenate(out, axis=1)

    def predict_with_error(self, alpha, alpha_name=None, block=None):
        """(mean, err): ``predict(alpha)`` bit for bit and its asymptotic standard deviation (pymbar's ``dA`` of
        compute_expectations), both with ``predict``'s dims.  One more pass over the samples per 8 targets; no re-solve.

        ``block=None`` assumes INDEPENDENT samples (Shirts & Chodera's Theta).  ``block=B`` (an int, or one int per state
        as ``timeseries.block_lengths`` returns them) is for CORRELATED series kept whole: every state is cut into
        contiguous blocks of B records (a last short one is kept, blocks never straddle two states), the first-order
        influences are summed per block, centred per state, and ``err^2 = sum_b (centred block sum)^2`` -- batch means,
        B beyond the correlation time (``blocking_curve`` shows whether the variance has levelled off).  Assumptions:
        first order, one stationary series per state, independent states, no nb / (nb - 1) factor; a state with a
        single block contributes exactly zero.  ``block=1`` is the per-state-centred sandwich estimator: equal to the
        Theta form asymptotically, not to rounding.  At most 255 observable columns with ``block``."""
        avals, alpha_name = self._alpha_values(alpha, alpha_name)
        us, xs, others, cshape = self._samples()
        sol = self._solution()
        if block is None:
            _, means = self._means(avals)
            _, _, yy, b = engine.mbar_cov_sums(xs, us, self.alpha0, sol, avals, means)
            var = engine.mbar_mean_variance(self._gram(), self._counts(), yy, b, pinv=self._reduced_pinv())
        else:
            means, res, C = self._block_gamma(avals, block)
            var = self._block_mean_variance(res, C)[0]
        dims, coords = (alpha_name, *others), {alpha_name: avals}
        mean = DataArray(means.cpu().numpy().reshape(len(avals), *cshape), dims, coords=coords)
        err = DataArray(_std(var).reshape(len(avals), *cshape), dims, coords=coords)
        return mean, err

    def blocking_curve(self, alpha, block, alpha_name=None):
        """The blocking curve of ``predict_with_error(alpha, block=...)``: ``(var, block_lengths, n_blocks)`` with
        ``var[l] = predict_with_error(alpha, block=block * 2**l)[1] ** 2`` (dims ``(level, alpha, *val_dims)``),
        ``block_lengths[l][s] = block[s] * 2**l`` and ``n_blocks[l][s]`` the blocks of state s at level l, for every
        level at which some state still has at least two blocks.  ONE block pass per 8 targets: block sums are additive,
        so each level merges the pairs of the level below within every state.  Where var stops growing the blocks are
        longer than the correlation time; a state that is down to one block contributes zero from that level on, and the
        last levels are noisy (relative standard deviation about ``sqrt(2 / (sum_s n_blocks - K))``)."""
        avals, alpha_name = self._alpha_values(alpha, alpha_name)
        us, _, others, cshape = self._samples()
        ns = [int(u.shape[0]) for u in us]
        blk = engine.mbar_block_lengths(block, ns)
        factors, _ = engine.mbar_block_levels(ns, blk)
        _, res, C = self._block_gamma(avals, blk, n_levels=len(factors))
        var = self._block_mean_variance(res, C)
        out = DataArray(var.reshape(len(factors), len(avals), *cshape), ("level", alpha_name, *others),
                        coords={"level": factors.copy(), alpha_name: avals})
        return out, factors[:, None] * np.minimum(blk, np.asarray(ns, dtype=np.int64))[None, :], res.nblocks

    def predict_with_covariance(self, alpha, alpha_name=None, cross_alpha=False, block=None):
        """(mean, cov): ``predict(alpha)`` bit for bit and the asymptotic covariance of the averages across the
        observable columns -- what the error bar of a sum, an integral over bins or a ratio of columns needs.  ``cov`` has
        dims (alpha, *val_dims, *[d + "_2" for d in val_dims]); its diagonal is ``predict_with_error``'s err squared.
        With ``cross_alpha=True`` the covariance also runs across the targets (at most 8): dims (alpha, *val_dims,
        alpha + "_2", *[d + "_2" ...]), which the error bar of a difference between two targets needs.  At most 255
        columns.  The assumptions are ``predict_with_error``'s: independent samples (``timeseries.decorrelate`` first),
        first order in the fluctuations.  Two more passes over the samples per 8 targets; no re-solve.

        ``block=B`` (an int or one int per state): the blocked form for correlated series kept whole, with the
        assumptions of ``predict_with_error(block=...)``; the Gram matrix of the block sums carries all targets of a
        call, so both forms of ``cross_alpha`` come from the same pass."""
        from types import SimpleNamespace

        avals, alpha_name = self._alpha_values(alpha, alpha_name)
        us, xs, others, cshape = self._samples()
        C = int(np.prod(cshape, dtype=np.int64))
        if C > engine.MBAR_CROSS_MAX_COLUMNS:
            raise ValueError(f"predict_with_covariance takes at most 255 observable columns, got {C}")
        if cross_alpha and len(avals) > engine.MBAR_CROSS_MAX_TARGETS:
            raise ValueError(f"predict_with_covariance(cross_alpha=True) takes at most {engine.MBAR_CROSS_MAX_TARGETS} targets, "
                             f"got {len(avals)}")
        sol = self._solution()
        na = len(avals)
        if block is not None:
            means, res, _ = self._block_gamma(avals, block)
            Gs, N, pinv = self._gram(), self._counts(), self._reduced_pinv()
            covs = []
            for gam, b, _ in res.slabs():
                L = engine.mbar_block_coef_mean(Gs, N, b, pinv=pinv)
                if cross_alpha:
                    covs.append(engine.mbar_block_covariance(gam[0], L))
                else:
                    covs += [engine.mbar_block_covariance(gam[0], L[a * C:(a + 1) * C]) for a in range(L.shape[0] // C)]
            cov = covs[0] if cross_alpha else np.stack(covs)
        else:
            _, means = self._means(avals)
            gram, b = engine.mbar_cross_cov_sums(xs, us, self.alpha0, sol, avals, means, cross_alpha=cross_alpha)
            if cross_alpha:
                gram, b = gram.reshape(na * C, na * C), b.reshape(na * C, -1)
            cov = engine.mbar_mean_covariance(self._gram(), self._counts(), gram, b, pinv=self._reduced_pinv())
        dims, coords = (alpha_name, *others), {alpha_name: avals}
        mean = DataArray(means.cpu().numpy().reshape(na, *cshape), dims, coords=coords)
        xv = self._samples_host()[0][1]
        src = SimpleNamespace(out_dims=list(others), out_shape=list(cshape), coords=dict(getattr(xv, "_coords", {})))
        al = DataArray(avals, (alpha_name,), coords=coords)
        if not cross_alpha:
            return mean, _delta.label_cov(cov, al, src)
        out = DataArray(cov.reshape(na, *cshape, na, *cshape),
                        (alpha_name, *others, alpha_name + "_2", *[d + "_2" for d in others]),
                        coords={alpha_name: avals, alpha_name + "_2": avals})
        return mean, _delta.cross_labels(out, src)

    def _histogram_values(self, values):
        """One 1-D CUDA tensor per state for ``histogram``'s ``values``, and whether they are integers."""
        us, xs, _, cshape = self._samples()
        if isinstance(values, str):
            if values != "u":
                raise ValueError(f'values = {values!r}: the only name is "u", the energy')
            return list(us), False
        if isinstance(values, (int, np.integer, tuple)):
            C = int(np.prod(cshape, dtype=np.int64))
            col = int(np.ravel_multi_index(tuple(int(i) for i in values), cshape)) if isinstance(values, tuple) else int(values)
            if not 0 <= col < C:
                raise IndexError(f"values = {values!r}: the observable has {C} columns")
            return [x[:, col].contiguous() for x in xs], False
        if len(values) != len(us):
            raise ValueError(f"values: need one 1-D array per state ({len(us)}), got {len(values)}")
        out, integral = [], True
        for s, v in enumerate(values):
            t = v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(getattr(v, "values", v)))
            if t.dim() != 1 or t.shape[0] != us[s].shape[0]:
                raise ValueError(f"values of state {s} must be ({us[s].shape[0]},), got {tuple(t.shape)}")
            integral = integral and not (t.is_floating_point() or t.is_complex() or t.dtype == torch.bool)
            out.append(t.to(us[s].device))
        return out, integral

    def histogram(self, alpha, bins, *, values=0, range=None, alpha_name=None, cov=True) -> "MBARHistogram":
        """The reweighted distribution of an order parameter at every target alpha, p_b(alpha) = sum_n W_na 1_b(n), with
        its asymptotic error bars and -- ``cov=True`` -- the covariance between the bins that a free-energy profile
        relative to a reference bin needs.  Nothing of size samples x bins is formed: one pass over the samples per 8
        targets gives every sum the covariance takes (engine.mbar_hist_sums); no re-solve.

        ``values``: ``"u"`` (the energy), an int or a tuple indexing the non-record dims of ``xv`` (that column), or a
        list of one 1-D array per state (any order parameter).  ``bins``: an int -- with ``range=(lo, hi)``, by default
        the pooled minimum and maximum, as ``numpy.histogram`` -- or a 1-D array of increasing edges; bins are closed on
        the left, the last one also on the right.  For 2-D or custom bins pass ``values`` as integer arrays with
        ``bins=int`` and ``range=None``: the values are then the bin indices themselves.  Samples outside the range
        count in the normalisation (``outside`` holds their weight).  At most 1023 bins.

        The assumptions are ``predict_with_error``'s: independent samples (``timeseries.decorrelate`` first), first order
        in the fluctuations.  Returns an ``MBARHistogram``."""
        avals, alpha_name = self._alpha_values(alpha, alpha_name)
        us, _, _, _ = self._samples()
        vals, integral = self._histogram_values(values)
        if np.ndim(bins) == 0:
            nb = int(bins)
            if nb < 1:
                raise ValueError(f"bins = {bins}: need at least one bin")
            if integral and range is None:
                edges = None                                       # the values are the bin indices
            else:
                if range is None:
                    lo, hi = min(float(v.min()) for v in vals), max(float(v.max()) for v in vals)
                else:
                    lo, hi = (float(r) for r in range)
                if not (np.isfinite(lo) and np.isfinite(hi)) or lo > hi:
                    raise ValueError(f"range = ({lo}, {hi}) is not a finite interval")
                edges = np.histogram_bin_edges(np.empty(0), bins=nb, range=(lo, hi))
        else:
            edges = np.asarray(bins, dtype=np.float64)
            if edges.ndim != 1 or len(edges) < 2 or not np.all(np.diff(edges) > 0):
                raise ValueError("bins must be an int or a 1-D array of increasing edges")
            nb = len(edges) - 1
        if nb > engine.HIST_MAX_BINS:
            raise ValueError(f"histogram takes at most {engine.HIST_MAX_BINS} bins, got {nb}")
        if edges is None:
            idx = [v.to(torch.int64).clamp(-1, nb).to(torch.int32) for v in vals]
            edges = np.arange(nb + 1, dtype=np.float64)
        else:
            idx = [engine.bin_index(v, edges) for v in vals]
        sol = self._solution()
        H, S, T, Q, _, _ = engine.mbar_hist_sums(idx, us, self.alpha0, sol, avals, nb)
        Gs, N, pinv = self._gram(), self._counts(), self._reduced_pinv()
        var = engine.mbar_hist_variance(Gs, N, H, S, T, pinv=pinv)
        covar = engine.mbar_hist_covariance(Gs, N, H, S, T, pinv=pinv) if cov else None
        return MBARHistogram(H[:, :nb].copy(), _std(var), covar, H[:, nb].copy(), edges, 1.0 / Q,
                             avals, alpha_name)

    def _target_sums(self, avals):
        """(Q, B, ln sum_n w_an) of the targets: the covariance pass over the first observable column only."""
        us, _, _, _ = self._samples()
        x1, means = self._means(avals, first_column=True)
        Q, B, _, _, lnw = engine.mbar_cov_sums(x1, us, self.alpha0, self._solution(), avals, means, with_lnw=True)
        return Q, B, lnw

    def _block_sampled_covariance(self, block) -> np.ndarray:
        """The blocked covariance of the sampled states' f_i - f_0, (K, K): one block pass at the target alpha0[0] over the
        first observable column (only the K sampled columns of Gamma are used)."""
        _, res, _ = self._block_gamma(np.asarray(self.alpha0, dtype=float)[:1], block, first_column=True)
        gam = res.gamma[0][0]
        L = engine.mbar_block_coef_sampled(self._gram(), self._counts(), gam.shape[0], pinv=self._reduced_pinv())
        return engine.mbar_block_covariance(gam, L)

    def free_energy_covariance(self, block=None) -> np.ndarray:
        """The K x K matrix Theta of the sampled states: var(f_i - f_j) = Theta_ii + Theta_jj - 2 Theta_ij.  With
        ``block=B`` (``predict_with_error``'s, for correlated series kept whole) the blocked covariance of f_i - f_0 and
        f_j - f_0, for which the same identity holds; its row and column 0 are zero."""
        if block is not None:
            return self._block_sampled_covariance(block)
        if "mbar_theta" not in self._cache:
            self._cache["mbar_theta"] = engine.mbar_theta(self._gram(), self._counts())
        return self._cache["mbar_theta"].copy()

    def free_energy(self, alpha=None, alpha_name=None, block=None):
        """(f, df) relative to state 0 (pymbar's compute_free_energy_differences, row 0): of the sampled states
        (``alpha=None``: the cached solution, df[0] = 0), or of the targets ``alpha``, f(a) = -ln sum_n e^{-a u_n - logD_n}.
        ``block=B``: df by batch means for correlated series kept whole (``predict_with_error``'s ``block``)."""
        if alpha is None:
            name = self.alpha_name if alpha_name is None else alpha_name
            if block is None:
                th = self.free_energy_covariance()
                var = np.diag(th) + th[0, 0] - 2.0 * th[0]
            else:
                var = np.diag(self._block_sampled_covariance(block)).copy()
            var[0] = 0.0
            return _along_alpha(np.array(self._solution().f, dtype=float), _std(var), name, np.asarray(self.alpha0, dtype=float))
        avals, alpha_name = self._alpha_values(alpha, alpha_name)
        if block is not None:
            _, res, C = self._block_gamma(avals, block, first_column=True)
            Gs, N, pinv = self._gram(), self._counts(), self._reduced_pinv()
            var = np.concatenate([engine.mbar_block_variance(gam[0], engine.mbar_block_coef_target(Gs, N, B, C, pinv=pinv))
                                  for gam, _, B in res.slabs()])
            return _along_alpha(-res.lnw - float(self._solution().f[0]), _std(var), alpha_name, avals)
        Q, B, lnw = self._target_sums(avals)
        K, N, Gs = len(self.states), self._counts(), self._gram()
        G = np.zeros((K + 1, K + 1))
        G[:K, :K] = Gs
        var = np.empty(len(avals))
        for i in range(len(avals)):
            G[:K, K] = G[K, :K] = B[i]
            G[K, K] = Q[i]
            th = engine.mbar_theta(G, np.append(N, 0.0))
            var[i] = th[K, K] + th[0, 0] - 2.0 * th[0, K]
        return _along_alpha(-lnw - float(self._solution().f[0]), _std(var), alpha_name, avals)

    def overlap(self) -> "MBAROverlap":
        """The overlap matrix O = G diag(N_k) of the sampled states (rows sum to 1; O_jk: the share of state k's samples
        in what state j sees), its eigenvalues in descending order and the scalar 1 - the second largest (pymbar's
        compute_overlap): near 0 when the states fall into groups that share no samples.  K = 1 gives the scalar 1."""
        return MBAROverlap(*engine.mbar_overlap(self._gram(), self._counts()))

    def effective_samples(self, alpha, alpha_name=None):
        """Kish's effective sample number of the pooled samples at every target: 1 / sum_n W_na^2."""
        avals, alpha_name = self._alpha_values(alpha, alpha_name)
        Q, _, _ = self._target_sums(avals)
        return DataArray(1.0 / Q, (alpha_name,), coords={alpha_name: avals})

    def resample(self, *args, **kwargs):
        raise NotImplementedError("resample not implemented for this class (MBARModel.bootstrap gives the replicates)")

    def bootstrap(self, sampler, rep_dim="rep"):
        """Bootstrap replicates of this model (the capability the reference's ``resample`` lacks, models.py:1109-1111):
        every replicate redraws N_s of the N_s samples of each state s and solves MBAR again.  ``sampler``: a mapping
        with ``"nrep"`` and ``"seed"`` or ``"rng"`` (a seed is drawn from it), optional ``"rep0"`` and ``"rep_dim"``;
        state s draws the stream replicates rep0 + s * nrep + r of the device sampler of that seed -- the draws
        ``StateCollection.resample`` makes for the same mapping.  Returns an ``MBARBootstrap``."""
        accepted = 'a mapping {"nrep": n, "seed": s} or {"nrep": n, "rng": rng} (optional "rep0", "rep_dim", "device": True)'
        if not isinstance(sampler, Mapping):
            raise NotImplementedError(f"MBARModel.bootstrap takes {accepted}, got {type(sampler).__name__}")
        if "indices" in sampler or "freq" in sampler:
            raise NotImplementedError(f"MBARModel.bootstrap takes {accepted}: explicit indices / freq tables are not supported")
        if "nrep" not in sampler:
            raise NotImplementedError(f"MBARModel.bootstrap takes {accepted}")
        if sampler.get("device") is not None and not sampler.get("device"):
            raise ValueError('MBARModel.bootstrap draws from the device sampler stream: "device": False (numpy index '
                             "draws have no replicate index) is not possible")
        nrep = int(sampler["nrep"])
        if nrep < 1:
            raise ValueError(f"nrep = {nrep}: need at least one replicate")
        seed = sampler.get("seed")
        if seed is None:
            from . import moments as cm

            seed = int(cm.validate_rng(sampler.get("rng")).integers(0, 2**63 - 1))
        rep0 = int(sampler.get("rep0", 0))
        us, _, _, _ = self._samples()
        samplers = [engine.DeviceSampler(int(seed), nrep, int(u.shape[0]), rep0=rep0 + s * nrep) for s, u in enumerate(us)]
        return MBARBootstrap(self, samplers, sampler.get("rep_dim") or rep_dim)


class MBARBootstrap:
    """The bootstrap replicates of an ``MBARModel`` (``MBARModel.bootstrap``): ``parent`` the model, ``nrep``, the
    per-state ``samplers`` and -- solved once, from the parent's point solution, and cached -- the replicates' free
    energies ``f`` (nrep, K), gauge f[:, 0] = 0."""

    def __init__(self, parent, samplers, rep_dim="rep"):
        self.parent = parent
        self.samplers = list(samplers)
        self.rep_dim = rep_dim
        self.nrep = int(self.samplers[0].nrep)
        self._f = None

    @property
    def f(self) -> np.ndarray:
        if self._f is None:
            us, _, _, _ = self.parent._samples()
            self._f = engine.mbar_bootstrap_solve(us, self.parent.alpha0, self.samplers, self.parent._solution())
        return self._f

    def predict(self, alpha, alpha_name=None):
        """<x> of every replicate at every alpha: dims (alpha_name, rep_dim, *the non-record dims of xv) --
        PerturbModel's resampled layout; a scalar alpha keeps a length-1 alpha dim, as ``MBARModel.predict``."""
        p = self.parent
        avals, alpha_name = p._alpha_values(alpha, alpha_name)
        us, xs, others, cshape = p._samples()
        out = engine.mbar_bootstrap_predict(xs, us, p.alpha0, self.samplers, self.f, p._solution(), avals)
        vals = np.moveaxis(out.cpu().numpy(), 0, 1).reshape(len(avals), self.nrep, *cshape)
        return DataArray(vals, (alpha_name, self.rep_dim, *others), coords={alpha_name: avals})
