"""The model side of the delta-method error bars: what ``derivs_cov`` / ``derivs_cross_cov``, their
``block=`` forms and ``predict_with_error`` / ``predict_cov`` of the four model classes share on the host -- the cached
device tables of one state, the batched tables of a collection, the contractions with the Taylor, Minkowski and Hermite
vectors, and the labelling of the results.  models.py keeps the public methods and their docstrings.

Every contraction keeps the ``np.einsum`` subscripts, the operand order and the order of the scalar operations around it
that the results were first recorded with (tests/golden/delta_parent.npz): the einsum subscripts are arguments, the
per-column forms pass ``"...cij..."``, the cross-column forms ``"...cidj..."``.
"""

from __future__ import annotations

import math

import numpy as np
import torch

from . import engine
from .xrlite import DataArray, concat


def check_block_type(block) -> int:
    """A block length of the blocked error bars as a Python int; TypeError for anything that is not an integer (its
    range depends on the number of records: ``engine.block_levels`` raises the ValueError)."""
    if isinstance(block, bool) or not isinstance(block, (int, np.integer)):
        raise TypeError(f"block must be an integer number of records, got {type(block).__name__}")
    return int(block)


# ---- device tables ----------------------------------------------------------------------------------------------------------
def extrap_table(model, order, minus_log, cross, block=None, curve=False):
    """The cached delta-method table of one ``ExtrapModel`` from ONE engine call: per column (``cross=False``,
    [n_out, order + 1, order + 1]) or across the columns (``cross=True``, [n_out, order + 1, n_out, order + 1], at most
    ``engine.CROSS_COV_MAX_COLUMNS`` columns).  ``block=None``: ``(cov, source)`` under ``("dcov" | "dxcov", order,
    minus_log)``.  With a block: ``(cov, source, block_lengths, n_blocks)`` under ``("dcov_block" | "dxcov_block", order,
    minus_log, block, curve)``, cov at ``block`` alone or, with ``curve``, with a leading axis over every level of
    ``engine.block_levels``.  An entry is neither read nor written by another form."""
    name = "dxcov" if cross else "dcov"
    if block is None:
        key = (name, order, minus_log)
    else:
        block = check_block_type(block)
        key = (name + "_block", order, minus_log, block, bool(curve))
    if key not in model._cache:
        x2, ut, wt, st, src = model._delta_operands()   # (first: an unsupported model says so, whatever its width or block)
        if cross and x2.shape[1] > engine.CROSS_COV_MAX_COLUMNS:
            raise ValueError(f"derivs_cross_cov / predict_cov: {x2.shape[1]} observable columns, the limit is "
                             f"{engine.CROSS_COV_MAX_COLUMNS} (the result has (columns * (order + 1))^2 entries)")
        if block is not None:
            lengths, counts = engine.block_levels(x2.shape[0], block)
        a, b, um, xm = model._delta_coefs(st, order, minus_log)
        args = (x2, ut, engine.to_device(a), engine.to_device(b), um, engine.to_device(xm))
        if block is None:
            cov = engine.influence_cross_cov(*args, w=wt) if cross else engine.influence_cov(*args, w=wt)[0]
            model._cache[key] = (cov, src)
        else:
            blocked = engine.influence_block_cross_cov if cross else engine.influence_block_cov
            cov, _ = blocked(*args, block, n_levels=len(lengths) if curve else 1, w=wt)
            model._cache[key] = (cov if curve else cov[0], src, lengths, counts)
    return model._cache[key]


def states_tables(states, order, minus_log, cross):
    """``(cov [S, ...] on the device, sources)`` of ``states`` from ONE copy of their stacked central states to the host,
    the coefficient algebra there and ONE ``engine.influence_cov_batched`` / ``influence_cross_cov_batched``.

    The host algebra runs state by state although symbolic.influence_coefs broadcasts: the single path hands it ``<u>``
    as a Python float, and ``float ** int`` need not round like ``ndarray ** int`` (it matters in the raw form, which
    expands about zero), so only the per-state call is certain to give the single call's coefficients."""
    ops = [st._delta_operands(device_state=True) for st in states]             # raises what a state raises
    host = torch.stack([op[3] for op in ops]).cpu().numpy()                    # [S, C, 2, K]: one copy
    co = [st._delta_coefs(host[s], order, minus_log) for s, st in enumerate(states)]
    batched = engine.influence_cross_cov_batched if cross else engine.influence_cov_batched
    out = batched([op[0] for op in ops], [op[1] for op in ops],
                  engine.to_device(np.stack([c[0] for c in co])), engine.to_device(np.stack([c[1] for c in co])),
                  np.array([c[2] for c in co]), engine.to_device(np.stack([c[3] for c in co])),
                  ws=None if ops[0][2] is None else [op[2] for op in ops])
    return (out if cross else out[0]), [op[4] for op in ops]


# ---- Taylor vectors ---------------------------------------------------------------------------------------------------------
def taylor_norm(order):
    """The ``1 / k!`` factors of ``norm=True``, k = 0 .. order."""
    return np.array([1.0 / math.factorial(i) for i in range(order + 1)])


def taylor_vectors(dalpha, order):
    """``t[a, k] = dalpha_a^k / k!``, (n_alpha, order + 1), over the flattened values of ``dalpha``."""
    d = np.asarray(dalpha.values, dtype=np.float64).reshape(-1)
    return np.stack([d**k / math.factorial(k) for k in range(order + 1)], axis=1)


# ---- labels -----------------------------------------------------------------------------------------------------------------
def cross_labels(out, src):
    """The coordinates of the value dims on ``out``, and their copies under the ``_2`` names."""
    out._inherit(src.coords)
    out._inherit({k + "_2": (tuple(d + "_2" for d in cd), cv) for k, (cd, cv) in src.coords.items()})
    return out


def label_std(var, al, src):
    """``sqrt(max(var, 0))`` [n_alpha, n_out] with the dims and coordinates of alpha ``al`` and of the values."""
    std = DataArray(np.sqrt(np.maximum(var, 0.0)).reshape((*al.shape, *src.out_shape)), (*al.dims, *src.out_dims))
    std._inherit(al._coords)
    std._inherit(src.coords)
    return std


def label_cov(pc, al, src):
    """A covariance [n_alpha, n_out, n_out] with dims ``(*alpha dims, *val_dims, *[d + "_2" for d in val_dims])``."""
    out = DataArray(pc.reshape((*al.shape, *src.out_shape, *src.out_shape)),
                    (*al.dims, *src.out_dims, *[d + "_2" for d in src.out_dims]))
    out._inherit(al._coords)
    return cross_labels(out, src)


def blocking_levels(table, label):
    """``(V, block_lengths, n_blocks)`` of a blocking curve from a ``curve=True`` entry of ``extrap_table``: every level's
    host table labelled by ``label(host, source)`` and joined along ``level``."""
    cov, src, lengths, counts = table
    host = cov.cpu().numpy()
    out = concat([label(host[l], src) for l in range(host.shape[0])], dim=DataArray(lengths.copy(), "level"))
    return out, lengths.copy(), counts.copy()


# ---- contractions of the multi-state models ---------------------------------------------------------------------------------
def minkowski_contract(model, al, order, method, covs, subscripts):
    """Per alpha of ``al``: ``sum_i (w_i / sum w)^2 t_i' V_i t_i`` over the two states ``ExtrapWeightedModel.predict`` picks,
    ``t_ik = (alpha - alpha0_i)^k / k!``, ``V_i = covs[i]`` contracted by ``subscripts``; stacked along alpha."""
    a0 = np.asarray(model.alpha0, dtype=np.float64)
    fact = np.array([math.factorial(k) for k in range(order + 1)], dtype=np.float64)
    out = []
    for a in np.asarray(al.values, dtype=np.float64).reshape(-1):
        idx = [0, 1] if len(model) == 2 else model._indices_alpha(float(a), method)
        dm = np.abs(a - a0[idx]) ** 20                                        # xr_weights_minkowski, m = 20
        w = 1.0 - dm / dm.sum()
        wn = w / w.sum()
        v = 0.0
        for wi, i in zip(wn, idx):
            t = (a - a0[i]) ** np.arange(order + 1) / fact
            v = v + wi * wi * np.einsum(subscripts, t, covs[i], t)
        out.append(v)
    return np.array(out)


def hermite_contract(inv, al, order, covs, subscripts):
    """``sum_s g_s' V_s g_s`` per alpha of ``al`` with ``g = (alpha^p) . inv`` (``InterpModel._hermite_inverse``,
    [porder, state * (order + 1)]) and ``V_s = covs[s]`` contracted by ``subscripts``."""
    av = np.asarray(al.values, dtype=np.float64).reshape(-1)
    g = (av[:, None] ** np.arange(inv.shape[0])[None, :]) @ inv     # (n_alpha, S (order + 1))
    g = g.reshape(len(av), len(covs), order + 1)
    return sum(np.einsum(subscripts, g[:, s], covs[s], g[:, s]) for s in range(len(covs)))


def per_alpha_pairs(model, alpha, alpha_name, method, one):
    """``one(idx, alpha)`` on the pair of states ``InterpModelPiecewise.predict`` chooses for each alpha, joined along
    ``alpha_name`` as ``predict`` joins its pieces."""
    from .models import _alpha_seq

    if len(model) == 2:
        return one((0, 1), alpha)
    seq = [float(a) for a in _alpha_seq(alpha)]
    outs = [one(model._indices_alpha(a, method), a) for a in seq]
    if len(outs) == 1:
        return outs[0]
    return concat(outs, dim=DataArray(np.asarray(seq), alpha_name))
