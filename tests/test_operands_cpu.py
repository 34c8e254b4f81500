"""The operand layout rules (thermoextrap_amd/_operands.py) and the slab bisection (engine._most_that_fit), pinned
without a GPU against frozen transcriptions of the conditionals they replaced.

Every engine entry point that takes an (N, C) sample matrix used to carry its own copy of "pass it as it is, with which
pitch, or copy it first".  The transcriptions below are those copies as they stood (the eight sites of engine.py before
the rules moved), as functions of (N, C, s0, s1); ``x.contiguous()`` is modelled as "the strides become (C, 1)".  Where
torch's contiguous() is a no-op although a site asked for it (an (N, 1) tensor with any stride(1) counts as contiguous)
the pitch a site derived afterwards is C = 1 all the same, so the model gives what the site passed; the tensor group at
the end checks that case on a real tensor."""

import itertools

import pytest
import torch

from thermoextrap_amd import _operands, engine
from thermoextrap_amd._operands import either_layout, resample_pitch_ok, rowmajor_layout


# ---------------------------------------------------------------------------
# the sites as they stood: (copy, ls) or (copy, ls, lc)
# ---------------------------------------------------------------------------
def _pitch_ok_then(ld, C):
    return 768 * int(ld) + int(C) <= 1 << 29


def site_reduce_vals(N, C, s0, s1):
    if C == 1:
        return True, 1, 1
    elif s1 == 1 and (N == 1 or s0 >= C):
        return False, (s0 if N > 1 else C), 1
    elif s0 == 1 and (C == 1 or s1 >= N):
        return False, 1, s1
    else:
        return True, C, 1


site_rowmajor_operands = site_reduce_vals   # engine._rowmajor_operands held a verbatim copy


def site_resample_x(N, C, s0, s1):
    copy = False
    if not (s1 == 1 or C == 1) or (N > 1 and (s0 < C or not _pitch_ok_then(s0, C))):
        copy, s0, s1 = True, C, 1
    if C == 1 and s1 != 1:
        copy, s0, s1 = True, C, 1
    return copy, max(s0 if N > 1 else C, C)


def site_resample_y(N, C, s0, s1):
    copy = False
    if s1 != 1 or (N > 1 and (s0 < C or not _pitch_ok_then(s0, C))):
        copy, s0, s1 = True, C, 1
    return copy, max(s0 if N > 1 else C, C)


def site_table_operands_y(N, C, s0, s1):
    if s1 != 1 or (N > 1 and (s0 < C or not _pitch_ok_then(s0, C))):
        return True, C
    return False, max(s0 if N > 1 else C, C)


def site_perturb(N, C, s0, s1):
    copy = False
    if s1 != 1 or (N > 1 and s0 < C):
        copy, s0, s1 = True, C, 1
    return copy, (max(s0, C) if N > 1 else C)


site_mbar_table = site_perturb        # the same two statements, on x of one state
site_lag_series_args = site_perturb   # ... and on the series of the lag sums

PITCH_LIMITED = [site_resample_x, site_resample_y, site_table_operands_y]
UNLIMITED = [site_perturb, site_mbar_table, site_lag_series_args]
EITHER = [site_reduce_vals, site_rowmajor_operands]


def _grid():
    for N, C in itertools.product((1, 2, 5), (1, 2, 3)):
        strides = sorted({0, 1, 2, C - 1, C, C + 1, N, N + 1, 2 * C})
        for s0, s1 in itertools.product(strides, strides):
            yield N, C, s0, s1


def test_grid_is_what_it_says():
    pts = list(_grid())
    assert len(pts) == len(set(pts))
    for N, C in itertools.product((1, 2, 5), (1, 2, 3)):
        want = {0, 1, 2, C - 1, C, C + 1, N, N + 1, 2 * C}
        assert {(s0, s1) for n, c, s0, s1 in pts if (n, c) == (N, C)} == set(itertools.product(want, want))


def test_rowmajor_layout_with_pitch_limit_is_every_bootstrap_site():
    for pt in _grid():
        for site in PITCH_LIMITED:
            assert rowmajor_layout(*pt, True) == site(*pt), (site.__name__, pt)


def test_rowmajor_layout_without_pitch_limit_is_every_other_rowmajor_site():
    for pt in _grid():
        for site in UNLIMITED:
            assert rowmajor_layout(*pt, False) == site(*pt), (site.__name__, pt)
        assert rowmajor_layout(*pt) == rowmajor_layout(*pt, False)


def test_either_layout_is_both_two_layout_sites():
    for pt in _grid():
        for site in EITHER:
            assert either_layout(*pt) == site(*pt), (site.__name__, pt)


def test_the_sites_agreed_with_each_other():
    """No finding to report: within each family the old copies gave one answer at every grid point."""
    for pt in _grid():
        assert len({site(*pt) for site in PITCH_LIMITED}) == 1, pt
        assert len({site(*pt) for site in UNLIMITED}) == 1, pt


# 768 ld + C <= 2^29: the last pitch that passes and the first that does not, for the grid's C and for the two C at
# which the boundary is met exactly / missed by one (2^29 = 768 * 699050 + 512)
PITCH_EDGE = [(1, 699050, True), (1, 699051, False), (2, 699050, True), (2, 699051, False), (3, 699050, True),
              (3, 699051, False), (512, 699050, True), (512, 699051, False), (513, 699050, False), (513, 699049, True)]


@pytest.mark.parametrize("C, ld, ok", PITCH_EDGE)
def test_pitch_limit_boundary(C, ld, ok):
    assert (768 * ld + C <= 2**29) is ok              # the arithmetic of the header's macro, no allocation
    assert resample_pitch_ok(ld, C) is ok
    assert engine.resample_pitch_ok is _operands.resample_pitch_ok
    for N in (2, 5):
        assert rowmajor_layout(N, C, ld, 1, True) == ((False, ld) if ok else (True, C))
        assert rowmajor_layout(N, C, ld, 1, False) == (False, ld)       # no limit outside the bootstrap kernels
        for site in PITCH_LIMITED:
            assert site(N, C, ld, 1) == rowmajor_layout(N, C, ld, 1, True), site.__name__
        for site in UNLIMITED:
            assert site(N, C, ld, 1) == (False, ld), site.__name__
    assert rowmajor_layout(1, C, ld, 1, True) == (False, C)             # one row has no pitch


# ---------------------------------------------------------------------------
# real tensors: what engine._place reads from them, and that (tensor, ls, lc) addresses the same values
# ---------------------------------------------------------------------------
N_, C_ = 5, 3


def _views():
    g = torch.Generator().manual_seed(7)
    r = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)  # noqa: E731
    odd = torch.empty_strided((N_, 1), (1, 7), dtype=torch.float64)
    odd.copy_(r(N_, 1))
    return {
        # name: (view, rowmajor expects (copy, ls), either expects (copy, ls, lc))
        "padded": (r(N_, 8)[:, :C_], (False, 8), (False, 8, 1)),
        "transposed": (r(C_, N_).T, (True, C_), (False, 1, N_)),
        "expanded": (r(1, C_).expand(N_, C_), (True, C_), (True, C_, 1)),
        "every_other_column": (r(N_, 2 * C_)[:, ::2], (True, C_), (True, C_, 1)),
        "one_row": (r(1, C_), (False, C_), (False, C_, 1)),
        "one_row_of_padded": (r(N_, 8)[2:3, :C_], (False, C_), (False, C_, 1)),
        "column_odd_stride1": (odd, (True, 1), (True, 1, 1)),
    }


def _read(t, ls, lc, shape):
    return torch.as_strided(t, shape, (ls, lc), t.storage_offset())


@pytest.mark.parametrize("name", list(_views()))
def test_place_on_real_tensors(name):
    x, want_row, want_either = _views()[name]
    shape = tuple(x.shape)
    for rule, want in (("rowmajor", (*want_row, 1)), ("rowmajor_pitch", (*want_row, 1)), ("either", want_either)):
        assert engine._layout(x, rule) == want, rule
        t, ls, lc = engine._place(x, rule)
        assert (ls, lc) == want[1:], rule
        if not want[0]:
            assert t is x, rule
        else:
            assert t.is_contiguous() and (t is x) == x.is_contiguous(), rule
        assert torch.equal(_read(t, ls, lc, shape), x), rule
    t, ls, lc = engine._place(x, "tight")
    assert t.is_contiguous() and (ls, lc) == (shape[1], 1) and torch.equal(t, x)
    assert (t is x) == x.is_contiguous()


def test_the_odd_stride_column_counts_as_contiguous():
    """The case the model of contiguous() above does not cover: the rule says copy, torch hands the tensor back, and the
    pitch passed is C = 1 either way."""
    x = _views()["column_odd_stride1"][0]
    assert x.stride() == (1, 7) and x.is_contiguous()
    t, ls, lc = engine._place(x, "rowmajor_pitch")
    assert t is x and (ls, lc) == (1, 1)


# ---------------------------------------------------------------------------
# the bisection "most replicates whose workspace fits the budget"
# ---------------------------------------------------------------------------
def slab_size_then(need, nrep, budget):
    if need(nrep) <= budget or nrep <= 128:
        return nrep
    lo, hi = 1, (nrep + 127) // 128
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if need(min(mid * 128, nrep)) <= budget:
            lo = mid
        else:
            hi = mid - 1
    return min(lo * 128, nrep)


def mbar_boot_slab_then(need, nrep, budget):
    if need(nrep) <= budget:
        return nrep
    lo, hi = 1, nrep
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if need(mid) <= budget:
            lo = mid
        else:
            hi = mid - 1
    return lo


NEEDS = {
    "affine": lambda n: 1000 * n + 4096,
    "steps": lambda n: 65536 * ((n + 63) // 64) + 512,     # grows in steps of 64 replicates
}


@pytest.mark.parametrize("kind", list(NEEDS))
def test_most_that_fit_is_both_bisections(kind):
    need = NEEDS[kind]
    for nrep in range(1, 701):
        budgets = {0, need(1) - 1, need(1), need(nrep) - 1, need(nrep), need(nrep) + 1, 10 * need(nrep)}
        budgets |= {need(n) + d for n in (2, 64, 65, 128, 129, 300, 640) for d in (-1, 0, 1, 300)}   # on and between steps
        for budget in sorted(budgets):
            assert engine._most_that_fit(need, nrep, budget, unit=128) == slab_size_then(need, nrep, budget), (nrep, budget)
            assert engine._most_that_fit(need, nrep, budget) == mbar_boot_slab_then(need, nrep, budget), (nrep, budget)
