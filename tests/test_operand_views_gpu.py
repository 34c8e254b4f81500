"""The copy branch of the operand layout rules (thermoextrap_amd/_operands.py) at every entry point that applies one: a
view the rule copies gives the bits of the same call on ``.contiguous()`` of it -- it is the same library call on the same
values, so there is no tolerance.

Views the rule passes through (a padded pitch, a column-contiguous transpose into ``reduce_vals``) reach another kernel
path than their clone and are not bit-equal by design; the kernel tests cover them (test_reduce_kernels_gpu.py,
test_resample_kernel_gpu.py, test_perturb_gpu.py, test_mbar_kernels_gpu.py)."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, C, ORDER, NREP = 37, 3, 2, 4


@pytest.fixture(scope="module")
def eng(txm):
    from thermoextrap_amd import engine

    return engine


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).cuda()


def make_view(kind, n, seed):
    """An (n, C) float64 CUDA view of the given kind over fresh random data."""
    rng = np.random.default_rng(seed)
    if kind == "every_other_column":
        return dev(rng.normal(0.3, 1.0, (n, 2 * C)))[:, ::2]
    if kind == "expanded":
        return dev(rng.normal(0.3, 1.0, (1, C))).expand(n, C)
    if kind == "transposed":
        return dev(rng.normal(0.3, 1.0, (C, n))).T
    raise AssertionError(kind)


def make_u(n, seed):
    return dev(np.random.default_rng(1000 + seed).normal(0.0, 1.0, n))


def same_bits(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same_bits(p, q) for p, q in zip(a, b))
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def copied(eng, x, rule):
    """The case is one the rule copies (else the test would compare a call with itself)."""
    assert eng._layout(x, rule)[0] and not x.is_contiguous()
    return x.contiguous()


EITHER_VIEWS = ["every_other_column", "expanded"]
ROWMAJOR_VIEWS = ["every_other_column", "expanded", "transposed"]


# ---------------------------------------------------------------------------
# the two-layout rule
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", EITHER_VIEWS)
def test_reduce_vals(eng, kind):
    x, u, w = make_view(kind, N, 1), make_u(N, 1), make_u(N, 2).abs()
    xc = copied(eng, x, "either")
    assert same_bits(eng.reduce_vals(x, u, ORDER), eng.reduce_vals(xc, u, ORDER))
    assert same_bits(eng.reduce_vals(x, u, ORDER, w), eng.reduce_vals(xc, u, ORDER, w))


def test_reduce_vals_one_row(eng):
    x, u = make_view("every_other_column", 1, 2), make_u(1, 2)
    assert same_bits(eng.reduce_vals(x, u, ORDER), eng.reduce_vals(copied(eng, x, "either"), u, ORDER))


@pytest.mark.parametrize("kind", EITHER_VIEWS)
def test_reduce_pivot_and_sums(eng, kind):
    x, u = make_view(kind, N, 3), make_u(N, 3)
    xc = copied(eng, x, "either")
    piv = eng.reduce_pivot(x, u)
    assert same_bits(piv, eng.reduce_pivot(xc, u))
    assert same_bits(eng.reduce_sums(x, u, ORDER, piv), eng.reduce_sums(xc, u, ORDER, piv))


@pytest.mark.parametrize("kind", EITHER_VIEWS)
def test_push_vals(eng, kind):
    x, u = make_view(kind, N, 4), make_u(N, 4)
    xc = copied(eng, x, "either")
    zeros = lambda: torch.zeros((C, 2, ORDER + 1), dtype=torch.float64, device="cuda")  # noqa: E731
    assert same_bits(eng.push_vals(zeros(), x, u), eng.push_vals(zeros(), xc, u))


@pytest.mark.parametrize("kind", EITHER_VIEWS)
def test_influence_cov(eng, kind):
    x, u = make_view(kind, N, 5), make_u(N, 5)
    xc = copied(eng, x, "either")
    rng = np.random.default_rng(55)
    a, b, cx = dev(rng.normal(size=(C, 2, 3))), dev(rng.normal(size=(C, 2, 3))), dev(rng.normal(0.3, 0.1, C))
    assert same_bits(eng.influence_cov(x, u, a, b, 0.05, cx), eng.influence_cov(xc, u, a, b, 0.05, cx))


# ---------------------------------------------------------------------------
# the row-major rule
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ROWMAJOR_VIEWS)
def test_resample_vals_x(eng, kind):
    x, u = make_view(kind, N, 6), make_u(N, 6)
    xc = copied(eng, x, "rowmajor_pitch")
    s = eng.DeviceSampler(seed=11, nrep=NREP, ndat=N)
    assert same_bits(eng.resample_vals(x, u, ORDER, sampler=s), eng.resample_vals(xc, u, ORDER, sampler=s))


@pytest.mark.parametrize("kind", ROWMAJOR_VIEWS)
def test_resample_vals_y(eng, kind):
    x, u, y = dev(np.random.default_rng(7).normal(0.3, 1.0, (N, C))), make_u(N, 7), make_view(kind, N, 8)
    yc = copied(eng, y, "rowmajor_pitch")
    s = eng.DeviceSampler(seed=12, nrep=NREP, ndat=N)
    got, want = eng.resample_vals(x, u, ORDER, sampler=s, y=y), eng.resample_vals(x, u, ORDER, sampler=s, y=yc)
    assert len(got) == 2 and same_bits(got, want)


@pytest.mark.parametrize("kind", ROWMAJOR_VIEWS)
def test_perturb(eng, kind):
    x, u = make_view(kind, N, 9), make_u(N, 9)
    xc = copied(eng, x, "rowmajor")
    da = np.linspace(-0.4, 0.5, 9)          # two passes of targets
    assert same_bits(eng.perturb(x, u, da), eng.perturb(xc, u, da))
    freq = eng.DeviceSampler(seed=13, nrep=NREP, ndat=N).freq()
    assert same_bits(eng.perturb(x, u, da, freq=freq), eng.perturb(xc, u, da, freq=freq))


def test_perturb_one_row(eng):
    x, u = make_view("every_other_column", 1, 10), make_u(1, 10)
    assert same_bits(eng.perturb(x, u, [0.1, -0.2]), eng.perturb(copied(eng, x, "rowmajor"), u, [0.1, -0.2]))


@pytest.mark.parametrize("kind", ROWMAJOR_VIEWS)
def test_mbar_predict(eng, kind):
    xs = [make_view(kind, N, 20), make_view(kind, N, 21)]
    us = [make_u(N, 20), make_u(N, 21) + 0.2]
    xc = [copied(eng, x, "rowmajor") for x in xs]
    alpha0, f, alphas = [1.0, 1.1], [0.0, 0.02], [0.95, 1.05, 1.2]
    assert same_bits(eng.mbar_predict(xs, us, alpha0, f, None, alphas), eng.mbar_predict(xc, us, alpha0, f, None, alphas))


@pytest.mark.parametrize("kind", ROWMAJOR_VIEWS)
def test_lag_sums(eng, kind):
    x, u = make_view(kind, N, 30), make_u(N, 30)
    xc = copied(eng, x, "rowmajor")
    pairs = list(range(1 + 2 * C))
    assert same_bits(eng.lag_sums(x, u, pairs, 0, eng.LAG_BLOCK), eng.lag_sums(xc, u, pairs, 0, eng.LAG_BLOCK))
