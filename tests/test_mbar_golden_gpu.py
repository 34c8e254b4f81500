"""Every MBAR pass over the pooled samples -- the engine's calls at a pinned solution, MBARModel and MBARBootstrap through
their public methods -- held to the bits of the build before the target passes were folded onto one host path
(engine.py's _mbar_* helpers) and the entry points onto one preamble (csrc/txm_mbar.h): tests/golden/mbar_parent.npz,
written once by tests/golden/make_mbar_golden.py on that build.  The kernels use no floating-point atomics and combine
their partials in a fixed order, so every value must be reproduced bit for bit (compared as bytes: NaN and the sign of
zero included), every labelled result with the same dims and the same coordinates (names, dims, values).  A model-level
value that the recording build itself did not reproduce in a second process is not in the file (make_mbar_golden.py
--drop); its dims and coordinates still are."""

import importlib.util
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden" / "mbar_parent.npz"


def _maker():
    spec = importlib.util.spec_from_file_location("make_mbar_golden", GOLDEN.parent / "make_mbar_golden.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden_and_got(txm):
    mod = _maker()
    g = np.load(GOLDEN)
    d = {k: g[k] for k in g.files if k.startswith("in_")}
    assert mod.check_inputs(d)
    got = mod.compute(txm, d)
    return {k: g[k] for k in g.files if not k.startswith("in_")}, got


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_every_entry_is_recomputed(golden_and_got):
    g, got = golden_and_got
    dropped = sorted(set(got) - set(g))
    assert not set(g) - set(got)
    # only model-level values may be missing from the file, at most a fifth of them; never an engine-level entry, a dim
    # or a coordinate
    assert all(k.startswith("out_m_") for k in dropped), dropped
    assert 5 * len(dropped) <= sum(k.startswith("out_m_") for k in got), dropped
    assert sum(k.startswith("out_e_") for k in got) == 355 and sum(k.startswith("out_m_") for k in got) == 77
    assert sum(k.startswith("dims_") for k in g) == 59


def test_engine_values_bit_for_bit(golden_and_got):
    g, got = golden_and_got
    bad = [k for k in g if k.startswith("out_e_") and not _same_bits(got[k], g[k])]
    assert not bad, bad


def test_model_values_bit_for_bit(golden_and_got):
    g, got = golden_and_got
    bad = [k for k in g if k.startswith("out_m_") and not _same_bits(got[k], g[k])]
    assert not bad, bad


def test_dims_and_coordinates(golden_and_got):
    g, got = golden_and_got
    bad = [k for k in g if k.startswith(("dims_", "cdims_")) and got[k].tolist() != g[k].tolist()]
    bad += [k for k in g if k.startswith("coord_") and not _same_bits(got[k], g[k])]
    assert not bad, bad
