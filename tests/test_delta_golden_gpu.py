"""The delta-method error bars through the public model API, held to the bits of the build before their host code was
folded onto shared helpers (thermoextrap_amd/_delta.py, the engine's influence helpers, csrc/txm_influence_common.h):
tests/golden/delta_parent.npz, written once by tests/golden/make_delta_golden.py on that build.  Every value must be
reproduced bit for bit, every labelled result with the same dims and the same coordinates (names, dims, values)."""

import importlib.util
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden" / "delta_parent.npz"


@pytest.fixture(scope="module")
def golden_and_got(txm):
    spec = importlib.util.spec_from_file_location("make_delta_golden", GOLDEN.parent / "make_delta_golden.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    g = np.load(GOLDEN)
    got = mod.compute(txm, {k: g[k] for k in g.files if k.startswith("in_")})
    return {k: g[k] for k in g.files if not k.startswith("in_")}, got


def test_every_entry_is_recomputed(golden_and_got):
    g, got = golden_and_got
    assert sorted(got) == sorted(g)
    assert sum(k.startswith("out_") for k in g) >= 60 and sum(k.startswith("dims_") for k in g) >= 50


def test_values_bit_for_bit(golden_and_got):
    g, got = golden_and_got
    bad = [k for k in g if k.startswith("out_") and not (got[k].shape == g[k].shape and np.array_equal(got[k], g[k]))]
    assert not bad, bad


def test_dims_and_coordinates(golden_and_got):
    g, got = golden_and_got
    bad = [k for k in g if k.startswith(("dims_", "cdims_")) and got[k].tolist() != g[k].tolist()]
    bad += [k for k in g if k.startswith("coord_") and not (got[k].shape == g[k].shape and np.array_equal(got[k], g[k]))]
    assert not bad, bad
