"""The bootstrap's plans and path rules are what they were: every size and path query of txm_resample.hip answers, over a grid
that holds every boundary the host code branches on, exactly what the library of the parent commit of the host-dispatch
refactor answered (tests/golden/resample_plan_parent.npz).  Callers keep pre-pass blocks across calls and size workspaces
from these queries, so "equal" is integer equality.  Host-only: no query touches a device (the CU count is 256 without one,
as on an MI355X).

The fixture is recorded from a checkout of the commit to compare against, with this file copied into its tests/:

    python tests/test_resample_plan_cpu.py --record        # builds that checkout's library, writes its tests/golden/...
"""

import itertools
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
FIXTURE = ROOT / "tests" / "golden" / "resample_plan_parent.npz"

# the boundaries plan_resample / plan_i8 / use_i8 / table_kernel_pays / narrow_table_pays / use_i8_batched branch on
NS = [1023, 1024, 2053, 262143, 262144, 786431, 786432, 1048575, 1048576, 4194304, 16777216, 67108864, 100000000]
CS = [1, 4, 5, 8, 9, 16, 17, 32, 33, 48, 49, 64, 2048, 2049]
NREPS = [1, 31, 32, 63, 64, 65, 99, 100, 127, 128, 129, 130, 255, 256, 383, 384, 1000]
ORDERS = list(range(9))
PATHS = [-1, 0, 1, 2, 3]          # TXM_PATH_AUTO, _FP64, _INT8, _INT8_FUSED, _INT8_TABLE
SS = [1, 2, 64, 65535]
SHAPES = list(itertools.product(NS, CS, NREPS, ORDERS))
# shapes outside the served range: every query's "0 / TXM_PATH_FP64" answer
BAD = [(0, 4, 100, 3), (1024, 0, 100, 3), (1024, 4, 0, 3), (1024, 4, 100, -1), (1024, 4, 100, 9)]


def _load():
    sys.path.insert(0, str(ROOT))
    from thermoextrap_amd import _build, _lib

    _build.build_library()
    return _lib.load()


def _aligned_operand(lib):
    """txm_resample_operands_aligned over pointer alignments, pitches and widths (host arithmetic on the pointer VALUE)."""
    out = []
    for C, (xoff, ldx_extra), y in itertools.product(CS, [(0, 0), (8, 0), (0, 1), (0, 2), (0, 3), (0, 4)], [None, 0, 8]):
        x = 4096 + xoff
        ldx = C + ldx_extra
        out.append(lib.txm_resample_operands_aligned(x, ldx, C, None if y is None else 8192 + y, ldx))
    out.append(lib.txm_resample_operands_aligned(None, 4, 4, None, 4))
    out.append(lib.txm_resample_operands_aligned(4096, 4, 0, None, 4))
    return np.asarray(out, np.int8)


def _auto_queries(lib, shapes):
    """What depends on the process-wide default: the rule, the kernel word, the workspace of a TXM_PATH_AUTO call, the batched rule."""
    path = np.asarray([lib.txm_resample_path(*s) for s in shapes], np.int8)
    kern = np.asarray([[lib.txm_resample_kernel(*s, -1, hy, 1) for hy in (0, 1)] for s in shapes], np.int16)
    ws = np.asarray([lib.txm_resample_vals_ws_bytes(*s) for s in shapes], np.int64)
    bpath = np.asarray([lib.txm_resample_batched_path(2, *s) for s in shapes], np.int8)
    return path, kern, ws, bpath


def record(lib):
    r = {}
    shapes = SHAPES + BAD
    assert lib.txm_set_resample_path(-1) == 0
    r["path"], r["kernel_auto"], r["ws"], r["bpath2"] = _auto_queries(lib, shapes)
    r["kernel"] = np.asarray([[[[lib.txm_resample_kernel(*s, p, hy, al) for al in (0, 1)] for hy in (0, 1)] for p in PATHS]
                              for s in shapes], np.int16)
    r["ws_opts"] = np.asarray([[[lib.txm_resample_vals_ws_bytes_opts(*s, p, hy) for hy in (0, 1)] for p in PATHS] for s in shapes],
                              np.int64)
    r["prep"] = np.asarray([lib.txm_resample_prep_bytes(*s) for s in shapes], np.int64)
    r["supported"] = np.asarray([lib.txm_resample_i8_supported(*s) for s in shapes], np.int8)
    r["y_ws"] = np.asarray([lib.txm_resample_y_ws_bytes(*s) for s in list(itertools.product(NS, CS, NREPS)) + [b[:3] for b in BAD]],
                           np.int64)
    r["aligned"] = _aligned_operand(lib)
    r["bpath"] = np.asarray([[lib.txm_resample_batched_path(S, *s) for S in [0] + SS] for s in shapes], np.int8)
    r["bprep"] = np.asarray([[lib.txm_resample_batched_prep_bytes(S, *s) for S in [0] + SS] for s in shapes], np.int64)
    r["bws"] = np.asarray([[lib.txm_resample_vals_batched_ws_bytes(S, *s) for S in [0] + SS] for s in shapes], np.int64)
    # txm_set_resample_path: each forced value, then back to -1 (and a word that is no path is refused and changes nothing)
    for forced in (0, 1, 2, 3):
        assert lib.txm_set_resample_path(forced) == 0
        try:
            r[f"forced{forced}_path"], r[f"forced{forced}_kernel"], r[f"forced{forced}_ws"], r[f"forced{forced}_bpath2"] = \
                _auto_queries(lib, shapes)
        finally:
            assert lib.txm_set_resample_path(-1) == 0
    assert lib.txm_set_resample_path(4) != 0
    r["back_path"], r["back_kernel"], r["back_ws"], r["back_bpath2"] = _auto_queries(lib, shapes)
    return r


@pytest.fixture(scope="module")
def answers():
    return record(_load())


@pytest.fixture(scope="module")
def parent():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def test_the_grid_holds_the_boundaries():
    assert {1023, 1024, 262143, 262144, 786431, 786432, 100000000} <= set(NS) and {16, 17, 32, 33, 2048, 2049} <= set(CS)
    assert {63, 64, 65, 127, 128, 129, 130, 383, 384, 1000} <= set(NREPS) and ORDERS == list(range(9)) and SS == [1, 2, 64, 65535]


def test_every_query_answers_what_the_parent_answered(answers, parent):
    assert sorted(answers) == sorted(parent)
    for k in sorted(parent):
        assert answers[k].dtype == parent[k].dtype and answers[k].shape == parent[k].shape, k
        bad = np.argwhere(answers[k] != parent[k])
        assert bad.size == 0, (k, len(bad), bad[:5].tolist(), answers[k][tuple(bad[0])], parent[k][tuple(bad[0])])


def test_the_recorded_answers_are_the_calibration_points(parent):
    """Two values written down independently of the recording (N = 1e8, C = 32, nrep = 1000, order 4), and the override left at -1."""
    i = SHAPES.index((100000000, 32, 1000, 4))
    assert parent["ws_opts"][i, PATHS.index(0), 0] == 6598246656
    assert parent["prep"][i] == 544256
    for k in ("path", "kernel", "ws", "bpath2"):
        assert np.array_equal(parent[f"back_{k}"], parent["kernel_auto" if k == "kernel" else k])


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit("usage: python tests/test_resample_plan_cpu.py --record")
    res = record(_load())
    np.savez_compressed(FIXTURE, **res)
    print(f"wrote {FIXTURE} ({FIXTURE.stat().st_size} bytes, {sum(v.size for v in res.values())} answers)")
