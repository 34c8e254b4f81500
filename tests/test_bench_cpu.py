"""bench.py's command line and its --dump-outputs writer, without a GPU."""

import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def _parse(monkeypatch, *argv):
    import bench

    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_a_plain_run_leaves_the_full_measurements_off(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    a = _parse(monkeypatch, "--full", "--dump-outputs", "out")
    assert a.full and a.dump_outputs == "out"


@pytest.mark.parametrize("argv", [("--steps", "0"), ("--warmup", "-1")])
def test_step_counts_are_checked(monkeypatch, argv):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, *argv)


def test_dump_outputs_writes_every_array_as_float(tmp_path):
    import bench

    rng = np.random.default_rng(1)
    arrays = {"a": rng.normal(size=(3, 4, 5)), "b": rng.normal(size=7).astype(np.float32), "c": np.arange(6).reshape(2, 3)}
    bench.dump_outputs(tmp_path / "d", arrays)
    got = {p.stem: np.load(p) for p in (tmp_path / "d").glob("*.npy")}
    assert sorted(got) == ["a", "b", "c"]
    assert got["a"].dtype == np.float64 and np.array_equal(got["a"], arrays["a"])
    assert got["b"].dtype == np.float32 and np.array_equal(got["b"], arrays["b"])
    assert got["c"].dtype == np.float64 and np.array_equal(got["c"], arrays["c"])


def test_dump_outputs_samples_a_large_output_the_same_way_every_time(tmp_path, monkeypatch):
    import bench

    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 40_000)
    rng = np.random.default_rng(2)
    arrays = {"big": rng.normal(size=(50, 100)), "small": rng.normal(size=(10, 100))}   # 48 000 bytes together
    bench.dump_outputs(tmp_path / "one", arrays)
    bench.dump_outputs(tmp_path / "two", arrays)
    files = sorted((tmp_path / "one").glob("*.npy"))
    assert sum(f.stat().st_size for f in files) <= 40_000
    for f in files:
        a, b = np.load(f), np.load(tmp_path / "two" / f.name)
        assert a.ndim == 1 and np.array_equal(a, b)
        full = arrays[f.stem].reshape(-1)
        assert 0 < a.size < full.size and np.isin(a, full).all()
