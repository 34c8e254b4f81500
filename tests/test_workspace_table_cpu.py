"""The contract table of tests/test_workspace_contract_gpu.py is complete and well-formed, and the guard-banded buffer
helper (tests/_bands.py) does what the GPU tests rely on -- all without a GPU: the size queries are host logic.

* every ``size_t txm_*bytes(`` declaration of include/txmom.h has a row in ``CONTRACTS``, and every row names a query
  the header declares: a new entry point cannot be added without one;
* every case of every row gets a non-zero size from this machine's build (a typo in a shape shows up here);
* ``Banded`` on ``device="cpu"``: layout, alignment, each fill, and ``check()`` turning false after a write into the
  front band and, separately, into the back band.
"""

from __future__ import annotations

import re
from pathlib import Path

import numpy as np
import pytest
import torch

import test_workspace_contract_gpu as wc
from _bands import ALIGN, BAND, BAND_BYTE, NAN_BITS, Banded

ROOT = Path(__file__).resolve().parent.parent


def header_queries():
    text = (ROOT / "include" / "txmom.h").read_text()
    # (every function that returns a size: the *_bytes queries and txm_resample_vals_ws_bytes_opts)
    return re.findall(r"^size_t\s+(txm_\w*bytes\w*)\s*\(", text, flags=re.M)


def test_the_header_declares_the_queries_this_file_expects_to_find():
    q = header_queries()
    assert len(q) == len(set(q)) >= 29 and "txm_resample_vals_ws_bytes_opts" in q and "txm_reduce_vals_ws_bytes" in q and "txm_lag_rows_batched_bytes" in q


def test_every_size_query_of_the_header_has_a_row():
    rows = [r.query for r in wc.CONTRACTS]
    assert len(rows) == len(set(rows))
    assert sorted(rows) == sorted(header_queries())


def test_every_row_is_well_formed():
    text = (ROOT / "include" / "txmom.h").read_text()
    for row in wc.CONTRACTS:
        assert row.calls and row.cases, row.query
        for call in row.calls:
            assert re.search(rf"^int {call}\(", text, flags=re.M), (row.query, call)
        ids = [c["id"] for c in row.cases]
        assert len(ids) == len(set(ids)), row.query
        assert row.short in ("standard", "none", "exact", "prep")


@pytest.mark.parametrize("row,case", wc.ALL, ids=[f"{row.query[4:]}-{case['id']}" for row, case in wc.ALL])
def test_every_case_has_a_nonzero_size_on_this_build(row, case):
    L = wc.lib()
    assert row.size(L, case) > 0


def test_the_bootstrap_cases_take_the_kernels_they_are_named_for():
    """txm_resample_kernel is host logic: the kernel word of every device-sampler bootstrap case, checked before the GPU
    visit (the GPU test repeats it and reads the info words the call wrote)."""
    L = wc.lib()
    seen = set()
    for case in wc.RS_AUTO + wc.RS_OPTS + wc.RS_Y + wc.RS_PREP:
        kern = wc.PATH_FP64 if case["freq"] else wc.rs_kernel(L, case) & 0xFF
        if case["kernel"] is not None:
            assert kern == case["kernel"], (case["id"], kern)
        else:
            assert kern in (wc.PATH_FUSED, wc.PATH_TABLE), (case["id"], kern)
        seen.add(kern)
    assert seen == {wc.PATH_FP64, wc.PATH_FUSED, wc.PATH_TABLE}
    tables = [c for c in wc.RS_OPTS if c["kernel"] == wc.PATH_TABLE]
    assert all(wc.rs_need(L, c) >= wc.rs_floor(L, c) for c in wc.RS_AUTO + wc.RS_OPTS + wc.RS_Y + wc.RS_PREP)
    assert tables and all(wc.rs_need(L, c) > wc.rs_floor(L, c) for c in tables)


@pytest.mark.parametrize("nbytes", [0, 1, 8, 255, 256, 4097, 790016])
def test_banded_layout_and_alignment(nbytes):
    b = Banded(nbytes, "zero", device="cpu")
    assert b.ptr % ALIGN == 0 and b.payload.numel() == nbytes and (nbytes == 0 or b.payload.data_ptr() == b.ptr)
    assert b.front.numel() == BAND == b.back.numel() == 65536
    assert b.front.data_ptr() + BAND == b.ptr and b.back.data_ptr() == b.ptr + nbytes
    assert b.raw.data_ptr() <= b.front.data_ptr() and b.back.data_ptr() + BAND <= b.raw.data_ptr() + b.raw.numel()
    assert bool((b.front == BAND_BYTE).all()) and bool((b.back == BAND_BYTE).all()) and BAND_BYTE == 0xA5
    assert b.check() and b.holds_fill()


def test_banded_fills():
    z = Banded(72, "zero", device="cpu")
    assert not z.payload.any() and z.holds_fill()
    n = Banded(72, "nan", device="cpu")
    assert bool((n.view(torch.int64) == NAN_BITS).all()) and torch.isnan(n.view(torch.float64)).all() and NAN_BITS == 0x7FF8000000000000
    halves = n.view(torch.int32).reshape(-1, 2)
    assert bool((halves[:, 0] == 0).all()) and bool((halves[:, 1] == 0x7FF80000).all())
    ragged = Banded(13, "nan", device="cpu")           # a size that is no multiple of 8 keeps the pattern's phase
    assert ragged.payload.tolist() == [0, 0, 0, 0, 0, 0, 0xF8, 0x7F, 0, 0, 0, 0, 0] and ragged.holds_fill()
    f = Banded(80, "value", dtype=torch.float64, device="cpu")
    assert torch.isnan(f.view()).all() and f.view().numel() == 10 and f.unwritten() == 10
    for dtype, size in ((torch.int64, 8), (torch.int32, 4), (torch.uint8, 1)):
        i = Banded(24 * size, "value", dtype=dtype, device="cpu")
        assert i.view().numel() == 24 and i.unwritten() == 24
        assert bool((i.view() == (255 if dtype == torch.uint8 else -1)).all())
    f.view()[3] = 1.5
    f.view()[7] = float("inf")
    assert f.unwritten() == 8 and f.painted().tolist() == [True, True, True, False, True, True, True, False, True, True]
    assert not f.holds_fill() and f.check()
    f.paint()
    assert f.unwritten() == 10 and f.holds_fill()
    with pytest.raises(ValueError):
        Banded(8, "ones", device="cpu")
    with pytest.raises(ValueError):
        n.unwritten()


@pytest.mark.parametrize("where", ["front_first", "front_last", "back_first", "back_last"])
def test_banded_check_sees_a_write_into_either_band(where):
    """The only writes into a band in the suite: on a CPU tensor, to show that ``check()`` reports them."""
    b = Banded(1000, "nan", device="cpu")
    assert b.check()
    band, i = (b.front if where.startswith("front") else b.back), (0 if where.endswith("first") else BAND - 1)
    band[i] = 0
    assert not b.check()
    assert b.holds_fill()                     # the payload is not what changed
    band[i] = BAND_BYTE
    assert b.check()


def test_ctx_refusal_and_success_checks_on_the_cpu(monkeypatch):
    """The bookkeeping of a run (wc.Ctx) on CPU buffers: an untouched output is 'refused', a fully written one is 'ok',
    a partially written one is neither."""
    monkeypatch.setattr(wc, "Banded", lambda *a, **k: Banded(*a, **{**k, "device": "cpu"}))
    monkeypatch.setattr(torch.cuda, "synchronize", lambda: None)
    ctx = wc.Ctx("nan", short=1)
    _, nb = ctx.ws(4096)
    assert nb == 4095
    ctx.out("out", (3, 5))
    ctx.verify_refused()
    with pytest.raises(AssertionError):
        ctx.verify_ok()
    out = ctx.bufs["out"][0]
    out.view()[:] = 2.0
    ctx.verify_ok()
    assert np.array_equal(ctx.results()["out"], np.full((3, 5), 2.0))
    with pytest.raises(AssertionError):
        ctx.verify_refused()
    out.view()[4] = float("nan")
    with pytest.raises(AssertionError):
        ctx.verify_ok()
