"""CPU-side checks of the drop-in boundary: the C-ABI library builds for gfx950,
loads without a GPU, exports every symbol include/txmom.h declares, and the
product refuses to compute without a device (no CPU fallback)."""

import ctypes as ct
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def lib():
    from thermoextrap_amd import _build, _lib

    _build.build_library()
    return _lib.load()


def header_symbols():
    text = (ROOT / "include" / "txmom.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(txm_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_expected_entry_points():
    syms = header_symbols()
    for must in ["txm_reduce_vals", "txm_resample_vals", "txm_resample_data", "txm_indices_to_freq",
                 "txm_sampler_tile_counts", "txm_convert_cov", "txm_eval_poly", "txm_init", "txm_last_error"]:
        assert must in syms


def test_library_exports_every_declared_symbol(lib):
    from thermoextrap_amd import _lib

    declared = header_symbols()
    for s in declared:
        assert hasattr(lib, s), f"libtxmom.so does not export {s}"
    # the ctypes binding covers exactly the header
    assert sorted(_lib.SIGNATURES) == declared


def test_abi_version(lib):
    from thermoextrap_amd import _lib

    hdr = int(re.search(r"#define TXM_ABI_VERSION (\d+)", (ROOT / "include" / "txmom.h").read_text()).group(1))
    assert lib.txm_abi_version() == hdr == _lib.ABI_VERSION == 2
    # the sampler stream the library draws == the one the committed vectors pin (tests/golden/sampler_stream_v3.json)
    import json

    sv = int(re.search(r"#define TXM_SAMPLER_STREAM_VERSION (\d+)", (ROOT / "include" / "txmom.h").read_text()).group(1))
    golden = json.load(open(ROOT / "tests" / "golden" / f"sampler_stream_v{sv}.json"))
    assert lib.txm_sampler_stream_version() == sv == _lib.SAMPLER_STREAM_VERSION == golden["stream_version"] == 3


# the entry points whose FULL argument list INTEGRATION.md quotes, as a C declaration or as `name(arg, ...)` in the text
# (its Python binding examples, `L.txm_...(...)`, span lines and pass expressions: they are not parsed)
DOC_SIGNATURES = ["txm_mbar_cov_ws_bytes", "txm_mbar_cov", "txm_influence_cov_ws_bytes", "txm_influence_cov",
                  "txm_resample_kernel", "txm_resample_operands_aligned", "txm_resample_vals_ws_bytes_opts",
                  "txm_resample_batched_path"]


def _quoted_arities(text, name):
    """The argument counts of every `name(...)` in text that is not a call through the binding (`L.name(...)`)."""
    out = []
    for m in re.finditer(rf"(?<![\w.]){name}\(", text):
        depth, i, commas = 1, m.end(), 0
        while depth:
            ch = text[i]
            depth += (ch == "(") - (ch == ")")
            commas += ch == "," and depth == 1
            i += 1
        out.append(commas + 1 if text[m.end():i - 1].strip() else 0)
    return out


def test_integration_doc_quotes_the_bound_arities():
    """INTEGRATION.md is what a binder is written from: every signature it quotes in full has the number of arguments the
    header declares and _lib.SIGNATURES binds (it once gave txm_resample_operands_aligned a sixth, `order`)."""
    from thermoextrap_amd import _lib

    text = (ROOT / "INTEGRATION.md").read_text()
    for name in DOC_SIGNATURES:
        got = _quoted_arities(text, name)
        assert got, f"INTEGRATION.md no longer quotes {name}"
        assert set(got) == {len(_lib.SIGNATURES[name][1])}, (name, got)
    assert _quoted_arities("f(a, g(b, c), d) and L.f(x) and f()", "f") == [3, 0]


def test_struct_layouts_match_the_header():
    """The ctypes mirrors of the header's host structs: field order, offsets and sizes (ABI 2: txm_sampler_spec.rep0,
    txm_resample_opts)."""
    from thermoextrap_amd import _lib

    text = (ROOT / "include" / "txmom.h").read_text()

    def fields(name):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        return [m.group(1) for m in re.finditer(r"(\w+);", body)]

    assert fields("txm_sampler_spec") == [f[0] for f in _lib.SamplerSpec._fields_] == ["seed", "nrep", "ndat", "nsamp", "rep0"]
    assert ct.sizeof(_lib.SamplerSpec) == 40 and _lib.SamplerSpec.rep0.offset == 32
    assert fields("txm_resample_opts") == [f[0] for f in _lib.ResampleOpts._fields_]
    assert ct.sizeof(_lib.ResampleOpts) == 56 and _lib.ResampleOpts.prep.offset == 8 and _lib.ResampleOpts.out_y.offset == 48
    assert fields("txm_state_ptrs") == [f[0] for f in _lib.StatePtrs._fields_]


def test_per_call_entry_points_validate_without_a_device(lib):
    """ABI 2 additions: the replicate offset is range-checked on the host, the index histogram takes its error
    word in caller scratch, the prep-block size is pure host logic."""
    from thermoextrap_amd import _lib

    sp = _lib.SamplerSpec(seed=1, nrep=4, ndat=5000, nsamp=0, rep0=0)
    assert lib.txm_sampler_counts_ws_bytes(ct.byref(sp)) > 0
    sp.rep0 = 2**32 - 4
    assert lib.txm_sampler_counts_ws_bytes(ct.byref(sp)) > 0
    sp.rep0 = 2**32 - 3                                    # stream replicates would pass 2^32
    assert lib.txm_sampler_counts_ws_bytes(ct.byref(sp)) == 0 and b"2^32" in lib.txm_last_error()
    sp.rep0 = -1
    assert lib.txm_sampler_counts_ws_bytes(ct.byref(sp)) == 0
    sp.rep0, sp.nrep = 0, 1 << 20                          # many replicates: no 65535 limit any more
    assert lib.txm_sampler_counts_ws_bytes(ct.byref(sp)) > 0
    assert lib.txm_indices_to_freq_ws_bytes() >= 4
    assert lib.txm_indices_to_freq(None, 1, 1, 1, None, None, 0, None) == -1
    p_small = lib.txm_resample_prep_bytes(1_000_000, 32, 1000, 4)
    p_wide = lib.txm_resample_prep_bytes(1_000_000, 64, 1000, 4)
    assert 0 < p_small < p_wide                           # one table set per 32-column group
    assert lib.txm_resample_prep_bytes(0, 32, 1000, 4) == 0
    assert lib.txm_resample_vals_ws_bytes(1_000_000, 32, 1000, 4) > p_small
    # the batched entry's pre-pass block: one for the S states of a narrow collection, none where the int8 path never applies
    b1 = lib.txm_resample_batched_prep_bytes(1, 1_000_000, 4, 100, 3)
    b64 = lib.txm_resample_batched_prep_bytes(64, 1_000_000, 4, 100, 3)
    assert 0 < b1 < b64 <= 64 * b1
    assert lib.txm_resample_batched_prep_bytes(64, 1_000_000, 32, 100, 3) == 0      # wide states: FP64 kernel only
    assert lib.txm_resample_batched_prep_bytes(64, 1_000_000, 4, 100, 0) == 0       # order 0: not a narrow-state shape
    assert lib.txm_resample_batched_prep_bytes(0, 1_000_000, 4, 100, 3) == 0
    assert lib.txm_resample_vals_batched_ws_bytes(64, 1_000_000, 4, 100, 3) > b64   # scratch of both paths + the block
    assert lib.txm_resample_vals_batched_opts(None, 1, 4, 1000, 4, 3, 10, None, None, None, None, None, None, 0, None) == -1


def test_no_gpu_means_loud_failure_not_fallback(lib):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from thermoextrap_amd import TxmError, require_gpu

    with pytest.raises(TxmError):
        require_gpu()
    n = ct.c_int(-1)
    rc = lib.txm_device_count(ct.byref(n))
    assert rc != 0 and n.value == 0
    assert b"HIP" in lib.txm_last_error()
    assert lib.txm_init(0) != 0


def test_argument_validation_needs_no_device(lib):
    # pure host-side validation paths return TXM_ERR_INVALID before touching HIP
    assert lib.txm_sampler_ntiles(1) == 1
    assert lib.txm_sampler_ntiles(1024) == 1
    assert lib.txm_sampler_ntiles(1025) == 2
    assert lib.txm_reduce_vals_ws_bytes(100, 0, 2) == 0
    assert lib.txm_resample_vals_ws_bytes(100, 4, 0, 2) == 0
    rc = lib.txm_reduce_vals(None, 1, 1, None, None, 10, 1, 2, None, None, 0, None)
    assert rc == -1 and b"null" in lib.txm_last_error()


def test_product_never_imports_oracle():
    pkg = ROOT / "thermoextrap_amd"
    pat = re.compile(r"^\s*(from|import)\s+oracle\b|importlib.*oracle|liboracle", re.M)
    for p in pkg.rglob("*.py"):
        assert not pat.search(p.read_text()), f"{p} reaches into oracle/"


def test_workspace_and_path_queries_are_pure_host_logic(lib, monkeypatch):
    """Sizing and dispatch queries need no device: the int8-sliced kernel is chosen where it was
    measured to win, the workspace covers whichever kernel runs, txm_set_resample_path overrides."""
    assert lib.txm_set_resample_path(-1) == 0
    big = 100_000_000
    assert lib.txm_resample_path(big, 32, 1000, 4) == 1
    assert lib.txm_resample_path(big, 32, 32, 4) == 1 and lib.txm_resample_path(big, 32, 16, 4) == 0   # long series: from 32 replicates
    assert lib.txm_resample_path(big, 12, 1000, 1) == 1     # narrow states: the int8 kernel from order 1 on ...
    assert lib.txm_resample_path(big, 4, 8, 2) == 1         # ... at any replicate count on a long series
    assert lib.txm_resample_path(300_000, 4, 64, 3) == 0 and lib.txm_resample_path(300_000, 4, 128, 3) == 1   # short series: from 128
    assert lib.txm_resample_path(big, 12, 1000, 0) == 0     # order 0 with <= 16 columns: a single 16-column FP64 block
    assert lib.txm_resample_path(big, 12, 1000, 4) == 1     # 8 < C <= 16: int8 kernel, two powers per column
    assert lib.txm_resample_path(big, 8, 1000, 4) == 1      # narrow state: int8 kernel, four powers per column
    assert lib.txm_resample_path(big, 32, 1000, 8) == 0     # order 8: FP64 kernel only
    assert lib.txm_resample_path(10_000, 32, 1000, 4) == 0  # short series
    w_small = lib.txm_resample_vals_ws_bytes(1_000_000, 32, 64, 4)
    w_big = lib.txm_resample_vals_ws_bytes(1_000_000, 32, 1000, 4)
    assert 0 < w_small < w_big < 2**33
    assert lib.txm_resample_vals_ws_bytes(0, 32, 64, 4) == 0
    assert lib.txm_set_resample_path(0) == 0
    assert lib.txm_resample_path(big, 32, 1000, 4) == 0
    assert lib.txm_set_resample_path(1) == 0
    assert lib.txm_resample_path(5000, 3, 2, 1) == 1
    assert lib.txm_resample_path(500, 3, 2, 1) == 0         # below one sampler tile: never
    assert lib.txm_set_resample_path(7) == -1 and b"not a path" in lib.txm_last_error()
    assert lib.txm_set_resample_path(-1) == 0
    assert lib.txm_resample_path(big, 32, 1000, 4) == 1


def test_dispatch_rule_matches_the_header_thresholds(lib):
    """include/txmom.h states the rule of TXM_PATH_AUTO in numbers; this calls txm_resample_path (and the batched predicate, and
    the workspace query that follows the int8 path's kernel choice) on BOTH sides of every threshold named there, so that the
    contract and the code cannot drift apart again (round-4 verdict: the header still described round 2's rule)."""
    assert lib.txm_set_resample_path(-1) == 0
    P = lib.txm_resample_path
    LONG, SHORT = 786432, 262144
    # needs N >= 262144 and order <= 7
    assert P(SHORT, 32, 1000, 4) == 1 and P(SHORT - 1, 32, 1000, 4) == 0
    assert P(LONG, 32, 1000, 7) == 1 and P(LONG, 32, 1000, 8) == 0
    # narrow states (C <= 16): order >= 1; long series at any replicate count, shorter ones from 128 replicates
    for C in (1, 4, 8, 16):
        assert P(LONG, C, 1, 1) == 1 and P(LONG, C, 1000, 0) == 0
        assert P(LONG - 1, C, 127, 3) == 0 and P(LONG - 1, C, 128, 3) == 1
        assert P(SHORT, C, 128, 1) == 1 and P(SHORT - 1, C, 128, 1) == 0
    assert P(LONG, 16, 4, 2) == 1 and P(LONG, 17, 4, 2) == 0   # 17 columns: a wide state, 32 replicates needed
    # wide states (C > 16), long series: order >= 1 from 32 replicates, order 0 from 100
    for C in (17, 32, 64, 48):
        assert P(LONG, C, 31, 1) == 0 and P(LONG, C, 32, 1) == 1
        assert P(LONG, C, 31, 7) == 0 and P(LONG, C, 32, 7) == 1
    assert P(LONG, 32, 99, 0) == 0 and P(LONG, 32, 100, 0) == 1
    # ... shorter series: order >= 3 from 64, orders 1-2 from 128, order 0 from 384
    assert P(LONG - 1, 32, 63, 3) == 0 and P(LONG - 1, 32, 64, 3) == 1
    assert P(LONG - 1, 32, 127, 2) == 0 and P(LONG - 1, 32, 128, 2) == 1
    assert P(LONG - 1, 32, 127, 1) == 0 and P(LONG - 1, 32, 128, 1) == 1
    assert P(LONG - 1, 32, 383, 0) == 0 and P(LONG - 1, 32, 384, 0) == 1
    # a last group of 1..16 columns behind full groups: allowed from order 1, keeps an order-0 call on FP64
    assert P(LONG, 40, 1000, 1) == 1 and P(LONG, 40, 1000, 0) == 0 and P(LONG, 49, 1000, 0) == 1
    # the batched entry: the narrow-state rule, whatever the number of states in the launch
    B = lib.txm_resample_batched_path
    for S in (1, 64):
        assert B(S, LONG, 4, 1, 1) == 1 and B(S, LONG, 4, 100, 0) == 0
        assert B(S, LONG - 1, 4, 127, 3) == 0 and B(S, LONG - 1, 4, 128, 3) == 1
        assert B(S, LONG, 32, 100, 3) == 0                    # wide states: the batched int8 launch does not serve them
    # which int8 kernel serves a wide call, seen through the workspace it asks for: the count table (one byte per sample and
    # replicate padded to 128) is part of it for every order (orders 3 and 4: from two replicate groups on), for every call with a second matrix, and never
    # when the padding to 128 replicates wastes more than 5/4 of the padding to 64
    W = lib.txm_resample_vals_ws_bytes_opts
    N = 10_000_000
    ntiles = -(-N // 1024)
    table = lambda nrep: -(-nrep // 128) * ntiles * 131072  # noqa: E731
    AUTO, FP64, INT8, FUSED, TABLE = -1, 0, 1, 2, 3
    for order in range(8):
        base = W(N, 32, 1000, order, FUSED, 0)
        with_table = W(N, 32, 1000, order, TABLE, 0)
        assert table(1000) <= with_table - base < table(1000) + 4096
        auto = W(N, 32, 1000, order, AUTO, 0)
        assert auto == with_table, order
        assert W(N, 32, 1000, order, AUTO, 1) == with_table            # a second matrix always rides the table kernel
        assert W(N, 32, 1000, order, INT8, 0) == auto and lib.txm_resample_vals_ws_bytes(N, 32, 1000, order) == auto
    assert W(N, 32, 128, 4, AUTO, 0) == W(N, 32, 128, 4, FUSED, 0)      # orders 3 and 4: only from two replicate groups on
    assert W(N, 32, 128, 3, AUTO, 0) == W(N, 32, 128, 3, FUSED, 0) and W(N, 32, 200, 3, AUTO, 0) == W(N, 32, 200, 3, TABLE, 0)
    assert W(N, 32, 129, 4, AUTO, 0) == W(N, 32, 129, 4, FUSED, 0)      # (129 -> 256 against 192: pads badly)
    assert W(N, 32, 200, 4, AUTO, 0) == W(N, 32, 200, 4, TABLE, 0)
    assert W(N, 32, 128, 4, AUTO, 1) == W(N, 32, 128, 4, TABLE, 1)
    assert W(N, 32, 64, 2, AUTO, 0) == W(N, 32, 64, 2, FUSED, 0)        # 64 replicates: padding to 128 doubles the work
    assert W(N, 32, 130, 2, AUTO, 0) == W(N, 32, 130, 2, FUSED, 0)      # 130 -> 256 against 192
    assert W(N, 32, 100, 2, AUTO, 0) == W(N, 32, 100, 2, TABLE, 0)      # 100 -> 128 either way
    assert W(N, 32, 260, 2, AUTO, 0) == W(N, 32, 260, 2, TABLE, 0)      # 260 -> 384 against 320
    # narrow states: the table kernel of txm_resample_i8gn.hip (order >= 1) from 65 replicates on where 128s pad no worse than 64s
    assert table(1000) <= W(N, 8, 1000, 2, TABLE, 0) - W(N, 8, 1000, 2, FUSED, 0) < table(1000) + 4096
    assert W(N, 8, 1000, 2, AUTO, 0) == W(N, 8, 1000, 2, TABLE, 0) and W(N, 8, 200, 4, AUTO, 0) == W(N, 8, 200, 4, TABLE, 0)
    assert W(N, 8, 128, 2, AUTO, 0) == W(N, 8, 128, 2, TABLE, 0) and W(N, 8, 100, 2, AUTO, 0) == W(N, 8, 100, 2, TABLE, 0)  # one group of 128
    assert W(N, 8, 64, 2, AUTO, 0) == W(N, 8, 64, 2, FUSED, 0) and W(N, 8, 130, 2, AUTO, 0) == W(N, 8, 130, 2, FUSED, 0)   # 64; 130 -> 256 against 192
    assert W(N, 16, 1000, 4, AUTO, 0) == W(N, 16, 1000, 4, FUSED, 0) and W(N, 12, 200, 4, AUTO, 0) == W(N, 12, 200, 4, FUSED, 0)  # four quads at order 4: one fused pass against two
    for C_, o_ in ((4, 3), (8, 3), (16, 5), (16, 2), (12, 6), (4, 1), (8, 4)):                # every other width and order (the sweep's ties included)
        assert W(N, C_, 1000, o_, AUTO, 0) == W(N, C_, 1000, o_, TABLE, 0), (C_, o_)
    assert W(786432, 8, 1000, 4, AUTO, 0) == W(786432, 8, 1000, 4, TABLE, 0) and W(786431, 8, 1000, 4, AUTO, 0) == W(786431, 8, 1000, 4, FUSED, 0)
    assert W(500_000, 8, 1000, 2, AUTO, 0) == W(500_000, 8, 1000, 2, FUSED, 0)  # short series
    assert W(N, 8, 1000, 0, TABLE, 0) == W(N, 8, 1000, 0, FUSED, 0)     # order 0 of a narrow state: no int8 kernel at all
    assert W(N, 32, 1000, 2, FP64, 0) <= W(N, 32, 1000, 2, FUSED, 0)
    assert lib.txm_sampler_count_table_bytes(N, 1000) == table(1000)


def test_kernel_word_is_what_a_prep_block_is_keyed_on(lib):
    """txm_resample_kernel: the concrete kernel of one call and whether it carries a second matrix -- what decides the content
    of a kept pre-pass block (round-5 advice: with y at order 4 the fused kernel below two replicate groups leaves no y tables,
    the table kernel above reads them)."""
    assert lib.txm_set_resample_path(-1) == 0
    Kn = lib.txm_resample_kernel
    N, FP64, FUSED, TABLE, WY = 10_000_000, 0, 2, 3, 0x100
    # order 4 + y: the rule's replicate thresholds flip both the kernel and who carries y
    assert Kn(N, 32, 64, 4, -1, 1, 1) == FUSED and Kn(N, 32, 129, 4, -1, 1, 1) == FUSED and Kn(N, 32, 192, 4, -1, 1, 1) == FUSED
    assert Kn(N, 32, 128, 4, -1, 1, 1) == TABLE | WY and Kn(N, 32, 1000, 4, -1, 1, 1) == TABLE | WY
    # other orders: the fused kernel carries y itself (a row set of its last pass)
    assert Kn(N, 32, 64, 6, -1, 1, 1) == FUSED | WY and Kn(N, 32, 1000, 6, -1, 1, 1) == TABLE | WY
    # without y: orders 3 and 4 from two replicate groups on
    assert Kn(N, 32, 128, 4, -1, 0, 1) == FUSED and Kn(N, 32, 256, 4, -1, 0, 1) == TABLE and Kn(N, 32, 1000, 2, -1, 0, 1) == TABLE
    # a forced path is honoured (a slab of 40 replicates of a table call), misaligned operands never ride the table; a second matrix
    # never rides a narrow call (txm_resample_i8gn.hip)
    assert Kn(N, 32, 40, 4, TABLE, 1, 1) == TABLE | WY and Kn(N, 32, 1000, 4, FUSED, 1, 1) == FUSED
    assert Kn(N, 32, 1000, 4, -1, 1, 0) == FUSED and Kn(N, 32, 1000, 4, TABLE, 0, 0) == FUSED
    assert Kn(N, 8, 1000, 4, -1, 1, 1) == TABLE and Kn(N, 8, 64, 4, -1, 0, 1) == FUSED and Kn(N, 8, 1000, 4, FUSED, 0, 1) == FUSED
    assert Kn(N, 8, 1000, 3, -1, 0, 1) == TABLE and Kn(N, 8, 100, 3, -1, 0, 1) == TABLE
    assert Kn(N, 8, 40, 3, TABLE, 0, 1) == TABLE and Kn(N, 8, 1000, 3, TABLE, 1, 1) == TABLE and Kn(N, 8, 1000, 4, -1, 0, 0) == FUSED
    assert Kn(N, 8, 1000, 3, TABLE, 0, 0) == FUSED and Kn(N, 8, 1000, 0, TABLE, 0, 1) == FUSED  # (order 0: no narrow variant)
    assert Kn(N, 32, 16, 4, -1, 0, 1) == FP64 and Kn(N, 32, 1000, 4, FP64, 1, 1) == FP64 and Kn(N, 32, 1000, 8, -1, 0, 1) == FP64
    assert Kn(0, 32, 1000, 4, -1, 0, 1) == FP64
    # `aligned` as the library itself judges a pair of operands (address bits and row pitches only: no device needed)
    import ctypes as ct

    Al = lib.txm_resample_operands_aligned
    p = lambda a: ct.c_void_p(a)  # noqa: E731
    assert Al(p(256), 32, 32, None, 0) == 1 and Al(p(256), 40, 34, p(4096), 36) == 1
    assert Al(p(264), 32, 32, None, 0) == 0          # x not 16-byte aligned
    assert Al(p(256), 33, 32, None, 0) == 0          # odd row pitch
    assert Al(p(256), 34, 34, None, 0) == 0          # 34 columns round up to 36: no room for the last quad in a 34-double row
    assert Al(p(256), 32, 32, p(520), 32) == 0 and Al(p(256), 32, 32, p(512), 31) == 0   # the second matrix likewise
    assert Al(None, 32, 32, None, 0) == 0
    # consistent with the workspace query: a call whose kernel word says TABLE is sized with the table
    W = lib.txm_resample_vals_ws_bytes_opts
    for nrep in (64, 128, 129, 200, 1000):
        for order in (2, 3, 4, 6):
            for has_y in (0, 1):
                table = (Kn(N, 32, nrep, order, -1, has_y, 1) & 0xFF) == TABLE
                assert (W(N, 32, nrep, order, -1, has_y) == W(N, 32, nrep, order, TABLE, has_y)) == table or \
                    W(N, 32, nrep, order, TABLE, has_y) == W(N, 32, nrep, order, FUSED, has_y), (nrep, order, has_y)


# ---------------------------------------------------------------------------
# static guard for inline assembly (round-5 verdict item 5): a GPU memory-access fault of that round came from an asm
# statement that wrote SCC without naming it as clobbered -- the compiler kept a live condition in SCC across it.  Source
# level, no disassembly: every `asm volatile` of the kernels is parsed and every instruction in it that writes M0, SCC, VCC
# or EXEC must be covered by the statement's clobber list (or by an output operand for the SGPR / VGPR it names).
# ---------------------------------------------------------------------------
_SCC_WRITERS = re.compile(
    r"^s_(cmp|cmpk|add|addc|sub|subb|and|andn\d|or|orn\d|xor|xnor|nand|nor|not|lshl|lshr|ashr|bfe|bfm_never|min|max|abs|absdiff|"
    r"bitcmp|wqm|quadmask|bcnt\d|ff\d|flbit|sext_never|lshl\d_add|mul_hi_never|addk|cselect_never|"
    r"and_saveexec|or_saveexec|xor_saveexec|andn\d_saveexec|orn\d_saveexec|nand_saveexec|nor_saveexec|xnor_saveexec)")
_SCC_SAFE = re.compile(r"^s_(mov|cmov|movk|mul_i32|mul_hi|nop|waitcnt|barrier|sleep|setprio|load|buffer_load|memtime|memrealtime|"
                       r"sendmsg|getreg|setreg|bfm|sext|brev|pack|getpc|branch|cbranch|endpgm|cselect|dcache|icache|trap|sethalt|"
                       r"ttrace|inst_prefetch|clause|code_end|version|round_mode|denorm_mode|wait_idle|wakeup|store|scratch|atomic)")


def _asm_statements(text):
    """(line number, template string, clobber list) of every asm statement of a source text."""
    out = []
    for m in re.finditer(r"\basm\s+volatile\s*\(", text):
        i, depth, in_str = m.end(), 1, False
        while depth and i < len(text):
            ch = text[i]
            if in_str:
                if ch == "\\":
                    i += 1
                elif ch == '"':
                    in_str = False
            elif ch == '"':
                in_str = True
            elif ch == "(":
                depth += 1
            elif ch == ")":
                depth -= 1
            i += 1
        body = text[m.end():i - 1]
        # split the top level at ':' outside strings and parentheses ("::" = an empty section)
        secs, cur, depth, in_str, k = [], "", 0, False, 0
        while k < len(body):
            ch = body[k]
            if in_str:
                cur += ch
                if ch == "\\":
                    cur += body[k + 1]
                    k += 1
                elif ch == '"':
                    in_str = False
            elif ch == '"':
                in_str = True
                cur += ch
            elif ch in "([":
                depth += 1
                cur += ch
            elif ch in ")]":
                depth -= 1
                cur += ch
            elif ch == ":" and depth == 0:
                secs.append(cur)
                cur = ""
            else:
                cur += ch
            k += 1
        secs.append(cur)
        template = "".join(re.findall(r'"((?:[^"\\]|\\.)*)"', secs[0])).replace("\\n", "\n").replace("\\t", " ")
        clob = set(re.findall(r'"([^"]*)"', secs[3])) if len(secs) > 3 else set()
        outputs = secs[1] if len(secs) > 1 else ""
        out.append((text.count("\n", 0, m.start()) + 1, template, clob, outputs))
    return out


def _asm_violations(text):
    bad = []
    for line, template, clob, outputs in _asm_statements(text):
        for ins in re.split(r"[\n;]", template):
            ins = ins.strip()
            if not ins:
                continue
            mnem, _, ops = ins.partition(" ")
            dst = ops.split(",")[0].strip() if ops else ""
            need = set()
            if dst == "m0" or re.match(r"^s_(mov|movk).*\bm0\b", ins) and dst == "m0":
                need.add("m0")
            if mnem.startswith("s_") and not _SCC_SAFE.match(mnem):
                if _SCC_WRITERS.match(mnem):
                    need.add("scc")
                else:
                    bad.append((line, ins, "scalar instruction the guard does not know: classify it (SCC writer or not)"))
            if dst in ("vcc", "vcc_lo", "vcc_hi") or (re.match(r"^v_cmp_", mnem) and not mnem.endswith("_e64")):
                need.add("vcc")
            if re.match(r"^v_(add|sub|subrev)_co_u32$", mnem) and len(ops.split(",")) >= 2 and ops.split(",")[1].strip().startswith("vcc"):
                need.add("vcc")
            if dst in ("exec", "exec_lo", "exec_hi") or mnem.startswith("v_cmpx") or "saveexec" in mnem:
                need.add("exec")
            for r in need:
                if r not in clob:
                    bad.append((line, ins, f"writes {r.upper()} but the statement's clobber list {sorted(clob)} does not name it"))
    return bad


def test_inline_asm_clobbers_are_complete():
    """Every asm statement of the kernels names what it writes behind the compiler's back.  The snippet of round 5's reverted
    scalar-condition experiment (gpurun_out/r5_chk12.log: a memory access fault on the first case) must FAIL the guard."""
    n = 0
    for f in sorted((ROOT / "thermoextrap_amd" / "csrc").glob("*.h*")):
        text = f.read_text()
        n += len(_asm_statements(text))
        assert not _asm_violations(text), (f.name, _asm_violations(text))
    assert n >= 25, n                                     # the scanner sees the statements (i8g: 21, i8t: 5, common: 4)
    # the statements that write M0 today are found and are covered
    m0 = []
    for name in ("txm_i8g.h", "txm_resample_i8g.hip", "txm_resample_i8gn.hip"):  # (the DMA helpers are shared by the two table kernels)
        m0 += [st for st in _asm_statements((ROOT / "thermoextrap_amd" / "csrc" / name).read_text()) if "s_mov_b32 m0" in st[1]]
    assert len(m0) >= 4 and all("m0" in st[2] for st in m0)
    # negative controls: round 5's faulting statement (SCC written, not clobbered), and the same mistakes for M0 / VCC / EXEC
    reverted = 'uint32_t c; asm volatile("s_lshr_b32 %0, %1, 1" : "=s"(c) : "s"(wave));'
    v = _asm_violations(reverted)
    assert len(v) == 1 and "SCC" in v[0][2]
    assert not _asm_violations('asm volatile("s_lshr_b32 %0, %1, 1" : "=s"(c) : "s"(wave) : "scc");')
    assert _asm_violations('asm volatile("s_mov_b32 m0, %0\\n\\tds_write_addtid_b32 %1" :: "s"(b), "v"(x) : "memory");')
    assert not _asm_violations('asm volatile("s_mov_b32 m0, %0\\n\\tds_write_addtid_b32 %1" :: "s"(b), "v"(x) : "memory", "m0");')
    assert _asm_violations('asm volatile("v_cmp_lt_u32 vcc, %0, %1" :: "v"(a), "v"(b));')
    assert _asm_violations('asm volatile("s_and_saveexec_b64 %0, vcc" : "=s"(m) :: "scc");')
    assert _asm_violations('asm volatile("s_cmp_eq_u32 %0, 0\\n\\ts_cselect_b32 %1, 1, 0" : "=s"(r) : "s"(a));')
    assert _asm_violations('asm volatile("s_frobnicate_b32 %0" : "=s"(r));')          # unknown scalar mnemonic: classify first


def test_csrc_sha_covers_the_public_header_and_the_build_flags(monkeypatch, tmp_path):
    """A library is current only if it was built from these sources WITH these flags against this header (round-5 advice:
    an edit of include/txmom.h or of _build.FLAGS did not trigger a rebuild)."""
    from thermoextrap_amd import _build

    base = _build.csrc_sha()
    monkeypatch.setattr(_build, "FLAGS", [*_build.FLAGS, "-DX=1"])
    assert _build.csrc_sha() != base
    monkeypatch.undo()
    monkeypatch.setattr(_build, "EXTRA_FLAGS", {**_build.EXTRA_FLAGS, "txm_api.hip": ["-DY"]})
    assert _build.csrc_sha() != base
    monkeypatch.undo()
    assert _build.csrc_sha() == base
    edited = tmp_path / "txmom.h"
    edited.write_bytes(_build.HEADER.read_bytes() + b"/* an edit */")
    monkeypatch.setattr(_build, "HEADER", edited)
    assert _build.csrc_sha() != base


def test_build_switches_are_the_five_kept_ones():
    """The kernel sources test no TXM_* build switch but the source hash and the four diagnostic builds (all of which still
    produce the right sums), the product flags define none, and DESIGN.md's switch table names the four."""
    from thermoextrap_amd import _build

    tested = set()
    for f in sorted(_build.CSRC.glob("*.hip")) + sorted(_build.CSRC.glob("*.h")):
        for line in f.read_text().splitlines():
            m = re.match(r"\s*#\s*(ifdef|ifndef|if|elif)\b(.*)", line)
            if not m:
                continue
            cond = re.sub(r"//.*|/\*.*?\*/", "", m.group(2))
            if m.group(1) in ("ifdef", "ifndef"):
                tested.update(re.findall(r"[A-Za-z_]\w*", cond)[:1])
            else:
                tested.update(w for w in re.findall(r"[A-Za-z_]\w*", cond) if w != "defined")
    diagnostic = {"TXM_G_TIMING", "TXM_I8T_TIMING", "TXM_GN_TIMING", "TXM_G_CLOCKS"}
    assert tested == {"TXM_CSRC_SHA"} | diagnostic, sorted(tested)
    for flags in [_build.FLAGS, *_build.EXTRA_FLAGS.values()]:
        assert not any("-DTXM_" in fl for fl in flags), flags
    table = [ln for ln in (ROOT / "DESIGN.md").read_text().splitlines() if ln.startswith("|")]
    for sw in diagnostic:
        assert any(ln.startswith(f"| `{sw}` |") for ln in table), f"{sw} is missing from DESIGN.md's switch table"


def test_graft_entry_build_runs(lib):
    """The driver's build check: __graft_entry__.build() compiles (a no-op when the library is current), loads and checks
    the ABI version the binding expects -- it carried a literal 1 into the round that made the ABI 2."""
    import importlib
    import sys

    sys.path.insert(0, str(ROOT))
    ge = importlib.import_module("__graft_entry__")
    ge.build()
