"""The host side of the blocked delta-method error bars, without a device: the workspace query of
txm_influence_block_cov, the entry's argument validation, and the level and tail bookkeeping of the blocking curve."""

from __future__ import annotations

import numpy as np
import pytest


def test_workspace_query_is_host_logic():
    """8 ceil(N / block) (C n_f + 1) + 256 bytes; 0 for bad arguments."""
    from thermoextrap_amd import _lib

    Q = _lib.load().txm_influence_block_cov_ws_bytes
    for N, C, nf, nq, block in [(1000, 3, 5, 5, 7), (1000, 3, 5, 5, 1000), (1000, 3, 5, 5, 4096), (1, 1, 1, 1, 1),
                                (10**8, 32, 5, 5, 1024), (10**8, 32, 9, 9, 1), (1001, 65535, 9, 2, 1000)]:
        assert Q(N, C, nf, nq, block) == 8 * -(-N // block) * (C * nf + 1) + 256, (N, C, nf, nq, block)
    assert Q(10**8, 32, 5, 5, 1024) <= 8 * 97657 * 161 + 256                  # 126 MB next to the 25.6 GB of samples
    for bad in [(0, 3, 5, 5, 7), (1000, 0, 5, 5, 7), (1000, 65536, 5, 5, 7), (1000, 3, 0, 5, 7), (1000, 3, 10, 5, 7),
                (1000, 3, 5, 0, 7), (1000, 3, 5, 10, 7), (1000, 3, 5, 5, 0), (1000, 3, 5, 5, -1), (-5, 3, 5, 5, 7)]:
        assert Q(*bad) == 0, bad


def test_entry_point_validates_without_a_device():
    """txm_influence_block_cov: every refusal comes back before any HIP call, one case each."""
    import ctypes as ct

    from thermoextrap_amd import _lib

    lib = _lib.load()
    p = ct.c_void_p(256)   # never dereferenced: every call below fails validation first
    names = ("x", "ls", "u", "w", "N", "C", "nf", "nq", "cu", "cx", "a", "b", "block", "nl", "cov", "mean", "ws", "wsb", "st")
    good = dict(x=p, ls=4, u=p, w=None, N=10, C=4, nf=3, nq=3, cu=0.0, cx=p, a=p, b=p, block=2, nl=3, cov=p, mean=p, ws=p,
                wsb=1 << 30, st=None)

    def call(**bad):
        return lib.txm_influence_block_cov(*[{**good, **bad}[n] for n in names])

    for ptr in ("x", "u", "cx", "a", "b", "cov", "mean", "ws"):
        assert call(**{ptr: None}) == -1 and b"null" in lib.txm_last_error(), ptr
    assert call(N=0) == -1
    assert call(C=0) == -1
    assert call(C=70000, ls=70000) == -1 and b"65535" in lib.txm_last_error()
    assert call(nf=10) == -1 and b"n_f" in lib.txm_last_error()
    assert call(nf=0) == -1 and b"n_f" in lib.txm_last_error()
    assert call(nq=0) == -1 and b"n_q" in lib.txm_last_error()
    assert call(nq=10) == -1 and b"n_q" in lib.txm_last_error()
    assert call(ls=3) == -1 and b"pitch" in lib.txm_last_error()
    assert call(cu=float("nan")) == -1 and b"NaN" in lib.txm_last_error()
    assert call(block=0) == -1 and b"block" in lib.txm_last_error()
    assert call(block=-4) == -1 and b"block" in lib.txm_last_error()
    assert call(nl=0) == -1 and b"n_levels" in lib.txm_last_error()
    assert call(nl=33) == -1 and b"n_levels" in lib.txm_last_error()
    need = lib.txm_influence_block_cov_ws_bytes(10, 4, 3, 3, 2)
    assert call(wsb=need - 1) == -3 and b"workspace" in lib.txm_last_error()


@pytest.mark.parametrize("N,block", [(1000, 7), (1024, 1), (1025, 1), (331, 7), (320, 5), (9, 1), (2, 1), (100, 50), (10**8, 1024),
                                     (2**40, 3)])
def test_block_levels_bookkeeping(N, block):
    """engine.block_levels: lengths block 2^l, counts ceil(N / length) -- the short last block counts -- while a level has
    at least two blocks, at most 32 levels; N no multiple of block 2^l."""
    from thermoextrap_amd import engine

    lengths, counts = engine.block_levels(N, block)
    assert lengths.dtype == counts.dtype == np.int64 and 1 <= len(lengths) == len(counts) <= 32
    for l, (b, nb) in enumerate(zip(lengths, counts)):
        assert b == block * 2**l and nb == -(-N // int(b)) and nb >= 2
        assert (nb - 1) * b < N <= nb * b                              # nb - 1 full blocks and a last one of 1 .. b rows
    assert len(lengths) == 32 or -(-N // (block * 2 ** len(lengths))) == 1          # the next level would be a single block
    # level l merges the pairs of level l - 1; an odd count leaves the last block unpaired
    for l in range(1, len(counts)):
        assert counts[l] == (counts[l - 1] + 1) // 2


def test_block_levels_refuses_fewer_than_two_blocks():
    from thermoextrap_amd import engine

    for N, block in [(10, 0), (10, -1), (10, 6), (10, 10), (1, 1), (3, 2)]:
        with pytest.raises(ValueError):
            engine.block_levels(N, block)
    assert list(engine.block_levels(10, 5)[1]) == [2]
