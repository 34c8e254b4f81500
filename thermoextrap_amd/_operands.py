"""When may an (N, C) sample matrix go to libtxmom as it is, with which strides, and when must it be copied first?

The two rules of the C ABI (include/txmom.h), as pure functions of shape and strides (in elements): no tensor, no
library, no GPU.  ``copy`` means "hand the library a tight row-major copy"; the strides returned are then that copy's.
engine.py applies them (``engine._place``); tests/test_operands_cpu.py pins them.
"""

from __future__ import annotations


def resample_pitch_ok(ld: int, C: int) -> bool:
    """include/txmom.h TXM_RESAMPLE_PITCH_OK: the row pitch the bootstrap kernels' 32-bit offsets hold; anything else is copied
    to a tight array -- which for C > 698140 is itself refused by the library."""
    return 768 * int(ld) + int(C) <= 1 << 29


def rowmajor_layout(N: int, C: int, s0: int, s1: int, pitch_limit: bool = False) -> tuple[bool, int]:
    """(copy, ls) for the entry points that take (rec, val) row-major with a row pitch ls >= C and nothing else: transposed
    views, broadcast rows (stride 0) and overlapping pitches are copied -- and, with ``pitch_limit`` (the bootstrap kernels),
    a pitch that fails ``resample_pitch_ok``.  A single row has no pitch of its own."""
    if s1 != 1 or (N > 1 and (s0 < C or (pitch_limit and not resample_pitch_ok(s0, C)))):
        return True, C
    return False, (s0 if N > 1 else C)


def either_layout(N: int, C: int, s0: int, s1: int) -> tuple[bool, int, int]:
    """(copy, ls, lc) for the entry points that take either layout of reduce_vals: (rec, val) row-major with pitch ls, or
    (val, rec) -- a transposed view of a (C, N) array -- with every column contiguous along the samples, lc apart."""
    if C == 1:
        return True, 1, 1  # a single contiguous series
    if s1 == 1 and (N == 1 or s0 >= C):
        return False, (s0 if N > 1 else C), 1
    if s0 == 1 and s1 >= N:
        return False, 1, s1
    return True, C, 1
