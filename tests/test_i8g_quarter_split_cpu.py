"""The rule that deals the replicate quarters of a two-row-set table pass out over six-quarter and four-quarter workgroups
(g_quarter_split in txm_resample_i8g.hip, exported host-only as txm_i8g_quarter_split): 6 n6 + 4 n4 >= Q with the fewest
padded quarters, ties to the larger n6 -- against a brute-force search, for every Q a call of up to 2048 replicates has."""

import ctypes as ct

import pytest


@pytest.fixture(scope="module")
def split():
    from thermoextrap_amd import _build, _lib

    _build.build_library()
    f = _lib.load().txm_i8g_quarter_split
    f.restype = None
    f.argtypes = [ct.c_int, ct.POINTER(ct.c_int), ct.POINTER(ct.c_int)]

    def call(Q):
        n6, n4 = ct.c_int(-1), ct.c_int(-1)
        f(Q, ct.byref(n6), ct.byref(n4))
        return n6.value, n4.value

    return call


def brute(Q):
    best = None
    for n6 in range(0, Q // 6 + 2):
        for n4 in range(0, Q // 4 + 2):
            if 6 * n6 + 4 * n4 >= Q and n6 + n4 > 0:
                key = (6 * n6 + 4 * n4 - Q, -n6, n4)
                if best is None or key < best[0]:
                    best = (key, (n6, n4))
    return best[1]


@pytest.mark.parametrize("Q", range(1, 65))
def test_split_is_the_brute_force_minimum(split, Q):
    n6, n4 = split(Q)
    assert n6 >= 0 and n4 >= 0 and 6 * n6 + 4 * n4 >= Q
    assert (n6, n4) == brute(Q)
    # six-quarter workgroups never pad more than four-quarter ones alone
    assert 6 * n6 + 4 * n4 - Q <= 4 * ((Q + 3) // 4) - Q


def test_named_cases(split):
    assert split(4) == (0, 1)      # nrep = 100
    assert split(6) == (1, 0)      # 192
    assert split(7) == (0, 2)      # 200: 4 + 4, not 6 + 4
    assert split(10) == (1, 1)     # 300
    assert split(11) == (2, 0)     # 330: the last group not full
    assert split(32) == (4, 2)     # 1000: the benchmark's call
    assert split(0) == (0, 0)
