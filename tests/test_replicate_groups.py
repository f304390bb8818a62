"""CPU tests of the grouping of replicate Michaelis-Menten experiments (csrc/replicate_groups.h through the C ABI,
smc_mm_group_replicates): two experiments share one integration when their S0 and all their data times are equal bit for bit."""
import ctypes

import numpy as np
import pytest


def _groups(pkg, t, S0):
    t = np.ascontiguousarray(t, dtype=np.float64)
    S0 = np.ascontiguousarray(S0, dtype=np.float64)
    n_ex, n_t = t.shape
    assert S0.shape == (n_ex,)
    primary = np.full(n_ex, -7, dtype=np.int32)
    partner = np.full(n_ex, -7, dtype=np.int32)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    n_solve = pkg.lib().smc_mm_group_replicates(t.ctypes.data_as(dp), S0.ctypes.data_as(dp), n_ex, n_t, primary.ctypes.data_as(ip),
                                                partner.ctypes.data_as(ip))
    assert 1 <= n_solve <= n_ex
    assert np.all(primary[n_solve:] == -1) and np.all(partner[n_solve:] == -1)      # unused entries
    return [(int(primary[g]), int(partner[g])) for g in range(n_solve)]


# three conditions: (S0, time row); the rows differ from each other in more than rounding
T = np.linspace(0.0, 30.0, 7)
COND = {"a": (2.0, T), "b": (0.5, T), "c": (2.0, T * 1.5)}


def _layout(names):
    return np.array([COND[k][1] for k in names]), np.array([COND[k][0] for k in names])


@pytest.mark.parametrize("names, expected", [
    ("aba", [(0, 2), (1, -1)]),
    ("aa", [(0, 1)]),
    ("aaa", [(0, 1), (2, -1)]),                              # pair + single
    ("ababccc", [(0, 2), (1, 3), (4, 5), (6, -1)]),
    ("abc", [(0, -1), (1, -1), (2, -1)]),                    # all distinct
    ("aaaaa", [(0, 1), (2, 3), (4, -1)]),                    # a, b, c, d, e of one condition: (a, b), (c, d), (e)
    ("a", [(0, -1)]),
])
def test_layouts(pkg, names, expected):
    t, S0 = _layout(names)
    assert _groups(pkg, t, S0) == expected


def test_golden_data_has_one_replicate_pair(pkg, data):
    g = _groups(pkg, data.t, data.S0)
    assert g == [(0, 5), (1, -1), (2, -1), (3, -1), (4, -1)]


def test_one_ulp_in_a_time_does_not_merge(pkg):
    t, S0 = _layout("aa")
    for k in (0, 3, t.shape[1] - 1):
        t2 = t.copy()
        t2[1, k] = np.nextafter(t2[1, k], np.inf)
        assert _groups(pkg, t2, S0) == [(0, -1), (1, -1)], k


def test_one_ulp_in_S0_does_not_merge(pkg):
    t, S0 = _layout("aa")
    S0[1] = np.nextafter(S0[1], 0.0)
    assert _groups(pkg, t, S0) == [(0, -1), (1, -1)]


def test_signed_zero_does_not_merge(pkg):
    t, S0 = _layout("aa")
    assert t[0, 0] == 0.0
    t[1, 0] = -0.0
    assert t[1, 0] == t[0, 0]                                # equal as numbers, different bits
    assert _groups(pkg, t, S0) == [(0, -1), (1, -1)]
    t, S0 = _layout("aa")
    S0[:] = [0.0, -0.0]
    assert _groups(pkg, t, S0) == [(0, -1), (1, -1)]


def test_single_time(pkg):
    t = np.array([[3.0], [3.0], [4.0], [3.0]])
    assert _groups(pkg, t, np.array([1.0, 1.0, 1.0, 2.0])) == [(0, 1), (2, -1), (3, -1)]


def test_bad_arguments_are_refused(pkg):
    t, S0 = _layout("aa")
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    out = np.zeros(2, dtype=np.int32)
    L = pkg.lib()
    assert L.smc_mm_group_replicates(t.ctypes.data_as(dp), S0.ctypes.data_as(dp), 0, 7, out.ctypes.data_as(ip), out.ctypes.data_as(ip)) == -1
    assert L.smc_mm_group_replicates(None, S0.ctypes.data_as(dp), 2, 7, out.ctypes.data_as(ip), out.ctypes.data_as(ip)) == -1
