"""wpt_sample_map_host against the Python-integer restatement of the definition
(tests/guided_fixtures.py), bit for bit, and the properties of the dealing.
No GPU: the host restatement calls the two functions the kernels call
(map_need, map_deal; wpt_guided.h)."""
import ctypes

import numpy as np
import pytest

import guided_fixtures as gx

INVALID = -4


@pytest.fixture(scope="module")
def itf(wpt):
    return wpt.interface


@pytest.mark.parametrize("mask", gx.MASKS)
@pytest.mark.parametrize("vp", gx.VIEWPORTS, ids=lambda v: f"{v[0]}x{v[1]}")
def test_host_against_python_integers(itf, vp, mask):
    """Every limit pair, both flag values and the budgets 0, 1, T - 1, T, T + 1
    and 2^32 - 1 of each: counts and totals equal; T >= 2^32 is refused."""
    cnt, ln, kind = gx.planes(*vp)
    member = gx.mask(itf, mask, *vp)
    seen_t, dealt, refused = set(), 0, 0
    for target, max_pp in gx.LIMITS:
        for flags in (0, gx.MISS_ONCE):
            _, T, _ = gx.reference(cnt, ln, kind, member, target, max_pp, 0, flags)
            seen_t.add(T)
            if T >= 2 ** 32:
                with pytest.raises(itf.WptError) as e:
                    itf.sample_map_host(cnt, ln, kind, member, target, max_pp, 0, flags)
                assert e.value.code == itf.ERR_INVALID_ARG
                refused += 1
                continue
            for budget in gx.budgets(T):
                want, wt, ws = gx.reference(cnt, ln, kind, member, target, max_pp, budget, flags)
                got = itf.sample_map_host(cnt, ln, kind, member, target, max_pp, budget, flags)
                gx.same(got, (np.array(want, np.uint32).reshape(cnt.shape), (wt, ws)), (vp, mask, target, max_pp, flags, budget))
                dealt += 0 < budget < T
    if mask == "none":
        assert seen_t == {0}
    else:
        assert dealt > 0
    if mask == "all" and vp[0] * vp[1] > 16:
        assert refused > 0


@pytest.mark.parametrize("vp", gx.VIEWPORTS[1:], ids=lambda v: f"{v[0]}x{v[1]}")
def test_dealing_properties(itf, vp):
    """sum count == budget, count <= need, count == 0 where need == 0."""
    cnt, ln, kind = gx.planes(*vp)
    member = gx.mask(itf, "all", *vp)
    for max_pp in (1, 3, gx.M32):
        need, (T, s) = itf.sample_map_host(cnt, ln, kind, member, gx.TARGET, max_pp, 0, 0)
        assert s == T == int(need.astype(np.uint64).sum()) and T > 1
        for budget in (1, T // 3, T // 2 + 1, T - 1):
            if not 0 < budget < T:
                continue
            count, (t2, s2) = itf.sample_map_host(cnt, ln, kind, member, gx.TARGET, max_pp, budget, 0)
            assert t2 == T and s2 == budget == int(count.astype(np.uint64).sum())
            assert np.all(count <= need) and not count[need == 0].any()


def test_need_rule(itf):
    """The rule on hand-made pixels: the saturation of cnt + len, the cap, the
    membership and WPT_MAP_MISS_ONCE."""
    M = gx.M32
    cnt = np.array([[0, 7, 8, 9, M, 5, 0, 3, 0, 2]], np.uint32)
    ln = np.array([[0, 0, 0, 0, 1, M - 3, 3, 0, 0, 0]], np.uint32)
    kind = np.array([[1, 1, 2, 1, 1, 1, 1, 1, 0, 0]], np.uint8)
    member = np.array([[1, 1, 1, 1, 1, 1, 1, 0, 1, 1]], np.uint8)
    count, tot = itf.sample_map_host(cnt, ln, kind, member, 8, M, 0, 0)
    assert count.tolist() == [[8, 1, 0, 0, 0, 0, 5, 0, 8, 6]] and tot == (28, 28)
    count, tot = itf.sample_map_host(cnt, ln, kind, member, 8, 2, 0, 0)
    assert count.tolist() == [[2, 1, 0, 0, 0, 0, 2, 0, 2, 2]] and tot == (9, 9)
    count, tot = itf.sample_map_host(cnt, ln, kind, member, 8, M, 0, gx.MISS_ONCE)
    assert count.tolist() == [[8, 1, 0, 0, 0, 0, 5, 0, 1, 0]] and tot == (15, 15)
    # the example of the equal-budget argument: half 1-sample, half 16-sample pixels
    cnt = np.array([[1] * 4 + [16] * 4], np.uint32)
    z = np.zeros((1, 8), np.uint32)
    count, tot = itf.sample_map_host(cnt, z, np.ones((1, 8), np.uint8), np.ones((1, 8), np.uint8), 16, M, 16, 0)
    assert count.tolist() == [[4, 4, 4, 4, 0, 0, 0, 0]] and tot == (60, 16)


def test_zero_and_overflow(itf):
    """T == 0 gives a map of zeros for every budget; T == 2^32 - 1 is the largest
    accepted, 2^32 is refused."""
    M = gx.M32
    one = np.ones((1, 2), np.uint8)
    z = np.zeros((1, 2), np.uint32)
    full = np.full((1, 2), 9, np.uint32)
    for budget in (0, 1, M):
        count, tot = itf.sample_map_host(full, z, one, one, 8, M, budget, 0)
        assert not count.any() and tot == (0, 0)
    cnt = np.array([[0, M - 1]], np.uint32)  # needs M and 1: T = 2^32
    with pytest.raises(itf.WptError) as e:
        itf.sample_map_host(cnt, z, one, one, M, M, 0, 0)
    assert e.value.code == itf.ERR_INVALID_ARG
    cnt = np.array([[1, M - 1]], np.uint32)  # needs M - 1 and 1: T = 2^32 - 1
    count, tot = itf.sample_map_host(cnt, z, one, one, M, M, 0, 0)
    assert count.tolist() == [[M - 1, 1]] and tot == (M, M)
    count, tot = itf.sample_map_host(cnt, z, one, one, M, M, M - 1, 0)  # products near 2^64
    assert count.tolist() == [[(M - 1) * (M - 1) // M, (M - 1) - (M - 1) * (M - 1) // M]] and tot == (M, M - 1)


def test_arguments(wpt, itf):
    L = wpt.lib()
    cnt, ln, kind = gx.planes(17, 16)
    member = np.ones((16, 17), np.uint8)
    ptr = [np.ascontiguousarray(a).ctypes.data for a in (cnt, ln, kind, member)]
    out = np.zeros((16, 17), np.uint32)
    tot = np.zeros(2, np.uint64)
    assert L.wpt_sample_map_host(17, 16, *ptr, 8, 8, 0, 0, out.ctypes.data, tot.ctypes.data) == 0
    assert L.wpt_sample_map_host(17, 16, *ptr, 8, 8, 0, 0, None, None) == 0
    assert L.wpt_sample_map_host(17, 16, *ptr, 0, 8, 0, 0, out.ctypes.data, tot.ctypes.data) == INVALID
    assert L.wpt_sample_map_host(17, 16, *ptr, 8, 0, 0, 0, out.ctypes.data, tot.ctypes.data) == INVALID
    assert L.wpt_sample_map_host(17, 16, *ptr, 8, 8, 0, 2, out.ctypes.data, tot.ctypes.data) == INVALID
    assert b"unknown flag" in L.wpt_last_error()
    for k in range(4):
        assert L.wpt_sample_map_host(17, 16, *ptr[:k], None, *ptr[k + 1:], 8, 8, 0, 0, out.ctypes.data,
                                     tot.ctypes.data) == INVALID
    assert L.wpt_sample_map_host(0, 16, *ptr, 8, 8, 0, 0, out.ctypes.data, tot.ctypes.data) == INVALID
    assert L.wpt_sample_map_host(65536, 65536, *ptr, 8, 8, 0, 0, out.ctypes.data, tot.ctypes.data) == INVALID
    # the session calls need a session
    assert L.wpt_compute_map(None) == -1
    assert L.wpt_sample_map(0, 8, 8, 0, 0, None, None) == -1
    assert L.wpt_sample_map_planes(17, 16, *ptr, 8, 8, 0, 0, out.ctypes.data, tot.ctypes.data) == -1
    assert itf.OPTIONS["map_mode"] == 47 and itf.MAP_MISS_ONCE == 1
    assert ctypes.sizeof(ctypes.c_uint64) * 2 == tot.nbytes
