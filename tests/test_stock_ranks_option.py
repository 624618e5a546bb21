"""WPT_OPT_STOCK_RANKS (42) and the read-only WPT_OPT_STOCK_RING_BYTES (43)
through the C ABI with no session (no GPU): 42 is a default of later inits,
43 cannot be set and reads 0 while no session holds a ring."""
import ctypes

STOCK_RANKS, RING_BYTES, DEFAULTS = 42, 43, 0


def _get(L, opt):
    v = ctypes.c_int64(-1)
    assert L.wpt_get_option(opt, ctypes.addressof(v)) == 0
    return v.value


def test_stock_ranks_is_a_sessionless_default(wpt):
    L = wpt.lib()
    itf = wpt.interface
    assert itf.OPTIONS["stock_ranks"] == STOCK_RANKS and itf.OPTIONS["stock_ring_bytes"] == RING_BYTES
    assert L.wpt_set_option(DEFAULTS, 0) == 0
    try:
        built_in = _get(L, STOCK_RANKS)
        assert built_in in (0, 1)
        for v in (1 - built_in, built_in, 1 - built_in):
            assert L.wpt_set_option(STOCK_RANKS, v) == 0
            assert _get(L, STOCK_RANKS) == v
            assert itf.get_option("stock_ranks") == v
        assert L.wpt_set_option(DEFAULTS, 0) == 0
        assert _get(L, STOCK_RANKS) == built_in
    finally:
        L.wpt_set_option(DEFAULTS, 0)


def test_stock_ranks_rejects_other_values(wpt):
    L = wpt.lib()
    itf = wpt.interface
    try:
        before = _get(L, STOCK_RANKS)
        for v in (2, -1):
            assert L.wpt_set_option(STOCK_RANKS, v) == itf.ERR_INVALID_ARG
        assert _get(L, STOCK_RANKS) == before
    finally:
        L.wpt_set_option(DEFAULTS, 0)


def test_ring_bytes_is_read_only(wpt):
    L = wpt.lib()
    itf = wpt.interface
    try:
        for v in (0, 1, 1 << 20):
            assert L.wpt_set_option(RING_BYTES, v) == itf.ERR_INVALID_ARG
        assert _get(L, RING_BYTES) == 0  # no session, no ring
    finally:
        L.wpt_set_option(DEFAULTS, 0)
