"""Adaptive round planner on the device: the production kernels and host walk
of Renderer::estimate_errors / plan_counts through the wpt_adaptive_error and
wpt_adaptive_plan hooks, and sessions that reach the same branches, against the
oracle's two stages bit for bit, on the frames and plan inputs of
adaptive_fixtures.py (their conditions: test_adaptive_cpu.py).

A NaN compares equal to a NaN (IEEE 754 leaves an invalid operation's sign and
payload to the implementation), though no frame here produces a NaN error.
"""
import ctypes
import functools

import numpy as np
import pytest

import adaptive_fixtures as fx

pytestmark = pytest.mark.gpu

SEED = 0xBABABEBE
SKY_CAM = (-0.9, 5.4, 0.4, -0.6, 3.14159)  # scene 101 from its camera's place, turned away and up: background only


@pytest.fixture
def itf(wpt):
    i = wpt.interface
    yield i
    try:
        i.shutdown()
    except i.WptError:
        pass
    i.set_option("defaults", 0)


def _start(itf, wpt, W=32, H=24, cam=None, types=(1, 1), adaptive=(1, 1), depth=2, lanes=None, stock=None):
    if stock is not None:
        itf.set_option("stock", stock)  # the default of the init below
    itf.init(W, H, 101, *(cam or wpt.scenes.scene_camera(101)))
    itf.update_settings(types[0], types[1], adaptive[0], adaptive[1], 0)
    itf.set_render_options(depth, SEED, 0)
    if lanes is not None:
        itf.set_lanes(lanes)


def _bits(a):
    a = np.ascontiguousarray(a, np.float32)
    b = a.view(np.uint32).copy()
    b[np.isnan(a)] = 0x7FC00000
    return b


def _assert_same(got, want, what, field, as_float=False):
    """Equal arrays, or the first differing element by its index."""
    g, w = (np.asarray(got), np.asarray(want))
    assert g.shape == w.shape, f"{what}: {field} shape {g.shape} != {w.shape}"
    gb, wb = (_bits(g), _bits(w)) if as_float else (g, w)
    if np.array_equal(gb, wb):
        return
    bad = np.argwhere(gb != wb)
    at = tuple(bad[0])
    raise AssertionError(f"{what}: {field} differs on {len(bad)} of {g.size} entries, first at {at}: "
                         f"{g[at]!r} != {w[at]!r}")


@functools.lru_cache(maxsize=None)
def _oracle_error(size, name, half):
    import pyoracle
    f = fx.frames(*size)[name]
    return pyoracle.adaptive_error(f.acc, f.cnt, half)


def _oracle_plan(c):
    import pyoracle
    return pyoracle.adaptive_plan(c.W, c.H, c.half, c.mse, c.stats, c.cnt, c.samp, c.first, c.adaptive)


def _check_plan(itf, c, what):
    got = itf.adaptive_plan(c.W, c.H, c.half, c.mse, c.stats, c.cnt, c.samp, c.first, c.adaptive)
    want = _oracle_plan(c)
    for field, g, w in zip(("count", "offset", "base", "view"), got, want):
        _assert_same(g, w, what, field)
    x0, x1 = fx.half_span(c.W, c.half)
    _assert_same(np.delete(got[3], np.s_[x0:x1], axis=1), np.delete(c.samp, np.s_[x0:x1], axis=1), what,
                 "the other half's view")
    assert got[1][-1] == got[0].sum(dtype=np.uint64)
    return got


# ---------------------------------------------------------------------------
# The hooks
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("size", fx.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_error_stage(wpt, itf, size):
    """Every frame of the size, both halves: the error bits and {sum, min,
    max} out of k_mse_tiled / k_mm_reduce / the k_sum_* chain and the host walk
    equal the oracle's. On the large frame (1025 tiles and 513 sum chunks per
    half) the walk's chunk count shows in wpt_stats."""
    _start(itf, wpt)
    chunks0 = itf.stats()["sum_chunks"]
    n_err = 0
    for name, f in fx.frames(*size).items():
        for half in (0, 1):
            mse, st = itf.adaptive_error(f.acc, f.cnt, half)
            want_mse, want_st = _oracle_error(size, name, half)
            what = f"{size[0]}x{size[1]} {name} half {half}"
            _assert_same(mse, want_mse, what, "error", as_float=True)
            _assert_same(st, want_st, what, "stats {sum, min, max}", as_float=True)
            n_err += mse.size
    chunks = itf.stats()["sum_chunks"] - chunks0
    print(f"{size}: {len(fx.frames(*size))} frames, {n_err} errors compared, sum chunks {chunks}")
    assert chunks > 0
    if size == fx.LARGE:
        assert chunks == 513 * 2 * len(fx.frames(*size))


@pytest.mark.parametrize("name", list(fx.plan_cases()))
def test_plan_stage(wpt, itf, name):
    """Every plan input: the counts, their offsets with the sentinel, the base
    counts and the view's bytes over the whole frame out of k_plan_round and the
    scan kernels equal the oracle's; the other half's view is as passed in."""
    _start(itf, wpt)
    _check_plan(itf, fx.plan_cases()[name], name)


@pytest.mark.parametrize("size,name", [((40, 24), "noise"), ((40, 24), "special"), ((62, 35), "noise"),
                                       ((33, 17), "special"), ((5, 3), "special"), (fx.LARGE, "noise"),
                                       (fx.LARGE, "special"), (fx.LARGE, "binades"), (fx.LARGE, "grey"),
                                       (fx.LARGE, "last_tile")],
                         ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}")
def test_both_stages_chained(wpt, itf, size, name):
    """wpt_adaptive_plan fed from wpt_adaptive_error on the device against the
    oracle chained the same way: on the large frame the scan's block sums go
    round k_scan_sums' loop three times (513 blocks)."""
    _start(itf, wpt)
    W, H = size
    f = fx.frames(W, H)[name]
    samp = np.random.default_rng(7).integers(0, 256, (H, W, 4), dtype=np.uint16).astype(np.uint8)
    samp[..., 3] = 255
    for half in (0, 1):
        mse, st = itf.adaptive_error(f.acc, f.cnt, half)
        c = fx.PlanCase(f"{W}x{H} {name} half {half} chained", W, H, half, mse, st, f.cnt, samp, False, True)
        want_mse, want_st = _oracle_error(size, name, half)
        want = _oracle_plan(c._replace(mse=want_mse, stats=want_st))
        got = itf.adaptive_plan(W, H, half, mse, st, f.cnt, samp)
        for field, g, w in zip(("count", "offset", "base", "view"), got, want):
            _assert_same(g, w, c.name, field)
        samp = got[3]  # the next half paints into this one's view, as a session's halves do


def test_hook_argument_errors(wpt, itf):
    """Null pointers, half > 1, W * H == 0 and a frame of 2^32 pixels are
    WPT_ERR_INVALID_ARG (nothing is read); an empty half (W == 1, left) returns
    no errors, the folds' start values and a plan of zeros."""
    _start(itf, wpt)
    L = wpt.lib()
    a = np.zeros(12, np.float32)
    c = np.ones(4, np.uint32)
    o = np.zeros(16, np.uint32)
    s = np.zeros(3, np.float32)
    v = np.zeros(16, np.uint8)
    P = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    bad = itf.ERR_INVALID_ARG
    assert L.wpt_adaptive_error(2, 2, P(a), P(c), 2, P(a), P(s)) == bad
    assert L.wpt_adaptive_error(0, 2, P(a), P(c), 0, P(a), P(s)) == bad
    assert L.wpt_adaptive_error(2, 0, P(a), P(c), 0, P(a), P(s)) == bad
    assert L.wpt_adaptive_error(65536, 65536, P(a), P(c), 0, P(a), P(s)) == bad
    for k in range(4):
        args = [P(a), P(c), P(a), P(s)]
        args[k] = None
        assert L.wpt_adaptive_error(2, 2, args[0], args[1], 0, args[2], args[3]) == bad
    assert L.wpt_adaptive_plan(2, 2, 2, 0, 1, P(a), P(s), P(c), P(o), P(o), P(o), P(v)) == bad
    assert L.wpt_adaptive_plan(0, 2, 0, 0, 1, P(a), P(s), P(c), P(o), P(o), P(o), P(v)) == bad
    assert L.wpt_adaptive_plan(65536, 65536, 0, 0, 1, P(a), P(s), P(c), P(o), P(o), P(o), P(v)) == bad
    for k in range(7):
        args = [P(a), P(s), P(c), P(o), P(o), P(o), P(v)]
        args[k] = None
        assert L.wpt_adaptive_plan(2, 2, 0, 0, 1, *args) == bad
    # W == 1: the left half is empty
    acc = np.full((4, 1, 3), 0.5, np.float32)
    cnt = np.ones((4, 1), np.uint32)
    mse, st = itf.adaptive_error(acc, cnt, 0)
    assert mse.shape == (4, 0) and st.tolist() == [0.0, np.inf, -np.inf]
    got = _check_plan(itf, fx.plan_cases()["empty_half"], "empty_half")
    assert not got[0].any() and not got[1].any()
    mse, st = itf.adaptive_error(acc, cnt, 1)
    _assert_same(mse, np.zeros((4, 1), np.float32), "1x4 right half", "error", as_float=True)


# ---------------------------------------------------------------------------
# Sessions
# ---------------------------------------------------------------------------
def _compare_session(itf, ref, W, H, what):
    acc_g, cnt_g = itf.read_radiance(W, H)
    acc_r, cnt_r, samp_r = ref.read()
    _assert_same(cnt_g, cnt_r, what, "sample count")
    _assert_same(acc_g, acc_r, what, "radiance", as_float=True)
    _assert_same(itf.results(1, W, H), samp_r, what, "sampling view")
    return cnt_g, samp_r


def test_session_uniform_frame(wpt, itf, oracle):
    """A camera turned to the empty sky, both halves adaptive: every error is
    0, so avg = 0, m < avg is false, scaled = 0.5 + 0.5 (0 / 0) = NaN,
    fminf(NaN, 1) = 1 and round 1 gives every pixel 33 samples and a black
    view (mn == mx); three rounds equal the oracle's."""
    W, H, depth = 40, 24, 2
    _start(itf, wpt, W, H, SKY_CAM, depth=depth)
    ref = oracle.OracleScene(101).adaptive(W, H, SKY_CAM, (1, 1), (1, 1), depth)
    view0 = itf.results(1, W, H)
    assert np.all(view0[..., 2] == 255) and not view0[..., :2].any()  # blue after the reset
    for rounds, spp in ((1, 4), (2, 37), (3, 70)):
        n = W * H * (spp if rounds == 1 else 33)
        itf.compute(n)
        ref.compute(n)
        cnt, view = _compare_session(itf, ref, W, H, f"sky, after round {rounds - 1}")
        assert np.all(cnt == spp)
        acc, _ = itf.read_radiance(W, H)
        assert not acc.any()
        if rounds >= 2:
            assert not view[..., :3].any() and np.all(view[..., 3] == 255)
    assert itf.stats()["sum_chunks"] == 2 * 2  # two estimates per half, 480 errors each


@pytest.mark.parametrize("stock", [0, 256])
@pytest.mark.parametrize("lanes", [1, 4])
def test_session_ragged_viewport(wpt, itf, oracle, lanes, stock):
    """Scene 101 at 37 x 19 (halves of 18 and 19 columns, two tile rows, the
    second three pixels high), both halves adaptive, chunks that cut three
    rounds and more at arbitrary points; 1 and 4 lanes, the stock on and off."""
    W, H, depth = 37, 19, 2
    cam = wpt.scenes.scene_camera(101)
    _start(itf, wpt, W, H, cam, depth=depth, lanes=lanes, stock=stock)
    ref = oracle.OracleScene(101).adaptive(W, H, cam, (1, 1), (1, 1), depth)
    for n in (W * H * 4 + 101, 9000, 211, 15000):
        itf.compute(n)
        ref.compute(n)
    cnt, _ = _compare_session(itf, ref, W, H, f"37x19 lanes {lanes} stock {stock}")
    assert cnt.max() > 8 and itf.stats()["sum_chunks"] >= 4
    if stock:
        assert itf.stats()["stock_consumed"] > 0


def test_session_below_the_stencil(wpt, itf, oracle):
    """Scene 101 at 5 x 3: every tap row and column leaves the viewport."""
    W, H, depth = 5, 3, 2
    cam = wpt.scenes.scene_camera(101)
    _start(itf, wpt, W, H, cam, depth=depth)
    ref = oracle.OracleScene(101).adaptive(W, H, cam, (1, 1), (1, 1), depth)
    for n in (W * H * 4 + 7, 300, 500):
        itf.compute(n)
        ref.compute(n)
    cnt, _ = _compare_session(itf, ref, W, H, "5x3")
    assert cnt.max() > 8


def test_hooks_leave_the_session_alone(wpt, itf, oracle):
    """Hook calls in the middle of a session (a frame of another size, both
    stages, between compute calls that cut rounds): the session's frame and
    view are untouched and its next rounds still equal the oracle's."""
    W, H, depth = 40, 24, 2
    cam = wpt.scenes.scene_camera(101)
    _start(itf, wpt, W, H, cam, depth=depth)
    ref = oracle.OracleScene(101).adaptive(W, H, cam, (1, 1), (1, 1), depth)
    c = fx.plan_cases()["all_counts_h1"]
    f = fx.frames(62, 35)["special"]
    for n in (W * H * 4 + 333, 7000, 9000):
        itf.compute(n)
        ref.compute(n)
        before = itf.read_radiance(W, H), itf.results(1, W, H)
        for half in (0, 1):
            mse, st = itf.adaptive_error(f.acc, f.cnt, half)
            _assert_same(mse, _oracle_error((62, 35), "special", half)[0], "mid-session", "error", as_float=True)
        _check_plan(itf, c, "mid-session all_counts_h1")
        after = itf.read_radiance(W, H), itf.results(1, W, H)
        _assert_same(after[0][0], before[0][0], "after the hooks", "radiance", as_float=True)
        _assert_same(after[0][1], before[0][1], "after the hooks", "sample count")
        _assert_same(after[1], before[1], "after the hooks", "sampling view")
    cnt, _ = _compare_session(itf, ref, W, H, "session with hook calls")
    assert cnt.max() > 8
