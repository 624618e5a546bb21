"""The a-trous filter's kernels against wpt_denoise_host, bit for bit
(tests/test_denoise_cpu.py holds wpt_denoise_host against a numpy restatement
of the definition on the same frames).

wpt_denoise_planes runs the kernels on the frames of tests/denoise_fixtures.py
at the viewports where a tile can go wrong, with the LDS kernels and with the
direct ones (WPT_OPT_DENOISE_LDS). wpt_denoise runs them on sessions: its result
is wpt_denoise_host of read_radiance() and first_hit(sample)'s planes, it leaves
the session untouched, and on scene 100 the filtered 4-spp frame is nearer the
1024-spp frame than the raw one.
"""
import ctypes

import numpy as np
import pytest

import denoise_fixtures as fx
import first_hit_fixtures as fh

pytestmark = pytest.mark.gpu

# wpt_stats words that no two runs agree on (tests/test_gpu_first_hit.py)
CLOCK_STATS = ("plan_us", "stock_us", "stock_waits")
GUIDES = ("t", "normal", "albedo", "kind")
SPP = 4


@pytest.fixture
def itf(wpt):
    i = wpt.interface
    yield i
    try:
        i.shutdown()
    except i.WptError:
        pass
    i.set_option("defaults", 0)


def _start(itf, c, vp, settings=(1, 1, 0, 0), depth=4):
    itf.init(vp[0], vp[1], c.scene_id, *c.cam)
    if c.mesh is not None:
        assert itf.store_mesh(1, c.mesh)
    if settings is not None:
        itf.update_settings(*settings, 0)
    itf.set_render_options(depth, fh.SEED, 0)


def _host_of_session(itf, vp, sample, **kw):
    acc, cnt = itf.read_radiance(*vp)
    g = itf.first_hit(sample, planes=GUIDES)
    return itf.denoise_host(acc, cnt, g["t"], g["normal"], g["albedo"], g["kind"], **kw)


@pytest.mark.parametrize("vp", fx.GPU_VIEWPORTS, ids=lambda v: f"{v[0]}x{v[1]}")
def test_planes_against_the_host(wpt, oracle, itf, vp):
    """1..5 iterations (steps 8 and 16 always read global memory), both flag
    values, steps 1, 2, 4 through LDS and direct."""
    c = fh.case(wpt, oracle, "box")
    f = fx.shared_frame(*vp)
    _start(itf, c, (8, 8))
    for it in range(1, 6):
        for flags in (0, fx.ALBEDO):
            kw = dict(iterations=it, sigma_c=float(fx.SIGMA_C), sigma_z=float(fx.SIGMA_Z), flags=flags)
            want = itf.denoise_host(*f, **kw)
            for lds in (7, 0, 5):
                itf.set_option("denoise_lds", lds)
                fx.same(itf.denoise_planes(*f, **kw), want, (vp, it, flags, lds))
    # the sigma pair at which the denormal depths give 0 / 0
    kw = dict(iterations=5, sigma_c=0.37, sigma_z=1e-5, flags=fx.ALBEDO)
    itf.set_option("denoise_lds", 7)
    fx.same(itf.denoise_planes(*f, **kw), itf.denoise_host(*f, **kw), (vp, "small sigma_z"))


def test_option_and_arguments(wpt, oracle, itf):
    L = wpt.lib()
    f = [np.ascontiguousarray(a) for a in fx.shared_frame(17, 16)]
    ptr = [a.ctypes.data for a in f]
    out = [np.zeros((16, 17, 3), np.float32), np.zeros((16, 17), np.uint8), np.zeros((16, 17, 4), np.uint8)]
    optr = [a.ctypes.data for a in out]
    one, tenth = ctypes.c_float(1.0), ctypes.c_float(0.1)
    # both device entry points need a session
    assert L.wpt_denoise(0, 3, one, tenth, 0, *optr) == -1
    assert L.wpt_denoise_planes(17, 16, *ptr, 3, one, tenth, 0, *optr) == -1
    assert itf.get_option("denoise_lds") == 7
    c = fh.case(wpt, oracle, "box")
    _start(itf, c, (17, 16))
    for bad in (-1, 8):
        with pytest.raises(itf.WptError):
            itf.set_option("denoise_lds", bad)
    INVALID = -4
    for fn, head in ((L.wpt_denoise, (0,)), (L.wpt_denoise_planes, (17, 16, *ptr))):
        assert fn(*head, 3, one, tenth, 0, *optr) == 0
        assert fn(*head, 3, one, tenth, 0, None, None, None) == 0
        assert fn(*head, 0, one, tenth, 0, *optr) == INVALID and fn(*head, 6, one, tenth, 0, *optr) == INVALID
        for s in (0.0, -1.0, float("inf"), float("nan")):
            assert fn(*head, 3, ctypes.c_float(s), tenth, 0, *optr) == INVALID
            assert fn(*head, 3, one, ctypes.c_float(s), 0, *optr) == INVALID
        assert fn(*head, 3, one, tenth, 2, *optr) == INVALID
    for k in range(6):
        assert L.wpt_denoise_planes(17, 16, *ptr[:k], None, *ptr[k + 1:], 3, one, tenth, 0, *optr) == INVALID
    assert L.wpt_denoise_planes(0, 16, *ptr, 3, one, tenth, 0, *optr) == INVALID
    assert L.wpt_denoise_planes(65536, 65536, *ptr, 3, one, tenth, 0, *optr) == INVALID
    # an output not asked for is not written; the others are the full call's
    itf.compute(17 * 16 * SPP)
    full = itf.denoise(7)
    for k in range(3):
        bufs = [np.full_like(a, 0xA5) if a.dtype == np.uint8 else np.full_like(a, np.float32(-7.0)) for a in out]
        p = [b.ctypes.data if j == k else None for j, b in enumerate(bufs)]
        d = itf.DENOISE_DEFAULTS
        assert L.wpt_denoise(7, d["iterations"], ctypes.c_float(d["sigma_c"]), ctypes.c_float(d["sigma_z"]),
                             d["flags"], *p) == 0
        assert np.array_equal(fx.bits(bufs[k]), fx.bits(full[k]))


@pytest.mark.parametrize("name,vp", [("default", (fh.W, fh.H)), ("museum", (fh.W, fh.H)), ("box", (fh.W, fh.H)),
                                     ("spheres", (fh.W, fh.H)), ("ragged", (37, 5))])
def test_sessions_against_the_host(wpt, oracle, itf, name, vp):
    """NEE, depth 4, 4 spp; samples 0 and 7: wpt_denoise = the host restatement
    on the frame and the first-hit planes the session gives."""
    c = fh.case(wpt, oracle, name)
    _start(itf, c, vp)
    itf.compute(vp[0] * vp[1] * SPP)
    kinds = set()
    for sample in fh.SAMPLES:
        for kw in (dict(), dict(iterations=5, sigma_c=0.5, sigma_z=0.05, flags=0)):
            got = itf.denoise(sample, **kw)
            want = _host_of_session(itf, vp, sample, **kw)
            fx.same(got, want, (name, sample, kw))
            assert got[0].shape == (vp[1], vp[0], 3) and np.all(got[1] == 1)
        kinds |= set(np.unique(itf.first_hit(sample, planes=("kind",))["kind"]))
    print(name, "kinds", sorted(kinds))
    # the filter did something
    acc, cnt = itf.read_radiance(*vp)
    assert not np.array_equal(got[0], acc / cnt[..., None].astype(np.float32))


def test_partition(wpt, oracle, itf):
    """Rank 0 of 2 with tile 8: the other rank's pixels have no samples."""
    c = fh.case(wpt, oracle, "default")
    vp = (fh.W, fh.H)
    _start(itf, c, vp)
    itf.set_partition(0, 2, 8)
    mine = np.zeros(vp[0] * vp[1], bool)
    mine[itf.partition_pixels()] = True
    mine = mine.reshape(vp[1], vp[0])
    assert 0 < mine.sum() < mine.size
    itf.compute(int(mine.sum()) * SPP)
    rgb, valid, rgba = got = itf.denoise(7)
    assert np.array_equal(valid.astype(bool), mine)
    assert np.all(fx.bits(rgb)[~mine] == 0) and np.all(rgba[~mine] == (0, 0, 0, 255))
    fx.same(got, _host_of_session(itf, vp, 7), "rank 0 of 2")


def _snapshot(itf, vp):
    acc, cnt = itf.read_radiance(*vp)
    st = itf.stats()
    return acc, cnt, itf.results(1, *vp), {k: v for k, v in st.items() if k not in CLOCK_STATS}, itf.kernel_times()


@pytest.mark.parametrize("session", ["nee", "init_default"])
def test_session_untouched(wpt, oracle, itf, session):
    """The frame, the counts, the sampling view, wpt_stats and wpt_kernel_times
    are the same before and after a call, and compute(n), denoise, compute(n)
    ends where compute(n), compute(n) does: on a plain NEE session and on the
    init-default one (adaptive right half, sample stock with refills in flight)."""
    c = fh.case(wpt, oracle, "default")
    vp = (fh.W, fh.H)
    n = vp[0] * vp[1] * 3 + 17
    kw = {"settings": (1, 1, 0, 0), "depth": 4} if session == "nee" else {"settings": None, "depth": 0}
    ends = []
    for middle in (True, False):
        _start(itf, c, vp, **kw)
        wpt.lib().wpt_set_profiling(1)
        itf.compute(n)
        if middle:
            before = _snapshot(itf, vp)
            got = itf.denoise(7)
            after = _snapshot(itf, vp)
            for a, b, what in zip(before[:3], after[:3], ("radiance", "counts", "sampling view")):
                assert np.array_equal(fx.bits(a), fx.bits(b)), what
            assert before[3] == after[3] and before[4] == after[4]
            fx.same(got, _host_of_session(itf, vp, 7), "mid-session")
        itf.compute(n)
        ends.append(_snapshot(itf, vp))
        itf.shutdown()
    (a1, c1, s1, st1, _), (a0, c0, s0, st0, _) = ends
    if session == "init_default":
        assert st0["stock_consumed"] > 0 and c0.max() > 3
    for a, b, what in ((a1, a0, "radiance"), (c1, c0, "counts"), (s1, s0, "sampling view")):
        assert np.array_equal(fx.bits(a), fx.bits(b)), what
    assert st1 == st0


def test_viewport_change(wpt, oracle, itf):
    """The scratch follows the viewport."""
    c = fh.case(wpt, oracle, "default")
    _start(itf, c, (fh.W, fh.H))
    itf.compute(fh.W * fh.H * SPP)
    itf.denoise(0)
    for vp in ((37, 5), (130, 70)):
        itf.update_viewport(*vp)
        itf.compute(vp[0] * vp[1] * SPP)
        fx.same(itf.denoise(0, iterations=5), _host_of_session(itf, vp, 0, iterations=5), vp)


def test_it_denoises(wpt, oracle, itf):
    """Scene 100 at 64 x 48, the documented defaults: the filtered 4-spp frame is
    nearer (relative L2) the 1024-spp frame of the same session type than the
    raw 4-spp frame is."""
    c = fh.case(wpt, oracle, "box")
    vp = (fh.W, fh.H)
    npx = vp[0] * vp[1]
    _start(itf, c, vp)
    itf.compute(npx * SPP)
    acc, cnt = itf.read_radiance(*vp)
    assert np.all(cnt == SPP)
    raw = acc / np.float32(SPP)
    rgb, valid, _ = itf.denoise(0)
    assert np.all(valid == 1)
    itf.compute(npx * (1024 - SPP))
    acc, cnt = itf.read_radiance(*vp)
    assert np.all(cnt == 1024)
    ref = acc / np.float32(1024)
    e_raw, e_dn = fx.rel_l2(raw, ref), fx.rel_l2(rgb, ref)
    print("relative L2 against 1024 spp: raw", e_raw, "denoised", e_dn)
    assert e_dn < e_raw
