"""k_reproject against wpt_reproject_host, bit for bit
(tests/test_reproject_cpu.py holds wpt_reproject_host against a numpy
restatement of the definition on the same frames).

wpt_reproject_planes runs the kernel on the frames of
tests/reproject_fixtures.py. wpt_reproject runs it on sessions that keep a
history and move the camera twice: every call is wpt_reproject_host of
read_radiance(), first_hit(sample) and the history as the test tracks it on the
host; wpt_denoise_merged is wpt_denoise_host of the call before it. The history
lives and dies as include/wpt.h says, the session is left untouched, and on
scene 100 the merged 4-spp frame is much nearer the 1024-spp frame than the raw
one.
"""
import ctypes

import numpy as np
import pytest

import denoise_fixtures as dn
import first_hit_fixtures as fh
import reproject_fixtures as fx

pytestmark = pytest.mark.gpu

# wpt_stats words that no two runs agree on (tests/test_gpu_first_hit.py)
CLOCK_STATS = ("plan_us", "stock_us", "stock_waits")
CUR = ("dir", "t", "id", "normal", "kind")
SPP = 4
INVALID = -4


@pytest.fixture
def itf(wpt):
    i = wpt.interface
    yield i
    try:
        i.shutdown()
    except i.WptError:
        pass
    i.set_option("defaults", 0)


def _start(itf, c, vp, settings=(1, 1, 0, 0), depth=4, cam=None):
    itf.init(vp[0], vp[1], c.scene_id, *(cam or c.cam))
    if c.mesh is not None:
        assert itf.store_mesh(1, c.mesh)
    if settings is not None:
        itf.update_settings(*settings, 0)
    itf.set_render_options(depth, fh.SEED, 0)


def _moved(cam, k):
    """The k-th camera of a session's walk."""
    step = ((0.0, 0.0, 0.0, 0.0, 0.0), (0.3, 0.1, 0.2, 0.05, -0.1), (-0.2, 0.05, 0.4, 0.02, 0.08))[k]
    return tuple(float(np.float32(a + b)) for a, b in zip(cam, step))


class Tracker:
    """The history as the host sees it: what reproject(KEEP) returned, the planes
    of its sample and its camera."""

    def __init__(self, itf, vp):
        self.itf, self.vp, self.cam, self.hist, self.pcam = itf, vp, None, None, None

    def current(self, sample):
        acc, cnt = self.itf.read_radiance(*self.vp)
        g = self.itf.first_hit(sample, planes=CUR)
        return [acc, cnt] + [g[k] for k in CUR]

    def expect(self, sample, flags=0, **kw):
        cur = self.current(sample)
        if self.hist is None:
            return (cur[0], cur[1], np.zeros(cur[1].shape, np.uint32)), cur
        return self.itf.reproject_host(self.cam, cur, self.pcam, self.hist, flags=flags & ~fx.KEEP, **kw), cur

    def call(self, sample, flags=0, what="", **kw):
        want, cur = self.expect(sample, flags, **kw)
        got = self.itf.reproject(sample, flags=flags, **kw)
        fx.same(got, want, (what, sample, flags, kw))
        if flags & fx.KEEP:
            self.hist = [got[0], got[1], cur[3], cur[4], cur[5], cur[6]]
            self.pcam = self.cam
        return got


@pytest.mark.parametrize("vp", fx.GPU_VIEWPORTS, ids=lambda v: f"{v[0]}x{v[1]}")
def test_planes_against_the_host(wpt, oracle, itf, vp):
    """Every camera pair and flag combination, the defaults and the extreme
    parameters, on frames that carry the edits."""
    c = fh.case(wpt, oracle, "box")
    _start(itf, c, (8, 8))
    kept = 0
    for pair in fx.PAIRS:
        cam, cur, pcam, hist, _ = fx.shared(wpt, oracle, *vp, pair)
        for flags in fx.FLAGS:
            for kw in (dict(), dict(max_len=1, cos_min=-1.0, eps_z=0.0), dict(max_len=1 << 24, cos_min=1.0, eps_z=0.5)):
                want = itf.reproject_host(cam, cur, pcam, hist, flags=flags, **kw)
                fx.same(itf.reproject_planes(cam, cur, pcam, hist, flags=flags, **kw), want, (vp, pair, flags, kw))
                kept += int((want[2] > 0).sum())
    assert kept > 0 or vp == (1, 1)


def test_arguments_and_outputs(wpt, oracle, itf):
    L = wpt.lib()
    cam, cur, pcam, hist, _ = fx.shared(wpt, oracle, 17, 16, "sideways")
    ins = [np.asarray(cam[:3], np.float32)] + [np.ascontiguousarray(a) for a in cur] + \
          [np.asarray(pcam, np.float32)] + [np.ascontiguousarray(a) for a in hist]
    ptr = [a.ctypes.data for a in ins]
    out = [np.zeros((16, 17, 3), np.float32), np.zeros((16, 17), np.uint32), np.zeros((16, 17), np.uint32)]
    optr = [a.ctypes.data for a in out]
    f = ctypes.c_float
    c = fh.case(wpt, oracle, "box")
    _start(itf, c, (17, 16))
    itf.compute(17 * 16 * SPP)
    for fn, head, keep_ok in ((L.wpt_reproject, (0,), True), (L.wpt_reproject_planes, (17, 16, *ptr), False)):
        assert fn(*head, f(0.9), f(0.05), 64, 0, *optr) == 0
        assert fn(*head, f(0.9), f(0.05), 64, 0, None, None, None) == 0
        for cm in (-1.5, 1.5, float("nan"), float("inf")):
            assert fn(*head, f(cm), f(0.05), 64, 0, *optr) == INVALID
        for ez in (-0.1, float("nan"), float("inf")):
            assert fn(*head, f(0.9), f(ez), 64, 0, *optr) == INVALID
        for ml in (0, (1 << 24) + 1):
            assert fn(*head, f(0.9), f(0.05), ml, 0, *optr) == INVALID
        assert fn(*head, f(0.9), f(0.05), 64, 8, *optr) == INVALID
        if not keep_ok:
            assert fn(*head, f(0.9), f(0.05), 64, fx.KEEP, *optr) == INVALID
    for k in range(len(ptr)):
        assert L.wpt_reproject_planes(17, 16, *ptr[:k], None, *ptr[k + 1:], f(0.9), f(0.05), 64, 0, *optr) == INVALID
    assert L.wpt_reproject_planes(0, 16, *ptr, f(0.9), f(0.05), 64, 0, *optr) == INVALID
    assert L.wpt_reproject_planes(65536, 65536, *ptr, f(0.9), f(0.05), 64, 0, *optr) == INVALID
    assert itf.get_option("history") == 0
    with pytest.raises(itf.WptError):
        itf.set_option("history", 1)
    # an output not asked for is not written; the others are the full call's: with a history
    tr = Tracker(itf, (17, 16))
    tr.cam = c.cam
    tr.call(0, fx.KEEP)
    tr.cam = _moved(c.cam, 1)
    itf.update_camera(*tr.cam)
    itf.compute(17 * 16 * SPP)
    full = tr.call(7)
    assert full[2].any()
    for k in range(3):
        bufs = [np.full_like(a, 0xA5A5A5A5) if a.dtype == np.uint32 else np.full_like(a, np.float32(-7.0)) for a in out]
        keep = [b.copy() for b in bufs]
        p = [b.ctypes.data if j == k else None for j, b in enumerate(bufs)]
        assert L.wpt_reproject(7, f(0.9), f(0.05), 64, 0, *p) == 0
        for j in range(3):
            assert np.array_equal(fx.bits(bufs[j]), fx.bits(full[j] if j == k else keep[j]))
        want = itf.reproject_host(cam, cur, pcam, hist)
        p = [b.ctypes.data if j == k else None for j, b in enumerate(bufs)]
        assert L.wpt_reproject_planes(17, 16, *ptr, f(0.9), f(0.05), 64, 0, *p) == 0
        assert np.array_equal(fx.bits(bufs[k]), fx.bits(want[k]))


@pytest.mark.parametrize("name,vp", [("default", (fh.W, fh.H)), ("museum", (fh.W, fh.H)), ("box", (fh.W, fh.H)),
                                     ("spheres", (fh.W, fh.H)), ("ragged", (37, 5))])
def test_sessions_against_the_host(wpt, oracle, itf, name, vp):
    """NEE, depth 4, 4 spp per camera: A, keep; B, merge, keep (the merged frame
    into the other history buffer); C, merge; then the filter over the last
    merged frame."""
    c = fh.case(wpt, oracle, name)
    _start(itf, c, vp)
    tr = Tracker(itf, vp)
    npx = vp[0] * vp[1]
    lens = []
    for k in range(3):
        tr.cam = _moved(c.cam, k)
        if k:
            itf.update_camera(*tr.cam)
            assert itf.get_option("history") == 1
        itf.compute(npx * SPP)
        if k:
            for sample in fh.SAMPLES:
                for flags in fx.FLAGS:
                    got = tr.call(sample, flags, (name, k))
                lens.append(int((got[2] > 0).sum()))
            tr.call(7, 0, (name, k, "other thresholds"), cos_min=0.5, eps_z=0.2, max_len=1 << 24)
        if k < 2:
            got = tr.call(fh.SAMPLES[k], fx.KEEP, (name, k, "keep"))
            assert itf.get_option("history") == 2
            if k == 0:
                assert not got[2].any()
    print(name, "pixels with a history per call", lens)
    assert min(lens) > 0
    # the filter over the merged frame, without a host round trip
    got = tr.call(7, fx.NEAREST, (name, "last"))
    g = itf.first_hit(7, planes=("t", "normal", "albedo", "kind"))
    for kw in (dict(), dict(iterations=5, sigma_c=0.5, sigma_z=0.05, flags=0)):
        want = itf.denoise_host(got[0], got[1], g["t"], g["normal"], g["albedo"], g["kind"], **kw)
        dn.same(itf.denoise_merged(**kw), want, (name, kw))
    # another first_hit or denoise in between does not disturb the merged frame
    itf.denoise(0)
    dn.same(itf.denoise_merged(**kw), want, (name, "after denoise"))


def test_life_cycle(wpt, oracle, itf):
    """WPT_OPT_HISTORY 0 / 2 / 1; the same-epoch call is an error and changes
    nothing; what drops the history and what keeps it."""
    L = wpt.lib()
    f = ctypes.c_float
    c = fh.case(wpt, oracle, "default")
    vp = (fh.W, fh.H)
    npx = vp[0] * vp[1]
    _start(itf, c, vp)
    assert itf.get_option("history") == 0
    with pytest.raises(itf.WptError) as e:
        itf.denoise_merged()
    assert e.value.code == itf.ERR_INVALID_ARG
    itf.compute(npx * SPP)
    tr = Tracker(itf, vp)
    tr.cam = c.cam
    first = tr.call(0, fx.KEEP)
    assert itf.get_option("history") == 2
    merged = itf.denoise_merged()
    out = [np.full((vp[1], vp[0], 3), -7.0, np.float32), np.full((vp[1], vp[0]), 0xA5, np.uint32),
           np.full((vp[1], vp[0]), 0xA5, np.uint32)]
    for flags in (0, fx.KEEP):
        assert L.wpt_reproject(0, f(0.9), f(0.05), 64, flags, *[a.ctypes.data for a in out]) == INVALID
        assert b"already holds" in L.wpt_last_error()
    assert np.all(out[0] == -7.0) and np.all(out[1] == 0xA5) and np.all(out[2] == 0xA5)
    assert itf.get_option("history") == 2
    dn.same(itf.denoise_merged(), merged, "after the refused call")
    acc, cnt = itf.read_radiance(*vp)
    assert np.array_equal(fx.bits(acc), fx.bits(first[0])) and np.array_equal(cnt, first[1])
    # resets of the accumulation keep it
    tr.cam = _moved(c.cam, 1)
    itf.update_camera(*tr.cam)
    assert itf.get_option("history") == 1
    itf.update_settings(1, 1, 0, 0, 0)
    itf.set_render_options(4, fh.SEED, 0)
    itf.set_partition(0, 1, 16)
    assert itf.get_option("history") == 1
    itf.compute(npx * SPP)
    assert tr.call(0)[2].any()
    # what drops it
    def keep_again():
        tr.hist = None
        itf.update_camera(*tr.cam)
        itf.compute(npx * SPP)
        tr.call(0, fx.KEEP)
        itf.update_camera(*tr.cam)
        assert itf.get_option("history") == 1

    itf.history_drop()
    assert itf.get_option("history") == 0
    tr.hist = None
    itf.compute(npx)
    assert not tr.call(0)[2].any()
    keep_again()
    itf.update_scene(c.scene_id)
    assert itf.get_option("history") == 0
    keep_again()
    assert itf.store_mesh(1, c.mesh)
    assert itf.get_option("history") == 0
    keep_again()
    itf.update_viewport(37, 5)
    assert itf.get_option("history") == 0
    with pytest.raises(itf.WptError):
        itf.denoise_merged()
    tr = Tracker(itf, (37, 5))
    tr.cam = _moved(c.cam, 1)
    itf.compute(37 * 5 * SPP)
    tr.call(0, fx.KEEP)
    itf.update_camera(*c.cam)
    tr.cam = c.cam
    itf.compute(37 * 5 * SPP)
    assert tr.call(0)[2].any()
    itf.shutdown()
    _start(itf, c, vp)
    assert itf.get_option("history") == 0


def test_partition(wpt, oracle, itf):
    """Rank 0 of 2 with tile 8: the other rank's pixels stay without samples in
    the kept history, and the calls still equal the host."""
    c = fh.case(wpt, oracle, "default")
    vp = (fh.W, fh.H)
    _start(itf, c, vp)
    itf.set_partition(0, 2, 8)
    mine = np.zeros(vp[0] * vp[1], bool)
    mine[itf.partition_pixels()] = True
    mine = mine.reshape(vp[1], vp[0])
    assert 0 < mine.sum() < mine.size
    itf.compute(int(mine.sum()) * SPP)
    tr = Tracker(itf, vp)
    tr.cam = c.cam
    acc, cnt, ln = tr.call(7, fx.KEEP)
    assert np.array_equal(cnt > 0, mine) and not ln.any()
    tr.cam = _moved(c.cam, 1)
    itf.update_camera(*tr.cam)
    itf.compute(int(mine.sum()) * SPP)
    acc, cnt, ln = tr.call(7)
    assert ln[mine].any()
    assert np.array_equal(tr.hist[1] > 0, mine)


def _snapshot(itf, vp):
    acc, cnt = itf.read_radiance(*vp)
    st = itf.stats()
    return acc, cnt, itf.results(1, *vp), {k: v for k, v in st.items() if k not in CLOCK_STATS}, itf.kernel_times()


@pytest.mark.parametrize("session", ["nee", "init_default"])
def test_session_untouched(wpt, oracle, itf, session):
    """The frame, the counts, the sampling view, wpt_stats and wpt_kernel_times
    are the same before and after the calls, with and without KEEP, and the
    session ends where the same session without them does: on a plain NEE
    session and on the init-default one (adaptive right half, sample stock with
    refills in flight)."""
    c = fh.case(wpt, oracle, "default")
    vp = (fh.W, fh.H)
    n = vp[0] * vp[1] * 3 + 17
    kw = {"settings": (1, 1, 0, 0), "depth": 4} if session == "nee" else {"settings": None, "depth": 0}
    cam_b = _moved(c.cam, 1)
    ends = []
    for middle in (True, False):
        _start(itf, c, vp, **kw)
        wpt.lib().wpt_set_profiling(1)
        itf.compute(n)
        tr = Tracker(itf, vp)
        tr.cam = c.cam
        if middle:
            before = _snapshot(itf, vp)
            tr.call(0, fx.KEEP)
            after = _snapshot(itf, vp)
            for a, b, what in zip(before[:3], after[:3], ("radiance", "counts", "sampling view")):
                assert np.array_equal(fx.bits(a), fx.bits(b)), what
            assert before[3] == after[3] and before[4] == after[4]
        itf.update_camera(*cam_b)
        tr.cam = cam_b
        itf.compute(n)
        if middle:
            before = _snapshot(itf, vp)
            got = tr.call(7)
            tr.call(7, fx.KEEP)
            itf.denoise_merged()
            after = _snapshot(itf, vp)
            assert got[2].any()
            for a, b, what in zip(before[:3], after[:3], ("radiance", "counts", "sampling view")):
                assert np.array_equal(fx.bits(a), fx.bits(b)), what
            assert before[3] == after[3] and before[4] == after[4]
        itf.compute(n)
        ends.append(_snapshot(itf, vp))
        itf.shutdown()
    (a1, c1, s1, st1, _), (a0, c0, s0, st0, _) = ends
    if session == "init_default":
        assert st0["stock_consumed"] > 0 and c0.max() > 3
    for a, b, what in ((a1, a0, "radiance"), (c1, c0, "counts"), (s1, s0, "sampling view")):
        assert np.array_equal(fx.bits(a), fx.bits(b)), what
    assert st1 == st0


def test_it_helps(wpt, oracle, itf):
    """Scene 100 at 64 x 48, NEE, depth 4, guides of sample 0, the documented
    defaults: 64 spp at the scene's camera, kept; 4 spp at a camera moved and
    turned; truth: the same session continued to 1024 spp. Under E(a) = mean
    |a - truth| / (|truth| + 0.01) the merged frame is less than half as far as
    the raw one, and at least 90 % of the pixels receive a history; with four
    taps and with one."""
    c = fh.case(wpt, oracle, "box")
    vp = (fh.W, fh.H)
    npx = vp[0] * vp[1]
    assert tuple(c.cam) == (0.0, 1.0, -3.5, 0.0, 0.0)
    _start(itf, c, vp)
    itf.compute(npx * 64)
    itf.reproject(0, flags=fx.KEEP)
    itf.update_camera(0.3, 1.1, -3.3, 0.05, -0.1)
    itf.compute(npx * SPP)
    acc, cnt = itf.read_radiance(*vp)
    assert np.all(cnt == SPP)
    raw = acc / np.float32(SPP)
    merged = {flags: itf.reproject(0, flags=flags) for flags in (0, fx.NEAREST)}
    itf.compute(npx * (1024 - SPP))
    acc, cnt = itf.read_radiance(*vp)
    assert np.all(cnt == 1024)
    truth = acc / np.float32(1024)
    e_raw = fx.bounded_error(raw, truth)
    for flags, (macc, mcnt, ln) in merged.items():
        e = fx.bounded_error(macc / mcnt[..., None].astype(np.float32), truth)
        share = float((ln > 0).mean())
        print("flags", flags, "E(raw 4 spp)", e_raw, "E(merged)", e, "share of pixels with len > 0", share)
        assert e < 0.5 * e_raw
        assert share >= 0.9
