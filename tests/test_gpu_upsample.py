"""The guided upsampler on the device (tests/test_upsample_cpu.py holds
wpt_upsample_host against a numpy restatement of the definition on the same
planes).

wpt_first_hit_scaled is compared with the oracle the way
tests/test_gpu_first_hit.py compares wpt_first_hit, over the primary rays of the
scaled viewport. wpt_upsample_planes runs the kernels on the planes of
tests/upsample_fixtures.py against wpt_upsample_host, bit for bit. wpt_upsample
runs them on sessions: its result is wpt_upsample_host of read_radiance() (or of
the last reproject's frame), first_hit(sample) and first_hit_scaled(scale,
sample); the session is left untouched.
"""
import ctypes

import numpy as np
import pytest

import denoise_fixtures as dn
import first_hit_fixtures as fh
import upsample_fixtures as fx

pytestmark = pytest.mark.gpu

# wpt_stats words that no two runs agree on (tests/test_gpu_first_hit.py)
CLOCK_STATS = ("plan_us", "stock_us", "stock_waits")
GUIDES = ("t", "normal", "albedo", "kind")
PLANES = ("dir", "t", "id", "visits", "normal", "albedo", "kind")
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


def _start(itf, c, vp, settings=(1, 1, 0, 0), depth=4):
    itf.init(vp[0], vp[1], c.scene_id, *c.cam)
    if c.mesh is not None:
        assert itf.store_mesh(1, c.mesh)
    if settings is not None:
        itf.update_settings(*settings, 0)
    itf.set_render_options(depth, fh.SEED, 0)


def _same(a, b, what):
    a, b = fx.bits(a).reshape(-1), fx.bits(b).reshape(-1)
    bad = np.nonzero(a != b)[0]
    assert a.shape == b.shape and len(bad) == 0, (what, len(bad), bad[:8], a[bad[:8]], b[bad[:8]])


def _guides(g):
    return tuple(g[k] for k in GUIDES)


def _host_of_session(itf, vp, scale, sample, frame=None, coarse_sample=None, **kw):
    acc, cnt = itf.read_radiance(*vp) if frame is None else frame
    g = itf.first_hit(sample if coarse_sample is None else coarse_sample, planes=GUIDES)
    hi = itf.first_hit_scaled(scale, sample, planes=GUIDES)
    return itf.upsample_host(scale, (acc, cnt) + _guides(g), _guides(hi), **kw)


# ---- wpt_first_hit_scaled ----------------------------------------------------
def test_scale_one_is_first_hit(wpt, oracle, itf):
    c = fh.case(wpt, oracle, "default")
    _start(itf, c, (fh.W, fh.H))
    for sample in fh.SAMPLES:
        want, got = itf.first_hit(sample), itf.first_hit_scaled(1, sample)
        for k in PLANES:
            _same(got[k], want[k], ("scale 1", sample, k))
    L = wpt.lib()
    assert L.wpt_first_hit_scaled(2, 0, None, None, None, None, None, None, None) == 0  # nothing wanted
    buf = np.zeros(5 * 5 * fh.W * fh.H, np.uint8)
    for bad in (0, 5, 0xFFFFFFFF):
        assert L.wpt_first_hit_scaled(bad, 0, None, None, None, None, None, None, buf.ctypes.data) == INVALID
    assert not buf.any()


def test_scaled_viewport_too_large(wpt, oracle, itf):
    """scale^2 W H >= 2^32 is refused before anything is launched."""
    c = fh.case(wpt, oracle, "box")
    _start(itf, c, (8, 8))
    L = wpt.lib()
    one = np.zeros(64 * 16, np.uint8)
    # on the plane hook: 32768^2 x 4 = 2^32 (no plane is read before the check)
    p = [one.ctypes.data] * 11
    f = ctypes.c_float
    assert L.wpt_upsample_planes(32768, 32768, 2, *p, 3, f(1.0), f(0.1), 0, None, None, one.ctypes.data) == INVALID
    assert L.wpt_upsample_planes(16384, 16384, 4, *p, 3, f(1.0), f(0.1), 0, None, None, one.ctypes.data) == INVALID
    assert not one.any()


@pytest.mark.parametrize("name,vp", [("box", (fh.W, fh.H)), ("default", (fh.W, fh.H)), ("museum", (fh.W, fh.H)),
                                     ("spheres", (fh.W, fh.H)), ("ragged", (37, 5))])
def test_scaled_planes_against_the_oracle(wpt, oracle, itf, name, vp):
    """Scales 2 and 3: every plane bit for bit, every fine pixel, against
    oracle.trace_rays over wpt_primary_rays(sW, sH, ...), as
    tests/test_gpu_first_hit.py derives the planes. Afterwards wpt_denoise of the
    same sample still is its host restatement: the coarse planes are intact."""
    c = fh.case(wpt, oracle, name)
    light = c.emissive()
    mats = c.dbg.materials()
    _start(itf, c, vp)
    itf.compute(vp[0] * vp[1] * SPP)
    for scale, s in ((2, 7), (3, 0)):
        fvp = (scale * vp[0], scale * vp[1])
        before = itf.denoise(s)
        g = itf.first_hit_scaled(scale, s)
        what = (name, vp, scale, s)
        assert all(g[k].shape[:2] == (fvp[1], fvp[0]) for k in PLANES)
        rays = c.rays(fvp, s)
        t_r, id_r, v_r = c.hits(fvp, s)
        _same(g["dir"].reshape(-1, 3), rays[:, 3:], (what, "dir"))
        _same(g["t"], t_r, (what, "t"))
        _same(g["id"], id_r, (what, "id"))
        _same(g["visits"], v_r, (what, "visits"))
        _same(g["normal"].reshape(-1, 3), c.normals(fvp, s), (what, "normal"))
        hit = id_r >= 0
        lit = hit & light[np.maximum(id_r, 0)]
        kind = np.where(lit, fh.KIND_EMISSIVE, np.where(hit, fh.KIND_DIFFUSE, fh.KIND_MISS)).astype(np.uint8)
        _same(g["kind"], kind, (what, "kind"))
        alb = g["albedo"].reshape(-1, 3)
        _same(alb[lit], c.radiance(fvp, s)[lit], (what, "albedo of emitters"))
        _same(alb[hit & ~lit], mats[id_r[hit & ~lit], :3], (what, "albedo of diffuse shapes"))
        _same(alb[~hit], np.zeros((int((~hit).sum()), 3), np.float32), (what, "albedo of misses"))
        # the coarse planes were not disturbed
        acc, cnt = itf.read_radiance(*vp)
        lo = itf.first_hit(s, planes=GUIDES)
        want = itf.denoise_host(acc, cnt, *_guides(lo))
        dn.same(itf.denoise(s), want, (what, "denoise after"))
        dn.same(before, want, (what, "denoise before"))


# ---- wpt_upsample_planes -----------------------------------------------------
@pytest.mark.parametrize("vp", fx.VIEWPORTS, ids=lambda v: f"{v[0]}x{v[1]}")
def test_planes_against_the_host(wpt, oracle, itf, vp):
    """Every scale, 0 / 3 / 5 passes, the passes through LDS and direct; 9 x 7
    at scale 2 is an 18 x 14 fine frame, ragged tiles on both axes."""
    c = fh.case(wpt, oracle, "box")
    _start(itf, c, (8, 8))
    seen = set()
    for s in fx.SCALES:
        coarse, fine = fx.shared_case(*vp, s)
        for it in (0, 3, 5):
            kw = dict(iterations=it, sigma_c=float(fx.SIGMA_C), sigma_z=float(fx.SIGMA_Z))
            want = itf.upsample_host(s, coarse, fine, fx.BACKGROUND, **kw)
            for lds in (7, 0):
                itf.set_option("denoise_lds", lds)
                got = itf.upsample_planes(s, coarse, fine, fx.BACKGROUND, **kw)
                fx.same(got, want, (vp, s, it, lds))
            seen |= set(np.unique(got[1]))
        # the sigma pair at which the denormal depths give 0 / 0
        kw = dict(iterations=3, sigma_c=0.37, sigma_z=float(fx.SMALL_SIGMA_Z))
        itf.set_option("denoise_lds", 7)
        fx.same(itf.upsample_planes(s, coarse, fine, fx.BACKGROUND, **kw),
                itf.upsample_host(s, coarse, fine, fx.BACKGROUND, **kw), (vp, s, "small sigma_z"))
    if vp[0] >= 8 and vp[1] >= 7:
        assert seen == {0, 1, 2}


def test_arguments(wpt, oracle, itf):
    L = wpt.lib()
    f = ctypes.c_float
    w, h, s = 9, 7, 2
    coarse, fine = fx.shared_case(w, h, s)
    ins = [np.ascontiguousarray(a) for a in coarse + fine] + [fx.BACKGROUND]
    ptr = [a.ctypes.data for a in ins]
    out = [np.zeros((s * h, s * w, 3), np.float32), np.zeros((s * h, s * w), np.uint8),
           np.zeros((s * h, s * w, 4), np.uint8)]
    optr = [a.ctypes.data for a in out]
    # both device entry points need a session
    assert L.wpt_upsample(2, 0, 3, f(1.0), f(0.1), 0, *optr) == -1
    assert L.wpt_upsample_planes(w, h, s, *ptr, 3, f(1.0), f(0.1), 0, *optr) == -1
    assert L.wpt_first_hit_scaled(2, 0, None, None, None, None, None, None, optr[1]) == -1
    c = fh.case(wpt, oracle, "box")
    _start(itf, c, (w, h))
    itf.compute(w * h * SPP)
    for fn in (lambda sc, *a: L.wpt_upsample(sc, 7, *a), lambda sc, *a: L.wpt_upsample_planes(w, h, sc, *ptr, *a)):
        assert fn(2, 3, f(1.0), f(0.1), 0, *optr) == 0
        assert fn(2, 0, f(1.0), f(0.1), 0, *optr) == 0
        assert fn(2, 3, f(1.0), f(0.1), 0, None, None, None) == 0
        for bad in (0, 1, 5):
            assert fn(bad, 3, f(1.0), f(0.1), 0, *optr) == INVALID
        assert fn(2, 6, f(1.0), f(0.1), 0, *optr) == INVALID
        for v in (0.0, -1.0, float("inf"), float("nan")):
            assert fn(2, 3, f(v), f(0.1), 0, *optr) == INVALID and fn(2, 3, f(1.0), f(v), 0, *optr) == INVALID
        assert fn(2, 3, f(1.0), f(0.1), 2, *optr) == INVALID
    assert L.wpt_upsample_planes(w, h, s, *ptr, 3, f(1.0), f(0.1), 1, *optr) == INVALID  # MERGED: the session call's
    for k in range(len(ptr)):
        assert L.wpt_upsample_planes(w, h, s, *ptr[:k], None, *ptr[k + 1:], 3, f(1.0), f(0.1), 0, *optr) == INVALID
    assert L.wpt_upsample_planes(0, h, s, *ptr, 3, f(1.0), f(0.1), 0, *optr) == INVALID
    # MERGED before any reproject: wpt_denoise_merged's error
    assert L.wpt_upsample(2, 7, 3, f(1.0), f(0.1), 1, *optr) == INVALID and b"wpt_reproject" in L.wpt_last_error()
    # an output not asked for is not written; the others are the full call's
    full = itf.upsample(2, 7)
    for k in range(3):
        bufs = [np.full_like(a, 0xA5) if a.dtype == np.uint8 else np.full_like(a, np.float32(-7.0)) for a in out]
        keep = [b.copy() for b in bufs]
        d = itf.UPSAMPLE_DEFAULTS
        assert L.wpt_upsample(2, 7, d["iterations"], f(d["sigma_c"]), f(d["sigma_z"]), 0,
                              *[b.ctypes.data if j == k else None for j, b in enumerate(bufs)]) == 0
        for j in range(3):
            assert np.array_equal(fx.bits(bufs[j]), fx.bits(full[j] if j == k else keep[j]))


# ---- wpt_upsample on sessions --------------------------------------------------
@pytest.mark.parametrize("name,vp,settings,depth", [
    ("default", (fh.W, fh.H), (1, 1, 0, 0), 4), ("museum", (fh.W, fh.H), (1, 1, 0, 0), 4),
    ("box", (fh.W, fh.H), (1, 1, 0, 0), 4), ("spheres", (fh.W, fh.H), (1, 1, 0, 0), 4),
    ("ragged", (37, 5), (1, 1, 0, 0), 4), ("init_default", (fh.W, fh.H), None, 0)])
def test_sessions_against_the_host(wpt, oracle, itf, name, vp, settings, depth):
    """NEE, depth 4, 4 spp (and the init-default session); samples 0 and 7:
    wpt_upsample = the host restatement on the frame and the planes the session
    gives."""
    c = fh.case(wpt, oracle, "default" if name == "init_default" else name)
    _start(itf, c, vp, settings, depth)
    itf.compute(vp[0] * vp[1] * SPP)
    valids = set()
    for sample, scale, kw in ((0, 2, dict()), (7, 3, dict(iterations=5, sigma_c=0.5, sigma_z=0.05)),
                              (7, 4, dict(iterations=0)), (0, 2, dict(iterations=0))):
        got = itf.upsample(scale, sample, **kw)
        fx.same(got, _host_of_session(itf, vp, scale, sample, **kw), (name, sample, scale, kw))
        assert got[0].shape == (scale * vp[1], scale * vp[0], 3)
        valids |= set(np.unique(got[1]))
    print(name, "valid values", sorted(valids))
    assert 1 in valids


def test_merged_source(wpt, oracle, itf):
    """keep, move, compute, reproject: WPT_UPSAMPLE_MERGED is the host
    restatement on that call's acc3 / cnt under the guides of its sample."""
    c = fh.case(wpt, oracle, "box")
    vp = (fh.W, fh.H)
    npx = vp[0] * vp[1]
    _start(itf, c, vp)
    itf.compute(npx * SPP)
    with pytest.raises(itf.WptError) as e:
        itf.upsample(2, 0, flags=itf.UPSAMPLE_MERGED)
    assert e.value.code == itf.ERR_INVALID_ARG
    itf.reproject(0, flags=itf.REPROJECT_KEEP)
    cam = list(c.cam)
    cam[4] += 0.03
    itf.update_camera(*cam)
    itf.compute(npx * SPP)
    acc, cnt, ln = itf.reproject(7)
    assert (ln > 0).any() and cnt.max() > SPP
    for scale, sample, kw in ((2, 7, dict()), (3, 0, dict(iterations=1))):
        got = itf.upsample(scale, sample, flags=itf.UPSAMPLE_MERGED, **kw)
        want = _host_of_session(itf, vp, scale, sample, frame=(acc, cnt), coarse_sample=7, **kw)
        fx.same(got, want, ("merged", scale, sample))
        # the default source still is the session's frame
        fx.same(itf.upsample(scale, sample, **kw), _host_of_session(itf, vp, scale, sample, **kw), ("plain", scale))
        assert not np.array_equal(got[0], itf.upsample(scale, sample, **kw)[0])
    # the merged frame is still there for the filter
    g = itf.first_hit(7, planes=GUIDES)
    dn.same(itf.denoise_merged(), itf.denoise_host(acc, cnt, *_guides(g)), "denoise_merged after upsample")


def test_partition(wpt, oracle, itf):
    """Rank 0 of 2 with tile 8: the other rank's coarse pixels have no samples
    and are never taps."""
    c = fh.case(wpt, oracle, "default")
    vp = (fh.W, fh.H)
    _start(itf, c, vp)
    itf.set_partition(0, 2, 8)
    n = len(itf.partition_pixels())
    assert 0 < n < vp[0] * vp[1]
    itf.compute(n * SPP)
    got = itf.upsample(2, 7)
    fx.same(got, _host_of_session(itf, vp, 2, 7), "rank 0 of 2")
    assert (got[1] == 0).any() and (got[1] == 1).any()


def test_viewport_change(wpt, oracle, itf):
    """The scaled planes and the scratch follow the viewport."""
    c = fh.case(wpt, oracle, "default")
    _start(itf, c, (fh.W, fh.H))
    itf.compute(fh.W * fh.H * SPP)
    itf.upsample(2, 0)
    for vp, scale in (((37, 5), 4), ((130, 70), 2)):
        itf.update_viewport(*vp)
        itf.compute(vp[0] * vp[1] * SPP)
        fx.same(itf.upsample(scale, 0), _host_of_session(itf, vp, scale, 0), (vp, scale))


def _snapshot(itf, vp):
    acc, cnt = itf.read_radiance(*vp)
    st = itf.stats()
    return (acc, cnt, itf.results(1, *vp), {k: v for k, v in st.items() if k not in CLOCK_STATS}, itf.kernel_times(),
            itf.get_option("history"), itf.get_option("map_mode"))


@pytest.mark.parametrize("session", ["nee", "init_default"])
def test_session_untouched(wpt, oracle, itf, session):
    """The frame, the counts, the sampling view, wpt_stats, wpt_kernel_times,
    WPT_OPT_HISTORY and WPT_OPT_MAP_MODE are the same before and after a call,
    and compute(n), upsample, compute(n) ends where compute(n), compute(n) does:
    on a plain NEE session and on the init-default one (adaptive right half,
    sample stock with refills in flight)."""
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
            got = itf.upsample(2, 7)
            itf.first_hit_scaled(3, 0)
            after = _snapshot(itf, vp)
            for a, b, what in zip(before[:3], after[:3], ("radiance", "counts", "sampling view")):
                assert np.array_equal(fx.bits(a), fx.bits(b)), what
            assert before[3:] == after[3:]
            fx.same(got, _host_of_session(itf, vp, 2, 7), "mid-session")
        itf.compute(n)
        ends.append(_snapshot(itf, vp))
        itf.shutdown()
    (a1, c1, s1, st1, *_), (a0, c0, s0, st0, *_) = ends
    if session == "init_default":
        assert st0["stock_consumed"] > 0 and c0.max() > 3
    for a, b, what in ((a1, a0, "radiance"), (c1, c0, "counts"), (s1, s0, "sampling view")):
        assert np.array_equal(fx.bits(a), fx.bits(b)), what
    assert st1 == st0


def test_quality(wpt, oracle, itf):
    """Scene 100: a 32 x 24 session, NEE, depth 4, 256 spp, upsampled x2 with no
    pass and with the filter defaults, beside the 2 x 2 replication of its means,
    all against the 1024-spp frame of a 64 x 48 session. A printed measurement:
    the inequality was decided on the CPU (tests/test_upsample_cpu.py,
    test_quality_on_the_oracle, which gives the figures and the cause) and does
    not hold. What is asserted is that the device frames are the host's."""
    c = fh.case(wpt, oracle, "box")
    lo, hi, s, spp = (32, 24), (64, 48), 2, 256
    _start(itf, c, lo)
    itf.compute(lo[0] * lo[1] * spp)
    acc, cnt = itf.read_radiance(*lo)
    assert np.all(cnt == spp)
    mean = acc / np.float32(spp)
    ups = {}
    for it in (0, itf.UPSAMPLE_DEFAULTS["iterations"]):
        ups[it] = itf.upsample(s, 0, iterations=it)
        fx.same(ups[it], _host_of_session(itf, lo, s, 0, iterations=it), ("quality", it))
    itf.shutdown()
    _start(itf, c, hi)
    itf.compute(hi[0] * hi[1] * 1024)
    acc, cnt = itf.read_radiance(*hi)
    assert np.all(cnt == 1024)
    ref = acc / np.float32(1024)
    e_rep = fx.rel_l2_pair(fx.replicate(mean, s), ref)
    print("relative L2 against 1024 spp (clamped, unclamped): replicated", e_rep)
    for it, (rgb, valid, _) in ups.items():
        e = fx.rel_l2_pair(rgb, ref)
        print("  upsampled, iterations", it, e, "below the replication (clamped):", e[0] < e_rep[0])
