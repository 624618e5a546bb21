"""wpt_first_hit on the device against the oracle, on the cases of
tests/first_hit_fixtures.py (tests/test_first_hit_cpu.py shows on the host that
the cases hold their conditions and that wpt_primary_rays makes the oracle's
own primary rays).

Every plane is compared bit for bit, every pixel: the direction with
wpt_primary_rays, (t, id, visits) with the oracle's Scene::trace_g of that ray
(visits = the reference's num_bvh_hits), the normal with the oracle's per-shape
trace, kind and the emitters' albedo with the oracle's emissive flag and
depth-1 radiance, the diffuse albedo with the host scene's material.
"""
import numpy as np
import pytest

import first_hit_fixtures as fx

pytestmark = pytest.mark.gpu

PLANES = ("dir", "t", "id", "visits", "normal", "albedo", "kind")
# wpt_stats words that are host wall-clock microseconds, or count which of two
# racing events came first (a round reaching its samples before the refill that
# traces them): no two runs of one session agree on them
CLOCK_STATS = ("plan_us", "stock_us", "stock_waits")


@pytest.fixture
def itf(wpt):
    i = wpt.interface
    yield i
    try:
        i.shutdown()
    except i.WptError:
        pass
    i.set_option("defaults", 0)


def _start(itf, scene_id, mesh, cam, vp, seed=fx.SEED, settings=(1, 1, 0, 0), depth=4):
    itf.init(vp[0], vp[1], scene_id, *cam)
    if mesh is not None:
        assert itf.store_mesh(1, mesh)
    if settings is not None:
        itf.update_settings(*settings, 0)
    itf.set_render_options(depth, seed, 0)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8 if a.dtype == np.uint8 else np.uint32)


def _same(a, b, what):
    a, b = _bits(a).reshape(-1), _bits(b).reshape(-1)
    bad = np.nonzero(a != b)[0]
    assert a.shape == b.shape and len(bad) == 0, (what, len(bad), bad[:8], a[bad[:8]], b[bad[:8]])


def _same_planes(got, want, what):
    assert set(got) == set(want)
    for k in want:
        _same(got[k], want[k], (what, k))


_FRESH = {}


def _fresh(itf, c, vp, sample, seed=fx.SEED, cam=None):
    """The full planes of a fresh session at these settings (made once)."""
    cam = tuple(c.cam if cam is None else cam)
    k = (c.name, vp, sample, seed, cam)
    if k not in _FRESH:
        _start(itf, c.scene_id, c.mesh, cam, vp, seed)
        _FRESH[k] = itf.first_hit(sample)
        itf.shutdown()
    return _FRESH[k]


@pytest.mark.parametrize("name", fx.CASES)
def test_planes_against_the_oracle(wpt, oracle, itf, name):
    c = fx.case(wpt, oracle, name)
    light = c.emissive()
    mats = c.dbg.materials()
    for vp in c.viewports:
        w, h = vp
        _start(itf, c.scene_id, c.mesh, c.cam, vp)
        for s in c.gpu_samples:
            g = itf.first_hit(s)
            what = (name, vp, s)
            assert all(g[k].shape[:2] == (h, w) for k in PLANES)
            rays = c.rays(vp, s)
            t_r, id_r, v_r = c.hits(vp, s)
            print(what, "visits", int(v_r.min()), int(v_r.max()), "device", int(g["visits"].min()),
                  int(g["visits"].max()), "differing", int((g["visits"].reshape(-1) != v_r).sum()))
            _same(g["dir"].reshape(-1, 3), rays[:, 3:], (what, "dir"))
            _same(g["t"], t_r, (what, "t"))
            _same(g["id"], id_r, (what, "id"))
            assert np.all(np.isposinf(t_r[id_r < 0]))
            _same(g["visits"], v_r, (what, "visits"))
            _same(g["normal"].reshape(-1, 3), c.normals(vp, s), (what, "normal"))
            hit = id_r >= 0
            lit = hit & light[np.maximum(id_r, 0)]
            kind = np.where(lit, fx.KIND_EMISSIVE, np.where(hit, fx.KIND_DIFFUSE, fx.KIND_MISS)).astype(np.uint8)
            _same(g["kind"], kind, (what, "kind"))
            alb = g["albedo"].reshape(-1, 3)
            _same(alb[lit], c.radiance(vp, s)[lit], (what, "albedo of emitters"))
            _same(alb[hit & ~lit], mats[id_r[hit & ~lit], :3], (what, "albedo of diffuse shapes"))
            _same(alb[~hit], np.zeros((int((~hit).sum()), 3), np.float32), (what, "albedo of misses"))
        itf.shutdown()


def test_pointer_subsets(wpt, oracle, itf):
    """Every plane on its own, and visits + t only: the full call's planes, and a
    plane not asked for is not written (its buffer keeps the sentinel)."""
    c = fx.case(wpt, oracle, "default")
    vp = c.viewports[0]
    w, h = vp
    _start(itf, c.scene_id, c.mesh, c.cam, vp)
    full = itf.first_hit(7)
    L = wpt.lib()
    assert L.wpt_first_hit(7, None, None, None, None, None, None, None) == 0  # nothing wanted: WPT_OK
    for subset in [(k,) for k in PLANES] + [("visits", "t")]:
        _same_planes(itf.first_hit(7, planes=subset), {k: full[k] for k in subset}, subset)
        bufs, ptr = {}, [None] * 7
        for k in PLANES:
            pos, dt, comp = itf.FIRST_HIT_PLANES[k]
            bufs[k] = np.frombuffer(b"\xa5" * (w * h * comp * np.dtype(dt).itemsize), dtype=dt).copy()
            if k in subset:
                ptr[pos] = bufs[k].ctypes.data
        assert L.wpt_first_hit(7, *ptr) == 0
        for k in PLANES:
            if k in subset:
                _same(bufs[k], full[k].reshape(-1), (subset, k))
            else:
                assert np.all(bufs[k].view(np.uint8) == 0xA5), (subset, k)


def _snapshot(itf, vp):
    acc, cnt = itf.read_radiance(*vp)
    st = itf.stats()
    return acc, cnt, itf.results(1, *vp), {k: v for k, v in st.items() if k not in CLOCK_STATS}


@pytest.mark.parametrize("session", ["nee", "init_default"])
def test_session_untouched(wpt, oracle, itf, session):
    """compute(n), first_hit, compute(n) leaves the radiance, the counts, the
    sampling view and wpt_stats as compute(n), compute(n) does: on a plain NEE
    session, and on the init-default session (right half PNEE + adaptive, RR
    only, sample stock on with refills in flight), where n cuts a round."""
    c = fx.case(wpt, oracle, "default")
    vp = c.viewports[0]
    n = vp[0] * vp[1] * 3 + 17
    kw = {"settings": (1, 1, 0, 0), "depth": 4} if session == "nee" else {"settings": None, "depth": 0}
    snaps = []
    for middle in (True, False):
        _start(itf, c.scene_id, c.mesh, c.cam, vp, **kw)
        itf.compute(n)
        if middle:
            g = itf.first_hit(7)
            for k, r in zip(("t", "id", "visits"), c.hits(vp, 7)):
                _same(g[k], r, ("mid-session", k))
        itf.compute(n)
        snaps.append(_snapshot(itf, vp))
        itf.shutdown()
    (a1, c1, s1, st1), (a0, c0, s0, st0) = snaps
    if session == "init_default":
        assert st0["stock_consumed"] > 0 and c0.max() > 3  # adaptive rounds ran from the stock
    print(session, {k: (st0[k], st1[k]) for k in st0 if st0[k] != st1[k]})
    _same(c1, c0, "counts")
    _same(a1, a0, "radiance")
    _same(s1, s0, "sampling view")
    assert st1 == st0


def test_after_a_change(wpt, oracle, itf):
    """After a camera update, a viewport update and another frame seed, the
    planes are those of a fresh session at those settings."""
    d, up, rg = (fx.case(wpt, oracle, k) for k in ("default", "up", "ragged"))
    seed2 = 0x12345678
    want_cam = _fresh(itf, up, (fx.W, fx.H), 0)
    want_vp = _fresh(itf, rg, (37, 5), 7)
    want_seed = _fresh(itf, rg, (37, 5), 0, seed=seed2)
    first_seed = _fresh(itf, rg, (37, 5), 0)
    _start(itf, d.scene_id, d.mesh, d.cam, (fx.W, fx.H))
    itf.compute(1000)
    itf.update_camera(*up.cam)
    _same_planes(itf.first_hit(0), want_cam, "camera")
    itf.update_camera(*d.cam)
    itf.update_viewport(37, 5)
    _same_planes(itf.first_hit(7), want_vp, "viewport")
    itf.set_render_options(4, seed2, 0)
    got = itf.first_hit(0)
    _same_planes(got, want_seed, "seed")
    assert not np.array_equal(got["dir"], first_seed["dir"])


def test_several_ranks(wpt, oracle, itf):
    """A rank of three gets the whole frame: the one-rank planes."""
    c = fx.case(wpt, oracle, "default")
    vp = c.viewports[0]
    want = _fresh(itf, c, vp, 7)
    _start(itf, c.scene_id, c.mesh, c.cam, vp)
    itf.set_partition(1, 3, 16)
    assert 0 < len(itf.partition_pixels()) < vp[0] * vp[1]
    _same_planes(itf.first_hit(7), want, "rank 1 of 3")
