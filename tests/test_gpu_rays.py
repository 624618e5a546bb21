"""The ray query on the device (wpt_radiance_rays, wpt_rays.h) against the oracle.

A query of wpt_primary_rays' rays with keys = the pixel indices is sample s of
a frame (the anchor); the one-pixel cameras of tests/rays_fixtures.py give
arbitrary origins with an exact expected value. Beyond those: the sum over spp,
sizes around the wave and the block, independence of every launch setting,
keys, invalid rays, the session left untouched, partitions, device pointers
and the argument errors. Every comparison is bit for bit.
"""
import numpy as np
import pytest

import pnee_fixtures as pf
import rays_fixtures as rf
import reproject_fixtures as rx

pytestmark = pytest.mark.gpu

INVALID = -4
SEED = rf.SEED
DEPTH = rf.DEPTH
DEFAULT_BATCH = 1 << 27


@pytest.fixture
def itf(wpt):
    i = wpt.interface
    yield i
    try:
        i.shutdown()
    except i.WptError:
        pass
    i.set_option("defaults", 0)


def _start(itf, sc, vp=(8, 8), settings=(0, 1, 0, 0), depth=DEPTH, batch=0, cam=None, photons=False):
    itf.init(vp[0], vp[1], sc.scene_id, *(cam or sc.cam))
    if sc.mesh is not None:
        assert itf.store_mesh(1, sc.mesh)
    if settings is not None:
        itf.update_settings(*settings, 0)
    itf.set_render_options(depth, SEED, batch)
    if photons:
        itf.install_photons(pf.octants())


def _same(got, want, what):
    bad = np.any(rf.bits(got) != rf.bits(want), axis=1)
    assert not bad.any(), (what, "differs on", int(bad.sum()), "of", len(bad), "rays, first", int(np.argmax(bad)),
                           got[np.argmax(bad)], want[np.argmax(bad)])


def _query(itf, *a, **kw):
    """(rgb, status, the rise of rays + shadow rays, the rise of paths)."""
    rgb, status, d = _query_counts(itf, *a, **kw)
    return rgb, status, d["rays"] + d["shadow_rays"], d["paths"]


def _query_counts(itf, *a, **kw):
    """(rgb, status, the rises of wpt_stats' paths, rays and shadow rays)."""
    s0 = itf.stats()
    rgb, status = itf.radiance_rays(*a, **kw)
    s1 = itf.stats()
    return rgb, status, {k: s1[k] - s0[k] for k in ("paths", "rays", "shadow_rays")}


# ---------------------------------------------------------------------------
# 1. The anchor: a query of a frame's primary rays is that frame's sample
# ---------------------------------------------------------------------------
ANCHORS = [("box", (37, 5), (0, 1, 2), DEPTH), ("box", (17, 16), (0, 1, 2), DEPTH), ("cloud", (33, 33), (0, 1, 2), DEPTH),
           ("museum", (17, 16), (0, 1), DEPTH), ("spheres", (17, 16), (0, 1), DEPTH),
           ("box", (17, 16), (0, 1), 0)]  # depth 0: Russian roulette only, k_finish runs


@pytest.mark.parametrize("name,vp,types,depth", ANCHORS, ids=lambda v: str(v).replace(" ", ""))
def test_anchor(wpt, oracle, itf, name, vp, types, depth):
    sc = rf.scene(wpt, oracle, name)
    _start(itf, sc, depth=depth, photons=2 in types)
    for t in types:
        for s in (0, 7):
            rays = sc.rays(vp, s)
            want, want_rays = sc.frame(vp, t, s, depth)
            rgb, status, d_rays, d_paths = _query(itf, rays, None, s, 1, t)
            assert status.all()
            _same(rgb, want, (name, vp, t, s, depth))
            assert d_rays == want_rays and d_paths == len(rays), (name, vp, t, s)
    if depth == 0:
        assert itf.stats()["finish_paths"] > 0


# ---------------------------------------------------------------------------
# 2. Arbitrary origins
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(rf.SCENES))
def test_probes(wpt, oracle, itf, name):
    sc = rf.scene(wpt, oracle, name)
    _start(itf, sc)
    keys = np.zeros(rf.PROBES, np.uint32)
    for t in (0, 1):
        want, want_rays = sc.probe_expect(t)
        rgb, status, d_rays, _ = _query(itf, sc.probe_rays(), keys, rf.PROBE_SAMPLE, 1, t)
        assert status.all()
        _same(rgb, want, (name, t))
        assert d_rays == want_rays


# ---------------------------------------------------------------------------
# 3. spp, 4. sizes
# ---------------------------------------------------------------------------
def test_spp_is_the_sequential_sum(wpt, oracle, itf):
    sc = rf.scene(wpt, oracle, "box")
    _start(itf, sc)
    rays = sc.rays((37, 5), 0)[:65]
    for t in (0, 1):
        parts = [itf.radiance_rays(rays, None, s, 1, t)[0] for s in (5, 6, 7)]
        got, _, _, d_paths = _query(itf, rays, None, 5, 3, t)
        _same(got, rf.seq_sum(parts), ("spp", t))
        assert d_paths == 3 * 65
        assert (rf.bits(parts[0]) != rf.bits(parts[1])).any()


def test_sizes_give_the_prefix(wpt, oracle, itf):
    sc = rf.scene(wpt, oracle, "box")
    _start(itf, sc)
    rays = sc.rays((33, 33), 0)[:257]
    full, status = itf.radiance_rays(rays, None, 2, 2, 1)
    assert status.all() and (full != 0).any()
    for n in (0, 1, 63, 64, 65, 255, 256, 257):
        s0 = itf.stats()
        rgb, st = itf.radiance_rays(rays[:n], None, 2, 2, 1)
        assert rgb.shape == (n, 3) and st.shape == (n,)
        _same(rgb, full[:n], ("n", n))
        if n == 0:
            assert itf.stats() == s0


# ---------------------------------------------------------------------------
# 5. Launch independence
# ---------------------------------------------------------------------------
def test_launch_independence(wpt, oracle, itf):
    sc = rf.scene(wpt, oracle, "box")
    rays = sc.rays((64, 48), 0)
    _start(itf, sc, batch=DEFAULT_BATCH)
    want = _query_counts(itf, rays, None, 3, 2, 1)
    assert want[2]["paths"] == 2 * len(rays) and want[2]["shadow_rays"] > 0
    for batch in (64, 5000, DEFAULT_BATCH):
        itf.set_render_options(DEPTH, SEED, batch)
        for lanes in (1, 2, 4):
            itf.set_lanes(lanes)
            got = _query_counts(itf, rays, None, 3, 2, 1)
            _same(got[0], want[0], ("batch", batch, "lanes", lanes))
            assert got[2] == want[2], ("batch", batch, "lanes", lanes)
    itf.set_render_options(DEPTH, SEED, DEFAULT_BATCH)
    for m in range(16):
        opts = {"presolve": m & 1, "drop_miss": (m >> 1) & 1, "presolve_shadow": (m >> 2) & 1, "fused": (m >> 3) & 1}
        for k, v in opts.items():
            itf.set_option(k, v)
        got = _query_counts(itf, rays, None, 3, 2, 1)
        _same(got[0], want[0], opts)
        assert got[2] == want[2], opts


def test_traversal_independence(wpt, oracle, itf):
    sc = rf.scene(wpt, oracle, "museum")
    rays = sc.rays((17, 16), 0)
    _start(itf, sc)
    res = []
    for trav in (0, 1):
        itf.set_option("traversal", trav)
        itf.set_option("traversal_sh", trav)
        assert itf.get_option("scene_traversal") == trav
        res.append(_query_counts(itf, rays, None, 0, 2, 1))
    _same(res[0][0], res[1][0], "traversal")
    assert res[0][2] == res[1][2] and (res[0][0] != 0).any()


# ---------------------------------------------------------------------------
# 6. Keys
# ---------------------------------------------------------------------------
def test_keys(wpt, oracle, itf):
    sc = rf.scene(wpt, oracle, "box")
    _start(itf, sc)
    rays = sc.rays((33, 33), 0)[:257]
    n = len(rays)
    base = itf.radiance_rays(rays, None, 1, 2, 1)[0]
    _same(itf.radiance_rays(rays, np.arange(n, dtype=np.uint32), 1, 2, 1)[0], base, "keys = arange")
    perm = np.random.default_rng(0x6B65).permutation(n)
    _same(itf.radiance_rays(rays[perm], perm.astype(np.uint32), 1, 2, 1)[0], base[perm], "permuted")
    other = itf.radiance_rays(rays, np.arange(1000, 1000 + n, dtype=np.uint32), 1, 2, 1)[0]
    assert (rf.bits(other) != rf.bits(base)).any()
    # equal rays with equal keys give equal results, wherever they stand
    twice = itf.radiance_rays(np.concatenate([rays[:5], rays[:5]]), np.tile(np.arange(5, dtype=np.uint32), 2), 1, 2, 1)[0]
    _same(twice[:5], twice[5:], "repeated")
    _same(twice[:5], base[:5], "repeated against the list")


# ---------------------------------------------------------------------------
# 7. Invalid rays
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("presolve", [1, 0])
def test_invalid_rays(wpt, oracle, itf, presolve):
    sc = rf.scene(wpt, oracle, "box")
    _start(itf, sc)
    itf.set_option("presolve", presolve)
    clean = sc.rays((33, 33), 0)[:130]
    n = len(clean)
    rays = np.array(clean, copy=True)
    rays[0, 1] = np.nan                # a NaN origin
    rays[63, 4] = np.inf               # an infinite direction
    rays[64, 3:] = (0.0, -0.0, 0.0)    # a direction of three zeros
    rays[n - 1, 5] = -np.nan
    bad = np.zeros(n, bool)
    bad[[0, 63, 64, n - 1]] = True
    assert np.array_equal(rf.valid(rays), (~bad).astype(np.uint8))
    want = itf.radiance_rays(clean, None, 4, 2, 1)[0]
    rgb, status, d_rays, d_paths = _query(itf, rays, None, 4, 2, 1)
    assert np.array_equal(status, (~bad).astype(np.uint8))
    assert np.all(rf.bits(rgb[bad]) == 0)
    _same(rgb[~bad], want[~bad], "the valid rays")
    assert d_paths == 2 * int((~bad).sum())
    # the invalid rays count no ray: the same rays as the list without them
    keys = np.arange(n, dtype=np.uint32)[~bad]
    only, st2, d_rays2, d_paths2 = _query(itf, rays[~bad], keys, 4, 2, 1)
    _same(only, want[~bad], "the list without them")
    assert st2.all() and d_rays2 == d_rays and d_paths2 == d_paths
    # a list of invalid rays only
    rgb0, st0, r0, p0 = _query(itf, rays[bad], None, 4, 2, 1)
    assert not st0.any() and np.all(rf.bits(rgb0) == 0) and r0 == 0 and p0 == 0
    # status may be NULL
    out = np.empty((n, 3), np.float32)
    r = np.ascontiguousarray(rays)
    assert wpt.lib().wpt_radiance_rays(n, r.ctypes.data, None, 4, 2, 1, 0, out.ctypes.data, None) == 0
    assert np.array_equal(rf.bits(out), rf.bits(rgb))


# ---------------------------------------------------------------------------
# 8. The session is not touched
# ---------------------------------------------------------------------------
def _session_state(itf, vp):
    acc, cnt = itf.read_radiance(*vp)
    return acc, cnt, itf.results(0, *vp), itf.results(1, *vp)


def _states_equal(a, b, what):
    for x, y, part in zip(a, b, ("radiance", "counts", "results(0)", "results(1)")):
        x, y = (rf.bits(x), rf.bits(y)) if x.dtype == np.float32 else (x, y)
        assert np.array_equal(x, y), (what, part)


@pytest.mark.parametrize("session", ["random", "init_default"])
def test_compute_continues_as_if_no_query(wpt, oracle, itf, session):
    """compute(a), queries, compute(b) against a twin session without the queries.
    random: two random halves, a cut mid-round. init_default: NEE random + PNEE
    adaptive with the sample stock and installed photons, a cut in the adaptive
    half's first round (4 samples per pixel)."""
    sc = rf.scene(wpt, oracle, "box")
    vp = (16, 16)
    a, b = 300, 3000
    kw = {"settings": (0, 1, 0, 0)} if session == "random" else {"settings": None, "photons": True}
    probes = sc.probe_rays()
    states = []
    for query in (True, False):
        _start(itf, sc, vp, **kw)
        itf.compute(a)
        mid = _session_state(itf, vp)
        assert mid[1].min() < mid[1].max()  # a round is cut
        if query:
            opts = {k: itf.get_option(k) for k in ("history", "map_mode")}
            for t in (1, 2) if session == "init_default" else (0, 1):
                rgb, status = itf.radiance_rays(probes, None, 1, 3, t)
                assert status.all() and (rgb != 0).any()
            _states_equal(_session_state(itf, vp), mid, "right after the query")
            assert opts == {k: itf.get_option(k) for k in ("history", "map_mode")}
        itf.compute(b)
        states.append(_session_state(itf, vp))
        if session == "init_default":
            assert itf.stats()["stock_consumed"] > 0
        itf.shutdown()
    _states_equal(states[0], states[1], session)


def test_history_and_map_survive_a_query(wpt, oracle, itf):
    """keep / move / reproject / sample_map, then a query or none, then the map
    is traced: WPT_OPT_HISTORY, WPT_OPT_MAP_MODE and the frame are the same."""
    sc = rf.scene(wpt, oracle, "box")
    vp = (16, 16)
    npx = vp[0] * vp[1]
    cam_a, cam_b = rx.PAIRS["sideways"]
    frames = []
    for query in (True, False):
        _start(itf, sc, vp, settings=(1, 1, 0, 0), cam=cam_a)
        itf.compute(4 * npx)
        itf.reproject(0, flags=rx.KEEP)
        itf.update_camera(*cam_b)
        itf.compute(npx)
        itf.reproject(0)
        count, (T, _) = itf.sample_map(0, target=6, max_per_pixel=6)
        assert T > 0
        opts = {k: itf.get_option(k) for k in ("history", "map_mode")}
        assert opts == {"history": 1, "map_mode": 0}
        if query:
            itf.radiance_rays(sc.probe_rays(), None, 0, 2, 1)
            assert opts == {k: itf.get_option(k) for k in ("history", "map_mode")}
        itf.compute_map(None)
        assert itf.get_option("map_mode") == 1
        if query:
            itf.radiance_rays(sc.probe_rays(), None, 0, 2, 0)
            assert itf.get_option("map_mode") == 1 and itf.get_option("history") == 1
        frames.append(itf.read_radiance(*vp) + (itf.reproject(0)[2],))
        assert np.array_equal(frames[-1][1], 1 + count)
        itf.shutdown()
    _states_equal(frames[0], frames[1], "map after a query")


# ---------------------------------------------------------------------------
# 9. Partition, 10. device pointers, 11. argument errors
# ---------------------------------------------------------------------------
def test_any_rank_answers_any_ray(wpt, oracle, itf):
    sc = rf.scene(wpt, oracle, "box")
    _start(itf, sc, (32, 32))
    rays = sc.rays((37, 5), 7)
    want = _query(itf, rays, None, 7, 1, 1)
    _same(want[0], sc.frame((37, 5), 1, 7)[0], "one rank")
    for rank in (0, 1):
        itf.set_partition(rank, 2, 8)
        got = _query(itf, rays, None, 7, 1, 1)
        _same(got[0], want[0], ("rank", rank))
        assert got[2:] == want[2:]
        assert not itf.read_radiance(32, 32)[1].any()


def test_device_pointers(wpt, oracle, itf):
    import torch

    sc = rf.scene(wpt, oracle, "box")
    _start(itf, sc)
    rays = np.array(sc.rays((33, 33), 0)[:257], copy=True)
    rays[100, 3:] = 0.0
    keys = np.random.default_rng(5).integers(0, 1 << 31, len(rays)).astype(np.uint32)
    dev = torch.device("cuda", torch.cuda.current_device())
    d_rays = torch.from_numpy(rays).to(dev)
    d_keys = torch.from_numpy(keys.view(np.int32)).to(dev)
    for k, dk in ((None, None), (keys, d_keys)):
        rgb, status, r0, p0 = _query(itf, rays, k, 2, 3, 1)
        d_rgb, d_status, r1, p1 = _query(itf, d_rays, dk, 2, 3, 1, device=True)
        assert d_rgb.device == d_rays.device and d_status.dtype == torch.uint8
        _same(d_rgb.cpu().numpy(), rgb, "device pointers")
        assert np.array_equal(d_status.cpu().numpy(), status) and status.sum() == len(rays) - 1
        assert (r0, p0) == (r1, p1)
    assert np.array_equal(d_rays.cpu().numpy().view(np.uint32), rays.view(np.uint32))  # the input is only read


def test_argument_errors(wpt, oracle, itf):
    sc = rf.scene(wpt, oracle, "box")
    _start(itf, sc)
    L = wpt.lib()
    rays = np.ascontiguousarray(sc.rays((37, 5), 0)[:20])
    keys = np.arange(20, dtype=np.uint32)
    rgb = np.full((20, 3), 7.25, np.float32)
    status = np.full(20, 9, np.uint8)
    r, k, o, s = rays.ctypes.data, keys.ctypes.data, rgb.ctypes.data, status.ctypes.data
    s0 = itf.stats()
    for c in ((20, None, k, 0, 1, 1, 0, o, s), (20, r, k, 0, 1, 1, 0, None, s), (20, r, k, 0, 0, 1, 0, o, s),
              (20, r, k, 0, 1, 3, 0, o, s), (20, r, k, 0, 1, 1, 2, o, s), (20, r, k, 0, 1, 1, 0x80000000, o, s),
              (20, r, k, 0xFFFFFFFF, 2, 1, 0, o, s), (20, r, k, 2, 0xFFFFFFFF, 1, 0, o, s),
              (1 << 32, r, k, 0, 1, 1, 0, o, s), (0, None, None, 0, 0, 1, 0, None, None)):
        assert L.wpt_radiance_rays(*c) == INVALID, c
        assert len(L.wpt_last_error()) > 0
    assert np.all(rgb == np.float32(7.25)) and np.all(status == 9)
    assert itf.stats() == s0
    # the largest sample index, and a degenerate call
    assert L.wpt_radiance_rays(20, r, k, 0xFFFFFFFE, 2, 1, 0, o, s) == 0 and status.all()
    assert L.wpt_radiance_rays(0, None, None, 0, 1, 1, 0, None, None) == 0
