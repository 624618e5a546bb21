"""Guided sampling on the device (wpt_guided.h).

wpt_sample_map_planes runs the planning kernels (k_map_need, the u64 scan,
k_map_deal) on the frames of tests/guided_fixtures.py against
wpt_sample_map_host, bit for bit (tests/test_guided_cpu.py holds the host against
Python integers). wpt_compute_map is held against the oracle: per pixel,
count[p] samples from sample cnt[p] on, added to the frame the session held. The
frame does not depend on batch size or lanes, other ranks' pixels are never
touched, map mode lives and dies as include/wpt.h says, wpt_sample_map leaves
the session untouched, and the loop keep / move / reproject / sample_map /
compute_map fills every pixel up to the target.
"""
import numpy as np
import pytest

import first_hit_fixtures as fh
import guided_fixtures as gx
import pnee_fixtures as pf
import reproject_fixtures as rx

pytestmark = pytest.mark.gpu

# wpt_stats words that no two runs agree on (tests/test_gpu_first_hit.py)
CLOCK_STATS = ("plan_us", "stock_us", "stock_waits")
INVALID = -4
SEED = fh.SEED
DEPTH = 4
# name -> (scene id, mesh)
SCENES = {"box": (100, None), "cloud": (2, "cloud")}
CAM_UP = (-0.9, 5.4, 0.4, -1.2, 0.0)  # the cloud from below (first_hit_fixtures' "up"): a sixth of the rays miss


@pytest.fixture
def itf(wpt):
    i = wpt.interface
    yield i
    try:
        i.shutdown()
    except i.WptError:
        pass
    i.set_option("defaults", 0)


_REF = {}


def _scene(wpt, oracle, name):
    """(scene id, mesh, camera, an oracle scene of this module's own that holds
    the small photon list of pnee_fixtures.octants)."""
    if name not in _REF:
        sid, mesh = SCENES[name]
        m = wpt.scenes.triangle_cloud(3000, seed=0x5EED) if mesh else None
        ref = oracle.OracleScene(sid, m)
        assert ref.num_lights == 2
        ref.set_photons(pf.octants())
        _REF[name] = (sid, m, tuple(wpt.scenes.scene_camera(sid)), ref)
    return _REF[name]


def _start(itf, sc, vp, settings=(0, 1, 0, 0), depth=DEPTH, batch=0, cam=None, photons=False):
    sid, mesh, scam, _ = sc
    itf.init(vp[0], vp[1], sid, *(cam or scam))
    if mesh is not None:
        assert itf.store_mesh(1, mesh)
    if settings is not None:
        itf.update_settings(*settings, 0)
    itf.set_render_options(depth, SEED, batch)
    if photons:
        itf.install_photons(pf.octants())


def _bits(a):
    return rx.bits(a)


def _random_map(vp, seed):
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([0, 1, 2, 5], np.uint32), (vp[1], vp[0]))


def _expect(ref, vp, cam, types, depth, acc0, cnt0, count, mine=None):
    """The frame after a map: per pixel the oracle's samples cnt0 .. cnt0 + count
    - 1 added, in order, to what the pixel held."""
    want = np.array(acc0, np.float32, copy=True)
    rays = 0
    for y, x in zip(*np.nonzero(count)):
        if mine is not None and not mine[y, x]:
            continue
        _, st = ref.render(vp[0], vp[1], cam, types[0], types[1], depth, SEED, s0=int(cnt0[y, x]),
                           spp=int(count[y, x]), region=(int(x), int(y), int(x) + 1, int(y) + 1), acc=want)
        rays += st["rays"]
    add = count if mine is None else np.where(mine, count, 0)
    return want, (cnt0 + add).astype(np.uint32), rays


def _frames_equal(got, want, what):
    assert np.array_equal(got[1], want[1]), (what, "counts")
    bad = np.any(_bits(got[0]) != _bits(want[0]), axis=2)
    assert not bad.any(), (what, "radiance differs on", int(bad.sum()), "pixels, first", np.argwhere(bad)[0])


# ---------------------------------------------------------------------------
# The planning kernels against the host
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("vp", gx.VIEWPORTS, ids=lambda v: f"{v[0]}x{v[1]}")
def test_planes_against_the_host(wpt, oracle, itf, vp):
    _start(itf, _scene(wpt, oracle, "box"), (8, 8))
    cnt, ln, kind = gx.planes(*vp)
    dealt = 0
    for mask in gx.MASKS:
        member = gx.mask(itf, mask, *vp)
        for target, max_pp in gx.LIMITS:
            for flags in (0, gx.MISS_ONCE):
                try:
                    _, (T, _) = itf.sample_map_host(cnt, ln, kind, member, target, max_pp, 0, flags)
                except itf.WptError:
                    with pytest.raises(itf.WptError) as e:
                        itf.sample_map_planes(cnt, ln, kind, member, target, max_pp, 0, flags)
                    assert e.value.code == itf.ERR_INVALID_ARG
                    continue
                for budget in gx.budgets(T):
                    want = itf.sample_map_host(cnt, ln, kind, member, target, max_pp, budget, flags)
                    got = itf.sample_map_planes(cnt, ln, kind, member, target, max_pp, budget, flags)
                    gx.same(got, want, (vp, mask, target, max_pp, flags, budget))
                    dealt += 0 < budget < T
    assert dealt > 0


def test_planes_past_one_pass_of_the_sum_scan(wpt, oracle, itf):
    """513 x 512: 257 scan chunks, one more than k_scan64_sums scans per pass, so
    both carries (chunk to chunk, pass to pass) are in the result."""
    vp = gx.BIG_VIEWPORT
    assert (vp[0] * vp[1] + 1 + 1023) // 1024 == 257
    _start(itf, _scene(wpt, oracle, "box"), (8, 8))
    cnt, ln, kind = gx.planes(*vp)
    for mask in ("all", "rank0of2"):
        member = gx.mask(itf, mask, *vp)
        for target, max_pp, flags in ((gx.TARGET, gx.M32, 0), (gx.TARGET, 3, gx.MISS_ONCE), (1000, 1000, 0)):
            _, (T, _) = itf.sample_map_host(cnt, ln, kind, member, target, max_pp, 0, flags)
            assert T > vp[0] * vp[1] // 4
            for budget in (0, 1, T // 3, T - 1, gx.M32):
                want = itf.sample_map_host(cnt, ln, kind, member, target, max_pp, budget, flags)
                gx.same(itf.sample_map_planes(cnt, ln, kind, member, target, max_pp, budget, flags), want,
                        (mask, target, max_pp, flags, budget))
    # the last pixel alone needs samples: its prefix carries nothing, its count the whole budget
    cnt2 = np.full((vp[1], vp[0]), gx.TARGET, np.uint32)
    cnt2[-1, -1] = 0
    z = np.zeros_like(cnt2)
    one = np.ones(cnt2.shape, np.uint8)
    got = itf.sample_map_planes(cnt2, z, one, one, gx.TARGET, gx.M32, 3, 0)
    assert got[1] == (gx.TARGET, 3) and got[0][-1, -1] == 3 and int(got[0].sum()) == 3


def test_plane_arguments(wpt, oracle, itf):
    L = wpt.lib()
    _start(itf, _scene(wpt, oracle, "box"), (8, 8))
    cnt, ln, kind = gx.planes(17, 16)
    member = np.ones((16, 17), np.uint8)
    ptr = [np.ascontiguousarray(a).ctypes.data for a in (cnt, ln, kind, member)]
    out = np.full((16, 17), 0xA5, np.uint32)
    tot = np.zeros(2, np.uint64)
    for fn, head in ((L.wpt_sample_map_planes, (17, 16, *ptr)), (L.wpt_sample_map, (0,))):
        assert fn(*head, 8, 8, 0, 0, out.ctypes.data, tot.ctypes.data) == 0
        assert fn(*head, 8, 8, 0, 0, None, None) == 0
        assert fn(*head, 0, 8, 0, 0, out.ctypes.data, tot.ctypes.data) == INVALID
        assert fn(*head, 8, 0, 0, 0, out.ctypes.data, tot.ctypes.data) == INVALID
        assert fn(*head, 8, 8, 0, 2, out.ctypes.data, tot.ctypes.data) == INVALID
    for k in range(4):
        assert L.wpt_sample_map_planes(17, 16, *ptr[:k], None, *ptr[k + 1:], 8, 8, 0, 0, out.ctypes.data,
                                       tot.ctypes.data) == INVALID
    assert L.wpt_sample_map_planes(0, 16, *ptr, 8, 8, 0, 0, out.ctypes.data, tot.ctypes.data) == INVALID
    assert L.wpt_sample_map_planes(65536, 65536, *ptr, 8, 8, 0, 0, out.ctypes.data, tot.ctypes.data) == INVALID


# ---------------------------------------------------------------------------
# wpt_compute_map against the oracle
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("types", [(0, 1), (1, 2)], ids=["NoNEE|NEE", "NEE|PNEE"])
@pytest.mark.parametrize("vp", [(24, 16), (37, 5)], ids=lambda v: f"{v[0]}x{v[1]}")
@pytest.mark.parametrize("name", list(SCENES))
def test_compute_map_against_the_oracle(wpt, oracle, itf, name, vp, types):
    """compute(2 * npix + 7) leaves a half mid-round; then two maps with entries
    from {0, 1, 2, 5} on both halves."""
    sc = _scene(wpt, oracle, name)
    npx = vp[0] * vp[1]
    _start(itf, sc, vp, settings=(*types, 0, 0), photons=types[1] == 2)
    itf.compute(2 * npx + 7)
    acc0, cnt0 = itf.read_radiance(*vp)
    assert len(np.unique(cnt0)) > 1 or vp[0] == 1
    assert itf.get_option("map_mode") == 0
    for k in range(2):
        st0 = itf.stats()
        count = _random_map(vp, 0x6D41 + 7 * k + vp[0])
        assert (count == 0).any() and (count[:, : vp[0] // 2] > 0).any() and (count[:, vp[0] // 2:] > 0).any()
        itf.compute_map(count)
        assert itf.get_option("map_mode") == 1
        want_acc, want_cnt, rays = _expect(sc[3], vp, sc[2], types, DEPTH, acc0, cnt0, count)
        got = itf.read_radiance(*vp)
        _frames_equal(got, (want_acc, want_cnt), (name, vp, types, k))
        st = itf.stats()
        assert st["paths"] - st0["paths"] == int(count.sum())
        assert st["rays"] + st["shadow_rays"] - st0["rays"] - st0["shadow_rays"] == rays
        assert st["photons"] == 0
        acc0, cnt0 = got


def _mapped_frame(itf, sc, vp, count, batch, lanes, small_lanes=None):
    _start(itf, sc, vp, settings=(0, 1, 0, 0), batch=batch)
    itf.set_lanes(lanes)
    if small_lanes is not None:
        itf.set_option("small_lanes", small_lanes)
    itf.compute(2 * vp[0] * vp[1] + 7)
    st0 = itf.stats()
    itf.compute_map(count)
    st = itf.stats()
    out = itf.read_radiance(*vp), st["rays"] - st0["rays"], st["shadow_rays"] - st0["shadow_rays"], \
        st["paths"] - st0["paths"]
    itf.shutdown()
    return out


def test_batches_and_lanes(wpt, oracle, itf):
    """The same map at 64 x 48 (about 6,000 paths) with batch_paths 64 (pixels
    straddle batches), 5,000 and the default, on 1, 2 and 4 lanes (pixels
    straddle lane slices): the frame and every count are identical."""
    sc = _scene(wpt, oracle, "box")
    vp = (fh.W, fh.H)
    count = _random_map(vp, 0xBA7C)
    assert int(count.sum()) > 4096
    base = _mapped_frame(itf, sc, vp, count, 0, 4)
    assert base[3] == int(count.sum())
    # (batch_paths, lanes, small_lanes): 64 and 777 cut pixels across batches on one lane; the default and 5,000
    # run slices of about 3,000, 1,500 and 1,250 paths on 2 and 4 lanes, which cut pixels across lanes
    for batch, lanes, small in ((0, 1, None), (64, 4, None), (64, 1, None), (777, 2, None), (0, 4, 4), (5000, 4, 4)):
        got = _mapped_frame(itf, sc, vp, count, batch, lanes, small)
        _frames_equal(got[0], base[0], (batch, lanes, small))
        assert got[1:] == base[1:], (batch, lanes, small)


def test_partition(wpt, oracle, itf):
    """Rank 0 of 2 with tile 8: only its own pixels change, whatever the map
    holds elsewhere, and they hold the oracle's samples."""
    sc = _scene(wpt, oracle, "box")
    vp = (24, 16)
    _start(itf, sc, vp)
    itf.set_partition(0, 2, 8)
    mine = np.zeros(vp[0] * vp[1], bool)
    mine[itf.partition_pixels()] = True
    mine = mine.reshape(vp[1], vp[0])
    assert 0 < mine.sum() < mine.size
    itf.compute(int(mine.sum()) * 2 + 3)
    acc0, cnt0 = itf.read_radiance(*vp)
    assert not cnt0[~mine].any() and len(np.unique(cnt0[mine])) == 2
    count = _random_map(vp, 0x9A47) + np.where(mine, 0, 3).astype(np.uint32)
    itf.compute_map(count)
    want_acc, want_cnt, _ = _expect(sc[3], vp, sc[2], (0, 1), DEPTH, acc0, cnt0, count, mine)
    got = itf.read_radiance(*vp)
    _frames_equal(got, (want_acc, want_cnt), "rank 0 of 2")
    assert not got[1][~mine].any() and not _bits(got[0])[~mine].any()
    assert itf.stats()["paths"] == int(mine.sum()) * 2 + 3 + int(count[mine].sum())
    # the planned map holds nothing outside the partition either
    planned, (T, s) = itf.sample_map(0, 9, 9)
    assert not planned[~mine].any() and np.array_equal(planned[mine], np.maximum(9 - got[1][mine].astype(np.int64), 0))
    assert T == s == int(planned.sum())


# ---------------------------------------------------------------------------
# Map mode, the device map, the session
# ---------------------------------------------------------------------------
def test_map_mode(wpt, oracle, itf):
    L = wpt.lib()
    sc = _scene(wpt, oracle, "box")
    vp = (24, 16)
    npx = vp[0] * vp[1]
    n = 2 * npx + 7
    _start(itf, sc, vp)
    itf.compute(n)
    fresh = itf.read_radiance(*vp)
    with pytest.raises(itf.WptError):
        itf.set_option("map_mode", 1)
    # a map of zeros: nothing launched, no map mode
    paths = itf.stats()["paths"]
    itf.compute_map(np.zeros((vp[1], vp[0]), np.uint32))
    assert itf.get_option("map_mode") == 0 and itf.stats()["paths"] == paths
    _frames_equal(itf.read_radiance(*vp), fresh, "a map of zeros")
    # the two overflows: nothing traced
    big = np.full((vp[1], vp[0]), 1 << 31, np.uint32)
    assert L.wpt_compute_map(big.ctypes.data) == INVALID and b"sum" in L.wpt_last_error()
    one = np.zeros((vp[1], vp[0]), np.uint32)
    one[3, 5] = gx.M32
    assert fresh[1][3, 5] > 0
    assert L.wpt_compute_map(one.ctypes.data) == INVALID and b"sample index" in L.wpt_last_error()
    assert itf.get_option("map_mode") == 0 and itf.stats()["paths"] == paths
    _frames_equal(itf.read_radiance(*vp), fresh, "refused maps")
    itf.compute(n)  # still allowed
    twice = itf.read_radiance(*vp)
    # a traced map
    count = _random_map(vp, 0x30DE)
    itf.compute_map(count)
    assert itf.get_option("map_mode") == 1
    mapped = itf.read_radiance(*vp)
    assert np.array_equal(mapped[1], twice[1] + count)
    assert L.wpt_compute(100) == INVALID and b"map mode" in L.wpt_last_error()
    _frames_equal(itf.read_radiance(*vp), mapped, "a refused compute")
    assert itf.stats()["paths"] == 2 * n + int(count.sum())
    itf.compute_map(count)  # any number of times
    assert np.array_equal(itf.read_radiance(*vp)[1], twice[1] + 2 * count)
    # a reset of the accumulation ends it
    itf.update_camera(*sc[2])
    assert itf.get_option("map_mode") == 0
    itf.compute(n)
    _frames_equal(itf.read_radiance(*vp), fresh, "after update_camera")
    itf.compute_map(count)
    assert itf.get_option("map_mode") == 1
    for reset in (lambda: itf.update_settings(0, 1, 0, 0, 0), lambda: itf.set_render_options(DEPTH, SEED, 0),
                  lambda: itf.set_partition(0, 1, 16), lambda: itf.update_viewport(*vp),
                  lambda: itf.update_scene(sc[0])):
        reset()
        assert itf.get_option("map_mode") == 0
        itf.compute_map(count)
        assert itf.get_option("map_mode") == 1


def test_device_map(wpt, oracle, itf):
    """sample_map then compute_map(NULL) equals compute_map(count_out) on a twin
    session; without a map of the current accumulation NULL is an error. The
    session's map is wpt_sample_map_host of its counts, first-hit kinds and
    (no reprojection yet) a len plane of zeros."""
    L = wpt.lib()
    sc = _scene(wpt, oracle, "cloud")
    vp = (37, 5)
    n = 2 * vp[0] * vp[1] + 7
    one = np.ones((vp[1], vp[0]), np.uint8)
    frames = []
    for twin in (False, True):
        _start(itf, sc, vp, cam=CAM_UP)
        assert L.wpt_compute_map(None) == INVALID and b"no sample map" in L.wpt_last_error()
        itf.compute(n)
        acc, cnt = itf.read_radiance(*vp)
        if not twin:
            kind = itf.first_hit(7, planes=("kind",))["kind"]
            assert (kind == 0).any() and (kind != 0).any()
            for kw in (dict(target=6, max_per_pixel=3), dict(target=6, max_per_pixel=3, budget=50),
                       dict(target=4, max_per_pixel=9, flags=gx.MISS_ONCE), dict(target=6, max_per_pixel=4, budget=61)):
                got = itf.sample_map(7, **kw)
                gx.same(got, itf.sample_map_host(cnt, np.zeros_like(cnt), kind, one, **kw), kw)
            count, (T, s) = got
            assert s == 61 < T
            itf.compute_map(None)
        else:
            itf.compute_map(count)
        frames.append(itf.read_radiance(*vp))
        assert np.array_equal(frames[-1][1], cnt + count)
        if not twin:
            # the map outlives its tracing, not a reset
            itf.compute_map(None)
            assert np.array_equal(itf.read_radiance(*vp)[1], cnt + 2 * count)
            itf.update_camera(*CAM_UP)
            assert L.wpt_compute_map(None) == INVALID
            itf.sample_map(0, 2, 2)
            itf.update_viewport(*vp)
            assert L.wpt_compute_map(None) == INVALID
            # a refused plan keeps no map
            itf.sample_map(0, 2, 2)
            assert L.wpt_sample_map(0, gx.M32, gx.M32, 0, 0, None, None) == INVALID
            assert L.wpt_compute_map(None) == INVALID
        itf.shutdown()
    _frames_equal(frames[0], frames[1], "device map against the caller's")


def _snapshot(itf, vp):
    acc, cnt = itf.read_radiance(*vp)
    st = itf.stats()
    return acc, cnt, itf.results(1, *vp), {k: v for k, v in st.items() if k not in CLOCK_STATS}, itf.kernel_times()


@pytest.mark.parametrize("session", ["nee", "init_default"])
def test_sample_map_leaves_the_session_untouched(wpt, oracle, itf, session):
    """Radiance, counts, the sampling view, wpt_stats without its clock words and
    wpt_kernel_times before and after wpt_sample_map, on a plain NEE session and on
    the init-default one (adaptive right half, sample stock)."""
    sc = _scene(wpt, oracle, "cloud")
    vp = (fh.W, fh.H)
    n = vp[0] * vp[1] * 3 + 17
    kw = {"settings": (1, 1, 0, 0), "depth": 4} if session == "nee" else {"settings": None, "depth": 0, "photons": True}
    _start(itf, sc, vp, cam=CAM_UP, **kw)
    wpt.lib().wpt_set_profiling(1)
    itf.compute(n)
    before = _snapshot(itf, vp)
    itf.sample_map(0, 8, 8)
    planned = itf.sample_map(7, 16, 5, budget=1000, flags=gx.MISS_ONCE)
    after = _snapshot(itf, vp)
    assert planned[1][1] == 1000
    for a, b, what in zip(before[:3], after[:3], ("radiance", "counts", "sampling view")):
        assert np.array_equal(_bits(a), _bits(b)), what
    assert before[3] == after[3] and before[4] == after[4]
    assert itf.get_option("map_mode") == 0
    itf.compute(n)  # and the session goes on


def test_init_default_session(wpt, oracle, itf):
    """Adaptive right half with the sample stock, uncapped depth: compute(n), then
    a map. The frame is the oracle's per pixel, the sampling view is unchanged and
    wpt_stats' paths rise by the map's total."""
    sc = _scene(wpt, oracle, "box")
    vp = (fh.W, fh.H)
    n = vp[0] * vp[1] * 3 + 17
    _start(itf, sc, vp, settings=None, depth=0, photons=True)
    itf.compute(n)
    st0 = itf.stats()
    assert st0["stock_consumed"] > 0
    acc0, cnt0 = itf.read_radiance(*vp)
    view0 = itf.results(1, *vp)
    count = _random_map(vp, 0x1D3F)
    itf.compute_map(count)
    want_acc, want_cnt, _ = _expect(sc[3], vp, sc[2], (1, 2), 0, acc0, cnt0, count)
    _frames_equal(itf.read_radiance(*vp), (want_acc, want_cnt), "init defaults")
    assert np.array_equal(itf.results(1, *vp), view0)
    assert itf.stats()["paths"] - st0["paths"] == int(count.sum())
    assert itf.get_option("map_mode") == 1


def test_the_loop(wpt, oracle, itf):
    """Scene 100 at 64 x 48: 16 spp, keep, move sideways, 1 spp, reproject, plan
    to a target of 8, trace, reproject again. Every pixel then holds at least 8
    merged samples (or is one the reprojection passes through for a non-finite
    sum), len is the same plane both times, and the map's total is the sum of
    max(8 - (1 + len), 0)."""
    sc = _scene(wpt, oracle, "box")
    vp = (fh.W, fh.H)
    npx = vp[0] * vp[1]
    cam_a, cam_b = rx.PAIRS["sideways"]
    _start(itf, sc, vp, settings=(1, 1, 0, 0), cam=cam_a)
    itf.compute(16 * npx)
    itf.reproject(0, flags=rx.KEEP)
    itf.update_camera(*cam_b)
    itf.compute(npx)
    acc, cnt = itf.read_radiance(*vp)
    assert np.all(cnt == 1)
    m_acc, m_cnt, ln = itf.reproject(0)
    assert (ln > 0).mean() > 0.5 and (ln == 0).any()
    count, (T, s) = itf.sample_map(0, target=8, max_per_pixel=8, budget=0)
    want = np.maximum(8 - (1 + ln.astype(np.int64)), 0)
    assert T == s == int(want.sum()) and np.array_equal(count, want)
    kind = itf.first_hit(0, planes=("kind",))["kind"]
    gx.same((count, (T, s)), itf.sample_map_host(cnt, ln, kind, np.ones_like(kind), 8, 8, 0, 0), "the session's len plane")
    itf.compute_map(None)
    acc2, cnt2 = itf.read_radiance(*vp)
    assert np.array_equal(cnt2, 1 + count)
    m2_acc, m2_cnt, ln2 = itf.reproject(0)
    assert np.array_equal(ln2, ln)
    through = ~np.all(np.isfinite(acc2), axis=2)
    assert np.all((m2_cnt >= 8) | through)
    print("the loop: pixels", npx, "with a history", int((ln > 0).sum()), "map total", T, "of", 7 * npx)
    # a later reset drops the len plane: the map is planned from the counts alone
    itf.update_camera(*cam_b)
    count3, (T3, _) = itf.sample_map(0, target=8, max_per_pixel=8)
    assert T3 == 8 * npx and np.all(count3 == 8)
