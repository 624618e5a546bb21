"""wpt_first_hit_rays and wpt_denoise_rays on the device.

wpt_first_hit_rays against the oracle's planes of the same rays
(tests/rayframe_fixtures.py: the adversarial sets of tests/rays_adversarial.py,
sizes around the wave and the block with invalid rays among them) and against
wpt_first_hit on wpt_primary_rays' rays; wpt_denoise_rays against its
definition, wpt_denoise_host on (wpt_radiance_rays, spp * status,
wpt_first_hit_rays) of the same call, and against wpt_denoise of a session
whose frame is the same sample. Beyond those: output selection, a clamped
grid, a grid past the query's chunk, device pointers, the session left
untouched, the argument errors, and the quality condition of the fisheye
frame. Every comparison is bit for bit unless said otherwise.
"""
import numpy as np
import pytest

import denoise_fixtures as dn
import rayframe_fixtures as rx
import rays_adversarial as ra
import rays_fixtures as rf
import reproject_fixtures as rp

pytestmark = pytest.mark.gpu

INVALID = -4
SEED, DEPTH = rf.SEED, rf.DEPTH
PLANES6 = rx.PLANES[:6]
# wpt_stats words that are host wall-clock microseconds, or count which of two
# racing events came first: no two runs of one session agree on them
CLOCK_STATS = ("plan_us", "stock_us", "stock_waits")
FH_SPILL_BYTES = 256 << 20      # kFhSpillBytes: the spill area a first-hit grid is clamped to


@pytest.fixture
def itf(wpt):
    i = wpt.interface
    yield i
    try:
        i.shutdown()
    except i.WptError:
        pass
    i.set_option("defaults", 0)


def _start(itf, scene_id, mesh=None, cam=None, vp=(8, 8), settings=(0, 1, 0, 0), depth=DEPTH, wpt=None):
    itf.init(vp[0], vp[1], scene_id, *(cam or wpt.scenes.scene_camera(scene_id)))
    if mesh is not None:
        assert itf.store_mesh(1, mesh)
    if settings is not None:
        itf.update_settings(*settings, 0)
    itf.set_render_options(depth, SEED, 0)


def _start_sc(itf, sc, vp=(8, 8), **kw):
    _start(itf, sc.scene_id, sc.mesh, sc.cam, vp, **kw)


def _against_trace_rays(itf, rays, got, what):
    """(t, id) of the valid rays equal wpt_trace_rays on them."""
    ok = got["status"].astype(bool)
    t, ids = itf.trace_rays(np.ascontiguousarray(rays[ok]))
    rx.same(got["t"][ok], t, (what, "t against trace_rays"))
    rx.same(got["id"][ok], ids, (what, "id against trace_rays"))


# ---------------------------------------------------------------------------
# 1. wpt_first_hit_rays against the oracle's planes: the adversarial sets
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ra.MESHES)
def test_mesh_sets(wpt, oracle, itf, name):
    mesh, _, rays, want = rx.mesh_planes(wpt, oracle, name)
    _start(itf, 2, mesh, wpt=wpt)
    for trav in (0, 1):
        itf.set_option("traversal", trav)
        got = itf.first_hit_rays(rays)
        print(name, trav, "visits", int(want["visits"].max()), "invalid", int((want["status"] == 0).sum()))
        rx.same_planes(got, want, (name, trav))
        _against_trace_rays(itf, rays, got, (name, trav))


@pytest.mark.parametrize("scene_id", list(ra.SHAPE_SCENES))
def test_shape_sets(wpt, oracle, itf, scene_id):
    sc, sets = rx.shape_planes(wpt, oracle, scene_id)
    _start_sc(itf, sc)
    for trav in (0, 1):
        itf.set_option("traversal", trav)
        for s, (rays, want) in sets.items():
            got = itf.first_hit_rays(rays)
            rx.same_planes(got, want, (scene_id, s, trav))
            _against_trace_rays(itf, rays, got, (scene_id, s, trav))


@pytest.mark.parametrize("name", ra.SCALED_MESHES)
def test_scaled_directions(wpt, oracle, itf, name):
    mesh, _, scaled = rx.scaled_planes(wpt, oracle, name)
    _start(itf, 2, mesh, wpt=wpt)
    for trav in (0, 1):
        itf.set_option("traversal", trav)
        for s, (rays, want) in scaled.items():
            got = itf.first_hit_rays(rays)
            rx.same_planes(got, want, (name, s, trav))
            _against_trace_rays(itf, rays, got, (name, s, trav))


# ---------------------------------------------------------------------------
# 2. Sizes around the wave and the block, invalid rays among valid ones
# ---------------------------------------------------------------------------
def test_sizes(wpt, oracle, itf):
    sc, rays, want = rx.box_rays(wpt, oracle)
    _start_sc(itf, sc)
    for n in (1, 63, 64, 65, 255, 256, 257, 1025):
        got = itf.first_hit_rays(rays[:n])
        assert all(got[k].shape[0] == n for k in rx.PLANES)
        rx.same_planes(got, {k: v[:n] for k, v in want.items()}, ("n", n))


INVALID_LAYOUTS = {
    "lane 0 and lane 63": [0, 63, 64, 127, 128 + 63, 1024],
    "a whole wave": list(range(64, 128)),
    "a whole block": list(range(256, 512)),
    "a wave and a block": list(range(128, 192)) + list(range(512, 768)),
}


@pytest.mark.parametrize("layout", list(INVALID_LAYOUTS))
def test_invalid_rays_among_valid_ones(wpt, oracle, itf, layout):
    sc, rays, want = rx.box_rays(wpt, oracle)
    where = np.array(INVALID_LAYOUTS[layout])
    bad = rx.with_invalid(rays, where)
    assert not rf.valid(bad)[where].any()
    _start_sc(itf, sc)
    got = itf.first_hit_rays(bad)
    rx.same_planes(got, rx.masked(want, where), layout)  # the invalid entries, and every neighbour unchanged


def test_only_invalid_rays(wpt, oracle, itf):
    sc, rays, _ = rx.box_rays(wpt, oracle)
    _start_sc(itf, sc)
    for n in (1, 64, 300):
        bad = rx.with_invalid(rays[:n], np.arange(n))
        rx.same_planes(itf.first_hit_rays(bad), rx.invalid_planes(n), ("only invalid", n))


# ---------------------------------------------------------------------------
# 3. Equality with wpt_first_hit on wpt_primary_rays' rays
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cloud", "museum", "box", "spheres"])
@pytest.mark.parametrize("vp", [(37, 5), (130, 70)], ids=lambda v: f"{v[0]}x{v[1]}")
def test_equals_first_hit(wpt, oracle, itf, name, vp):
    sc = rf.scene(wpt, oracle, name)
    _start_sc(itf, sc, vp)
    for s in (0, 7):
        g = itf.first_hit(s)
        got = itf.first_hit_rays(sc.rays(vp, s))
        assert got["status"].all()
        for k in PLANES6:
            rx.same(got[k], g[k], (name, vp, s, k))
        rx.same(sc.rays(vp, s)[:, 3:], g["dir"], (name, vp, s, "dir"))


# ---------------------------------------------------------------------------
# 4. Output selection
# ---------------------------------------------------------------------------
def _snapshot(itf):
    return {k: v for k, v in itf.stats().items() if k not in CLOCK_STATS}, itf.kernel_times()


def test_output_selection(wpt, oracle, itf):
    sc, rays, _ = rx.box_rays(wpt, oracle)
    rays = np.ascontiguousarray(rx.with_invalid(rays[:300], [5, 64]))
    n = len(rays)
    _start_sc(itf, sc)
    itf.compute(200)
    full = itf.first_hit_rays(rays)
    L = wpt.lib()
    snap = _snapshot(itf)
    assert L.wpt_first_hit_rays(n, rays.ctypes.data, 0, *[None] * 7) == 0
    assert L.wpt_first_hit_rays(n, None, 0, *[None] * 7) == 0
    sentinel = np.full(4, 7.25, np.float32)
    assert L.wpt_first_hit_rays(0, rays.ctypes.data, 0, sentinel.ctypes.data, *[None] * 6) == 0
    assert L.wpt_first_hit_rays(0, None, 0, sentinel.ctypes.data, *[None] * 6) == 0
    assert np.all(sentinel == np.float32(7.25))
    assert _snapshot(itf) == snap
    for subset in [(k,) for k in rx.PLANES] + [("visits", "t"), ("kind", "status")]:
        rx.same_planes(itf.first_hit_rays(rays, planes=subset), full, subset, subset)
        bufs, ptr = {}, [None] * 7
        for k in rx.PLANES:
            pos, dt, comp = itf.FIRST_HIT_RAYS_PLANES[k]
            bufs[k] = np.frombuffer(b"\xa5" * (n * comp * np.dtype(dt).itemsize), dtype=dt).copy()
            if k in subset:
                ptr[pos] = bufs[k].ctypes.data
        assert L.wpt_first_hit_rays(n, rays.ctypes.data, 0, *ptr) == 0
        for k in rx.PLANES:
            if k in subset:
                rx.same(bufs[k], full[k].reshape(-1), (subset, k))
            else:
                assert np.all(bufs[k].view(np.uint8) == 0xA5), (subset, k)
    assert _snapshot(itf) == snap  # neither counted nor timed


# ---------------------------------------------------------------------------
# 5. A clamped grid: blocks take a second trip
# ---------------------------------------------------------------------------
def test_clamped_grid(wpt, oracle, itf):
    """One launch over more rays than its grid covers in one trip. The grid is
    min(ceil(n / 256), 256 MiB / (spill slots * 256 lanes * 8 B)) blocks, spill
    slots = max(stack cap - 9, 1), stack cap = max(BVH2 depth + 2, 3 * BVH4
    depth + 4): on the box under the exact BVH2 (no BVH4: depth 0) that is one
    slot unless the tree is deeper than 8, 131,072 blocks, 33,554,432 rays a
    trip. A deeper stack than assumed only lowers the clamp. Host rays go
    through in chunks of 2^21, which never reach it, so the rays are device
    tensors: the box rays tiled as rays_adversarial.chunk_case tiles them."""
    import torch

    sc, base, _ = ra.chunk_case(wpt, oracle)
    _start_sc(itf, sc)
    itf.set_option("traversal", 0)
    slots = max(max(itf.bvh_depth() + 2, 4) - rx.LDS_SLOTS, 1)
    trip = FH_SPILL_BYTES // (slots * rx.BLOCK * 8) * rx.BLOCK
    n = trip + rx.BLOCK + 1
    print("clamped grid: spill slots", slots, "rays per trip", trip, "n", n)
    assert trip % rx.BLOCK == 0 and n < 1 << 32
    names = ("t", "id", "kind")
    want = itf.first_hit_rays(base, planes=names)
    rx.same_planes(want, rx.expected_planes(oracle, sc.ref, itf.DebugScene(100, None).materials(), base), "base", names)
    dev = torch.device("cuda", torch.cuda.current_device())
    index = torch.arange(n, device=dev) % ra.CHUNK_BASE
    d_rays = torch.from_numpy(np.array(base)).to(dev)[index].contiguous()
    got = itf.first_hit_rays(d_rays, planes=names, device=True)
    for k in names:
        w = torch.from_numpy(rx.bits(want[k]).view(np.int32 if want[k].dtype != np.uint8 else np.uint8)).to(dev)[index]
        g = got[k].view(torch.int32) if got[k].dtype != torch.uint8 else got[k]
        bad = int((g != w).sum().item())
        assert bad == 0, (k, bad, "of", n, "first", int(torch.nonzero(g != w)[0].item()))


# ---------------------------------------------------------------------------
# 6. Device pointers
# ---------------------------------------------------------------------------
def test_first_hit_rays_device_pointers(wpt, oracle, itf):
    import torch

    sc, rays, want = rx.box_rays(wpt, oracle)
    rays = rx.with_invalid(rays[:257], [100])
    _start_sc(itf, sc)
    host = itf.first_hit_rays(rays)
    dev = torch.device("cuda", torch.cuda.current_device())
    d_rays = torch.from_numpy(rays).to(dev)
    got = itf.first_hit_rays(d_rays, device=True)
    for k in rx.PLANES:
        assert got[k].device == d_rays.device
        rx.same(got[k].cpu().numpy(), host[k], ("device pointers", k))
    rx.same_planes(host, rx.masked({k: v[:257] for k, v in want.items()}, [100]), "host pointers")
    one = itf.first_hit_rays(d_rays, planes=("status",), device=True)
    assert np.array_equal(one["status"].cpu().numpy(), host["status"]) and host["status"].sum() == 256
    assert np.array_equal(d_rays.cpu().numpy().view(np.uint32), rays.view(np.uint32))  # the input is only read


def test_denoise_rays_device_pointers(wpt, oracle, itf):
    import torch

    sc = rf.scene(wpt, oracle, "box")
    w, h = 37, 5
    rays = np.array(rx.fisheye(vp=(w, h)), copy=True)
    keys = np.random.default_rng(5).integers(0, 1 << 31, w * h).astype(np.uint32)
    _start_sc(itf, sc)
    dev = torch.device("cuda", torch.cuda.current_device())
    d_rays = torch.from_numpy(rays).to(dev)
    d_keys = torch.from_numpy(keys.view(np.int32)).to(dev)
    for k, dk in ((None, None), (keys, d_keys)):
        s0 = itf.stats()
        host = itf.denoise_rays(rays, w, h, k, 2, 3, 1)
        s1 = itf.stats()
        got = itf.denoise_rays(d_rays, w, h, dk, 2, 3, 1, device=True)
        s2 = itf.stats()
        for name in itf.DENOISE_RAYS_OUTPUTS:
            assert got[name].device == d_rays.device
            rx.same(got[name].cpu().numpy(), host[name], ("device pointers", name, k is not None))
        assert all(s2[c] - s1[c] == s1[c] - s0[c] for c in ("paths", "rays", "shadow_rays"))
        one = itf.denoise_rays(d_rays, w, h, dk, 2, 3, 1, outputs=("rgba",), device=True)
        rx.same(one["rgba"].cpu().numpy(), host["rgba"], "rgba alone")
    assert 0 < host["status"].sum() < w * h
    assert np.array_equal(d_rays.cpu().numpy().view(np.uint32), rays.view(np.uint32))


# ---------------------------------------------------------------------------
# 7. wpt_denoise_rays against the host composition
# ---------------------------------------------------------------------------
def _composition(itf, wpt, rays, w, h, keys, sample, spp, rtype, it, sc_, sz, fl):
    """wpt_denoise_host on (wpt_radiance_rays, spp * status, wpt_first_hit_rays) of the same call."""
    raw, status = itf.radiance_rays(rays, keys, sample, spp, rtype)
    planes = itf.first_hit_rays(rays, planes=rx.GUIDES)
    return raw, status, rx.host_filter(wpt, w, h, raw, status, spp, planes, it, sc_, sz, fl)


def _check_call(itf, wpt, rays, w, h, keys, sample, spp, rtype, it, fl, what, sc_=dn.SIGMA_C, sz=dn.SIGMA_Z):
    raw, status, want = _composition(itf, wpt, rays, w, h, keys, sample, spp, rtype, it, sc_, sz, fl)
    got = itf.denoise_rays(rays, w, h, keys, sample, spp, rtype, it, sc_, sz, fl)
    rx.same(got["raw"], raw, (what, "raw"))
    rx.same(got["status"], status, (what, "status"))
    dn.same((got["rgb"], got["valid"], got["rgba"]), want, what)
    return got


@pytest.mark.parametrize("vp", dn.GPU_VIEWPORTS, ids=lambda v: f"{v[0]}x{v[1]}")
def test_fisheye_against_the_host_composition(wpt, oracle, itf, vp):
    """Grids cut from the fisheye at (0, 1, -1.5) on scene 100: iterations 1..5,
    both dn_flags, WPT_OPT_DENOISE_LDS 0 and 7, spp 1 and 4, NoNEE and NEE, one
    case with keys; raw3 and status against the oracle's radiance_rays."""
    w, h = vp
    sc = rf.scene(wpt, oracle, "box")
    rays = rx.fisheye(vp=vp)
    _start_sc(itf, sc)
    keys = np.random.default_rng(w * 1000 + h).integers(0, 1 << 32, w * h, dtype=np.uint64).astype(np.uint32)
    for lds in (0, 7):
        itf.set_option("denoise_lds", lds)
        for it in range(1, 6):
            fl = it & 1
            _check_call(itf, wpt, rays, w, h, None, 0, 4, 1, it, fl, (vp, lds, it, fl, "NEE 4 spp"))
            _check_call(itf, wpt, rays, w, h, None, 3, 1, 0, it, fl ^ 1, (vp, lds, it, fl ^ 1, "NoNEE 1 spp"))
    got = _check_call(itf, wpt, rays, w, h, keys, 5, 4, 0, 3, 1, (vp, "keys"))
    for rtype, k, sample, spp in ((0, keys, 5, 4), (1, None, 0, 4)):
        o_rgb, o_status, _ = ra.expect(sc.ref, ("fisheye", vp), rays, k, sample, spp, rtype)
        g = got if k is not None else itf.denoise_rays(rays, w, h, None, sample, spp, rtype, outputs=("raw", "status"))
        rx.same(g["raw"].reshape(-1, 3), o_rgb, (vp, rtype, "raw against the oracle"))
        rx.same(g["status"].reshape(-1), o_status, (vp, rtype, "status against the oracle"))


@pytest.mark.parametrize("vp", dn.GPU_VIEWPORTS, ids=lambda v: f"{v[0]}x{v[1]}")
def test_cloud_frame_against_the_host_composition(wpt, oracle, itf, vp):
    """A wpt_primary_rays frame on scene 2 (cloud)."""
    w, h = vp
    sc = rf.scene(wpt, oracle, "cloud")
    rays = sc.rays(vp, 0)
    _start_sc(itf, sc)
    for lds in (0, 7):
        itf.set_option("denoise_lds", lds)
        for it in range(1, 6):
            fl = (it & 1) ^ 1
            _check_call(itf, wpt, rays, w, h, None, 0, 4 if it & 1 else 1, it & 1, it, fl, (vp, lds, it, fl))


# ---------------------------------------------------------------------------
# 8. wpt_denoise_rays against the session's wpt_denoise
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("rtype", [0, 1], ids=["NoNEE", "NEE"])
@pytest.mark.parametrize("vp", [(64, 48), (37, 5)], ids=lambda v: f"{v[0]}x{v[1]}")
def test_equals_the_session(wpt, oracle, itf, rtype, vp):
    """One sample per pixel is the only case in which the session's and the
    query's primary rays coincide: a session with both halves of one render
    type that traced exactly W * H paths, filtered, against the query of
    wpt_primary_rays(W, H, cam, seed, 0) at spp 1, sample 0. wpt_compute deals
    its paths to the two screen halves evenly, so on an odd width (37: 18 and
    19 columns) W * H paths leave pixels with two samples and pixels with none;
    there the W * H paths are traced as a sample map of one sample per pixel."""
    w, h = vp
    sc = rf.scene(wpt, oracle, "box")
    _start_sc(itf, sc, vp, settings=(rtype, rtype, 0, 0))
    if w % 2 == 0:
        itf.compute(w * h)
    else:
        itf.compute_map(np.ones((h, w), np.uint32))
    acc, cnt = itf.read_radiance(w, h)
    assert np.all(cnt == 1)
    for fl in (0, 1):
        want = itf.denoise(0, flags=fl)
        got = itf.denoise_rays(sc.rays(vp, 0), w, h, None, 0, 1, rtype, flags=fl)
        dn.same((got["rgb"], got["valid"], got["rgba"]), want, (vp, rtype, fl))
        rx.same(got["raw"], acc, (vp, rtype, "raw is the frame"))
        assert got["status"].all()


# ---------------------------------------------------------------------------
# 9. Stats, the query's chunk
# ---------------------------------------------------------------------------
def test_stats_are_the_bare_query(wpt, oracle, itf):
    sc = rf.scene(wpt, oracle, "box")
    rays = rx.fisheye()
    _start_sc(itf, sc)
    snaps = [_snapshot(itf)[0]]
    itf.radiance_rays(rays, None, 0, 4, 1)
    snaps.append(_snapshot(itf)[0])
    itf.denoise_rays(rays, rx.FISH_W, rx.FISH_H, None, 0, 4, 1)
    snaps.append(_snapshot(itf)[0])
    itf.denoise_rays(rays, rx.FISH_W, rx.FISH_H, None, 0, 4, 1, outputs=("rgba",))
    snaps.append(_snapshot(itf)[0])
    d = [{k: b[k] - a[k] for k in a} for a, b in zip(snaps, snaps[1:])]
    assert d[0]["paths"] == 4 * (rx.FISH_W * rx.FISH_H - rx.FISH_INVALID) and d[0]["shadow_rays"] > 0
    assert d[1] == d[0] and d[2] == d[0], {k: (d[0][k], d[1][k], d[2][k]) for k in d[0] if not d[0][k] == d[1][k] == d[2][k]}


def test_past_the_query_chunk(wpt, oracle, itf):
    """A 2048 x 1025 grid of tiled box rays (2^21 + 2048 rays: two chunks of the
    query) is filtered as one frame; the filter's scratch grows well past the
    64 x 48 session's, whose wpt_denoise still equals the host afterwards."""
    w, h = 2048, 1025
    assert w * h > ra.CHUNK
    sc, base, _ = ra.chunk_case(wpt, oracle)
    vp = (64, 48)
    _start_sc(itf, sc, vp, settings=(0, 0, 0, 0), depth=1)
    itf.compute(vp[0] * vp[1] * 2)
    rays = np.ascontiguousarray(base[np.arange(w * h) % ra.CHUNK_BASE])
    raw, status, want = _composition(itf, wpt, rays, w, h, None, 0, 1, 0, 2, dn.SIGMA_C, dn.SIGMA_Z, 1)
    got = itf.denoise_rays(rays, w, h, None, 0, 1, 0, 2, dn.SIGMA_C, dn.SIGMA_Z, 1)
    rx.same(got["raw"], raw, "raw")
    rx.same(got["status"], status, "status")
    dn.same((got["rgb"], got["valid"], got["rgba"]), want, "2048 x 1025")
    assert status.all() and (raw[ra.CHUNK:] != 0).any()
    acc, cnt = itf.read_radiance(*vp)
    g = itf.first_hit(0)
    host = itf.denoise_host(acc, cnt, g["t"], g["normal"], g["albedo"], g["kind"])
    dn.same(itf.denoise(0), host, "the session's filter after the large grid")


# ---------------------------------------------------------------------------
# 10. The session is not touched
# ---------------------------------------------------------------------------
def _state(itf, vp):
    acc, cnt = itf.read_radiance(*vp)
    st = {k: v for k, v in itf.stats().items() if k not in CLOCK_STATS}
    return {"radiance": acc, "counts": cnt, "sampling": itf.results(1, *vp), "stats": st,
            "options": {k: itf.get_option(k) for k in ("history", "map_mode")}}


def _states_equal(a, b, what, skip=()):
    for k in a:
        if k in skip:
            continue
        if isinstance(a[k], dict):
            assert a[k] == b[k], (what, k, {j: (a[k][j], b[k][j]) for j in a[k] if a[k][j] != b[k][j]})
        else:
            rx.same(a[k], b[k], (what, k))


def _calls(itf, sc, which):
    """The call under test in the middle of a session; returns nothing of it."""
    rays = rx.fisheye()
    if which == "first_hit_rays":
        got = itf.first_hit_rays(rays)
        assert 0 < got["status"].sum() < len(rays) and (got["kind"] == 2).any()
    else:
        got = itf.denoise_rays(rays, rx.FISH_W, rx.FISH_H, None, 1, 2, 1)
        assert got["valid"].any() and (got["raw"] != 0).any()


@pytest.mark.parametrize("which", ["first_hit_rays", "denoise_rays"])
def test_random_session_untouched(wpt, oracle, itf, which):
    """Two random halves (NoNEE | NEE), a cut mid-round: the state is the same
    right after the call (wpt_denoise_rays counts its paths and rays as the
    query does, nothing else), wpt_denoise gives what it gave before, and the
    compute that completes the rounds equals the oracle."""
    sc = rf.scene(wpt, oracle, "box")
    vp = (16, 16)
    npx = vp[0] * vp[1]
    _start_sc(itf, sc, vp, settings=(0, 1, 0, 0))
    itf.compute(npx + 78)
    before = _state(itf, vp)
    assert before["counts"].min() < before["counts"].max()
    d0 = itf.denoise(0)
    _calls(itf, sc, which)
    after = _state(itf, vp)
    _states_equal(before, after, which, skip=() if which == "first_hit_rays" else ("stats",))
    dn.same(itf.denoise(0), d0, "wpt_denoise after the call: the guide buffers were not disturbed")
    itf.compute(2 * npx - 78)
    acc, cnt = itf.read_radiance(*vp)
    want, _ = sc.ref.render(vp[0], vp[1], sc.cam, 0, 1, DEPTH, SEED, 0, 3, threads=4)
    assert np.all(cnt == 3)
    rx.same(acc, want, (which, "the following compute against the oracle"))


@pytest.mark.parametrize("which", ["first_hit_rays", "denoise_rays"])
def test_init_default_session_untouched(wpt, oracle, itf, which):
    """The init-default session (NEE random + PNEE adaptive, the sample stock on)
    with a kept history and a planned sample map: the same checks, the following
    compute against a twin session without the call."""
    import pnee_fixtures as pf

    sc = rf.scene(wpt, oracle, "box")
    vp = (16, 16)
    ends = []
    for call in (True, False):
        _start_sc(itf, sc, vp, settings=None)
        itf.install_photons(pf.octants())
        itf.compute(300)
        itf.reproject(0, flags=rp.KEEP)
        itf.sample_map(0, target=6, max_per_pixel=6)
        before = _state(itf, vp)
        assert before["counts"].min() < before["counts"].max() and before["options"]["history"] == 2
        d0 = itf.denoise(0)
        if call:
            _calls(itf, sc, which)
            _states_equal(before, _state(itf, vp), which, skip=() if which == "first_hit_rays" else ("stats",))
            dn.same(itf.denoise(0), d0, "wpt_denoise after the call")
        itf.compute(3000)
        end = _state(itf, vp)
        assert end["stats"]["stock_consumed"] > 0
        ends.append(end)
        itf.shutdown()
    _states_equal(ends[0], ends[1], (which, "against the twin"), skip=() if which == "first_hit_rays" else ("stats",))


# ---------------------------------------------------------------------------
# 11. Argument errors
# ---------------------------------------------------------------------------
def test_first_hit_rays_argument_errors(wpt, oracle, itf):
    sc, rays, _ = rx.box_rays(wpt, oracle)
    rays = np.ascontiguousarray(rays[:20])
    _start_sc(itf, sc)
    L = wpt.lib()
    bufs = {}
    for k in rx.PLANES:
        _, dt, comp = itf.FIRST_HIT_RAYS_PLANES[k]
        bufs[k] = np.frombuffer(b"\xa5" * (20 * comp * np.dtype(dt).itemsize), dtype=dt).copy()
    out = [bufs[k].ctypes.data for k in sorted(bufs, key=lambda k: itf.FIRST_HIT_RAYS_PLANES[k][0])]
    r = rays.ctypes.data
    snap = _snapshot(itf)
    for c in ((20, None, 0), (20, r, 2), (20, r, 0x80000000), (1 << 32, r, 0), (20, None, 1)):
        assert L.wpt_first_hit_rays(*c, *out) == INVALID, c
        assert len(L.wpt_last_error()) > 0
    assert L.wpt_first_hit_rays(20, None, 0, *[None] * 6, out[6]) == INVALID  # status alone is an output wanted
    assert all(np.all(b.view(np.uint8) == 0xA5) for b in bufs.values())
    assert _snapshot(itf) == snap
    assert L.wpt_first_hit_rays(20, r, 0, *out) == 0 and bufs["status"].all()


def test_denoise_rays_argument_errors(wpt, oracle, itf):
    sc = rf.scene(wpt, oracle, "box")
    w, h = 5, 4
    rays = np.ascontiguousarray(rx.fisheye(vp=(w, h)))
    keys = np.arange(w * h, dtype=np.uint32)
    _start_sc(itf, sc)
    L = wpt.lib()
    rgb = np.full((h, w, 3), 7.25, np.float32)
    raw = np.full((h, w, 3), 7.25, np.float32)
    valid, status = np.full((h, w), 9, np.uint8), np.full((h, w), 9, np.uint8)
    rgba = np.full((h, w, 4), 9, np.uint8)
    o = (rgb.ctypes.data, valid.ctypes.data, rgba.ctypes.data, raw.ctypes.data, status.ctypes.data)
    r, k = rays.ctypes.data, keys.ctypes.data
    nan, inf = float("nan"), float("inf")
    snap = _snapshot(itf)
    #        W  H  rays keys sample spp type it sc   sz   dn_flags flags
    good = (w, h, r, k, 0, 1, 1, 3, 1.0, 0.1, 0, 0)
    bad = {0: 0, 1: 0, 2: None, 5: 0, 6: 3, 7: 0, 8: 0.0, 9: -1.0, 10: 2, 11: 2}
    cases = [good[:i] + (v,) + good[i + 1:] for i, v in bad.items()]
    cases += [good[:7] + (6,) + good[8:], good[:8] + (nan,) + good[9:], good[:9] + (inf,) + good[10:],
              good[:11] + (0x80000000,), good[:4] + (0xFFFFFFFF, 2) + good[6:], (1 << 16, 1 << 16) + good[2:],
              good[:10] + (0x80000000,) + good[11:]]
    for c in cases:
        assert L.wpt_denoise_rays(*c, *o) == INVALID, c
        assert len(L.wpt_last_error()) > 0
    assert np.all(rgb == np.float32(7.25)) and np.all(raw == np.float32(7.25))
    assert np.all(valid == 9) and np.all(status == 9) and np.all(rgba == 9)
    assert _snapshot(itf) == snap
    # all outputs NULL: nothing is launched
    assert L.wpt_denoise_rays(*good, None, None, None, None, None) == 0
    assert _snapshot(itf) == snap
    assert L.wpt_denoise_rays(*good, *o) == 0 and 0 < status.sum() < w * h


# ---------------------------------------------------------------------------
# 12. It helps
# ---------------------------------------------------------------------------
def test_the_filter_helps_the_fisheye_frame(wpt, oracle, itf):
    """Scene 100, the fisheye at (0, 1, -1.5), 64 x 48, NEE, depth cap 4, the
    defaults with dn_flags 0: the error of the 4-spp call's rgb3 is below half
    the error of its raw3 / 4, both the relative L2 of clamp(., 0, 1) over the
    valid pixels against the 1,024-spp raw3 / 1024 of samples 1000..2023. The
    oracle's frames through wpt_denoise_host gave 0.5476 -> 0.2063 (0.377),
    0.4745 -> 0.1828 (0.385) and 0.4448 -> 0.1776 (0.399) at the three origins
    (tests/test_rayframe_cpu.py prints them). The condition is asserted at the
    first origin; the other two are printed beside it."""
    sc = rf.scene(wpt, oracle, "box")
    _start_sc(itf, sc)
    print("origin | raw 4 spp | filtered | ratio")
    for i, origin in enumerate(rx.FISH_ORIGINS):
        rays = rx.fisheye(origin)
        got = itf.denoise_rays(rays, rx.FISH_W, rx.FISH_H, None, 0, rx.FISH_SPP, 1, flags=0)
        ref = itf.denoise_rays(rays, rx.FISH_W, rx.FISH_H, None, rx.FISH_REF[0], rx.FISH_REF[1], 1,
                               outputs=("raw",))["raw"] / np.float32(rx.FISH_REF[1])
        m = got["status"].astype(bool)
        raw_e = rx.clamp_error(got["raw"] / np.float32(rx.FISH_SPP), ref, m)
        fil_e = rx.clamp_error(got["rgb"], ref, m)
        print(f"{origin} | {raw_e:.4f} | {fil_e:.4f} | {fil_e / raw_e:.3f}")
        assert np.array_equal(got["valid"], got["status"]) and int((~m).sum()) == rx.FISH_INVALID
        if i == 0:
            assert fil_e < rx.HELP_RATIO * raw_e, (origin, raw_e, fil_e)
