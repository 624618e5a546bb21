"""Primary rays shaded by their generator on the device (WPT_OPT_GEN_SHADE).

k_generate_shade shades a primary ray it resolves at once instead of writing
it to the back of stream 0 for k_shade(0) to read back. Such a ray is in no
stream; it is counted in its own slot and reported as `gen_shaded_rays`, a
part of `presolved_rays`. Frames, sample counts and every other count must be
the same bits with the option on, off and without the presolve, and equal the
oracle's. PNEE and stock batches keep k_generate_ps.

The shares of resolved primary rays asserted below are the host presolve's
(DebugScene.presolve) at pixel centres, on the CPU objects alone.
"""
import numpy as np
import pytest

from test_presolve import camera_rays, scene_mesh

pytestmark = pytest.mark.gpu

SEED = 0xBABABEBE
COUNTS = ("paths", "rays", "shadow_rays", "bounces", "presolved_rays", "dropped_rays", "shadow_presolved_rays")
SKY = (0.0, 5.0, -3.0, -1.0, 3.14159)  # up and away from the back wall, the lights behind it


@pytest.fixture
def itf(wpt):
    i = wpt.interface
    yield i
    try:
        i.shutdown()
    except i.WptError:
        pass
    i.set_option("defaults", 0)


def _render(itf, wpt, scene_id, W, H, spp, depth, mesh=None, cam=None, lanes=None, partition=None, types=(1, 1),
            debug=0, **opts):
    """One progressive session: (acc, cnt, stats, this rank's pixels)."""
    cam = cam if cam is not None else wpt.scenes.scene_camera(scene_id)
    for k, v in opts.items():
        itf.set_option(k, v)  # the defaults of the init below
    itf.init(W, H, scene_id, *cam)
    try:
        if mesh is not None:
            itf.store_mesh(1, mesh)
        itf.update_settings(types[0], types[1], 0, 0, debug)
        itf.set_render_options(depth, SEED, 0)
        if lanes is not None:
            itf.set_lanes(lanes)
        if partition is not None:
            itf.set_partition(partition[0], partition[1], 16)
        px = itf.partition_pixels()
        itf.compute(len(px) * spp)
        acc, cnt = itf.read_radiance(W, H)
        st = itf.stats()
    finally:
        itf.shutdown()
        itf.set_option("defaults", 0)
    return acc, cnt, st, px


def _same(a, b):
    return np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


_REF = {}


def _oracle(oracle, scene_id, mesh, W, H, cam, depth, spp, types=(1, 1), debug=0):
    key = (scene_id, W, H, tuple(cam), depth, spp, types, debug)
    if key not in _REF:
        _REF[key] = oracle.OracleScene(scene_id, mesh).render(W, H, cam, types[0], types[1], depth, SEED, 0, spp,
                                                              threads=4, light_debug=debug)
    return _REF[key]


_SHARES = {}


def _shares(wpt, scene_id, W, H, cam=None):
    """Host presolve of the camera's rays at pixel centres: (plane, miss, unresolved) shares."""
    key = (scene_id, W, H, None if cam is None else tuple(cam))
    if key not in _SHARES:
        dbg = wpt.interface.DebugScene(scene_id, scene_mesh(wpt, scene_id))
        res, _, ids = dbg.presolve(camera_rays(wpt, scene_id, W, H, cam))
        res = res.astype(bool)
        _SHARES[key] = (float(np.mean(res & (ids >= 0))), float(np.mean(res & (ids < 0))), float(np.mean(~res)))
    return _SHARES[key]


def _check_counts(on, off, keys=COUNTS):
    for k in keys:
        assert on[2][k] == off[2][k], (k, on[2][k], off[2][k])
    assert off[2]["gen_shaded_rays"] == 0


# the separate kernels (k_extend, k_shade, k_shadow) and the fused k_trace; lanes 1 and 4
FORMS = [("separate", {"fused": 0, "fused_below": 0}, 1), ("separate", {"fused": 0, "fused_below": 0}, 4),
         ("fused", {"fused": 1, "fused_below": 0}, 1), ("fused", {"fused": 1, "fused_below": 0}, 4)]


@pytest.mark.parametrize("form,opts,lanes", FORMS)
@pytest.mark.parametrize("depth", [8, 2, 1])
def test_scene2_on_off_and_without_presolve(wpt, oracle, itf, form, opts, lanes, depth):
    W, H, spp = 64, 48, 4
    plane, miss, unres = _shares(wpt, 2, W, H)
    assert abs(plane - 0.904) < 0.0005 and miss == 0.0, (plane, miss, unres)
    mesh = scene_mesh(wpt, 2)
    cam = wpt.scenes.scene_camera(2)
    on = _render(itf, wpt, 2, W, H, spp, depth, mesh, lanes=lanes, gen_shade=1, **opts)
    off = _render(itf, wpt, 2, W, H, spp, depth, mesh, lanes=lanes, gen_shade=0, **opts)
    nops = _render(itf, wpt, 2, W, H, spp, depth, mesh, lanes=lanes, presolve=0, **opts)
    ref, rst = _oracle(oracle, 2, mesh, W, H, cam, depth, spp)
    print(f"{form} lanes {lanes} depth {depth}: rays {on[2]['rays']}, presolved {on[2]['presolved_rays']}, "
          f"gen-shaded {on[2]['gen_shaded_rays']}")
    assert np.all(on[1] == spp)
    assert _same(on, off) and _same(on, nops)
    assert np.array_equal(on[0].view(np.uint32), ref.view(np.uint32))
    _check_counts(on, off)
    for k in ("rays", "shadow_rays", "paths", "bounces"):
        assert on[2][k] == nops[2][k], k
    assert on[2]["rays"] + on[2]["shadow_rays"] == rst["rays"]
    assert nops[2]["gen_shaded_rays"] == 0
    assert 0 < on[2]["gen_shaded_rays"] <= on[2]["presolved_rays"]
    assert on[2]["gen_shaded_rays"] <= W * H * spp


@pytest.mark.parametrize("drop_miss", [0, 1])
@pytest.mark.parametrize("presolve_shadow", [0, 1])
def test_with_the_other_presolve_options(wpt, oracle, itf, drop_miss, presolve_shadow):
    W, H, spp, depth = 64, 48, 4, 8
    mesh = scene_mesh(wpt, 2)
    cam = wpt.scenes.scene_camera(2)
    o = {"drop_miss": drop_miss, "presolve_shadow": presolve_shadow}
    on = _render(itf, wpt, 2, W, H, spp, depth, mesh, gen_shade=1, **o)
    off = _render(itf, wpt, 2, W, H, spp, depth, mesh, gen_shade=0, **o)
    ref, rst = _oracle(oracle, 2, mesh, W, H, cam, depth, spp)
    assert _same(on, off)
    assert np.array_equal(on[0].view(np.uint32), ref.view(np.uint32))
    _check_counts(on, off)
    assert on[2]["rays"] + on[2]["shadow_rays"] == rst["rays"]
    assert 0 < on[2]["gen_shaded_rays"] <= on[2]["presolved_rays"]
    assert (on[2]["dropped_rays"] > 0) == bool(drop_miss)
    assert (on[2]["shadow_presolved_rays"] > 0) == bool(presolve_shadow)


@pytest.mark.parametrize("types,debug", [((0, 0), 0), ((1, 1), 0), ((0, 1), 0), ((1, 1), 1)])
def test_render_types_and_debug_mode(wpt, oracle, itf, types, debug):
    W, H, spp, depth = 64, 48, 4, 8
    mesh = scene_mesh(wpt, 2)
    cam = wpt.scenes.scene_camera(2)
    on = _render(itf, wpt, 2, W, H, spp, depth, mesh, types=types, debug=debug, gen_shade=1)
    off = _render(itf, wpt, 2, W, H, spp, depth, mesh, types=types, debug=debug, gen_shade=0)
    ref, rst = _oracle(oracle, 2, mesh, W, H, cam, depth, spp, types, debug)
    assert _same(on, off)
    assert np.array_equal(on[0].view(np.uint32), ref.view(np.uint32))
    _check_counts(on, off)
    assert on[2]["rays"] + on[2]["shadow_rays"] == rst["rays"]
    assert 0 < on[2]["gen_shaded_rays"] <= on[2]["presolved_rays"]


@pytest.mark.parametrize("W,H,spp,lanes", [(50, 37, 3, 1), (50, 37, 3, 4), (7, 5, 1, 1)])
def test_odd_batches(wpt, oracle, itf, W, H, spp, lanes):
    """5 550 paths: a partial last block; 35 paths: less than one block. (An odd
    width's halves differ in size and a call gives each half of its paths, as
    the reference does: the 7 x 5 frame is compared with the oracle's session.)"""
    depth = 8
    mesh = scene_mesh(wpt, 2)
    cam = wpt.scenes.scene_camera(2)
    on = _render(itf, wpt, 2, W, H, spp, depth, mesh, lanes=lanes, gen_shade=1)
    off = _render(itf, wpt, 2, W, H, spp, depth, mesh, lanes=lanes, gen_shade=0)
    assert _same(on, off)
    _check_counts(on, off)
    assert on[2]["paths"] == W * H * spp
    if W % 2 == 0:
        ref, rst = _oracle(oracle, 2, mesh, W, H, cam, depth, spp)
        assert np.all(on[1] == spp)
        assert on[2]["rays"] + on[2]["shadow_rays"] == rst["rays"]
    else:
        ses = oracle.OracleScene(2, mesh).adaptive(W, H, cam, (1, 1), (0, 0), depth)
        ses.compute(W * H * spp)
        ref, cnt_r, _ = ses.read()
        assert np.array_equal(on[1], cnt_r)
    assert np.array_equal(on[0].view(np.uint32), ref.view(np.uint32))
    assert 0 < on[2]["gen_shaded_rays"] <= on[2]["presolved_rays"] <= on[2]["rays"]


def test_session_of_calls_that_cut_rounds(wpt, oracle, itf):
    """Partial rounds in raster order: on against off and the oracle after every call."""
    W, H, depth = 40, 24, 8
    mesh = scene_mesh(wpt, 2)
    cam = wpt.scenes.scene_camera(2)
    chunks = (W * H * 2 + 17, 211, W * H)
    out = {}
    for gs in (1, 0):
        itf.set_option("gen_shade", gs)
        itf.init(W, H, 2, *cam)
        itf.store_mesh(1, mesh)
        itf.update_settings(1, 1, 0, 0, 0)
        itf.set_render_options(depth, SEED, 0)
        per_call = []
        for n in chunks:
            itf.compute(n)
            st = itf.stats()
            per_call.append((*itf.read_radiance(W, H), st))
        out[gs] = per_call
        itf.shutdown()
        itf.set_option("defaults", 0)
    ref = oracle.OracleScene(2, mesh).adaptive(W, H, cam, (1, 1), (0, 0), depth)
    for k, n in enumerate(chunks):
        ref.compute(n)
        acc_r, cnt_r, _ = ref.read()
        on, off = out[1][k], out[0][k]
        assert _same(on, off), k
        assert np.array_equal(on[1], cnt_r), k
        assert np.array_equal(on[0].view(np.uint32), acc_r.view(np.uint32)), k
        _check_counts(on, off)
        assert 0 < on[2]["gen_shaded_rays"] <= on[2]["presolved_rays"]


def test_camera_that_resolves_nothing(wpt, oracle, itf):
    """Every primary ray takes the front of stream 0."""
    W, H, spp, depth = 64, 48, 4, 8
    cam = (0.1, 0.2, 4.0, 0.0, 0.0)
    plane, miss, unres = _shares(wpt, 2, W, H, cam)
    assert plane == 0.0 and miss == 0.0 and unres == 1.0
    mesh = scene_mesh(wpt, 2)
    on = _render(itf, wpt, 2, W, H, spp, depth, mesh, cam=cam, gen_shade=1)
    off = _render(itf, wpt, 2, W, H, spp, depth, mesh, cam=cam, gen_shade=0)
    ref, rst = _oracle(oracle, 2, mesh, W, H, cam, depth, spp)
    assert _same(on, off)
    assert np.array_equal(on[0].view(np.uint32), ref.view(np.uint32))
    _check_counts(on, off)
    assert on[2]["rays"] + on[2]["shadow_rays"] == rst["rays"]
    assert on[2]["gen_shaded_rays"] == 0


def test_camera_of_mixed_blocks(wpt, oracle, itf):
    """0.19 of the primary rays resolve to a plane, 0.81 do not: both kinds in a block."""
    W, H, spp, depth = 64, 48, 4, 8
    cam = (0.1, 0.2, 3.0, 0.0, 0.0)
    plane, miss, unres = _shares(wpt, 2, W, H, cam)
    assert abs(plane - 0.19) < 0.005 and abs(unres - 0.81) < 0.005 and miss == 0.0, (plane, miss, unres)
    mesh = scene_mesh(wpt, 2)
    on = _render(itf, wpt, 2, W, H, spp, depth, mesh, cam=cam, gen_shade=1)
    off = _render(itf, wpt, 2, W, H, spp, depth, mesh, cam=cam, gen_shade=0)
    ref, rst = _oracle(oracle, 2, mesh, W, H, cam, depth, spp)
    assert _same(on, off)
    assert np.array_equal(on[0].view(np.uint32), ref.view(np.uint32))
    _check_counts(on, off)
    assert on[2]["rays"] + on[2]["shadow_rays"] == rst["rays"]
    assert 0 < on[2]["gen_shaded_rays"] < W * H * spp


@pytest.mark.parametrize("drop_miss", [1, 0])
def test_sky_camera(wpt, oracle, itf, drop_miss):
    """Every primary ray a miss: dropped, or through shade_path's miss branch in the new kernel."""
    W, H, spp, depth = 64, 48, 4, 8
    plane, miss, unres = _shares(wpt, 2, W, H, SKY)
    assert plane == 0.0 and miss == 1.0 and unres == 0.0
    mesh = scene_mesh(wpt, 2)
    on = _render(itf, wpt, 2, W, H, spp, depth, mesh, cam=SKY, gen_shade=1, drop_miss=drop_miss)
    off = _render(itf, wpt, 2, W, H, spp, depth, mesh, cam=SKY, gen_shade=0, drop_miss=drop_miss)
    ref, rst = _oracle(oracle, 2, mesh, W, H, SKY, depth, spp)
    assert np.all(on[1] == spp)
    assert _same(on, off)
    assert not on[0].view(np.uint32).any()
    assert np.array_equal(on[0].view(np.uint32), ref.view(np.uint32))
    _check_counts(on, off)
    assert on[2]["presolved_rays"] == on[2]["rays"] == rst["rays"] == W * H * spp
    assert on[2]["shadow_rays"] == 0
    if drop_miss:
        assert on[2]["dropped_rays"] == W * H * spp and on[2]["gen_shaded_rays"] == 0
    else:
        assert on[2]["dropped_rays"] == 0 and on[2]["gen_shaded_rays"] == W * H * spp


@pytest.mark.parametrize("scene_id,share", [(0, 0.385), (100, 0.940), (101, 0.0)])
def test_other_scenes(wpt, oracle, itf, scene_id, share):
    """Scene 0: other shapes than triangles (the `false` instantiation); scene 101: no BVH, nothing presolved."""
    W, H, spp, depth = 32, 24, 2, 8
    plane, miss, unres = _shares(wpt, scene_id, W, H)
    if scene_id == 101:
        assert plane == 0.0 and miss == 0.0
    else:
        assert abs(plane - share) < 0.0005, (plane, miss, unres)
    cam = wpt.scenes.scene_camera(scene_id)
    on = _render(itf, wpt, scene_id, W, H, spp, depth, gen_shade=1)
    off = _render(itf, wpt, scene_id, W, H, spp, depth, gen_shade=0)
    ref, rst = _oracle(oracle, scene_id, None, W, H, cam, depth, spp)
    assert _same(on, off)
    assert np.array_equal(on[0].view(np.uint32), ref.view(np.uint32))
    _check_counts(on, off)
    assert on[2]["rays"] + on[2]["shadow_rays"] == rst["rays"]
    if scene_id == 101:
        assert on[2]["presolved_rays"] == 0 and on[2]["gen_shaded_rays"] == 0
    else:
        assert 0 < on[2]["gen_shaded_rays"] <= on[2]["presolved_rays"]


def test_partition_of_two_ranks(wpt, oracle, itf):
    W, H, spp, depth = 64, 48, 4, 8
    mesh = scene_mesh(wpt, 2)
    ref, _ = _oracle(oracle, 2, mesh, W, H, wpt.scenes.scene_camera(2), depth, spp)
    seen = np.zeros(W * H, bool)
    for rank in (0, 1):
        on = _render(itf, wpt, 2, W, H, spp, depth, mesh, partition=(rank, 2), gen_shade=1)
        off = _render(itf, wpt, 2, W, H, spp, depth, mesh, partition=(rank, 2), gen_shade=0)
        px = on[3]
        assert _same(on, off)
        _check_counts(on, off)
        assert 0 < on[2]["gen_shaded_rays"] <= on[2]["presolved_rays"]
        assert np.array_equal(on[0].reshape(-1, 3)[px].view(np.uint32), ref.reshape(-1, 3)[px].view(np.uint32))
        seen[px] = True
    assert seen.all()


def test_pnee_session_keeps_todays_kernels(wpt, itf):
    """Types (2, 2): k_shade stages the octree, so the batch runs k_generate_ps."""
    W, H, spp, depth = 64, 48, 4, 8
    mesh = scene_mesh(wpt, 2)
    on = _render(itf, wpt, 2, W, H, spp, depth, mesh, types=(2, 2), gen_shade=1)
    off = _render(itf, wpt, 2, W, H, spp, depth, mesh, types=(2, 2), gen_shade=0)
    assert np.all(on[1] == spp)
    assert _same(on, off)
    _check_counts(on, off)
    assert on[2]["presolved_rays"] > 0 and on[2]["gen_shaded_rays"] == 0


def test_adaptive_session_with_the_stock(wpt, oracle, itf):
    """Stock batches (the CR count word) keep k_generate_ps; a session of them is the same bits on and off."""
    W, H, depth, types, adaptive = 40, 24, 8, (1, 1), (1, 1)
    mesh = scene_mesh(wpt, 2)
    cam = wpt.scenes.scene_camera(2)
    chunks = (W * H * 5, W * H * 3 + 17, 211, W * H * 9 + 5)
    out = {}
    for gs in (1, 0):
        for k, v in {"stock": 256, "stock_ahead": 6, "stock_extra": 2, "stock_every": 2, "gen_shade": gs}.items():
            itf.set_option(k, v)
        itf.init(W, H, 2, *cam)
        itf.store_mesh(1, mesh)
        itf.update_settings(types[0], types[1], adaptive[0], adaptive[1], 0)
        itf.set_render_options(depth, SEED, 0)
        per_call = []
        for n in chunks:
            itf.compute(n)
            st = itf.stats()
            per_call.append((st["rays"], st["shadow_rays"], st["paths"]))
        out[gs] = (*itf.read_radiance(W, H), per_call, st)
        itf.shutdown()
        itf.set_option("defaults", 0)
    ref = oracle.OracleScene(2, mesh).adaptive(W, H, cam, types, adaptive, depth)
    for n in chunks:
        ref.compute(n)
    acc_r, cnt_r, _ = ref.read()
    assert _same(out[1], out[0])
    assert out[1][2] == out[0][2]  # rays, shadow rays and paths after every call
    assert np.array_equal(out[1][1], cnt_r)
    assert np.array_equal(out[1][0].view(np.uint32), acc_r.view(np.uint32))
    assert out[1][3]["stock_consumed"] > 0
    assert out[1][3]["presolved_rays"] == out[0][3]["presolved_rays"]
    assert out[1][3]["gen_shaded_rays"] == 0 and out[0][3]["gen_shaded_rays"] == 0
