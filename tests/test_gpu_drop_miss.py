"""Dropped misses on the device (WPT_OPT_DROP_MISS) and k_generate_ps's tiles.

A ray its producer resolves to a miss whose throughput * background is +0 is
written to no stream; it is counted in the high word of the presolved slot and
reported as `dropped_rays`, a part of `presolved_rays`. Frames, sample counts
and every ray count must be the same bits with the option on, off and without
the presolve, and equal the oracle's. k_generate_ps reserves its stream ranges
once per kGenTile tiles of 256 paths: the odd batch covers the partial last
tile and block.
"""
import numpy as np
import pytest

from test_presolve import camera_rays, scene_mesh

pytestmark = pytest.mark.gpu

SEED = 0xBABABEBE


@pytest.fixture
def itf(wpt):
    i = wpt.interface
    yield i
    try:
        i.shutdown()
    except i.WptError:
        pass
    i.set_option("defaults", 0)


def _render(itf, wpt, scene_id, W, H, spp, depth, mesh=None, cam=None, lanes=None, partition=None, **opts):
    """One progressive session: (acc, cnt, stats, this rank's pixels)."""
    cam = cam if cam is not None else wpt.scenes.scene_camera(scene_id)
    for k, v in opts.items():
        itf.set_option(k, v)  # the defaults of the init below
    itf.init(W, H, scene_id, *cam)
    try:
        if mesh is not None:
            itf.store_mesh(1, mesh)
        itf.update_settings(1, 1, 0, 0, 0)
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


def _oracle(oracle, scene_id, mesh, W, H, cam, depth, spp):
    key = (scene_id, W, H, tuple(cam), depth, spp)
    if key not in _REF:
        _REF[key] = oracle.OracleScene(scene_id, mesh).render(W, H, cam, 1, 1, depth, SEED, 0, spp, threads=4)
    return _REF[key]


# the separate kernels (k_extend, k_shade, k_shadow) and the fused k_trace; lanes 1 and 4
FORMS = [("separate", {"fused": 0, "fused_below": 0}, 1), ("separate", {"fused": 0, "fused_below": 0}, 4),
         ("fused", {"fused": 1, "fused_below": 0}, 1), ("fused", {"fused": 1, "fused_below": 0}, 4)]


@pytest.mark.parametrize("form,opts,lanes", FORMS)
@pytest.mark.parametrize("depth", [8, 1])
def test_scene2_on_off_and_without_presolve(wpt, oracle, itf, form, opts, lanes, depth):
    W, H, spp = 64, 48, 4
    mesh = scene_mesh(wpt, 2)
    cam = wpt.scenes.scene_camera(2)
    on = _render(itf, wpt, 2, W, H, spp, depth, mesh, lanes=lanes, drop_miss=1, **opts)
    off = _render(itf, wpt, 2, W, H, spp, depth, mesh, lanes=lanes, drop_miss=0, **opts)
    nops = _render(itf, wpt, 2, W, H, spp, depth, mesh, lanes=lanes, presolve=0, **opts)
    ref, rst = _oracle(oracle, 2, mesh, W, H, cam, depth, spp)
    print(f"{form} lanes {lanes} depth {depth}: rays {on[2]['rays']}, presolved {on[2]['presolved_rays']}, "
          f"dropped {on[2]['dropped_rays']}")
    assert np.all(on[1] == spp)
    assert _same(on, off) and _same(on, nops)
    assert np.array_equal(on[0].view(np.uint32), ref.view(np.uint32))
    for k in ("rays", "shadow_rays", "paths", "bounces"):
        assert on[2][k] == off[2][k] == nops[2][k], k
    assert on[2]["rays"] + on[2]["shadow_rays"] == rst["rays"]
    assert on[2]["presolved_rays"] == off[2]["presolved_rays"]
    assert off[2]["dropped_rays"] == 0 and nops[2]["dropped_rays"] == 0
    if depth == 8:
        assert 0 < on[2]["dropped_rays"] <= on[2]["presolved_rays"]
    else:
        assert on[2]["dropped_rays"] == 0


def test_sky_camera_drops_every_primary_ray(wpt, oracle, itf):
    """k_generate_ps dropping: each path is one ray, written to no stream."""
    W, H, spp, depth = 64, 48, 4, 8
    mesh = scene_mesh(wpt, 2)
    cam = (0.0, 5.0, -3.0, -1.0, 3.14159)  # up and away from the back wall, the lights behind it
    _, id_r, _ = oracle.OracleScene(2, mesh).trace_rays(camera_rays(wpt, 2, W, H, cam))
    assert np.all(id_r == -1)  # the oracle alone: every primary ray misses
    on = _render(itf, wpt, 2, W, H, spp, depth, mesh, cam=cam, drop_miss=1)
    ref, rst = _oracle(oracle, 2, mesh, W, H, cam, depth, spp)
    assert np.all(on[1] == spp)
    assert not on[0].view(np.uint32).any()
    assert np.array_equal(on[0].view(np.uint32), ref.view(np.uint32))
    assert on[2]["dropped_rays"] == on[2]["presolved_rays"] == on[2]["rays"] == rst["rays"] == W * H * spp
    assert on[2]["shadow_rays"] == 0


@pytest.mark.parametrize("lanes", [1, 4])
def test_odd_batch(wpt, oracle, itf, lanes):
    """5 550 paths: no multiple of 256 nor of 256 * kGenTile (the partial last tile and block)."""
    W, H, spp, depth = 50, 37, 3, 8
    mesh = scene_mesh(wpt, 2)
    cam = wpt.scenes.scene_camera(2)
    on = _render(itf, wpt, 2, W, H, spp, depth, mesh, lanes=lanes, drop_miss=1)
    ref, rst = _oracle(oracle, 2, mesh, W, H, cam, depth, spp)
    assert np.all(on[1] == spp)
    assert np.array_equal(on[0].view(np.uint32), ref.view(np.uint32))
    assert on[2]["paths"] == W * H * spp
    assert on[2]["rays"] + on[2]["shadow_rays"] == rst["rays"]
    assert 0 < on[2]["dropped_rays"] <= on[2]["presolved_rays"] <= on[2]["rays"]


def test_adaptive_session_with_the_stock(wpt, oracle, itf):
    """Stock refills run the ray-counting k_shade: a dropped ray's producer writes the path's count word."""
    W, H, depth, types, adaptive = 40, 24, 8, (1, 1), (1, 1)
    mesh = scene_mesh(wpt, 2)
    cam = wpt.scenes.scene_camera(2)
    chunks = (W * H * 5, W * H * 3 + 17, 211, W * H * 9 + 5)
    out = {}
    for drop in (1, 0):
        for k, v in {"stock": 256, "stock_ahead": 6, "stock_extra": 2, "stock_every": 2, "drop_miss": drop}.items():
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
        out[drop] = (*itf.read_radiance(W, H), per_call, st)
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
    assert out[1][3]["dropped_rays"] > 0 and out[0][3]["dropped_rays"] == 0
    assert out[1][3]["presolved_rays"] == out[0][3]["presolved_rays"]


def test_partition_of_two_ranks(wpt, oracle, itf):
    W, H, spp, depth = 64, 48, 4, 8
    mesh = scene_mesh(wpt, 2)
    ref, _ = _oracle(oracle, 2, mesh, W, H, wpt.scenes.scene_camera(2), depth, spp)
    seen = np.zeros(W * H, bool)
    for rank in (0, 1):
        on = _render(itf, wpt, 2, W, H, spp, depth, mesh, partition=(rank, 2), drop_miss=1)
        off = _render(itf, wpt, 2, W, H, spp, depth, mesh, partition=(rank, 2), drop_miss=0)
        px = on[3]
        assert _same(on, off) and on[2]["rays"] == off[2]["rays"] and on[2]["shadow_rays"] == off[2]["shadow_rays"]
        assert on[2]["dropped_rays"] > 0 and off[2]["dropped_rays"] == 0
        assert np.array_equal(on[0].reshape(-1, 3)[px].view(np.uint32), ref.reshape(-1, 3)[px].view(np.uint32))
        seen[px] = True
    assert seen.all()


@pytest.mark.parametrize("scene_id", [0, 101])
def test_other_scenes(wpt, oracle, itf, scene_id):
    """Scene 0: the BVH4 walk (other shapes than triangles); scene 101: no BVH, nothing resolved or dropped."""
    W, H, spp, depth = 32, 24, 2, 8
    cam = wpt.scenes.scene_camera(scene_id)
    on = _render(itf, wpt, scene_id, W, H, spp, depth, drop_miss=1)
    off = _render(itf, wpt, scene_id, W, H, spp, depth, drop_miss=0)
    ref, rst = _oracle(oracle, scene_id, None, W, H, cam, depth, spp)
    assert _same(on, off)
    assert np.array_equal(on[0].view(np.uint32), ref.view(np.uint32))
    assert on[2]["rays"] == off[2]["rays"] and on[2]["shadow_rays"] == off[2]["shadow_rays"]
    assert on[2]["rays"] + on[2]["shadow_rays"] == rst["rays"]
    assert on[2]["presolved_rays"] == off[2]["presolved_rays"] and off[2]["dropped_rays"] == 0
    if scene_id == 101:
        assert on[2]["dropped_rays"] == 0 and on[2]["presolved_rays"] == 0
