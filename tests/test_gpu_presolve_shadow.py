"""The shadow presolve on the device (WPT_OPT_PRESOLVE_SHADOW).

k_shade's presolving variants add the contribution of a shadow ray that
presolve_shadow proves unoccluded and write it to no stream; it is counted in
its own slot per bounce and reported as `shadow_presolved_rays`, a part of
`shadow_rays`. The device hook must equal the host restatement flag for flag
on the sets of tests/test_presolve_shadow.py, the unchanged k_shadow must call
every resolved ray unoccluded, and frames, sample counts and every ray count
must be the same bits with the option on and off and equal the oracle's.
"""
import numpy as np
import pytest

from test_presolve import scene_mesh
from test_presolve_shadow import SCENES, shadow_sets

pytestmark = pytest.mark.gpu

SEED = 0xBABABEBE
COUNTS = ("rays", "shadow_rays", "presolved_rays", "dropped_rays", "paths", "bounces")


@pytest.fixture
def itf(wpt):
    i = wpt.interface
    yield i
    try:
        i.shutdown()
    except i.WptError:
        pass
    i.set_option("defaults", 0)


def _render(itf, wpt, scene_id, W, H, spp, depth, mesh=None, lanes=None, types=(1, 1), debug=0, **opts):
    """One progressive session: (acc, cnt, stats)."""
    cam = wpt.scenes.scene_camera(scene_id)
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
        itf.compute(W * H * spp)
        acc, cnt = itf.read_radiance(W, H)
        st = itf.stats()
    finally:
        itf.shutdown()
        itf.set_option("defaults", 0)
    return acc, cnt, st


def _same(a, b):
    return np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


_REF = {}


def _oracle(oracle, wpt, scene_id, mesh, W, H, depth, spp, types=(1, 1), debug=0):
    key = (scene_id, W, H, depth, spp, types, debug)
    if key not in _REF:
        cam = wpt.scenes.scene_camera(scene_id)
        _REF[key] = oracle.OracleScene(scene_id, mesh).render(W, H, cam, types[0], types[1], depth, SEED, 0, spp,
                                                              threads=4, light_debug=debug)
    return _REF[key]


@pytest.mark.parametrize("scene_id", SCENES)
def test_device_hook_equals_host_restatement_and_k_shadow_agrees(wpt, oracle, itf, scene_id):
    mesh = scene_mesh(wpt, scene_id)
    dbg = wpt.interface.DebugScene(scene_id, mesh)
    ref = oracle.OracleScene(scene_id, mesh)
    itf.init(32, 24, scene_id, *wpt.scenes.scene_camera(scene_id))
    if mesh is not None:
        itf.store_mesh(1, mesh)
    for name, (pq, li) in shadow_sets(wpt, ref, scene_id, dbg).items():
        res_h = dbg.presolve_shadow(pq, li)
        res_d = itf.presolve_shadow_rays(pq, li)
        print(f"scene {scene_id} {name}: {len(pq)} rays, resolved {res_d.mean():.3f}")
        assert np.array_equal(res_d, res_h), (scene_id, name, int(np.sum(res_d != res_h)))
        if res_d.any():  # the production shadow kernel on the resolved ones
            assert not itf.shadow_rays(pq[res_d], li[res_d]).any(), (scene_id, name)


# the separate kernels (k_extend, k_shade, k_shadow) and the fused k_trace; lanes 1 and 4
FORMS = [("separate", {"fused": 0, "fused_below": 0}, 1), ("separate", {"fused": 0, "fused_below": 0}, 4),
         ("fused", {"fused": 1, "fused_below": 0}, 1), ("fused", {"fused": 1, "fused_below": 0}, 4)]


def _check_pair(on, off, spp):
    assert np.all(on[1] == spp)
    assert _same(on, off)
    for k in COUNTS:
        assert on[2][k] == off[2][k], k
    assert off[2]["shadow_presolved_rays"] == 0
    assert on[2]["shadow_presolved_rays"] <= on[2]["shadow_rays"]


# (the fused form never runs the BVH4 fast path)
CASES = [(f, o, l, t) for f, o, l in FORMS for t in ("bvh2", "bvh4") if not (f == "fused" and t == "bvh4")]


@pytest.mark.parametrize("form,opts,lanes,traversal", CASES)
def test_scene2_frames_and_counts_on_and_off(wpt, oracle, itf, form, opts, lanes, traversal):
    W, H, spp, depth = 64, 48, 4, 8
    mesh = scene_mesh(wpt, 2)
    o = dict(opts, traversal=traversal, traversal_sh=traversal)
    on = _render(itf, wpt, 2, W, H, spp, depth, mesh, lanes=lanes, presolve_shadow=1, **o)
    off = _render(itf, wpt, 2, W, H, spp, depth, mesh, lanes=lanes, presolve_shadow=0, **o)
    ref, rst = _oracle(oracle, wpt, 2, mesh, W, H, depth, spp)
    print(f"{form} {traversal} lanes {lanes}: shadow rays {on[2]['shadow_rays']}, "
          f"resolved {on[2]['shadow_presolved_rays']}")
    _check_pair(on, off, spp)
    assert np.array_equal(on[0].view(np.uint32), ref.view(np.uint32))
    assert on[2]["rays"] + on[2]["shadow_rays"] == rst["rays"]
    assert 0 < on[2]["shadow_presolved_rays"] <= on[2]["shadow_rays"]


def test_without_the_extension_presolve_nothing_is_resolved(wpt, oracle, itf):
    W, H, spp, depth = 64, 48, 4, 8
    mesh = scene_mesh(wpt, 2)
    on = _render(itf, wpt, 2, W, H, spp, depth, mesh, presolve=0, presolve_shadow=1)
    ref, rst = _oracle(oracle, wpt, 2, mesh, W, H, depth, spp)
    assert np.array_equal(on[0].view(np.uint32), ref.view(np.uint32))
    assert on[2]["shadow_presolved_rays"] == 0 and on[2]["rays"] + on[2]["shadow_rays"] == rst["rays"]


@pytest.mark.parametrize("name,types,debug,depth", [("pnee", (2, 2), 0, 4), ("light_debug", (1, 1), 1, 8)])
def test_scene2_pnee_and_light_debug(wpt, oracle, itf, name, types, debug, depth):
    W, H, spp = 64, 48, 4
    mesh = scene_mesh(wpt, 2)
    on = _render(itf, wpt, 2, W, H, spp, depth, mesh, types=types, debug=debug, presolve_shadow=1)
    off = _render(itf, wpt, 2, W, H, spp, depth, mesh, types=types, debug=debug, presolve_shadow=0)
    ref, rst = _oracle(oracle, wpt, 2, mesh, W, H, depth, spp, types, debug)
    print(f"{name}: shadow rays {on[2]['shadow_rays']}, resolved {on[2]['shadow_presolved_rays']}")
    _check_pair(on, off, spp)
    assert np.array_equal(on[0].view(np.uint32), ref.view(np.uint32))
    if debug:
        assert on[2]["shadow_rays"] == 0  # no shadow ray in the debug view


@pytest.mark.parametrize("scene_id", [0, 100])
def test_other_scenes(wpt, oracle, itf, scene_id):
    """Scene 0: the lights share guards with tori and rectangles (the BVH4 walk); scene 100: the box."""
    W, H, spp, depth = 32, 24, 2, 8
    on = _render(itf, wpt, scene_id, W, H, spp, depth, presolve_shadow=1)
    off = _render(itf, wpt, scene_id, W, H, spp, depth, presolve_shadow=0)
    ref, rst = _oracle(oracle, wpt, scene_id, None, W, H, depth, spp)
    print(f"scene {scene_id}: shadow rays {on[2]['shadow_rays']}, resolved {on[2]['shadow_presolved_rays']}")
    _check_pair(on, off, spp)
    assert np.array_equal(on[0].view(np.uint32), ref.view(np.uint32))
    assert on[2]["rays"] + on[2]["shadow_rays"] == rst["rays"]


def test_adaptive_session_with_the_stock(wpt, oracle, itf):
    """Stock refills run the ray-counting k_shade: images, per-pixel counts and the ray counts after every call."""
    W, H, depth, types, adaptive = 40, 24, 8, (1, 1), (1, 1)
    mesh = scene_mesh(wpt, 2)
    cam = wpt.scenes.scene_camera(2)
    chunks = (W * H * 5, W * H * 3 + 17, 211, W * H * 9 + 5)
    out = {}
    for sps in (1, 0):
        for k, v in {"stock": 256, "stock_ahead": 6, "stock_extra": 2, "stock_every": 2, "presolve_shadow": sps}.items():
            itf.set_option(k, v)
        itf.init(W, H, 2, *cam)
        itf.store_mesh(1, mesh)
        itf.update_settings(types[0], types[1], adaptive[0], adaptive[1], 0)
        itf.set_render_options(depth, SEED, 0)
        per_call = []
        for n in chunks:
            itf.compute(n)
            st = itf.stats()
            per_call.append(tuple(st[k] for k in ("rays", "shadow_rays", "presolved_rays", "dropped_rays", "paths")))
        out[sps] = (*itf.read_radiance(W, H), per_call, st)
        itf.shutdown()
        itf.set_option("defaults", 0)
    ref = oracle.OracleScene(2, mesh).adaptive(W, H, cam, types, adaptive, depth)
    for n in chunks:
        ref.compute(n)
    acc_r, cnt_r, _ = ref.read()
    assert _same(out[1], out[0])
    assert out[1][2] == out[0][2]  # the counts after every call
    assert np.array_equal(out[1][1], cnt_r)
    assert np.array_equal(out[1][0].view(np.uint32), acc_r.view(np.uint32))
    assert out[1][3]["stock_consumed"] > 0
    assert out[1][3]["stock_rays"] == out[0][3]["stock_rays"] and out[1][3]["stock_rays_used"] == out[0][3]["stock_rays_used"]
    assert out[1][3]["shadow_presolved_rays"] > 0 and out[0][3]["shadow_presolved_rays"] == 0
