"""The adversarial fixtures of tests/adversarial.py through the device.

Every (t, id) of wpt_trace_rays and every verdict of wpt_shadow_rays is
compared bit for bit with the oracle on rays built to sit where the kernels
decide: exact ties across leaves and with the seeding plane (accept4's tie
flag and the BVH2 re-trace, leaf_test's t <= max_dis, step's ties-go-right and
the pop test), NaN slab products (box_entry), stacks deeper than the LDS slots
(stack_store / stack_load), tangents and surface origins of the analytic
shapes, degenerate and NaN triangles. tests/test_adversarial_cpu.py shows on
the oracle alone that the rays produce those conditions.

Sessions: traversal and traversal_sh bvh4 and bvh2, the LDS treelet on and
off, and refill / refill_sh 1 and 64 (another wave composition around a ray).
"""
import numpy as np
import pytest

import adversarial as adv
from test_adversarial_cpu import RENDER_CAM, fixtures
from test_presolve import ray_sets, scene_mesh

pytestmark = pytest.mark.gpu

SEED = 0xBABABEBE
CONFIGS = [("bvh4", 0, None), ("bvh4", 1, None), ("bvh2", 0, None), ("bvh2", 1, None),
           ("bvh4", 1, 1), ("bvh2", 1, 1), ("bvh4", 1, 64), ("bvh2", 1, 64)]
MESHES = ("A", "B", "Bwall", "Bulp", "C", "D", "E", "F", "G", "BA")


@pytest.fixture(params=CONFIGS, ids=lambda c: f"{c[0]}-treelet{c[1]}" + (f"-refill{c[2]}" if c[2] else ""))
def config(request):
    """(traversal, treelet, refill or None)"""
    return request.param


@pytest.fixture
def session(wpt, config):
    itf = wpt.interface
    trav, treelet, refill = config
    itf.set_option("traversal", trav)
    itf.set_option("traversal_sh", trav)
    itf.set_option("treelet", treelet)
    if refill is not None:
        itf.set_option("refill", refill)
        itf.set_option("refill_sh", refill)
    yield itf
    try:
        itf.shutdown()
    except itf.WptError:
        pass
    itf.set_option("defaults", 0)


def _start(itf, wpt, scene_id, mesh=None):
    itf.init(32, 24, scene_id, *wpt.scenes.scene_camera(scene_id))
    if mesh is not None:
        assert itf.store_mesh(1, mesh)
    itf.update_settings(1, 1, 0, 0, 0)
    itf.set_render_options(4, SEED, 0)


def _same_hits(itf, rays, t_r, id_r, what):
    t_g, id_g = itf.trace_rays(rays)
    bad = np.nonzero((id_g != id_r) | (t_g.view(np.uint32) != t_r.view(np.uint32)))[0]
    assert len(bad) == 0, (what, len(bad), bad[:5], rays[bad[:5]], t_g[bad[:5]], id_g[bad[:5]], t_r[bad[:5]],
                           id_r[bad[:5]])
    return t_g, id_g


@pytest.mark.parametrize("name", MESHES)
def test_closest_hit_meshes(wpt, oracle, session, name):
    """Every scene-2 fixture with every ray set: (t, id) bitwise. The compute call
    at the end reports a traversal stack overflow of the hook's launches, if
    there was one (the hook itself does not read the flag)."""
    mesh, ref, _, sets, hits = fixtures(wpt, oracle)[name]
    _start(session, wpt, 2, mesh)
    for s, rays in sets.items():
        _same_hits(session, rays, *hits[s], (name, s))
    session.compute(2)


_SHAPES = {}


def _shape_case(oracle, sid):
    if sid not in _SHAPES:
        ref = oracle.OracleScene(sid)
        sets = adv.shape_sets(sid, ref.shapes())
        _SHAPES[sid] = (ref, {k: (r, *ref.trace_rays(r)[:2]) for k, (r, _) in sets.items()})
    return _SHAPES[sid]


@pytest.mark.parametrize("scene_id", [0, 100, 101])
def test_closest_hit_shape_sets(wpt, oracle, session, scene_id):
    """Spheres (scene 101, linear scan), AA rects (100, 0) and tori (0): grazes,
    surface and centre origins, corners, axis and tangent rays."""
    _, sets = _shape_case(oracle, scene_id)
    _start(session, wpt, scene_id)
    for s, (rays, t_r, id_r) in sets.items():
        _same_hits(session, rays, t_r, id_r, (scene_id, s))
    session.compute(2)


_PRE = {}


def _presolve_case(wpt, oracle, sid):
    if sid not in _PRE:
        mesh = scene_mesh(wpt, sid)
        ref = oracle.OracleScene(sid, mesh)
        sets = ray_sets(wpt, sid, wpt.interface.DebugScene(sid, mesh))
        _PRE[sid] = (mesh, {k: (r, *ref.trace_rays(r)[:2]) for k, r in sets.items()})
    return _PRE[sid]


@pytest.mark.parametrize("scene_id", [2, 0, 100])
def test_presolve_ray_sets_through_the_traversal(wpt, oracle, session, scene_id):
    """tests/test_presolve.py's sets (guard faces and corners, zero components)
    through the traversal kernels that must agree with the presolve, and the
    device presolve against those hits."""
    mesh, sets = _presolve_case(wpt, oracle, scene_id)
    _start(session, wpt, scene_id, mesh)
    for s, (rays, t_r, id_r) in sets.items():
        t_g, id_g = _same_hits(session, rays, t_r, id_r, (scene_id, s))
        res, t_p, id_p = session.presolve_rays(rays)
        assert np.array_equal(id_p[res], id_g[res]), (scene_id, s)
        assert np.array_equal(t_p[res].view(np.uint32), t_g[res].view(np.uint32)), (scene_id, s)


@pytest.mark.parametrize("name", MESHES)
def test_presolve_agrees_with_the_traversal(wpt, oracle, session, name):
    """Every ray the device presolve resolves has the (t, id) bits trace_rays returns."""
    mesh, _, dbg, sets, _ = fixtures(wpt, oracle)[name]
    _start(session, wpt, 2, mesh)
    total = 0
    for s, rays in sets.items():
        res, t_p, id_p = session.presolve_rays(rays)
        t_g, id_g = session.trace_rays(rays)
        assert np.all(id_p[res] < dbg.num_inf), (name, s)
        assert np.array_equal(id_p[res], id_g[res]), (name, s)
        assert np.array_equal(t_p[res].view(np.uint32), t_g[res].view(np.uint32)), (name, s)
        total += int(res.sum())
    assert total > 0


def test_sheet_a_vertex_rays_in_small_batches(wpt, oracle, session):
    """Batches of 1, 63, 64, 65 and 257 rays: part of a wave, a whole one, one more, more than a block."""
    mesh, _, _, sets, hits = fixtures(wpt, oracle)["A"]
    _start(session, wpt, 2, mesh)
    rays, (t_r, id_r) = sets["vertices"], hits["vertices"]
    assert len(rays) >= 257
    for n in (1, 63, 64, 65, 257):
        for k0 in (0, len(rays) - n):
            _same_hits(session, rays[k0: k0 + n], t_r[k0: k0 + n], id_r[k0: k0 + n], ("A", n, k0))


def _fallbacks(itf, wpt, mesh, work):
    """fallback_ext / fallback_sh of `work` in a fresh session: the counters are
    read at the end of a compute call, so the same compute(2) runs with and
    without the work before it and the difference is the work's."""
    out = []
    for do in (False, True):
        _start(itf, wpt, 2, mesh)
        if do:
            work()
        itf.compute(2)
        st = itf.stats()
        out.append((st["fallback_ext"], st["fallback_sh"]))
        itf.shutdown()
    return out[1][0] - out[0][0], out[1][1] - out[0][1], out[1]


@pytest.mark.parametrize("name", adv.TIE_MESHES)
def test_tie_sets_are_retraced_by_the_bvh4_path_only(wpt, oracle, session, config, name):
    """The BVH4 fast path flags a tie and re-traces the ray with the BVH2 machine
    (fallback_ext > 0 after a tie set); a bvh2 session never re-traces."""
    mesh, _, _, sets, hits = fixtures(wpt, oracle)[name]
    rays = np.concatenate([sets[s] for s in ("vertices", "edges", "interior")])
    ext, _, total = _fallbacks(session, wpt, mesh, lambda: session.trace_rays(rays))
    print(f"{config} {name}: fallback_ext {ext} of {len(rays)} tie rays")
    if config[0] == "bvh4":
        assert 0 < ext <= len(rays)
    else:
        assert total == (0, 0)


_SHADOW = {}


def _shadow_case(wpt, oracle):
    if not _SHADOW:
        mesh, ref, _, _, _ = fixtures(wpt, oracle)["G"]
        pq, li, qc, pc = adv.shadow_set(ref.shapes())
        _SHADOW["G"] = (mesh, pq, li, ref.shadow_rays(pq, li))
    return _SHADOW["G"]


def test_shadow_segments_on_the_coplanar_sheets(wpt, oracle, session, config):
    """Segments to light vertices, the lights' shared diagonal, a light edge
    inside a coplanar sheet and interior points, from sheet vertices, the
    floor, the lights' plane, above the lights and anywhere: verdicts bitwise,
    including the BVH4 early exit's !(t < ek) guard. Zero-length segments
    (p = q) are left out of the set: their direction is 0 / 0."""
    mesh, pq, li, occ_r = _shadow_case(wpt, oracle)
    _start(session, wpt, 2, mesh)
    occ_g = session.shadow_rays(pq, li)
    bad = np.nonzero(occ_g != occ_r)[0]
    assert len(bad) == 0, (len(bad), bad[:5], pq[bad[:5]], li[bad[:5]], occ_r[bad[:5]])
    for n in (1, 63, 65):
        assert np.array_equal(session.shadow_rays(pq[-n:], li[-n:]), occ_r[-n:])
    session.shutdown()
    _, sh, total = _fallbacks(session, wpt, mesh, lambda: session.shadow_rays(pq, li))
    print(f"{config} G: fallback_sh {sh} of {len(pq)} segments")
    if config[0] == "bvh4":
        assert 0 < sh <= len(pq)
    else:
        assert total == (0, 0)


@pytest.mark.parametrize("name", ["A", "B", "C", "F", "Bwall"])
def test_gpu_build_of_the_sheets(wpt, name):
    """The GPU BVH2 build on sheets (a centroid axis of zero extent is an edge
    of the binning) and on the overlap mesh: the host build's tree, bit for bit."""
    from test_gpu_bvh_build import _same_scene
    _same_scene(wpt.interface, 2, adv.scene2_meshes(wpt)[name])


# ---- renders through the ties -------------------------------------------------
@pytest.fixture
def itf(wpt):
    i = wpt.interface
    yield i
    try:
        i.shutdown()
    except i.WptError:
        pass
    i.set_option("defaults", 0)


def _render(itf, W, H, spp, depth, mesh, lanes, **opts):
    for k, v in opts.items():
        itf.set_option(k, v)
    itf.init(W, H, 2, *RENDER_CAM)
    try:
        itf.store_mesh(1, mesh)
        itf.update_settings(1, 1, 0, 0, 0)
        itf.set_render_options(depth, SEED, 0)
        itf.set_lanes(lanes)
        itf.compute(W * H * spp)
        acc, cnt = itf.read_radiance(W, H)
        st = itf.stats()
    finally:
        itf.shutdown()
        itf.set_option("defaults", 0)
    return acc, cnt, st


_REF = {}


def _oracle_render(wpt, oracle, W, H, depth, spp):
    key = (W, H, depth, spp)
    if key not in _REF:
        ref = fixtures(wpt, oracle)["BA"][1]
        _REF[key] = ref.render(W, H, RENDER_CAM, 1, 1, depth, SEED, 0, spp, threads=4)
    return _REF[key]


FORMS = [("separate", {"fused": 0, "fused_below": 0}, 1), ("separate", {"fused": 0, "fused_below": 0}, 4),
         ("fused", {"fused": 1, "fused_below": 0}, 1), ("fused", {"fused": 1, "fused_below": 0}, 4)]


@pytest.mark.parametrize("traversal", ["bvh4", "bvh2"])
@pytest.mark.parametrize("form,opts,lanes", FORMS)
@pytest.mark.parametrize("depth", [4, 1])
def test_render_through_the_ties(wpt, oracle, itf, form, opts, lanes, depth, traversal):
    """Scene 2 with the floor sheet and sheet A from a camera whose primary rays
    end in plane / triangle ties (test_render_camera_sees_the_ties): frame and
    ray counts bitwise against the oracle, the presolve and drop_miss on and off."""
    W, H, spp = 32, 24, 2
    mesh = fixtures(wpt, oracle)["BA"][0]
    ref, rst = _oracle_render(wpt, oracle, W, H, depth, spp)
    for presolve, drop in ((1, 1), (1, 0), (0, 0)):
        acc, cnt, st = _render(itf, W, H, spp, depth, mesh, lanes, presolve=presolve, drop_miss=drop,
                               traversal=traversal, traversal_sh=traversal, **opts)
        assert np.all(cnt == spp)
        assert np.array_equal(acc.view(np.uint32), ref.view(np.uint32)), (form, lanes, depth, presolve, drop)
        assert st["rays"] + st["shadow_rays"] == rst["rays"]
        assert (st["presolved_rays"] > 0) == bool(presolve)
    assert ref.max() > 0


@pytest.mark.parametrize("lanes", [1, 4])
def test_finish_tail_through_the_ties(wpt, oracle, itf, lanes):
    """RR-only paths (depth 0) handed to k_finish as soon as the wavefront reads
    the live count (finish_below 2^30), with a small sample count."""
    W, H, spp = 32, 24, 2
    mesh = fixtures(wpt, oracle)["BA"][0]
    ref, rst = _oracle_render(wpt, oracle, W, H, 0, spp)
    for presolve in (1, 0):
        acc, cnt, st = _render(itf, W, H, spp, 0, mesh, lanes, presolve=presolve, finish_below=1 << 30,
                               fused=0, fused_below=0)
        assert np.all(cnt == spp)
        assert np.array_equal(acc.view(np.uint32), ref.view(np.uint32)), (lanes, presolve)
        assert st["rays"] + st["shadow_rays"] == rst["rays"]
        assert st["finish_paths"] > 0
