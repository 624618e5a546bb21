"""The ray query on the device (wpt_radiance_rays) against the oracle's ray
query, on the adversarial families of tests/rays_adversarial.py.

Every comparison is the device against OracleScene.radiance_rays: rgb bit for
bit, the status bytes equal, the rise of rays + shadow rays in wpt_stats equal
to the oracle's ray count and the rise of paths equal to valid * spp. What the
rays are built for (ties, surface origins, BVH bounds, denormal and scaled
directions, block and chunk straddles, 32-bit keys) and that they produce it
is asserted on the oracle alone in tests/test_rays_oracle_cpu.py.
"""
import numpy as np
import pytest

import adversarial as adv
import pnee_fixtures as pf
import rays_adversarial as ra
import rays_fixtures as rf

pytestmark = pytest.mark.gpu

SEED, DEPTH = rf.SEED, rf.DEPTH
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


def _start(itf, wpt, scene_id, mesh=None, depth=DEPTH, batch=0, types=(0, 1), light_debug=0, photons=False):
    itf.init(8, 8, scene_id, *wpt.scenes.scene_camera(scene_id))
    if mesh is not None:
        assert itf.store_mesh(1, mesh)
    itf.update_settings(types[0], types[1], 0, 0, light_debug)
    itf.set_render_options(depth, SEED, batch)
    if photons:
        itf.install_photons(pf.octants())


def _check(itf, want, what, rays, keys=None, sample=0, spp=1, rtype=1):
    """One query against the oracle's (rgb, status, stats); returns the device's rgb."""
    w_rgb, w_status, w_st = want
    s0 = itf.stats()
    rgb, status = itf.radiance_rays(rays, keys, sample, spp, rtype)
    s1 = itf.stats()
    assert np.array_equal(status, w_status), what
    bad = np.any(rf.bits(rgb) != rf.bits(w_rgb), axis=1)
    assert not bad.any(), (what, "differs on", int(bad.sum()), "of", len(bad), "rays, first", int(np.argmax(bad)),
                           rays[np.argmax(bad)], rgb[np.argmax(bad)], w_rgb[np.argmax(bad)])
    d = {k: s1[k] - s0[k] for k in ("paths", "rays", "shadow_rays")}
    assert d["rays"] + d["shadow_rays"] == w_st["rays"], (what, d, w_st)
    assert d["paths"] == int(w_status.sum()) * spp, (what, d)
    return rgb


# ---------------------------------------------------------------------------
# 1. The scene-2 fixtures' sets
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ra.MESHES)
def test_mesh_sets(wpt, oracle, itf, name):
    """Types 0 and 1 at depth 4 through the presolving producer
    (k_generate_rays_ps) and, presolve off, through k_generate_rays; the tie
    meshes under both traversals."""
    mesh, ref, rays = ra.mesh_case(wpt, oracle, name)
    _start(itf, wpt, 2, mesh)
    travs = (0, 1) if name in adv.TIE_MESHES else (None,)
    for trav in travs:
        if trav is not None:
            itf.set_option("traversal", trav)
            itf.set_option("traversal_sh", trav)
        for presolve in (1, 0):
            itf.set_option("presolve", presolve)
            p0 = itf.stats()["presolved_rays"]
            for t in (0, 1):
                _check(itf, ra.expect(ref, ("mesh", name), rays, rtype=t), (name, trav, presolve, t), rays, rtype=t)
            assert (itf.stats()["presolved_rays"] > p0) == bool(presolve)


def test_mesh_a_depths_0_and_1(wpt, oracle, itf):
    """Depth 0 (Russian roulette only: k_generate_rays, k_finish takes the tails) and depth 1."""
    mesh, ref, rays = ra.mesh_case(wpt, oracle, "A")
    for depth in (0, 1):
        _start(itf, wpt, 2, mesh, depth=depth)
        for t in (0, 1):
            _check(itf, ra.expect(ref, ("mesh", "A"), rays, rtype=t, depth=depth), ("A", depth, t), rays, rtype=t)
        if depth == 0:
            assert itf.stats()["finish_paths"] > 0
        itf.shutdown()


# ---------------------------------------------------------------------------
# 2. Tori, AA rects and spheres
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("scene_id", list(ra.SHAPE_SCENES))
def test_shape_sets(wpt, oracle, itf, scene_id):
    sc, sets = ra.shape_case(wpt, oracle, scene_id)
    spp = ra.MUSEUM_SPP if scene_id == 0 else 1
    _start(itf, wpt, scene_id)
    for trav in (0, 1) if scene_id == 0 else (None,):
        if trav is not None:
            itf.set_option("traversal", trav)
            itf.set_option("traversal_sh", trav)
        for s, rays in sets.items():
            for t in (0, 1):
                _check(itf, ra.expect(sc.ref, ("shapes", scene_id, s), rays, None, 0, spp, t), (scene_id, s, trav, t),
                       rays, None, 0, spp, t)


# ---------------------------------------------------------------------------
# 3. PNEE, 4. light debug
# ---------------------------------------------------------------------------
def test_pnee(wpt, oracle, itf):
    """Type 2 under pnee_fixtures.octants() on the box set, on the cloud's probes and on mesh A's sets."""
    sc, rays = ra.box_set(wpt, oracle)
    _start(itf, wpt, 100, photons=True)
    _check(itf, ra.expect(sc.ref, "box_set", rays, rtype=2), "box", rays, rtype=2)
    itf.shutdown()
    cloud = rf.scene(wpt, oracle, "cloud")
    keys = np.zeros(rf.PROBES, np.uint32)
    _start(itf, wpt, 2, cloud.mesh, photons=True)
    _check(itf, ra.expect(cloud.ref, "cloud_probes", cloud.probe_rays(), keys, 3, 1, 2), "cloud", cloud.probe_rays(), keys, 3, 1, 2)
    itf.shutdown()
    mesh, ref, rays = ra.pnee_mesh_case(wpt, oracle)
    assert ref.num_lights == 2
    _start(itf, wpt, 2, mesh, photons=True)
    for presolve in (1, 0):
        itf.set_option("presolve", presolve)
        _check(itf, ra.expect(ref, "pnee_mesh", rays, rtype=2), ("A", presolve), rays, rtype=2)


def test_light_debug(wpt, oracle, itf):
    sc, rays = ra.box_set(wpt, oracle)
    for t in (0, 1, 2):
        _start(itf, wpt, 100, types=(t, t), light_debug=1, photons=t == 2)
        _check(itf, ra.expect(sc.ref, "box_set", rays, rtype=t, light_debug=1), ("light debug", t), rays, rtype=t)
        assert itf.stats()["shadow_rays"] == 0
        itf.shutdown()


# ---------------------------------------------------------------------------
# 5. Scaled directions
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ra.SCALED_MESHES)
def test_scaled_directions(wpt, oracle, itf, name):
    """The direction is used as given: seven scales from denormal to near
    overflow, and on the device too the power-of-two scales give the unit
    direction's bits."""
    mesh, ref, unit, scaled = ra.scaled_case(wpt, oracle, name)
    _start(itf, wpt, 2, mesh)
    for t in (0, 1):
        base = _check(itf, ra.expect(ref, ("scaled", name, 1.0), unit, rtype=t), (name, 1.0, t), unit, rtype=t)
        for s in ra.SCALES:
            rgb = _check(itf, ra.expect(ref, ("scaled", name, s), scaled[s], rtype=t), (name, s, t), scaled[s], rtype=t)
            if s in ra.EXACT_SCALES:
                assert np.array_equal(rf.bits(rgb), rf.bits(base)), (name, s, t)


# ---------------------------------------------------------------------------
# 6. spp and block straddles
# ---------------------------------------------------------------------------
def test_spp_values(wpt, oracle, itf):
    sc, rays = ra.spp_case(wpt, oracle)
    _start(itf, wpt, 100, batch=DEFAULT_BATCH)
    for spp in ra.SPPS:
        _check(itf, ra.expect(sc.ref, "spp", rays, None, ra.SPP_SAMPLE, spp), ("spp", spp), rays, None, ra.SPP_SAMPLE, spp)


@pytest.mark.parametrize("spp", ra.STRADDLE_SPPS)
def test_blocks_that_start_inside_a_ray(wpt, oracle, itf, spp):
    """Batches of 64, 100 and 257 positions cut inside a ray's samples, so a
    generator block starts at rem0 != 0 (query_path's head = spp - rem0)."""
    sc, rays = ra.spp_case(wpt, oracle)
    want = ra.expect(sc.ref, "spp", rays, None, ra.SPP_SAMPLE, spp)
    _start(itf, wpt, 100)
    for batch in ra.STRADDLE_BATCHES:
        assert (ra.block_starts(len(rays) * spp, batch) % spp != 0).any()
        itf.set_render_options(DEPTH, SEED, batch)
        for lanes in (1, 4):
            itf.set_lanes(lanes)
            _check(itf, want, ("spp", spp, "batch", batch, "lanes", lanes), rays, None, ra.SPP_SAMPLE, spp)


# ---------------------------------------------------------------------------
# 7. Keys
# ---------------------------------------------------------------------------
def test_keys_against_the_oracle(wpt, oracle, itf):
    _start(itf, wpt, 100)
    sc, rays, keys = ra.keys_case(wpt, oracle)
    _, one, one_keys = ra.one_ray_case(wpt, oracle)
    for sample, spp in ra.KEY_SAMPLES:
        _check(itf, ra.expect(sc.ref, "keys", rays, keys, sample, spp), ("keys", sample, spp), rays, keys, sample, spp)
        _check(itf, ra.expect(sc.ref, "one_ray", one, one_keys, sample, spp), ("one ray", sample, spp), one, one_keys,
               sample, spp)
        want = ra.expect(sc.ref, "keys", rays, None, sample, spp)
        _check(itf, want, ("no keys", sample, spp), rays, None, sample, spp)
        _check(itf, want, ("arange", sample, spp), rays, np.arange(len(rays), dtype=np.uint32), sample, spp)


# ---------------------------------------------------------------------------
# 8. The chunk boundary
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["host", "device"])
def test_chunk_boundary(wpt, oracle, itf, route):
    """2^21 + 257 rays are two chunks. With the explicit keys `base index` the
    answer is the base answer tiled; without keys the rays around the boundary
    answer as the oracle does under keys = their positions (the second chunk's
    keys go on at 2^21)."""
    sc, base, index = ra.chunk_case(wpt, oracle)
    want = ra.expect(sc.ref, "chunk_base", base, None, 0, 1, 1, ra.CHUNK_DEPTH)
    a, b = ra.CHUNK_TAIL
    pos = np.arange(a, b, dtype=np.uint32)
    want_tail = ra.expect(sc.ref, "chunk_tail", base[index[a:b]], pos, 0, 1, 1, ra.CHUNK_DEPTH)
    assert want[1].all() and want_tail[1].all()
    rays = np.ascontiguousarray(base[index])
    n = len(rays)
    assert n == ra.CHUNK_N
    _start(itf, wpt, 100, depth=ra.CHUNK_DEPTH)
    _check(itf, want, "the base list", base)
    if route == "device":
        import torch

        dev = torch.device("cuda", torch.cuda.current_device())
        d_rays = torch.from_numpy(rays).to(dev)
        d_keys = torch.from_numpy(index.view(np.int32).copy()).to(dev)

        def query(keyed):
            rgb, status = itf.radiance_rays(d_rays, d_keys if keyed else None, 0, 1, 1, device=True)
            return rgb.cpu().numpy(), status.cpu().numpy()
    else:
        def query(keyed):
            return itf.radiance_rays(rays, index if keyed else None, 0, 1, 1)
    for keyed in (True, False):
        s0 = itf.stats()
        rgb, status = query(keyed)
        s1 = itf.stats()
        assert status.shape == (n,) and status.all()
        assert s1["paths"] - s0["paths"] == n
        if keyed:
            assert np.array_equal(rf.bits(rgb), rf.bits(want[0])[index]), "tiled keys"
            assert s1["rays"] + s1["shadow_rays"] - s0["rays"] - s0["shadow_rays"] == \
                int(np.bincount(index, minlength=len(base)) @ _rays_per_ray(sc, base))
        else:
            bad = np.any(rf.bits(rgb[a:b]) != rf.bits(want_tail[0]), axis=1)
            assert not bad.any(), ("positions as keys: differs at", a + np.nonzero(bad)[0][:8], int(bad.sum()))
            # and the first chunk's head: keys 0 .. 4098 are the base list's
            assert np.array_equal(rf.bits(rgb[: len(base)]), rf.bits(want[0]))


def _rays_per_ray(sc, base):
    """The oracle's rays + shadow rays of each base ray alone (depth 1: at most 2)."""
    return ra.once("chunk_rays_per_ray", lambda: np.array(
        [sc.ref.radiance_rays(base[i: i + 1], np.array([i], np.uint32), 0, 1, 1, ra.CHUNK_DEPTH, SEED)[2]["rays"]
         for i in range(len(base))], np.int64))
