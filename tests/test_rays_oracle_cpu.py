"""The oracle's ray query (OracleScene.radiance_rays) without a GPU.

First the entry itself against the established oracle: a query of a frame's
primary rays is render()'s sample of that frame, bit for bit and ray for ray
(the anchors and probes tests/test_gpu_rays.py uses), for any thread count;
spp is the sequential f32 sum; keys select the stream; the status rule is the
table's. Then the conditions tests/rays_adversarial.py is built for, asserted
on the oracle alone, so that tests/test_gpu_rays_adversarial.py cannot pass
vacuously. Measured values: profiles/rayparity/README.md.
"""
import numpy as np
import pytest

import adversarial as adv
import rays_adversarial as ra
import rays_fixtures as rf
from test_gpu_rays import ANCHORS

SEED, DEPTH = rf.SEED, rf.DEPTH


def _same(got, want, what):
    bad = np.any(rf.bits(got) != rf.bits(want), axis=1)
    assert not bad.any(), (what, "differs on", int(bad.sum()), "of", len(bad), "rays, first", int(np.argmax(bad)),
                           got[np.argmax(bad)], want[np.argmax(bad)])


def _nonzero(rgb):
    return float(np.mean((rgb != 0).any(axis=1)))


def _differ(a, b):
    return float(np.mean((rf.bits(a) != rf.bits(b)).any(axis=1)))


# ---------------------------------------------------------------------------
# The entry against render()
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,vp,types,depth", ANCHORS, ids=lambda v: str(v).replace(" ", ""))
def test_frame_rays_give_the_frame(wpt, oracle, name, vp, types, depth):
    sc = rf.scene(wpt, oracle, name)
    for t in types:
        for s in (0, 7):
            acc, st = sc.ref.render(vp[0], vp[1], sc.cam, t, t, depth, SEED, s0=s, spp=1, threads=4)
            rgb, status, qst = sc.ref.radiance_rays(sc.rays(vp, s), None, s, 1, t, depth, SEED, threads=4)
            assert status.all()
            _same(rgb, acc.reshape(-1, 3), (name, vp, t, s, depth))
            assert qst == st, (name, vp, t, s, depth)
            assert st["rays"] > 0 and (st["shadow_rays"] > 0) == (t != 0)


@pytest.mark.parametrize("name", list(rf.SCENES))
def test_probes_give_the_one_pixel_frames(wpt, oracle, name):
    sc = rf.scene(wpt, oracle, name)
    keys = np.zeros(rf.PROBES, np.uint32)
    for t in (0, 1):
        want, want_rays = sc.probe_expect(t)
        rgb, status, st = sc.ref.radiance_rays(sc.probe_rays(), keys, rf.PROBE_SAMPLE, 1, t, DEPTH, SEED)
        assert status.all()
        _same(rgb, want, (name, t))
        assert st["rays"] == want_rays


def test_thread_counts_give_the_same_bits(wpt, oracle):
    sc, rays = ra.box_set(wpt, oracle)
    for t in (1, 2):
        res = [sc.ref.radiance_rays(rays, None, 2, 3, t, DEPTH, SEED, threads=n) for n in (1, 3, 8)]
        for r in res[1:]:
            _same(r[0], res[0][0], ("threads", t))
            assert np.array_equal(r[1], res[0][1]) and r[2] == res[0][2]
        assert res[0][2]["shadow_rays"] > 0 and _nonzero(res[0][0]) > 0


def test_spp_is_the_sequential_sum(wpt, oracle):
    sc, rays = ra.box_set(wpt, oracle)
    for t in (0, 1):
        parts = [sc.ref.radiance_rays(rays, None, s, 1, t, DEPTH, SEED) for s in (5, 6, 7)]
        got, _, st = sc.ref.radiance_rays(rays, None, 5, 3, t, DEPTH, SEED)
        _same(got, rf.seq_sum([p[0] for p in parts]), ("spp", t))
        assert st == {k: sum(p[2][k] for p in parts) for k in st}
        assert (rf.bits(parts[0][0]) != rf.bits(parts[1][0])).any()


def test_keys(wpt, oracle):
    sc, rays = ra.box_set(wpt, oracle)
    n = len(rays)
    q = lambda r, k: sc.ref.radiance_rays(r, k, 1, 2, 1, DEPTH, SEED)[0]  # noqa: E731
    base = q(rays, None)
    _same(q(rays, np.arange(n, dtype=np.uint32)), base, "keys = arange")
    perm = np.random.default_rng(0x6B65).permutation(n)
    _same(q(rays[perm], perm.astype(np.uint32)), base[perm], "permuted")
    # a key is 32 bits: 2^32 - 1 is a key like any other, and not key 0's stream
    hi = q(rays, np.full(n, 0xFFFFFFFF, np.uint32))
    assert _differ(hi, q(rays, np.zeros(n, np.uint32))) > 0
    sc, one, keys = ra.one_ray_case(wpt, oracle)
    for sample, spp in ra.KEY_SAMPLES:
        rgb = ra.expect(sc.ref, "one_ray", one, keys, sample, spp)[0]
        distinct = len(np.unique(rf.bits(rgb), axis=0))
        print(f"one ray, 300 keys, sample {sample:#x} spp {spp}: {distinct} distinct answers")
        assert distinct > 100


def test_status_rule(wpt, oracle):
    """The oracle's restatement of the validity rule on the table, against its
    numpy twin and the product's host export; an invalid ray is +0 and counts nothing."""
    sc = rf.scene(wpt, oracle, "box")
    rays = np.array([v[0] for v in rf.VALIDITY], np.float32)
    want = np.array([v[1] for v in rf.VALIDITY], np.uint8)
    rgb, status, st = sc.ref.radiance_rays(rays, None, 0, 2, 1, DEPTH, SEED)
    assert np.array_equal(status, want) and np.array_equal(rf.valid(rays), want)
    assert np.array_equal(wpt.interface.rays_valid(rays), want)
    assert np.all(rf.bits(rgb[want == 0]) == 0)
    _, st_valid, st2 = sc.ref.radiance_rays(rays[want == 1], np.nonzero(want)[0].astype(np.uint32), 0, 2, 1, DEPTH, SEED)
    assert st_valid.all() and st2 == st
    rgb0, st0, none = sc.ref.radiance_rays(rays[want == 0], None, 0, 2, 1, DEPTH, SEED)
    assert not st0.any() and np.all(rf.bits(rgb0) == 0) and none == {"rays": 0, "shadow_rays": 0, "node_visits": 0}
    assert sc.ref.radiance_rays(np.zeros((0, 6), np.float32))[0].shape == (0, 3)


# ---------------------------------------------------------------------------
# The conditions the families are built for
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ra.MESHES)
def test_mesh_sets_produce_their_conditions(wpt, oracle, name):
    """Per scene-2 mesh, over its concatenated sets at depth 4: every answer is
    finite; the NEE answers (type 1: light at every lit diffuse hit; a type-0
    path only finds the light by chance) are non-zero on 5 % .. 95 % of the
    rays; types 0 and 1 differ on at least 5 %; at least 10 % of the rays hit a
    finite shape first and at least 10 % a plane or nothing, so both ends of
    the presolving producer's stream are used."""
    mesh, ref, rays = ra.mesh_case(wpt, oracle, name)
    assert len(rays) <= ra.MAX_SET_RAYS and rf.valid(rays).all()
    r0, s0, _ = ra.expect(ref, ("mesh", name), rays, rtype=0)
    r1, s1, st1 = ra.expect(ref, ("mesh", name), rays, rtype=1)
    assert s0.all() and s1.all()
    assert np.isfinite(r0).all() and np.isfinite(r1).all()
    ids = ref.trace_rays(rays)[1]
    finite_first = float(np.mean(ids >= ref.num_inf))
    print(f"{name}: {len(rays)} rays, non-zero type 0 {_nonzero(r0):.3f} type 1 {_nonzero(r1):.3f}, "
          f"types differ {_differ(r0, r1):.3f}, finite shape first {finite_first:.3f}, shadow rays {st1['shadow_rays']}")
    assert 0.05 <= _nonzero(r1) <= 0.95
    assert _differ(r0, r1) >= 0.05
    assert finite_first >= 0.10 and 1.0 - finite_first >= 0.10
    assert np.all(ref.shapes()[: ref.num_inf, 12] == adv.KIND_PLANE)   # ids below num_inf are the planes


@pytest.mark.parametrize("scene_id", list(ra.SHAPE_SCENES))
def test_shape_sets_produce_their_conditions(wpt, oracle, scene_id):
    """Finite everywhere; the museum's torus and aarect sets at spp 16 are
    non-zero on at least 5 % of their rays."""
    sc, sets = ra.shape_case(wpt, oracle, scene_id)
    spp = ra.MUSEUM_SPP if scene_id == 0 else 1
    for s, rays in sets.items():
        assert rf.valid(rays).all()
        for t in (0, 1):
            rgb = ra.expect(sc.ref, ("shapes", scene_id, s), rays, None, 0, spp, t)[0]
            assert np.isfinite(rgb).all()
            print(f"scene {scene_id} {s}: {len(rays)} rays, spp {spp}, type {t}: non-zero {_nonzero(rgb):.3f}")
            if scene_id == 0 and t == 1:
                assert _nonzero(rgb) >= 0.05
    sc, rays = ra.box_set(wpt, oracle)
    for t in (0, 1, 2):
        assert np.isfinite(ra.expect(sc.ref, "box_set", rays, rtype=t)[0]).all()
    assert _differ(ra.expect(sc.ref, "box_set", rays, rtype=1)[0], ra.expect(sc.ref, "box_set", rays, rtype=2)[0]) > 0
    # PNEE on a scene-2 fixture and on the cloud's probes
    _, ref, rays = ra.pnee_mesh_case(wpt, oracle)
    rgb = ra.expect(ref, "pnee_mesh", rays, rtype=2)[0]
    assert np.isfinite(rgb).all() and _differ(rgb, ra.expect(ref, "pnee_mesh", rays, rtype=1)[0]) > 0.05
    cloud = rf.scene(wpt, oracle, "cloud")
    assert np.isfinite(ra.expect(cloud.ref, "cloud_probes", cloud.probe_rays(), np.zeros(rf.PROBES, np.uint32), 3, 1, 2)[0]).all()


@pytest.mark.parametrize("name", ra.SCALED_MESHES)
def test_scaled_directions_produce_their_conditions(wpt, oracle, name):
    """No scaled ray is rejected; every answer is finite; at 2^-20 and 2^20
    every answer is the unit direction's, bit for bit (every product and
    quotient of the path scales exactly); at 1e-37 and 3e38 at least 3 % differ
    from it and at 1e-42 at least 30 %: the family reaches denormal and
    near-overflow arithmetic."""
    mesh, ref, unit, scaled = ra.scaled_case(wpt, oracle, name)
    assert len(unit) == 600 and rf.valid(unit).all()
    for t in (0, 1):
        base = ra.expect(ref, ("scaled", name, 1.0), unit, rtype=t)[0]
        assert np.isfinite(base).all()
        for s in ra.SCALES:
            assert rf.valid(scaled[s]).all()
            rgb, status, _ = ra.expect(ref, ("scaled", name, s), scaled[s], rtype=t)
            assert status.all() and np.isfinite(rgb).all()
            d = _differ(rgb, base)
            print(f"{name} type {t} scale {s:g}: differ from the unit direction's {d:.3f}, non-zero {_nonzero(rgb):.3f}")
            if s in ra.EXACT_SCALES:
                assert d == 0.0
            # (type 0 is non-zero on under 2 % of these rays: it cannot differ on more)
            if t == 1 and s in (1e-37, 3e38):
                assert d >= 0.03
            if t == 1 and s == 1e-42:
                assert d >= 0.30


def test_spp_family_produces_its_conditions(wpt, oracle):
    """Zero and non-zero answers at every spp; every straddle case of the GPU
    test starts a block inside a ray's samples (rem0 != 0), and so does the
    default batch at every odd spp."""
    sc, rays = ra.spp_case(wpt, oracle)
    assert len(rays) == 100
    for spp in ra.SPPS:
        rgb = ra.expect(sc.ref, "spp", rays, None, ra.SPP_SAMPLE, spp)[0]
        assert np.isfinite(rgb).all() and 0.0 < _nonzero(rgb) < 1.0, spp
    for spp in ra.STRADDLE_SPPS:
        for batch in ra.STRADDLE_BATCHES + (1 << 27,):
            assert (ra.block_starts(100 * spp, batch) % spp != 0).any(), (spp, batch)


def test_keys_family_produces_its_conditions(wpt, oracle):
    sc, rays, keys = ra.keys_case(wpt, oracle)
    assert rays.shape == (300, 6) and keys.dtype == np.uint32 and set(ra.EDGE_KEYS) <= set(keys.tolist())
    assert len(np.unique(keys)) < 300 and (keys > 0x7FFFFFFF).sum() > 50
    for sample, spp in ra.KEY_SAMPLES:
        rgb = ra.expect(sc.ref, "keys", rays, keys, sample, spp)[0]
        assert np.isfinite(rgb).all() and 0.0 < _nonzero(rgb) < 1.0
        # the keys matter: the same rays under keys = the position give other answers
        assert _differ(rgb, ra.expect(sc.ref, "keys", rays, None, sample, spp)[0]) > 0.05


def test_chunk_family_produces_its_conditions(wpt, oracle):
    """The base answers at depth 1 are finite and mixed; in the tail past the
    chunk boundary the position keys give other answers than the base keys, so
    a second chunk that started its keys at 0 again would show."""
    sc, base, index = ra.chunk_case(wpt, oracle)
    assert len(base) == ra.CHUNK_BASE and len(index) == ra.CHUNK_N == (1 << 21) + 257
    rgb = ra.expect(sc.ref, "chunk_base", base, None, 0, 1, 1, ra.CHUNK_DEPTH)[0]
    assert np.isfinite(rgb).all() and 0.05 < _nonzero(rgb) < 0.95
    a, b = ra.CHUNK_TAIL
    assert a < ra.CHUNK < b
    pos = np.arange(a, b, dtype=np.uint32)
    tail = ra.expect(sc.ref, "chunk_tail", base[index[a:b]], pos, 0, 1, 1, ra.CHUNK_DEPTH)[0]
    in_second = pos >= ra.CHUNK
    restarted = sc.ref.radiance_rays(base[index[a:b]], (pos - np.uint32(ra.CHUNK)).astype(np.uint32), 0, 1, 1, ra.CHUNK_DEPTH, SEED)[0]
    assert _differ(tail[in_second], restarted[in_second]) > 0.05
    assert _differ(tail, rgb[index[a:b]]) > 0.05


def test_light_debug_produces_its_conditions(wpt, oracle):
    """Light debug on the box set: no shadow ray, and more non-zero answers
    than without it (every light sample that faces the point counts)."""
    sc, rays = ra.box_set(wpt, oracle)
    for t in (1, 2):
        plain = ra.expect(sc.ref, "box_set", rays, rtype=t)
        dbg = ra.expect(sc.ref, "box_set", rays, rtype=t, light_debug=1)
        print(f"type {t}: non-zero {_nonzero(dbg[0]):.3f} with light debug, {_nonzero(plain[0]):.3f} without")
        assert np.isfinite(dbg[0]).all()
        assert dbg[2]["shadow_rays"] == 0 and plain[2]["shadow_rays"] > 0
        assert _nonzero(dbg[0]) > _nonzero(plain[0])
    assert np.isfinite(ra.expect(sc.ref, "box_set", rays, rtype=0, light_debug=1)[0]).all()
