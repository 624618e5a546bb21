"""The exact presolve of NEE shadow rays (presolve_shadow, wpt_presolve.h),
host restatement.

A shadow ray the presolve resolves must be one the reference's
Scene::shadow_ray calls unoccluded: checked against the oracle on {p, q} sets
built to sit on the decision's edges (planes between, the other light
triangle, guard corners / edges / faces, segments ending just before and
behind a guard, zero direction components, degenerate lengths, origins inside
a guard). No tolerance and no exceptions. CPU only;
tests/test_gpu_presolve_shadow.py runs the same sets through the device.
"""
import numpy as np
import pytest

from test_presolve import _box_points, _corners, camera_rays, scene_mesh

SCENES = (2, 0, 100)
K_MAX_GUARD_LIGHTS = 4


def _light_points(rng, shapes, lights, n):
    """n random points on random lights (Triangle::pick_random's form) and their shape ids."""
    li = lights[rng.integers(0, len(lights), n)]
    v = shapes[li, :9].reshape(n, 3, 3).astype(np.float32)
    q1s, q2 = np.sqrt(rng.random(n, dtype=np.float32)), rng.random(n, dtype=np.float32)
    q = v[:, 0] * (1 - q1s)[:, None] + v[:, 1] * (q1s * (1 - q2))[:, None] + v[:, 2] * (q2 * q1s)[:, None]
    return q.astype(np.float32), li.astype(np.int32)


def shadow_sets(wpt, ref, scene_id, dbg, seed=23):
    """name -> ((n, 6) f32 {p, q}, (n,) i32 light shape ids); see the module docstring."""
    rng = np.random.default_rng(seed + scene_id)
    shapes = dbg.shapes()
    lights = dbg.lights().astype(np.int64)
    planes = shapes[: dbg.num_inf]
    root, guards, _ = dbg.guards()
    mask, _ = dbg.guard_lights()
    wide = np.concatenate([root[:3] - 2.0, root[3:] + 2.0]).astype(np.float32)
    sets = {}

    def put(name, p, q, li):
        sets[name] = (np.concatenate([p, q], axis=1).astype(np.float32), np.asarray(li, np.int32))

    # path points: the camera rays' hit points on non-emissive shapes
    rays = camera_rays(wpt, scene_id)
    t_r, id_r, _ = ref.trace_rays(rays)
    ok = (id_r >= 0) & np.isfinite(t_r)
    ok[ok] = shapes[id_r[ok], 13] == 0.0
    hp = (rays[ok, :3] + rays[ok, 3:] * t_r[ok, None]).astype(np.float32)
    hp = hp[rng.permutation(len(hp))[:700]]
    q, li = _light_points(rng, shapes, lights, len(hp))
    put("path", hp, q, li)
    below_p, below_q, below_l = [], [], []
    for pl in planes:  # the same points pushed below each plane: the plane lies between
        p = hp[:250] - (pl[3:6] / np.float32(np.linalg.norm(pl[3:6]))) * np.float32(1e-3)
        q, li = _light_points(rng, shapes, lights, len(p))
        below_p.append(p), below_q.append(q), below_l.append(li)
    if below_p:
        put("path_below", np.concatenate(below_p), np.concatenate(below_q), np.concatenate(below_l))

    # light edges: vertices, edge points (the diagonal shared with the coplanar
    # neighbour among them), with the triangle itself and its neighbour as the light
    tgt, tl = [], []
    for k, sid in enumerate(lights):
        v = shapes[sid, :9].reshape(3, 3).astype(np.float32)
        pts = [v[0], v[1], v[2]]
        for a, b in ((0, 1), (1, 2), (2, 0)):
            for s in (0.25, 0.5, 0.75):
                pts.append((v[a] * np.float32(1 - s) + v[b] * np.float32(s)).astype(np.float32))
        for other in (sid, lights[(k + 1) % len(lights)]):
            tgt += pts
            tl += [other] * len(pts)
    tgt, tl = np.array(tgt, np.float32), np.array(tl, np.int32)
    rep = max(1, 1000 // len(tgt))
    tgt, tl = np.tile(tgt, (rep, 1)), np.tile(tl, rep)
    src = np.concatenate([hp[rng.integers(0, len(hp), len(tgt) // 2)], _box_points(rng, wide, len(tgt) - len(tgt) // 2)])
    put("light_edges", src, tgt, tl)

    # guard geometry
    gp, gq, gl = [], [], []
    fp, fq, fl = [], [], []
    ip, iq, il = [], [], []
    for gi, g in enumerate(guards):
        c = _corners(g)
        e = np.concatenate([c, (c[[0, 0, 0, 7, 7, 7]] + c[[1, 2, 4, 6, 5, 3]]) * np.float32(0.5)])
        f = _box_points(rng, g, 12)
        for k in range(12):
            f[k, k % 3] = g[k % 3 + 3 * ((k // 3) % 2)]  # points on the faces
        e = np.concatenate([e, f])
        on_plane = _box_points(rng, wide, len(e))
        if len(planes):
            pl = planes[gi % len(planes)]
            nrm = pl[3:6] / np.float32(np.linalg.norm(pl[3:6]))
            on_plane = (on_plane - ((on_plane - pl[:3]) @ nrm)[:, None] * nrm + nrm * np.float32(2e-4)).astype(np.float32)
        for src in (_box_points(rng, wide, len(e)), on_plane):
            # the segment ends just before, at and just behind the point, and far behind it
            for s in (0.999, 0.99999, 1.0, 1.00001, 1.001, 3.0):
                gp.append(src)
                gq.append((src + (e - src) * np.float32(s)).astype(np.float32))
                gl.append(lights[rng.integers(0, len(lights), len(e))])
        # origins exactly on a guard face
        p = _box_points(rng, g, 120)
        for k in range(120):
            p[k, k % 3] = g[k % 3 + 3 * ((k // 3) % 2)]
        q, li = _light_points(rng, shapes, lights, len(p))
        fp.append(p), fq.append(q), fl.append(li)
        # origins inside an ordinary guard, far enough from its faces that the
        # ray's own origin p + d * EPSILON is inside too (flat guards have no such points)
        inner = np.concatenate([g[:3] + np.float32(1e-3), g[3:] - np.float32(1e-3)]).astype(np.float32)
        if not (mask >> gi) & 1 and np.all(inner[:3] < inner[3:]):
            p = _box_points(rng, inner, 250)
            q, li = _light_points(rng, shapes, lights, len(p))
            ip.append(p), iq.append(q), il.append(li)
    put("guard", np.concatenate(gp), np.concatenate(gq), np.concatenate(gl))
    put("guard_face", np.concatenate(fp), np.concatenate(fq), np.concatenate(fl))
    if ip:
        put("interior", np.concatenate(ip), np.concatenate(iq), np.concatenate(il))

    # one or two direction components exactly 0
    p = np.concatenate([_box_points(rng, wide, 300), hp[rng.integers(0, len(hp), 300)]])
    q, li = _light_points(rng, shapes, lights, len(p))
    for k in range(len(p)):
        q[k, k % 3] = p[k, k % 3]
        if k % 4 == 0:
            q[k, (k + 1) % 3] = p[k, (k + 1) % 3]
    put("zero", p, q, li)

    # degenerate lengths: p == q, and |q - p| below EPSILON
    p = np.concatenate([hp[:200], _box_points(rng, wide, 200)])
    d = rng.normal(size=(len(p), 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
    q = p.copy()
    q[200:300] = p[200:300] + d[200:300] * np.float32(1e-5)
    q[100:200] = p[100:200] + d[100:200] * np.float32(1e-4)
    _, li = _light_points(rng, shapes, lights, len(p))
    put("degenerate", p, q, li)
    return sets


_CASES = {}


def shadow_case(wpt, oracle, sid):
    """Per scene: the debug scene, the sets, the presolve's verdicts and the oracle's, made once."""
    if sid in _CASES:
        return _CASES[sid]
    mesh = scene_mesh(wpt, sid)
    dbg = wpt.interface.DebugScene(sid, mesh)
    ref = oracle.OracleScene(sid, mesh)
    out = {}
    for name, (pq, li) in shadow_sets(wpt, ref, sid, dbg).items():
        out[name] = (pq, li, dbg.presolve_shadow(pq, li), ref.shadow_rays(pq, li).astype(bool))
    _CASES[sid] = (sid, dbg, out)
    return _CASES[sid]


@pytest.mark.parametrize("scene_id", SCENES)
def test_resolved_shadow_rays_are_unoccluded_by_the_oracle(wpt, oracle, scene_id):
    sid, _, sets = shadow_case(wpt, oracle, scene_id)
    for name, (pq, li, res, occ) in sets.items():
        print(f"scene {sid} {name}: {len(pq)} rays, resolved {res.mean():.3f}, oracle unoccluded {(~occ).mean():.3f}")
        assert not np.any(occ[res]), (sid, name, int(np.sum(occ[res])))


@pytest.mark.parametrize("scene_id", SCENES)
def test_zero_component_shadow_rays_are_never_resolved(wpt, oracle, scene_id):
    _, _, sets = shadow_case(wpt, oracle, scene_id)
    pq, _, res, _ = sets["zero"]
    assert np.all(np.any(pq[:, 3:] == pq[:, :3], axis=1))
    assert not res.any()


@pytest.mark.parametrize("scene_id", SCENES)
def test_origins_inside_an_ordinary_guard_are_never_resolved(wpt, oracle, scene_id):
    _, _, sets = shadow_case(wpt, oracle, scene_id)
    assert "interior" in sets or scene_id != 2  # scene 2: the cloud's guard
    if "interior" in sets:
        assert len(sets["interior"][0]) >= 250 and not sets["interior"][2].any()


@pytest.mark.parametrize("scene_id", SCENES)
def test_degenerate_lengths_are_never_resolved_when_p_equals_q(wpt, oracle, scene_id):
    _, _, sets = shadow_case(wpt, oracle, scene_id)
    pq, _, res, _ = sets["degenerate"]
    same = np.all(pq[:, :3] == pq[:, 3:], axis=1)
    assert same.sum() >= 200 and not res[same].any()


def test_no_bvh_scene_resolves_no_shadow_ray(wpt):
    dbg = wpt.interface.DebugScene(101)
    rng = np.random.default_rng(5)
    pq = rng.uniform(-3, 3, (500, 6)).astype(np.float32)
    li = np.full(500, dbg.num_inf, np.int32)
    assert not dbg.presolve_shadow(pq, li).any()


@pytest.mark.parametrize("scene_id", SCENES)
def test_light_guards_hold_only_a_few_emissive_triangles(wpt, oracle, scene_id):
    sid, dbg, _ = shadow_case(wpt, oracle, scene_id)
    mask, ids = dbg.guard_lights()
    _, guards, leaf_guard = dbg.guards()
    shapes, nodes = dbg.shapes(), dbg.nodes()
    assert len(ids) <= K_MAX_GUARD_LIGHTS and mask < (1 << len(guards))
    assert (mask == 0) == (len(ids) == 0)
    held = []
    for n in np.nonzero(leaf_guard != 0xFFFFFFFF)[0]:
        if (mask >> int(leaf_guard[n])) & 1:
            held += list(range(dbg.num_inf + int(nodes[n, 6]), dbg.num_inf + int(nodes[n, 6]) + int(nodes[n, 7])))
    assert sorted(held) == sorted(ids.tolist())  # exactly the primitives of the light guards' leaves
    for s in held:
        assert shapes[s, 12] == 0.0 and shapes[s, 13] == 1.0  # an emissive triangle
    if sid == 2:  # {cloud}, {lights}: the lights' group is the light guard
        top = max(range(len(guards)), key=lambda k: float(guards[k][1]))
        assert mask == 1 << top and sorted(ids.tolist()) == sorted(dbg.lights().tolist())


def test_not_vacuous_on_the_scene_2_path_points(wpt, oracle):
    _, _, sets = shadow_case(wpt, oracle, 2)
    _, _, res, occ = sets["path"]
    share = res[~occ].mean()
    print(f"scene 2 path points: {len(res)} rays, unoccluded {(~occ).mean():.3f}, resolved of those {share:.3f}")
    assert (~occ).sum() > 300 and share >= 0.5
