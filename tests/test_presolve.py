"""The exact presolve of extension rays (wpt_presolve.h), host restatement.

A ray the presolve resolves must be one the reference's machine ends on a
plane or in the background, with the same (t, id) bits: checked against the
oracle's Scene::trace on ray sets built to sit on the decision's edges. The
guard boxes must partition the BVH2's leaves and contain them bit for bit.
CPU only; tests/test_gpu_presolve.py runs the same sets through the device.
"""
import numpy as np
import pytest

SCENES = (2, 0, 100)
NOT_LEAF = 0xFFFFFFFF


def scene_mesh(wpt, scene_id):
    return wpt.scenes.triangle_cloud(2000) if scene_id == 2 else None


def _unit(v):
    v = np.asarray(v, np.float32)
    return (v / np.linalg.norm(v, axis=1, keepdims=True).astype(np.float32)).astype(np.float32)


def camera_rays(wpt, scene_id, W=64, H=48, cam=None):
    """tracer.rs:175-193 at pixel centres (f32; not the kernel's bits, any ray
    will do): origin = camera, direction through the pixel, rot_x then rot_y."""
    cx, cy, cz, rx, ry = cam if cam is not None else wpt.scenes.scene_camera(scene_id)
    x, y = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    fx = ((x.ravel() + np.float32(0.5)) / np.float32(W) - np.float32(0.5)) * np.float32(W / H)
    fy = np.float32(0.5) - (y.ravel() + np.float32(0.5)) / np.float32(H)
    v = _unit(np.stack([fx, fy, np.full_like(fx, 0.8)], axis=1))
    c, s = np.float32(np.cos(rx)), np.float32(np.sin(rx))
    v = np.stack([v[:, 0], c * v[:, 1] - s * v[:, 2], s * v[:, 1] + c * v[:, 2]], axis=1)
    c, s = np.float32(np.cos(ry)), np.float32(np.sin(ry))
    v = np.stack([c * v[:, 0] + s * v[:, 2], v[:, 1], -s * v[:, 0] + c * v[:, 2]], axis=1)
    o = np.tile(np.array([cx, cy, cz], np.float32), (v.shape[0], 1))
    return np.concatenate([o, v], axis=1).astype(np.float32)


def _box_points(rng, box, n):
    return rng.uniform(box[:3], np.maximum(box[3:], box[:3]), (n, 3)).astype(np.float32)


def _corners(box):
    return np.array([[box[3 * i], box[1 + 3 * j], box[2 + 3 * k]] for i in (0, 1) for j in (0, 1) for k in (0, 1)],
                    np.float32)


def ray_sets(wpt, scene_id, dbg, seed=11):
    """name -> (n, 6) f32 rays; see the module docstring."""
    rng = np.random.default_rng(seed + scene_id)
    root, guards, _ = dbg.guards()
    cam = np.array(wpt.scenes.scene_camera(scene_id)[:3], np.float32)
    wide = np.concatenate([root[:3] - 2.0, root[3:] + 2.0]).astype(np.float32)
    sets = {"camera": camera_rays(wpt, scene_id)}
    # one or two direction components exactly 0 (1/d = inf in the slab test)
    o = np.concatenate([_box_points(rng, wide, 300), np.tile(cam, (300, 1))])
    d = _unit(rng.normal(size=(600, 3)))
    for k in range(600):
        d[k, k % 3] = 0.0
        if k % 4 == 0:
            d[k, (k + 1) % 3] = 0.0
    sets["zero"] = np.concatenate([o, d], axis=1).astype(np.float32)
    planes = dbg.shapes()[: dbg.num_inf]
    face, aim, inside = [], [], []
    for g in guards:
        # origins on a guard face (the coordinate is the box's own f32 value)
        p = _box_points(rng, g, 240)
        for k in range(240):
            p[k, k % 3] = g[k % 3 + 3 * ((k // 3) % 2)]
        face.append(np.concatenate([p, _unit(rng.normal(size=(240, 3)))], axis=1))
        # aimed at its corners and edge points, from the camera and from around the scene
        c = _corners(g)
        e = np.concatenate([c, (c[[0, 0, 0, 7, 7, 7]] + c[[1, 2, 4, 6, 5, 3]]) * np.float32(0.5)])
        tgt = np.tile(e, (12, 1))
        src = np.concatenate([np.tile(cam, (len(tgt) // 2, 1)), _box_points(rng, wide, len(tgt) - len(tgt) // 2)])
        dd = (tgt - src).astype(np.float32)
        aim.append(np.concatenate([src, dd], axis=1))
        aim.append(np.concatenate([src, _unit(dd)], axis=1))
        # plane hits inside the guard: aim at the guard's points projected onto each plane
        for pl in planes:
            loc, nrm = pl[:3], pl[3:6]
            q = _box_points(rng, g, 200)
            q = (q - ((q - loc) @ nrm)[:, None] * nrm / np.float32(nrm @ nrm)).astype(np.float32)
            keep = np.all((q >= g[:3]) & (q <= g[3:]), axis=1)
            q = q[keep]
            if len(q):
                src = (q + nrm * rng.uniform(0.5, 4.0, (len(q), 1)) + rng.normal(size=(len(q), 3)) * 0.7).astype(np.float32)
                inside.append(np.concatenate([src, (q - src).astype(np.float32)], axis=1))
    sets["face"] = np.concatenate(face).astype(np.float32)
    sets["aim"] = np.concatenate(aim).astype(np.float32)
    if inside:
        sets["inside"] = np.concatenate(inside).astype(np.float32)
    # cosine-weighted hemisphere rays leaving the planes (the diffuse bounce, material.rs:97-118)
    hemi = []
    for pl in planes[:2]:
        loc, nrm = pl[:3], _unit(pl[None, 3:6])[0]
        n = 400
        a = np.array([1.0, 0.0, 0.0], np.float32) if abs(nrm[0]) < 0.9 else np.array([0.0, 1.0, 0.0], np.float32)
        u = _unit(np.cross(nrm, a)[None])[0]
        w = np.cross(nrm, u).astype(np.float32)
        q = _box_points(rng, wide, n)
        q = (q - ((q - loc) @ nrm)[:, None] * nrm + nrm * np.float32(0.0002)).astype(np.float32)
        r1, r2 = rng.random(n, dtype=np.float32), rng.random(n, dtype=np.float32)
        ang = np.float32(2 * np.pi) * r1
        d = (np.cos(ang) * np.sqrt(1 - r2))[:, None] * u + np.sqrt(r2)[:, None] * nrm + \
            (np.sin(ang) * np.sqrt(1 - r2))[:, None] * w
        hemi.append(np.concatenate([q, _unit(d)], axis=1))
    sets["hemisphere"] = np.concatenate(hemi).astype(np.float32)
    return sets


_CASES = {}


def _case(wpt, oracle, sid):
    """Per scene: the debug scene, the ray sets, the presolve's verdicts and the oracle's hits, made once."""
    if sid in _CASES:
        return _CASES[sid]
    mesh = scene_mesh(wpt, sid)
    dbg = wpt.interface.DebugScene(sid, mesh)
    ref = oracle.OracleScene(sid, mesh)
    out = {}
    for name, rays in ray_sets(wpt, sid, dbg).items():
        res, t, ids = dbg.presolve(rays)
        t_r, id_r, _ = ref.trace_rays(rays)
        out[name] = (rays, res, t, ids, t_r, id_r)
    _CASES[sid] = (sid, dbg, out)
    return _CASES[sid]


@pytest.mark.parametrize("scene_id", SCENES)
def test_resolved_rays_are_plane_or_miss_with_the_oracles_bits(wpt, oracle, scene_id):
    sid, dbg, sets = _case(wpt, oracle, scene_id)
    total = 0
    for name, (rays, res, t, ids, t_r, id_r) in sets.items():
        print(f"scene {sid} {name}: {len(rays)} rays, resolved {res.mean():.3f}, oracle plane-or-miss "
              f"{(id_r < dbg.num_inf).mean():.3f}")
        assert np.all(id_r[res] < dbg.num_inf), (sid, name, int(np.sum(id_r[res] >= dbg.num_inf)))
        assert np.array_equal(ids[res], id_r[res]), (sid, name)
        assert np.array_equal(t[res].view(np.uint32), t_r[res].view(np.uint32)), (sid, name)
        total += int(res.sum())
    assert total > 0  # every scene resolves something over the sets


def test_not_vacuous_on_the_scene_2_camera_set(wpt, oracle):
    _, _, sets = _case(wpt, oracle, 2)
    _, res, _, _, _, id_r = sets["camera"]
    assert res.any() and not res.all()
    assert res.mean() >= 0.5, res.mean()
    assert (id_r >= 2).any()  # the camera sees the mesh: those rays cannot be resolved


@pytest.mark.parametrize("scene_id", SCENES)
def test_zero_component_rays_are_never_resolved(wpt, oracle, scene_id):
    _, _, sets = _case(wpt, oracle, scene_id)
    rays, res = sets["zero"][0], sets["zero"][1]
    assert np.all(np.any(rays[:, 3:] == 0.0, axis=1))
    assert not res.any()


@pytest.mark.parametrize("scene_id", SCENES)
def test_guards_partition_the_leaves_and_contain_them(wpt, oracle, scene_id):
    sid, dbg, _ = _case(wpt, oracle, scene_id)
    root, guards, leaf_guard = dbg.guards()
    nodes = dbg.nodes()
    bounds = nodes[:, :6].view(np.float32)
    leaves, todo = [], [0]
    while todo:
        n = todo.pop()
        if nodes[n, 7] != 0:
            leaves.append(n)
        else:
            todo += [int(nodes[n, 6]), int(nodes[n, 6]) + 1]
    leaves = np.array(sorted(leaves))
    assert 1 <= len(guards) <= 4
    assert np.array_equal(root, bounds[0])
    g = leaf_guard[leaves]
    assert np.all(g < len(guards))                       # every leaf is in exactly one group
    others = np.setdiff1d(np.arange(len(nodes)), leaves)
    assert np.all(leaf_guard[others] == NOT_LEAF)        # and nothing else is
    for k, box in enumerate(guards):
        mine = bounds[leaves[g == k]]
        assert len(mine) > 0
        assert np.all(mine[:, :3] >= box[:3]) and np.all(mine[:, 3:] <= box[3:])
        assert np.array_equal(box[:3], mine[:, :3].min(axis=0)) and np.array_equal(box[3:], mine[:, 3:].max(axis=0))
    if sid == 2:  # {cloud}, {lights}: the two light triangles lie in the plane y = 7, alone in their guard
        assert len(guards) == 2
        top = max(guards, key=lambda b: float(b[1]))  # (leaf boxes are padded by a few ulps)
        assert abs(float(top[1]) - 7.0) < 1e-3 and abs(float(top[4]) - 7.0) < 1e-3


def test_no_bvh_scene_resolves_nothing(wpt):
    dbg = wpt.interface.DebugScene(101)
    res, _, _ = dbg.presolve(camera_rays(wpt, 101))
    assert not res.any()
