"""Cases of the first-hit planes and the filter along a caller's rays
(wpt_first_hit_rays, wpt_denoise_rays).

A plain helper module (no pytest hooks): tests/test_rayframe_cpu.py checks on
the oracle alone that the ray sets produce the conditions they are built for
and that the filter helps the fisheye frame; tests/test_gpu_rayframe.py compares
the device with the same expectations, bit for bit. Everything is computed once
per process and shared; nothing returned here is modified.

The expected planes of arbitrary rays come from what the oracle offers, the way
first_hit_fixtures.Case gets them for a camera's pixels: (t, id, visits) from
OracleScene.trace_rays, the normal from oracle_shape_trace on the reported
shape, kind from the oracle's emissive flag, an emitter's albedo from the
oracle's depth-1 NoNEE radiance_rays, a diffuse shape's albedo from the host
scene's materials. Rays the status rule rejects get the invalid entries and
never reach the oracle.
"""
import numpy as np

import denoise_fixtures as dn
import first_hit_fixtures as fh
import rays_adversarial as ra
import rays_fixtures as rf

F32 = np.float32
SEED = rf.SEED
PLANES = ("t", "id", "visits", "normal", "albedo", "kind", "status")
GUIDES = ("t", "normal", "albedo", "kind")
LDS_SLOTS = 9                    # WPT_LDS_SLOTS: traversal stack entries kept in LDS
WAVE, BLOCK = 64, 256            # a wave's rays, kTBlock

# the fisheye frame: a 64 x 48 equidistant 180 degree fisheye looking along +z
FISH_W, FISH_H = 64, 48
FISH_ORIGINS = ((0.0, 1.0, -1.5), (0.3, 0.7, -0.2), (-0.5, 1.5, 0.5))
FISH_INVALID = 1268              # rays outside the image circle at 64 x 48
FISH_SCENE = 100
FISH_DEPTH = 4
FISH_SPP = 4                     # samples 0..3
FISH_REF = (1000, 1024)          # the reference frame: samples 1000..2023
HELP_RATIO = 0.5                 # the filtered error is below half the raw error

_CACHE = {}


def once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _frozen(a):
    a.setflags(write=False)
    return a


def fisheye_rays(w, h, origin):
    """(w * h, 6) f32, raster order: pixel (x, y) looks along
    (sin th cos ph, sin th sin ph, cos th) with u = ((x + 0.5) / w * 2 - 1) * (w / h),
    v = 1 - (y + 0.5) / h * 2, r = sqrt(u^2 + v^2), th = r * pi / 2, ph = atan2(v, u),
    the direction divided by its norm; (0, 0, 0) where r > 1. All in numpy f32."""
    one, two, half = F32(1.0), F32(2.0), F32(0.5)
    x = np.arange(w, dtype=F32)[None, :].repeat(h, 0)
    y = np.arange(h, dtype=F32)[:, None].repeat(w, 1)
    u = ((x + half) / F32(w) * two - one) * (F32(w) / F32(h))
    v = one - (y + half) / F32(h) * two
    r = np.sqrt(u * u + v * v)
    th = r * F32(np.pi) / two
    ph = np.arctan2(v, u)
    d = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], axis=-1).astype(F32)
    d = (d / np.sqrt((d * d).sum(-1, keepdims=True))).astype(F32)
    d[r > one] = 0
    rays = np.empty((h * w, 6), F32)
    rays[:, :3] = np.asarray(origin, F32)
    rays[:, 3:] = d.reshape(-1, 3)
    return rays


def fisheye(origin=FISH_ORIGINS[0], vp=(FISH_W, FISH_H)):
    return once(("fisheye", tuple(origin), vp), lambda: _frozen(fisheye_rays(vp[0], vp[1], origin)))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8 if a.dtype == np.uint8 else np.uint32)


def same(a, b, what):
    a, b = bits(a).reshape(-1), bits(b).reshape(-1)
    bad = np.nonzero(a != b)[0]
    assert a.shape == b.shape and len(bad) == 0, (what, len(bad), bad[:8], a[bad[:8]], b[bad[:8]])


def same_planes(got, want, what, names=None):
    for k in names or want:
        same(got[k], want[k], (what, k))


def invalid_planes(n):
    """The entries of n rays that are never started."""
    return {"t": np.full(n, np.inf, F32), "id": np.full(n, -1, np.int32), "visits": np.zeros(n, np.uint32),
            "normal": np.zeros((n, 3), F32), "albedo": np.zeros((n, 3), F32), "kind": np.zeros(n, np.uint8),
            "status": np.zeros(n, np.uint8)}


def expected_planes(oracle, ref, mats, rays):
    """The seven planes of `rays` (n, 6) on oracle scene `ref`; mats: the host
    scene's materials (DebugScene.materials())."""
    rays = np.ascontiguousarray(rays, F32).reshape(-1, 6)
    n = len(rays)
    out = invalid_planes(n)
    ok = rf.valid(rays).astype(bool)
    out["status"] = ok.astype(np.uint8)
    if not ok.any():
        return out
    live = np.ascontiguousarray(rays[ok])
    t, ids, visits = ref.trace_rays(live)
    hit = ids >= 0
    assert np.all(np.isposinf(t[~hit]))
    shapes = np.ascontiguousarray(ref.shapes(), F32)
    light = shapes[:, 13] != 0
    lit = hit & light[np.maximum(ids, 0)]
    fn = oracle.lib().oracle_shape_trace
    normal = np.zeros((len(live), 3), F32)
    ts, nn = np.zeros(1, F32), np.zeros(3, F32)
    for i in np.nonzero(hit)[0]:
        j = int(ids[i])
        assert fn(int(shapes[j, 12]), shapes.ctypes.data + 64 * j, live.ctypes.data + 24 * int(i), ts.ctypes.data,
                  nn.ctypes.data), (i, j)
        normal[i] = nn
    albedo = np.zeros((len(live), 3), F32)
    if lit.any():
        # one Scene::trace per path: the emitter's intensity
        albedo[lit] = ref.radiance_rays(live[lit], None, 0, 1, 0, 1, SEED, 0, ra.THREADS)[0]
    albedo[hit & ~lit] = mats[ids[hit & ~lit], :3]
    kind = np.where(lit, fh.KIND_EMISSIVE, np.where(hit, fh.KIND_DIFFUSE, fh.KIND_MISS)).astype(np.uint8)
    for k, v in (("t", t), ("id", ids), ("visits", visits), ("normal", normal), ("albedo", albedo), ("kind", kind)):
        out[k][ok] = v
    return out


def mesh_planes(wpt, oracle, name):
    """(mesh, oracle scene, rays, expected planes) of a scene-2 fixture's sets."""
    def make():
        mesh, ref, rays = ra.mesh_case(wpt, oracle, name)
        want = expected_planes(oracle, ref, wpt.interface.DebugScene(2, mesh).materials(), rays)
        return mesh, ref, rays, {k: _frozen(v) for k, v in want.items()}
    return once(("mesh_planes", name), make)


# rays that leave every scene: from far above, upwards (a closed room has no miss from inside)
AWAY_RAYS = np.array([[0, 1000, 0, 0, 1, 0], [3, 2000, -4, 0.6, 0.8, 0], [-7, 1500, 2, 0, 0.8, -0.6],
                      [1, 1e6, 1, 0, 1, 0]], F32)


def shape_planes(wpt, oracle, scene_id):
    """(rays_fixtures scene, {set: (rays, expected planes)}) of scenes 0, 100,
    101: rays_adversarial's shape sets, and a set `around` of the scene's probes,
    the primary rays of a 64 x 62 frame, AWAY_RAYS and a ray at each emitter, so that the scene's sets
    together hold misses, diffuse hits and emitters."""
    def make():
        sc, sets = ra.shape_case(wpt, oracle, scene_id)
        sets = dict(sets)
        # towards the emitters: from the camera at the first point of each emissive shape's record
        shapes = sc.ref.shapes()
        at = shapes[shapes[:, 13] != 0, :3].astype(np.float64)
        d = at - np.asarray(sc.cam[:3], np.float64)
        d /= np.sqrt((d * d).sum(1, keepdims=True))
        lit = np.concatenate([np.tile(np.asarray(sc.cam[:3], F32), (len(d), 1)), d.astype(F32)], axis=1)
        sets["around"] = _frozen(np.concatenate([sc.probe_rays(), AWAY_RAYS, lit, sc.rays((64, 62), 1)]).astype(F32))
        mats = wpt.interface.DebugScene(scene_id, None).materials()
        return sc, {k: (r, expected_planes(oracle, sc.ref, mats, r)) for k, r in sets.items()}
    return once(("shape_planes", scene_id), make)


def scaled_planes(wpt, oracle, name):
    """(mesh, oracle scene, {scale: (rays, expected planes)}) of a mesh's scaled directions."""
    def make():
        mesh, ref, _, scaled = ra.scaled_case(wpt, oracle, name)
        mats = wpt.interface.DebugScene(2, mesh).materials()
        return mesh, ref, {s: (r, expected_planes(oracle, ref, mats, r)) for s, r in scaled.items()}
    return once(("scaled_planes", name), make)


def box_rays(wpt, oracle):
    """(rays_fixtures scene, 1025 rays, expected planes): AWAY_RAYS, then the
    box set and the primary rays of a 64 x 62 frame, shuffled: hits of every
    kind among the first 64."""
    def make():
        sc, pool = ra._box_pool(wpt, oracle)
        rng = np.random.default_rng(0x726179)
        rays = _frozen(np.ascontiguousarray(np.concatenate([AWAY_RAYS, pool[rng.permutation(len(pool))[:1021]]])))
        mats = wpt.interface.DebugScene(100, None).materials()
        return sc, rays, expected_planes(oracle, sc.ref, mats, rays)
    return once("box_rays", make)


INVALID_RAYS = np.array([[np.nan, 0, 0, 0, 0, 1], [0, 1, 0, np.inf, 0, 0], [0, 1, 0, 0, -0.0, 0],
                         [0, -np.inf, 0, 0, 1, 0]], F32)


def with_invalid(rays, where):
    """A copy of `rays` whose entries `where` are invalid rays, in turn a NaN
    origin, an infinite direction, a direction of three zeros, an infinite origin."""
    out = np.array(rays, copy=True)
    where = np.asarray(where)
    out[where] = INVALID_RAYS[np.arange(len(where)) % len(INVALID_RAYS)]
    return out


def masked(planes, where):
    """`planes` with the invalid entries at `where`."""
    out = {k: np.array(v, copy=True) for k, v in planes.items()}
    inv = invalid_planes(1)
    for k in out:
        out[k][where] = inv[k][0]
    return out


# ---- the fisheye frame and the filter ----------------------------------------
def clamp_error(a, ref, mask):
    """Relative L2 of clamp(., 0, 1) over the pixels of `mask`."""
    a = np.clip(np.asarray(a, np.float64), 0.0, 1.0)[mask]
    ref = np.clip(np.asarray(ref, np.float64), 0.0, 1.0)[mask]
    return float(np.linalg.norm(a - ref) / np.linalg.norm(ref))


def fisheye_reference(wpt, oracle, origin):
    """The oracle's 1,024-spp mean of the fisheye frame at `origin`: (H * W, 3) f32."""
    def make():
        sc = rf.scene(wpt, oracle, "box")
        rgb, _, _ = sc.ref.radiance_rays(fisheye(origin), None, FISH_REF[0], FISH_REF[1], 1, FISH_DEPTH, SEED, 0, 8)
        return _frozen((rgb / F32(FISH_REF[1])).astype(F32))
    return once(("fisheye_ref", tuple(origin)), make)


def fisheye_oracle_frame(wpt, oracle, origin):
    """The oracle's 4-spp frame at `origin` and its planes: (raw (n, 3), status, planes)."""
    def make():
        sc = rf.scene(wpt, oracle, "box")
        rays = fisheye(origin)
        raw, status, _ = sc.ref.radiance_rays(rays, None, 0, FISH_SPP, 1, FISH_DEPTH, SEED, 0, ra.THREADS)
        planes = expected_planes(oracle, sc.ref, wpt.interface.DebugScene(FISH_SCENE, None).materials(), rays)
        return _frozen(raw), _frozen(status), planes
    return once(("fisheye_frame", tuple(origin)), make)


def host_filter(wpt, w, h, raw, status, spp, planes, iterations, sigma_c, sigma_z, flags):
    """wpt_denoise_host on a query's outputs: acc = raw, cnt = spp * status."""
    cnt = (np.asarray(status, np.uint32) * np.uint32(spp)).reshape(h, w)
    return wpt.interface.denoise_host(np.asarray(raw, F32).reshape(h, w, 3), cnt, planes["t"].reshape(h, w),
                                      planes["normal"].reshape(h, w, 3), planes["albedo"].reshape(h, w, 3),
                                      planes["kind"].reshape(h, w), iterations, sigma_c, sigma_z, flags)


def fisheye_row(wpt, oracle, origin):
    """(raw error, filtered error, valid == status) of the oracle's frame through wpt_denoise_host."""
    raw, status, planes = fisheye_oracle_frame(wpt, oracle, origin)
    ref = fisheye_reference(wpt, oracle, origin)
    rgb, valid, _ = host_filter(wpt, FISH_W, FISH_H, raw, status, FISH_SPP, planes, 3, dn.SIGMA_C, dn.SIGMA_Z, 0)
    m = status.astype(bool)
    return (clamp_error(raw / F32(FISH_SPP), ref, m), clamp_error(rgb.reshape(-1, 3), ref, m),
            bool(np.array_equal(valid.reshape(-1), status)))
