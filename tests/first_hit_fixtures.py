"""Cases of the first-hit feature planes (wpt_first_hit, wpt_primary_rays).

A plain helper module (no pytest hooks): tests/test_first_hit_cpu.py checks on
the host that wpt_primary_rays makes the oracle's own primary rays and that
each case produces the conditions it is built for; tests/test_gpu_first_hit.py
compares the device planes with the oracle on the same cases. Everything is
computed once per process and shared; nothing returned here is modified.
"""
import numpy as np

import adversarial as adv

F32 = np.float32
W, H = 64, 48
SEED = 0xBABABEBE
SAMPLES = (0, 7)
KIND_MISS, KIND_DIFFUSE, KIND_EMISSIVE = 0, 1, 2

# name -> (scene id, mesh (None: the scene has none), camera (None: the scene's own), viewports, GPU samples)
_DEFS = {
    "default": (2, "cloud", None, ((W, H),), SAMPLES),
    "up": (2, "cloud", (-0.9, 5.4, 0.4, -1.2, 0.0), ((W, H),), SAMPLES),
    "deep": (2, "F", (0.0, 0.875, 5.0, 0.3, 0.7), ((W, H),), SAMPLES[:1]),  # ~5,900 visits per ray: one sample
    "E": (2, "E", None, ((W, H),), SAMPLES),
    "C": (2, "C", (0.0, 3.0, 3.0, 0.9, 0.0), ((W, H),), SAMPLES),
    "museum": (0, None, None, ((W, H),), SAMPLES),
    "box": (100, None, None, ((W, H),), SAMPLES),
    "spheres": (101, None, None, ((W, H),), SAMPLES),
    "ragged": (2, "cloud", None, ((37, 5), (1, 1)), SAMPLES),
}
CASES = tuple(_DEFS)


def _mesh(wpt, name):
    if name is None:
        return None
    if name == "cloud":
        return wpt.scenes.triangle_cloud(3000, seed=0x5EED)
    return {"F": adv.mesh_f, "C": adv.mesh_c, "E": lambda: adv.mesh_e(wpt)}[name]()


class Case:
    """One case: its scene, camera, viewports, and per (viewport, sample) the
    host rays, the oracle's hits of them and the expected planes."""

    def __init__(self, wpt, oracle, name):
        self.name = name
        self.scene_id, mesh, cam, self.viewports, self.gpu_samples = _DEFS[name]
        self.mesh = _mesh(wpt, mesh)
        self.cam = tuple(cam if cam is not None else wpt.scenes.scene_camera(self.scene_id))
        self.ref = oracle.OracleScene(self.scene_id, self.mesh)
        self.dbg = wpt.interface.DebugScene(self.scene_id, self.mesh)
        self._wpt, self._oracle = wpt, oracle
        self._rays, self._hits, self._normals, self._rad = {}, {}, {}, {}

    def rays(self, vp, sample):
        """wpt_primary_rays of the case: (w * h, 6) f32."""
        k = (vp, sample)
        if k not in self._rays:
            r = self._wpt.interface.primary_rays(vp[0], vp[1], self.cam, SEED, sample)
            r.setflags(write=False)
            self._rays[k] = r
        return self._rays[k]

    def hits(self, vp, sample):
        """The oracle's (t, id, visits) of those rays."""
        k = (vp, sample)
        if k not in self._hits:
            self._hits[k] = self.ref.trace_rays(self.rays(vp, sample))
        return self._hits[k]

    def radiance(self, vp, sample):
        """The oracle's depth-1 NoNEE radiance per pixel (one Scene::trace per
        path: the emitter's intensity, or nothing): (w * h, 3) f32."""
        k = (vp, sample)
        if k not in self._rad:
            acc, _ = self.ref.render(vp[0], vp[1], self.cam, 0, 0, max_depth=1, seed=SEED, s0=sample, spp=1)
            self._rad[k] = acc.reshape(-1, 3)
        return self._rad[k]

    def emissive(self):
        """Per shape id: the oracle's emissive flag."""
        return self.ref.shapes()[:, 13] != 0

    def normals(self, vp, sample):
        """Hit.normal of the traced shape per pixel through the oracle's
        per-shape trace (oracle_shape_trace); +0 on misses."""
        k = (vp, sample)
        if k not in self._normals:
            fn = self._oracle.lib().oracle_shape_trace
            shapes = np.ascontiguousarray(self.ref.shapes(), F32)
            rays = self.rays(vp, sample)
            _, ids, _ = self.hits(vp, sample)
            out = np.zeros((len(rays), 3), F32)
            t = np.zeros(1, F32)
            n = np.zeros(3, F32)
            for i in np.nonzero(ids >= 0)[0]:
                j = int(ids[i])
                ok = fn(int(shapes[j, 12]), shapes.ctypes.data + 64 * j, rays.ctypes.data + 24 * int(i), t.ctypes.data,
                        n.ctypes.data)
                assert ok, (self.name, i, j)  # the shape Scene::trace reports is hit by its own trace
                out[i] = n
            self._normals[k] = out
        return self._normals[k]


_CASES = {}


def case(wpt, oracle, name):
    if name not in _CASES:
        _CASES[name] = Case(wpt, oracle, name)
    return _CASES[name]


def numpy_primary_rays(oracle, w, h, cam, seed, sample):
    """tracer.rs:178-191 in numpy f32 with gen_path's op order: the stream of
    (pixel, sample) from oracle_path_seed, its two jitter draws from
    oracle_rng_floats, normalize as v * (1 / sqrt((x^2 + y^2) + z^2)), rot_x,
    rot_y with oracle_cosf / oracle_sinf."""
    L = oracle.lib()
    n = w * h
    jit = np.empty((n, 2), F32)
    two = np.empty(2, F32)
    for p in range(n):
        L.oracle_rng_floats(L.oracle_path_seed(seed, p, sample), 2, two.ctypes.data)
        jit[p] = two
    x = (np.arange(n) % w).astype(F32)
    y = (np.arange(n) // w).astype(F32)
    fw, fh = F32(w), F32(h)
    w_inv, h_inv, ar = F32(1.0) / fw, F32(1.0) / fh, fw / fh
    fx = (((x + jit[:, 0]) * w_inv - F32(0.5)) * ar).astype(F32)
    fy = (F32(0.5) - (y + jit[:, 1]) * h_inv).astype(F32)
    fz = np.full(n, 0.8, F32)
    m = (F32(1.0) / np.sqrt((fx * fx + fy * fy) + fz * fz)).astype(F32)
    vx, vy, vz = m * fx, m * fy, m * fz
    cx, sx = F32(L.oracle_cosf(cam[3])), F32(L.oracle_sinf(cam[3]))
    cy, sy = F32(L.oracle_cosf(cam[4])), F32(L.oracle_sinf(cam[4]))
    vy, vz = cx * vy - sx * vz, sx * vy + cx * vz      # rot_x (vec3.rs:108-119)
    vx, vz = cy * vx + sy * vz, (-sy) * vx + cy * vz   # rot_y (vec3.rs:95-106)
    out = np.empty((n, 6), F32)
    out[:, :3] = np.asarray(cam[:3], F32)
    out[:, 3], out[:, 4], out[:, 5] = vx, vy, vz
    return out
