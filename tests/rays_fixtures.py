"""Cases of the ray query (wpt_radiance_rays).

A plain helper module (no pytest hooks): tests/test_rays_cpu.py checks on the
oracle alone that the cases produce the conditions they are built for;
tests/test_gpu_rays.py compares the device's answers with the oracle, bit for
bit. Everything is computed once per process and shared; nothing returned here
is modified.

Two sources of rays with an exact expected value:
 - frames: the rays wpt_primary_rays makes for a W x H frame of a scene's camera
   at sample s, keys = the pixel indices; the oracle's answer is sample s of
   every pixel of that frame.
 - probes: 40 seeded cameras per scene on a 1 x 1 viewport; ray j is
   wpt_primary_rays(1, 1, cam_j, SEED, PROBE_SAMPLE)[0] with key 0, the oracle's
   answer render(1, 1, cam_j, ..., s0=PROBE_SAMPLE, spp=1): arbitrary origins
   and directions.
"""
import numpy as np

import first_hit_fixtures as fh
import pnee_fixtures as pf

F32 = np.float32
SEED = fh.SEED
DEPTH = 4
PROBES = 40
PROBE_SAMPLE = 3
PROBE_SEED = 1  # chosen so that every scene has zero and non-zero answers (tests/test_rays_cpu.py asserts it)
# name -> (scene id, has the cloud mesh, half extent the probe cameras' positions are drawn from around the scene's camera)
SCENES = {"box": (100, False, 1.0), "cloud": (2, True, 2.0), "museum": (0, False, 8.0), "spheres": (101, False, 1.0)}
PNEE_SCENES = ("box", "cloud")  # two lights: pnee_fixtures.octants() installs


class Scene:
    def __init__(self, wpt, oracle, name):
        self.name = name
        self.scene_id, mesh, self.extent = SCENES[name]
        self.mesh = wpt.scenes.triangle_cloud(3000, seed=0x5EED) if mesh else None
        self.cam = tuple(wpt.scenes.scene_camera(self.scene_id))
        self.ref = oracle.OracleScene(self.scene_id, self.mesh)
        if name in PNEE_SCENES:
            assert self.ref.num_lights == 2
            self.ref.set_photons(pf.octants())
        self._wpt = wpt
        self._rays, self._frames, self._probes = {}, {}, {}

    def rays(self, vp, sample):
        """wpt_primary_rays of the scene's camera: (w * h, 6) f32."""
        k = (vp, sample)
        if k not in self._rays:
            r = self._wpt.interface.primary_rays(vp[0], vp[1], self.cam, SEED, sample)
            r.setflags(write=False)
            self._rays[k] = r
        return self._rays[k]

    def frame(self, vp, rtype, sample, depth=DEPTH):
        """The oracle's sample `sample` of every pixel: ((w * h, 3) f32, rays + shadow rays)."""
        k = (vp, rtype, sample, depth)
        if k not in self._frames:
            acc, st = self.ref.render(vp[0], vp[1], self.cam, rtype, rtype, depth, SEED, s0=sample, spp=1, threads=4)
            acc = acc.reshape(-1, 3)
            acc.setflags(write=False)
            self._frames[k] = (acc, st["rays"])
        return self._frames[k]

    def probe_cams(self):
        """PROBES cameras: the position within the scene's extent of its own
        camera, rot_x in [-1.2, 1.2], rot_y any."""
        rng = np.random.default_rng([PROBE_SEED, self.scene_id])
        pos = np.asarray(self.cam[:3]) + rng.uniform(-self.extent, self.extent, (PROBES, 3))
        rx = rng.uniform(-1.2, 1.2, PROBES)
        ry = rng.uniform(-np.pi, np.pi, PROBES)
        return np.column_stack([pos, rx, ry]).astype(F32)

    def probe_rays(self):
        """(PROBES, 6) f32: ray j of camera j's 1 x 1 frame."""
        if "rays" not in self._probes:
            r = np.concatenate([self._wpt.interface.primary_rays(1, 1, c, SEED, PROBE_SAMPLE) for c in self.probe_cams()])
            r.setflags(write=False)
            self._probes["rays"] = r
        return self._probes["rays"]

    def probe_expect(self, rtype, depth=DEPTH):
        """The oracle's answers to the probes: ((PROBES, 3) f32, rays + shadow rays)."""
        k = (rtype, depth)
        if k not in self._probes:
            out = np.zeros((PROBES, 3), F32)
            rays = 0
            for j, c in enumerate(self.probe_cams()):
                acc, st = self.ref.render(1, 1, c, rtype, rtype, depth, SEED, s0=PROBE_SAMPLE, spp=1)
                out[j] = acc.reshape(3)
                rays += st["rays"]
            out.setflags(write=False)
            self._probes[k] = (out, rays)
        return self._probes[k]


_SCENES = {}


def scene(wpt, oracle, name):
    if name not in _SCENES:
        _SCENES[name] = Scene(wpt, oracle, name)
    return _SCENES[name]


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def valid(rays):
    """The status rule in numpy: six finite components, a direction that is not
    three zeros (of either sign)."""
    r = np.asarray(rays, F32).reshape(-1, 6)
    return (np.isfinite(r).all(axis=1) & ((bits(r[:, 3:]) & 0x7FFFFFFF) != 0).any(axis=1)).astype(np.uint8)


def seq_sum(parts):
    """((+0 + a) + b) + ... in f32, elementwise."""
    s = np.zeros_like(parts[0], dtype=F32)
    for p in parts:
        s = (s + p).astype(F32)
    return s


# Rays for the validity rule: (ray, expected status)
_NAN, _INF = F32(np.nan), F32(np.inf)
_DEN = np.uint32(1).view(F32)  # the smallest denormal
VALIDITY = (
    ((0, 0, 0, 0, 0, 1), 1),
    ((_NAN, 0, 0, 0, 0, 1), 0), ((0, _NAN, 0, 0, 0, 1), 0), ((0, 0, _NAN, 0, 0, 1), 0),
    ((0, 0, 0, _NAN, 0, 1), 0), ((0, 0, 0, 0, _NAN, 1), 0), ((0, 0, 0, 0, 0, _NAN), 0),
    ((_INF, 0, 0, 0, 0, 1), 0), ((0, -_INF, 0, 0, 0, 1), 0), ((0, 0, 0, _INF, 0, 0), 0), ((0, 0, 0, 1, 0, -_INF), 0),
    ((1, 2, 3, 0, 0, 0), 0), ((1, 2, 3, -0.0, -0.0, -0.0), 0), ((1, 2, 3, 0, -0.0, 0), 0),
    ((1, 2, 3, -0.0, 1, 0), 1), ((1, 2, 3, -0.0, -0.0, -1), 1),
    ((1, 2, 3, _DEN, 0, 0), 1), ((1, 2, 3, 0, -_DEN, 0), 1), ((_DEN, -_DEN, 0, 0, 0, _DEN), 1),
    ((-0.0, -0.0, -0.0, 0, 1, 0), 1), ((3e38, -3e38, 0, 3e38, 0, 0), 1),
)
