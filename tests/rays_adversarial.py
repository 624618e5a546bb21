"""Adversarial cases of the ray query (wpt_radiance_rays) with an exact
expected value: the oracle's own ray query (OracleScene.radiance_rays).

A plain helper module (no pytest hooks): tests/test_rays_oracle_cpu.py ties the
oracle's entry to the established one (render) and asserts on the oracle alone
that the families produce the conditions they are built for;
tests/test_gpu_rays_adversarial.py compares the device with the same
expectations, bit for bit. Everything is deterministic, computed once per
process and shared; nothing returned here is modified.

Families:
 - sets: per scene-2 mesh of adversarial.scene2_meshes the concatenation of
   its ray sets (vertices, edges, ties, surface origins, BVH bounds with +-0
   components, denormal and unnormalised directions, origins 1e6 away), and for
   scenes 0, 100, 101 the torus / aarect / sphere sets.
 - scaled: interior rays of meshes A, D, E, the unit direction times SCALES.
 - spp: 100 box rays at SPPS, sample SPP_SAMPLE.
 - keys: 300 box rays under edge and random 32-bit keys with repeats, and one
   ray with a non-zero answer under 300 different keys.
 - chunk: 4,099 box rays tiled past the query's chunk of 2^21 rays.
"""
import numpy as np

import adversarial as adv
import rays_fixtures as rf
from test_adversarial_cpu import fixtures

F32 = rf.F32
SEED = rf.SEED
DEPTH = rf.DEPTH
THREADS = 4
MESHES = ("A", "B", "Bwall", "Bulp", "C", "D", "E", "F", "G", "BA")
MAX_SET_RAYS = 7500
F_AROUND = 900
F_AROUND_BOX = np.array([-4.0, -0.9, 1.0, 4.0, 5.0, 9.0], F32)   # around adversarial.F_WORLD_BOX, above the floor
SHAPE_SCENES = {0: "museum", 100: "box", 101: "spheres"}   # scene id -> rays_fixtures name
MUSEUM_SPP = 16

SCALED_MESHES = ("A", "D", "E")
SCALES = (2.0 ** -20, 2.0 ** 20, 1e-30, 1e-37, 1e-42, 1e30, 3e38)
EXACT_SCALES = (2.0 ** -20, 2.0 ** 20)   # powers of two well inside the range: every product and quotient scales exactly

SPPS = (2, 3, 5, 7, 64, 255, 256, 257, 300)
SPP_SAMPLE = 5
STRADDLE_SPPS = (3, 7, 257)
STRADDLE_BATCHES = (64, 100, 257)
BLOCK = 256                     # kBlock: positions per block of the generators

EDGE_KEYS = (0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF)
KEY_SAMPLES = ((0, 2), (0xFFFFFFFE, 1), (0xFFFFFFFE, 2))   # (sample, spp)

CHUNK = 1 << 21                 # kQueryChunk (wpt_render.hip)
CHUNK_BASE = 4099               # prime: a tiling never lines up with blocks of 256
CHUNK_N = CHUNK + 257
CHUNK_TAIL = (CHUNK - 64, CHUNK_N)
CHUNK_DEPTH = 1                 # one launch round


def _frozen(a):
    a.setflags(write=False)
    return a


_CACHE = {}


def once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def expect(ref, tag, rays, keys=None, sample=0, spp=1, rtype=1, depth=DEPTH, light_debug=0):
    """The oracle's answer (rgb, status, stats), computed once per `tag` (which
    names the scene and the rays) and call."""
    def make():
        rgb, status, st = ref.radiance_rays(rays, keys, sample, spp, rtype, depth, SEED, light_debug, THREADS)
        return _frozen(rgb), _frozen(status), st
    return once(("expect", tag, None if keys is None else keys.tobytes(), sample, spp, rtype, depth, light_debug), make)


# ---- sets -------------------------------------------------------------------
def mesh_case(wpt, oracle, name):
    """(mesh, oracle scene, rays (n, 6)) of one scene-2 fixture: its sets
    concatenated. Mesh F is the exception twice. Its sets hold 7,630 rays, and
    the mesh fills its box, so 93 % of them hit a triangle first and next to
    nothing reaches the resolved end of the presolving producer's stream. So F
    gets F_AROUND more rays (random origins in F_AROUND_BOX, a box around the
    mesh's, random directions: about half of them pass the mesh by), and its
    `inside` set is cut to what then fits MAX_SET_RAYS."""
    def make():
        mesh, ref, _, sets, _ = fixtures(wpt, oracle)[name]
        parts = [r for k, r in sets.items() if k != "inside"]
        if "inside" in sets:
            parts.append(adv.inside_rays(F_AROUND_BOX, seed=13, limit=F_AROUND))
            room = MAX_SET_RAYS - sum(len(r) for r in parts)
            parts.append(sets["inside"][:room])
        rays = np.ascontiguousarray(np.concatenate(parts), F32)
        assert 0 < len(rays) <= MAX_SET_RAYS
        return mesh, ref, _frozen(rays)
    return once(("mesh", name), make)


def shape_case(wpt, oracle, scene_id):
    """(rays_fixtures scene, {set name: rays}) for scenes 0, 100, 101."""
    def make():
        sc = rf.scene(wpt, oracle, SHAPE_SCENES[scene_id])
        return sc, {k: _frozen(np.ascontiguousarray(r, F32)) for k, (r, _) in adv.shape_sets(scene_id, sc.ref.shapes()).items()}
    return once(("shapes", scene_id), make)


def box_set(wpt, oracle):
    """The box's aarect set and its 40 probes: (rays_fixtures scene, rays)."""
    def make():
        sc, sets = shape_case(wpt, oracle, 100)
        return sc, _frozen(np.concatenate([sets["aarect"], sc.probe_rays()]))
    return once("box_set", make)


def pnee_mesh_case(wpt, oracle, name="A"):
    """A scene-2 fixture with pnee_fixtures.octants() installed in an oracle
    scene of its own (the shared one of test_adversarial_cpu.fixtures keeps its
    shot tree): (mesh, oracle scene, rays)."""
    import pnee_fixtures as pf

    def make():
        mesh, _, rays = mesh_case(wpt, oracle, name)
        ref = oracle.OracleScene(2, mesh)
        assert ref.num_lights == 2   # the two lights octants() names
        ref.set_photons(pf.octants())
        return mesh, ref, rays
    return once(("pnee_mesh", name), make)


# ---- scaled -----------------------------------------------------------------
def scaled_case(wpt, oracle, name):
    """(mesh, oracle scene, unit-direction rays, {scale: rays}) from the
    interior rays of a mesh: the direction normalised in f64, rounded to f32,
    times f32(scale) in f32."""
    def make():
        mesh, ref, _, sets, _ = fixtures(wpt, oracle)[name]
        base = sets["interior"]
        d = adv._unit(base[:, 3:]).astype(F32)
        unit = _frozen(np.concatenate([base[:, :3], d], axis=1).astype(F32))
        out = {}
        with np.errstate(under="ignore"):
            for s in SCALES:
                out[s] = _frozen(np.concatenate([base[:, :3], (d * F32(s)).astype(F32)], axis=1).astype(F32))
        return mesh, ref, unit, out
    return once(("scaled", name), make)


# ---- spp, keys, chunk: box rays ----------------------------------------------
def _box_pool(wpt, oracle):
    """The box set followed by the primary rays of a 64 x 62 frame: 4,148 rays."""
    def make():
        sc, rays = box_set(wpt, oracle)
        return sc, _frozen(np.concatenate([rays, sc.rays((64, 62), 1)]))
    return once("box_pool", make)


def spp_case(wpt, oracle):
    """(scene, 100 rays): every other ray of the aarect set (60) and the probes (40)."""
    def make():
        sc, sets = shape_case(wpt, oracle, 100)
        return sc, _frozen(np.concatenate([sets["aarect"][::2][:60], sc.probe_rays()]))
    return once("spp", make)


def block_starts(total, batch):
    """The chunk positions at which a generator block starts when `total`
    positions run in batches of `batch` on one lane."""
    return np.array([k0 + j for k0 in range(0, total, batch) for j in range(0, min(batch, total - k0), BLOCK)])


def keys_case(wpt, oracle):
    """(scene, rays (300, 6), keys (300,) u32): the five edge keys, 200 random
    32-bit keys, and 95 repeats of keys already in the list, shuffled."""
    def make():
        sc, pool = _box_pool(wpt, oracle)
        rng = np.random.default_rng(0x6B657973)
        keys = np.concatenate([np.array(EDGE_KEYS, np.uint32), rng.integers(0, 1 << 32, 200, dtype=np.uint64).astype(np.uint32)])
        keys = np.concatenate([keys, keys[rng.integers(0, len(keys), 95)]])
        rays = pool[np.sort(rng.choice(len(pool), 300, replace=False))]
        return sc, _frozen(np.ascontiguousarray(rays)), _frozen(keys[rng.permutation(300)])
    return once("keys", make)


def one_ray_case(wpt, oracle):
    """(scene, one ray 300 times, 300 distinct keys): the first ray of the box
    set whose NEE answer at key 0 is not zero."""
    def make():
        sc, rays = box_set(wpt, oracle)
        rgb = expect(sc.ref, "box_set", rays, np.zeros(len(rays), np.uint32))[0]
        j = int(np.argmax((rgb != 0).any(axis=1)))
        assert (rgb[j] != 0).any()
        rng = np.random.default_rng(0x6F6E65)
        keys = np.concatenate([np.array(EDGE_KEYS, np.uint32), np.arange(2, 100, dtype=np.uint32)])
        more = rng.integers(100, 1 << 32, 400, dtype=np.uint64).astype(np.uint32)
        keys = np.concatenate([keys, np.unique(more)[:300 - len(keys)]])
        assert len(np.unique(keys)) == 300
        return sc, _frozen(np.tile(rays[j], (300, 1))), _frozen(keys[rng.permutation(300)])
    return once("one_ray", make)


def chunk_case(wpt, oracle):
    """(scene, base rays (4099, 6), index (CHUNK_N,) u32 = position % 4099):
    the tiled list is base[index], its explicit keys are index."""
    def make():
        sc, pool = _box_pool(wpt, oracle)
        base = _frozen(np.ascontiguousarray(pool[:CHUNK_BASE]))
        assert len(base) == CHUNK_BASE
        return sc, base, _frozen((np.arange(CHUNK_N, dtype=np.uint64) % CHUNK_BASE).astype(np.uint32))
    return once("chunk", make)
