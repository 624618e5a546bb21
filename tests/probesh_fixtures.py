"""Cases of the SH projection of a point's gathers (wpt_probe_sh, wpt_sh_basis).

A plain helper module (no pytest hooks): tests/test_probesh_cpu.py holds
wpt_sh_basis against the numpy-f32 restatement below and checks on the oracle
alone that the point sets give the GPU test power; tests/test_gpu_probesh.py
compares the device's answers with `expected`, bit for bit. Everything is
computed once per process and shared; nothing returned here is modified.

The restatement of sh_basis (csrc/wpt_sh.h) is written from the
definition: each operation through numpy.float32, the constants from math.pi in
f64 rounded once to f32.

The expected value of a record's coefficient k is the sequential f32 sum over
its traced samples of Y_k(w_j) * c_j: c_j is OracleScene.radiance_rays (spp = 1)
along wpt_point_rays' ray (o_j, w_j), the loop of points_fixtures.expected.
"""
import math

import numpy as np

import points_fixtures as px
import rayframe_fixtures as rfr

F32 = np.float32
SEED = px.SEED
DEPTH = px.DEPTH
MAX_ORDER = 2

# the f32 nearest to the f64 values
C0 = F32(math.sqrt(1.0 / (4.0 * math.pi)))
C1 = F32(math.sqrt(3.0 / (4.0 * math.pi)))
C2 = F32(math.sqrt(15.0 / (4.0 * math.pi)))
C3 = F32(math.sqrt(5.0 / (16.0 * math.pi)))
C4 = F32(math.sqrt(15.0 / (16.0 * math.pi)))
CONSTANTS = (C0, C1, C2, C3, C4)


def ncoef(order):
    return (order + 1) ** 2


def basis(dirs, order=MAX_ORDER):
    """sh_basis restated: (n, (order + 1)^2) f32 of directions (n, 3), used as
    given. Every product, sum and difference is one numpy.float32 operation."""
    d = np.asarray(dirs, F32).reshape(-1, 3)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    one, three = F32(1.0), F32(3.0)
    with np.errstate(all="ignore"):
        Y = [np.full(len(d), C0, F32), C1 * y, C1 * z, C1 * x,
             C2 * (x * y), C2 * (y * z), C3 * ((three * (z * z)) - one), C2 * (x * z), C4 * ((x * x) - (y * y))]
    for v in Y:
        assert v.dtype == F32
    return np.ascontiguousarray(np.stack(Y[:ncoef(order)], axis=1))


def basis_f64(dirs):
    """The closed form in f64 with f64 constants: (n, 9)."""
    d = np.asarray(dirs, np.float64).reshape(-1, 3)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    pi = math.pi
    c0, c1, c2 = math.sqrt(1 / (4 * pi)), math.sqrt(3 / (4 * pi)), math.sqrt(15 / (4 * pi))
    c3, c4 = math.sqrt(5 / (16 * pi)), math.sqrt(15 / (16 * pi))
    return np.stack([np.full(len(d), c0), c1 * y, c1 * z, c1 * x, c2 * x * y, c2 * y * z, c3 * (3 * z * z - 1), c2 * x * z,
                     c4 * (x * x - y * y)], axis=1)


# ---- the decision directions ---------------------------------------------------
def _up(v):
    return np.nextafter(F32(v), F32(np.inf))


def _down(v):
    return np.nextafter(F32(v), F32(-np.inf))


def decision_dirs():
    """{family: (n, 3) f32}."""
    def make():
        out = {}
        axes = []
        for a in range(3):
            for s in (1.0, -1.0):
                v = [0.0, 0.0, 0.0]
                v[a] = s
                axes.append(v)
        out["axes"] = np.array(axes, F32)
        r = F32(1.0 / math.sqrt(3.0))
        out["diagonals"] = np.array([[sx * r, sy * r, sz * r] for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)], F32)
        out["negative zeros"] = np.array([[-0.0, 1, 0], [1, -0.0, 0], [0, 1, -0.0], [-0.0, -0.0, 1], [-0.0, -0.0, -1],
                                          [-1, -0.0, -0.0], [-0.0, -1, -0.0], [-0.0, -0.0, -0.0]], F32)
        t, m = F32(2.0 ** -149), F32(2.0 ** -127)  # the smallest denormal, and one below the normals
        out["denormals"] = np.array([[t, 1, 0], [1, t, 0], [0, 1, t], [-t, -t, 1], [m, m, 1], [m, -1, m], [t, t, t],
                                     [m, m, m], [1, m, -t], [F32(2.0 ** -75), F32(2.0 ** -75), 1]], F32)
        # z * z on each side of 1 / 3: 3 * (z * z) - 1 changes sign between the neighbours
        z0 = F32(math.sqrt(1.0 / 3.0))
        zs = [_down(_down(z0)), _down(z0), z0, _up(z0), _up(_up(z0))]
        third = []
        for z in zs:
            for s in (1.0, -1.0):
                q = math.sqrt(max(0.0, 1.0 - float(z) ** 2))
                third.append([q * 0.6, q * 0.8, s * float(z)])
        out["z*z about 1/3"] = np.array(third, F32)
        # |x| = |y|: x * x - y * y is exactly 0
        eq = []
        for a in (0.25, 0.5, float(F32(0.7071067)), float(F32(0.1)), 2.0 ** -70):
            for sx in (1, -1):
                for sy in (1, -1):
                    eq.append([sx * a, sy * a, math.sqrt(max(0.0, 1.0 - 2 * a * a))])
        out["|x| = |y|"] = np.array(eq, F32)
        return {k: rfr_frozen(v) for k, v in out.items()}
    return rfr.once(("probesh decision dirs",), make)


def rfr_frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def table_dirs(wpt):
    """The unit directions wpt_point_rays makes for the unit-normal records of
    points_fixtures' decision table, both distributions, every table sample."""
    def make():
        kind = px.table_records()[2]
        parts = []
        for sample in px.SAMPLES:
            recs, keys = px.table_case(sample)
            unit = np.repeat(np.array([k == "unit" for k in kind]), len(px.table_keys(sample)))
            for dist in (px.COSINE, px.SPHERE):
                parts.append(wpt.interface.point_rays(recs[unit], keys[unit], SEED, sample, dist)[:, 3:])
        return rfr_frozen(np.concatenate(parts))
    return rfr.once(("probesh table dirs",), make)


def seeded_unit_dirs(n=4096, seed=0x5348):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, 3))
    return np.ascontiguousarray((v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32))


# ---- the expected value --------------------------------------------------------
def samples(wpt, ref, recs, keys, sample, spp, rtype, dist, depth=DEPTH, light_debug=0, threads=4):
    """points_fixtures.expected's loop, kept per sample: (c (spp, n, 3) f32, w (spp,
    n, 3) f32, traced (spp, n) bool, status (n,) u8, {'paths', 'rays',
    'shadow_rays'})."""
    recs = np.ascontiguousarray(recs, F32).reshape(-1, 6)
    n = len(recs)
    k = np.arange(n, dtype=np.uint32) if keys is None else np.asarray(keys, np.uint32)
    c = np.zeros((spp, n, 3), F32)
    w = np.zeros((spp, n, 3), F32)
    traced = np.zeros((spp, n), bool)
    counts = {"paths": 0, "rays": 0, "shadow_rays": 0}
    for j in range(spp):
        rays = wpt.interface.point_rays(recs, k, SEED, sample + j, dist)
        cj, st, stats = ref.radiance_rays(rays, k, sample + j, 1, rtype, depth, SEED, light_debug, threads)
        c[j], w[j], traced[j] = cj, rays[:, 3:], st.astype(bool)
        counts["paths"] += int(st.sum())
        counts["rays"] += stats["rays"] - stats["shadow_rays"]  # the oracle's "rays" holds both kinds
        counts["shadow_rays"] += stats["shadow_rays"]
    return c, w, traced, px.valid(recs), counts


def project(c, w, traced, order=MAX_ORDER):
    """The definition's sum: (n, nc, 3) f32 = ((+0 + Y_k(w_0) * c_0) + Y_k(w_1) *
    c_1) + ..., a product and an addition of numpy.float32 per traced sample; an
    untraced sample is skipped (its direction is never used)."""
    spp, n, _ = c.shape
    nc = ncoef(order)
    sh = np.zeros((n, nc, 3), F32)
    with np.errstate(all="ignore"):
        for j in range(spp):
            t = traced[j]
            if not t.any():
                continue
            Y = basis(np.where(t[:, None], w[j], F32(0.0)), order)  # (n, nc)
            term = (Y[:, :, None] * c[j][:, None, :]).astype(F32)
            sh[t] = (sh[t] + term[t]).astype(F32)
    return sh


def expected(wpt, ref, recs, keys, sample, spp, rtype, dist, order=MAX_ORDER, depth=DEPTH, light_debug=0, threads=4):
    """(sh (n, nc, 3) f32, status (n,) u8, counts, traced (spp, n) bool)."""
    c, w, traced, status, counts = samples(wpt, ref, recs, keys, sample, spp, rtype, dist, depth, light_debug, threads)
    return project(c, w, traced, order), status, counts, traced


def set_samples(wpt, oracle, name, rtype, dist, sample=0, spp=px.SET_SPP, depth=DEPTH, light_debug=0):
    """`samples` of points_fixtures.point_set(name), once per process."""
    def make():
        sc, recs = px.point_set(wpt, oracle, name)
        out = samples(wpt, sc.ref, recs, None, sample, spp, rtype, dist, depth, light_debug)
        return tuple(rfr_frozen(a) if isinstance(a, np.ndarray) else a for a in out)
    return rfr.once(("probesh set_samples", name, rtype, dist, sample, spp, depth, light_debug), make)


def set_expected(wpt, oracle, name, rtype, dist, sample=0, spp=px.SET_SPP, depth=DEPTH, light_debug=0, order=MAX_ORDER):
    c, w, traced, status, counts = set_samples(wpt, oracle, name, rtype, dist, sample, spp, depth, light_debug)
    return project(c, w, traced, order), status, counts, traced


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)
