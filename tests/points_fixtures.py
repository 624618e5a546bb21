"""Cases of the point query (wpt_radiance_points, wpt_point_rays).

A plain helper module (no pytest hooks): tests/test_points_cpu.py holds
wpt_point_rays against the Python restatement below and checks on the oracle
alone that the point sets produce the conditions they are built for;
tests/test_gpu_points.py compares the device's answers with the oracle, bit for
bit. Everything is computed once per process and shared; nothing returned here
is modified.

The restatement of point_ray (csrc/wpt_points.h) is written from
the definition: xorshift32 and path_seed on Python integers, every f32 step
through numpy.float32, msin / mcos from wpt_math.h's published algorithm (musl's
sinf / cosf) with Python doubles for the kernels.

The expected value of a point's sum is the sequential f32 sum over its samples
of OracleScene.radiance_rays (spp = 1) along wpt_point_rays' rays.
"""
import numpy as np

import rayframe_fixtures as rfr
import rays_fixtures as rf

F32 = np.float32
SEED = rf.SEED
DEPTH = rf.DEPTH
COSINE, SPHERE = 0, 1
M32 = 0xFFFFFFFF
EPSILON = F32(0.0002)
PI = F32(3.14159274101257324)
SAMPLES = (0, 7, M32)  # the sample indices of the decision table


# ---- the streams -------------------------------------------------------------
def xs_next_u32(s):
    s ^= (s << 13) & M32
    s ^= s >> 17
    s ^= (s << 5) & M32
    return s


def fmix32(h):
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h


def _sample_word(sample):
    return (sample * 0x27D4EB2F + 0x165667B1) & M32


def path_seed(seed, key, sample):
    h = fmix32(seed ^ 0x9E3779B9)
    h = fmix32(h ^ key)
    h = fmix32(h ^ _sample_word(sample))
    return h if h else 0x6D2B79F5


def to_unit(u):
    """xs_next's float: (float)u * (1.0f / (float)0xFFFFFFFFu)."""
    return F32(F32(u) * (F32(1.0) / F32(M32)))


# The hash and the generator are bijections of 32-bit words: the key whose stream
# (under `seed`, at `sample`) starts with the draws (u1, u2) or (u1, *) is found
# by running them backwards, not by a search.
def _unshift_left(x, k):
    y = x
    for _ in range(32 // k + 1):
        y = x ^ ((y << k) & M32)
    return y


def _unshift_right(x, k):
    y = x
    for _ in range(32 // k + 1):
        y = x ^ (y >> k)
    return y


def xs_prev_u32(s):
    return _unshift_left(_unshift_right(_unshift_left(s, 5), 17), 13)


def fmix32_inv(h):
    h = _unshift_right(h, 16)
    h = (h * pow(0xC2B2AE35, -1, 1 << 32)) & M32
    h = _unshift_right(h, 13)
    h = (h * pow(0x85EBCA6B, -1, 1 << 32)) & M32
    return _unshift_right(h, 16)


def key_for(seed, sample, u1=None, u2=None):
    """The key k with xs draws (u1, u2) first on path_seed(seed, k, sample); give
    one of the two (the other follows from it)."""
    st = xs_prev_u32(u1) if u1 is not None else xs_prev_u32(xs_prev_u32(u2))
    assert st != 0 and st != 0x6D2B79F5
    key = fmix32_inv(fmix32_inv(st) ^ _sample_word(sample)) ^ fmix32(seed ^ 0x9E3779B9)
    assert path_seed(seed, key, sample) == st
    return key


# ---- msin / mcos ---------------------------------------------------------------
def _sindf(x):
    S1, S2, S3, S4 = -0x15555554cbac77 * 2.0**-55, 0x111110896efbb2 * 2.0**-59, -0x1a00f9e2cae774 * 2.0**-65, \
        0x16cd878c3b46a7 * 2.0**-71
    z = x * x
    w = z * z
    r = S3 + z * S4
    s = z * x
    return (x + s * (S1 + z * S2)) + s * w * r


def _cosdf(x):
    C0, C1, C2, C3 = -0x1ffffffd0c5e81 * 2.0**-54, 0x155553e1053a42 * 2.0**-57, -0x16c087e80f1e27 * 2.0**-62, \
        0x199342e0ee5069 * 2.0**-68
    z = x * x
    w = z * z
    r = C2 + z * C3
    return ((1.0 + z * C0) + w * C1) + (w * z) * r


def _rem_pio2f(x):
    toint = 1.5 / 2.220446049250313080847e-16
    pio4 = float.fromhex("0x1.921fb6p-1")
    invpio2, pio2_1, pio2_1t = 6.36619772367581382433e-01, 1.57079631090164184570e+00, 1.58932547735281966916e-08
    fn = x * invpio2 + toint - toint
    n = int(fn)
    y = x - fn * pio2_1 - fn * pio2_1t
    if y < -pio4:
        n -= 1
        fn -= 1
        y = x - fn * pio2_1 - fn * pio2_1t
    elif y > pio4:
        n += 1
        fn += 1
        y = x - fn * pio2_1 - fn * pio2_1t
    return n, y


_P1 = 1.57079632679489661923
_P2, _P3, _P4 = 2 * _P1, 3 * _P1, 4 * _P1
# the branches of msin / mcos by |x|'s bits; "rem" needs |x| > 9 pi / 4
BRANCHES = ("tiny", "pi/4", "3pi/4", "5pi/4", "7pi/4", "9pi/4", "rem")


def trig_branch(x):
    ix = int(F32(x).view(np.uint32)) & 0x7FFFFFFF
    for name, top in zip(BRANCHES, (0x397FFFFF, 0x3F490FDA, 0x4016CBE3, 0x407B53D1, 0x40AFEDDF, 0x40E231D5)):
        if ix <= top:
            return name
    return "rem"


def msin(x):
    x = F32(x)
    xd = float(x)
    sign = xd < 0 or (xd == 0 and np.signbit(x))
    b = trig_branch(x)
    if b == "tiny":
        return x
    if b == "pi/4":
        return F32(_sindf(xd))
    if b == "3pi/4":
        return F32(-F32(_cosdf(xd + _P1))) if sign else F32(_cosdf(xd - _P1))
    if b == "5pi/4":
        return F32(_sindf(-(xd + _P2) if sign else -(xd - _P2)))
    if b == "7pi/4":
        return F32(_cosdf(xd + _P3)) if sign else F32(-F32(_cosdf(xd - _P3)))
    if b == "9pi/4":
        return F32(_sindf(xd + _P4 if sign else xd - _P4))
    if not np.isfinite(x):
        return F32(np.nan)
    n, y = _rem_pio2f(xd)
    return (F32(_sindf(y)), F32(_cosdf(y)), F32(_sindf(-y)), F32(-F32(_cosdf(y))))[n & 3]


def mcos(x):
    x = F32(x)
    xd = float(x)
    sign = xd < 0 or (xd == 0 and np.signbit(x))
    b = trig_branch(x)
    if b == "tiny":
        return F32(1.0)
    if b == "pi/4":
        return F32(_cosdf(xd))
    if b == "3pi/4":
        return F32(_sindf(xd + _P1)) if sign else F32(_sindf(_P1 - xd))
    if b == "5pi/4":
        return F32(-F32(_cosdf(xd + _P2 if sign else xd - _P2)))
    if b == "7pi/4":
        return F32(_sindf(-xd - _P3)) if sign else F32(_sindf(xd - _P3))
    if b == "9pi/4":
        return F32(_cosdf(xd + _P4 if sign else xd - _P4))
    if not np.isfinite(x):
        return F32(np.nan)
    n, y = _rem_pio2f(xd)
    return (F32(_cosdf(y)), F32(_sindf(-y)), F32(-F32(_cosdf(y))), F32(_sindf(y)))[n & 3]


# ---- the vector operations of wpt_math.h, f32 step by step ----------------------
def _dot(a, b):
    return F32(F32(F32(a[0] * b[0]) + F32(a[1] * b[1])) + F32(a[2] * b[2]))


def _scale(a, m):
    return (F32(m * a[0]), F32(m * a[1]), F32(m * a[2]))


def _add(a, b):
    return (F32(a[0] + b[0]), F32(a[1] + b[1]), F32(a[2] + b[2]))


def _normalize(a):
    return _scale(a, F32(F32(1.0) / np.sqrt(_dot(a, a))))


def _cross(s, t):
    return (F32(F32(s[1] * t[2]) - F32(s[2] * t[1])), F32(F32(s[2] * t[0]) - F32(s[0] * t[2])),
            F32(F32(s[0] * t[1]) - F32(s[1] * t[0])))


def orthogonal_branch(s):
    if abs(F32(s[2])) > F32(0.1):
        return 0
    return 1 if abs(F32(s[0])) > F32(0.1) else 2


def _orthogonal(s):
    one = F32(1.0)
    b = orthogonal_branch(s)
    if b == 0:
        return _normalize((one, one, F32(F32(-F32(F32(s[0] * one) + F32(s[1] * one))) / s[2])))
    if b == 1:
        return _normalize((F32(F32(-F32(F32(s[1] * one) + F32(s[2] * one))) / s[0]), one, one))
    return _normalize((one, F32(F32(-F32(F32(s[0] * one) + F32(s[2] * one))) / s[1]), one))


def valid(recs):
    """ray_valid on (n, 6) records or rays."""
    return rf.valid(recs)


def point_ray(rec, key, seed, sample, dist):
    """The restatement: (six f32 of the generated ray, the stream's state), or
    None for a record the status rule rejects."""
    rec = np.asarray(rec, F32).reshape(6)
    if not valid(rec[None])[0]:
        return None
    with np.errstate(all="ignore"):
        st = path_seed(seed, key, sample)
        st = xs_next_u32(st)
        r1 = to_unit(st)
        st = xs_next_u32(st)
        r2 = to_unit(st)
        ang = F32(F32(F32(2.0) * PI) * r1)
        one = F32(1.0)
        if dist == SPHERE:
            y = F32(one - F32(F32(2.0) * r2))
            q = np.sqrt(F32(one - F32(y * y)))
            x = F32(mcos(ang) * q)
            z = F32(msin(ang) * q)
        else:
            x = F32(mcos(ang) * np.sqrt(F32(one - r2)))
            y = np.sqrt(r2)
            z = F32(msin(ang) * np.sqrt(F32(one - r2)))
        p, n = tuple(rec[:3]), tuple(rec[3:])
        xn = _orthogonal(n)
        zn = _cross(n, xn)
        wi = _normalize(_add(_add(_scale(xn, x), _scale(n, y)), _scale(zn, z)))
        o = _add(p, _scale(wi, EPSILON))
    return np.array(o + wi, F32), st


def point_rays(recs, keys, seed, sample, dist):
    """wpt_point_rays by the restatement: (n, 6) f32, six +0 for an invalid record."""
    recs = np.asarray(recs, F32).reshape(-1, 6)
    out = np.zeros((len(recs), 6), F32)
    for i, rec in enumerate(recs):
        r = point_ray(rec, int(keys[i]) if keys is not None else i, seed, sample, dist)
        if r is not None:
            out[i] = r[0]
    return out


# ---- the decision table --------------------------------------------------------
def _up(x):
    return np.nextafter(F32(x), F32(np.inf))


def _down(x):
    return np.nextafter(F32(x), F32(-np.inf))


def _unit_with(x=None, z=None, y_sign=1.0):
    """An f32 normal of length 1 (to rounding) with the given x and / or z."""
    x = F32(0.3) if x is None else F32(x)
    z = F32(0.05) if z is None else F32(z)
    y = F32(y_sign * np.sqrt(1.0 - float(x) ** 2 - float(z) ** 2))
    return (x, y, z)


T = F32(0.1)  # orthogonal's threshold
# (normal, orthogonal's branch): |s.z| and |s.x| just above, at and just below 0.1
NORMALS = (
    (_unit_with(z=_up(T)), 0), (_unit_with(z=-_up(T)), 0), (_unit_with(z=T), 1), (_unit_with(z=_down(T)), 1),
    (_unit_with(x=_up(T), z=_down(T)), 1), (_unit_with(x=-_up(T), z=T), 1), (_unit_with(x=T, z=T), 2),
    (_unit_with(x=_down(T), z=-_down(T), y_sign=-1.0), 2),
    ((0, 1, 0), 2), ((0, -1, 0), 2), ((0, 0, 1), 0), ((0, 0, -1), 0), ((1, 0, 0), 1), ((-1, 0, 0), 1),
    ((F32(0.6), F32(0.64), F32(0.48)), 0),
)
TABLE_POINT = (F32(0.25), F32(1.5), F32(-2.0))
_NAN, _INF = F32(np.nan), F32(np.inf)
INVALID_RECORDS = np.array([
    [_NAN, 0, 0, 0, 1, 0], [0, 0, _NAN, 0, 1, 0], [0, 0, 0, _NAN, 0, 1], [0, 0, 0, 0, 1, -_NAN],
    [_INF, 0, 0, 0, 1, 0], [0, -_INF, 0, 0, 1, 0], [0, 1, 0, _INF, 0, 0], [0, 1, 0, 0, 0, -_INF],
    [1, 2, 3, 0, 0, 0], [1, 2, 3, -0.0, -0.0, -0.0], [1, 2, 3, 0, -0.0, 0]], F32)
# Normals far from unit length: 2^-70 (orthogonal divides by a zero component or
# the frame underflows) and 1e30 (the squared length overflows, 1 / inf = 0, a
# direction of three zeros): the generated rays are not finite or are zero.
# MIXED_NORMAL's length puts the squared length of xn * x + n * y + zn * z
# around f32's largest number, so that it overflows for some samples only.
TINY, HUGE = F32(2.0 ** -70), F32(1e30)
FAR_NORMALS = ((0, 0, TINY), (TINY, 0, 0), (0, 0, HUGE), (0, HUGE, 0), (F32(0.6) * HUGE, 0, F32(0.8) * HUGE))
MIXED_NORMAL = (0, F32(2.0e19), 0)


def table_records():
    """(records (n, 6), orthogonal's branch per record or -1, kind per record:
    'unit', 'invalid', 'far', 'mixed')."""
    recs, branch, kind = [], [], []
    for n, b in NORMALS:
        recs.append(TABLE_POINT + tuple(F32(c) for c in n))
        branch.append(b)
        kind.append("unit")
    for r in INVALID_RECORDS:
        recs.append(tuple(r))
        branch.append(-1)
        kind.append("invalid")
    for n in FAR_NORMALS + (MIXED_NORMAL,):
        recs.append(TABLE_POINT + tuple(F32(c) for c in n))
        branch.append(-1)
        kind.append("mixed" if n is MIXED_NORMAL else "far")
    return np.array(recs, F32), np.array(branch), kind


# First draws u1 that put ang = 2 pi * r1 into each branch of msin / mcos an angle
# of [0, 2 pi] can reach: r1 <= 1.0f, so ang <= 2 pi (f32) < 9 pi / 4 and the
# rem_pio2f path beyond it is not reachable from a draw.
U1 = {"tiny": 100000, "pi/4": int(0.05 * 2 ** 32), "3pi/4": int(0.3 * 2 ** 32), "5pi/4": 1 << 31,
      "7pi/4": int(0.8 * 2 ** 32), "9pi/4": int(0.95 * 2 ** 32)}
U1_ONE = M32  # r1 == 1.0f exactly: ang is 2 pi
# r2: xs_next's word is never 0 (xorshift32 has no zero state), so r2 >= 2^-32 and
# r2 == 0 does not exist for any key; the nearest is the word 1. r2 == 1.0f exactly
# is every word >= 2^32 - 128 (they round to 2^32 as floats).
U2_NEAREST_ZERO, U2_ONE = 1, M32 - 5


def table_keys(sample):
    """{what: key} under SEED at `sample`: one key per reachable trig branch, r1 =
    1, r2 nearest 0, r2 = 1."""
    keys = {b: key_for(SEED, sample, u1=u) for b, u in U1.items()}
    keys["r1=1"] = key_for(SEED, sample, u1=U1_ONE)
    keys["r2~0"] = key_for(SEED, sample, u2=U2_NEAREST_ZERO)
    keys["r2=1"] = key_for(SEED, sample, u2=U2_ONE)
    return keys


def draws(key, sample, seed=SEED):
    """(r1, r2, ang) of the stream."""
    st = xs_next_u32(path_seed(seed, key, sample))
    r1 = to_unit(st)
    r2 = to_unit(xs_next_u32(st))
    return r1, r2, F32(F32(F32(2.0) * PI) * r1)


def table_case(sample):
    """The table at one sample index: every record under every key of
    table_keys(sample): (records (n, 6), keys (n,) u32)."""
    recs, _, _ = table_records()
    keys = list(table_keys(sample).values())
    return (np.ascontiguousarray(np.repeat(recs, len(keys), axis=0)),
            np.tile(np.array(keys, np.uint32), len(recs)))


# ---- the point sets ------------------------------------------------------------
FREE_NORMALS = np.array([[0, 1, 0], [0, -1, 0], [1, 0, 0], [-1, 0, 0], [0, 0, 1], [0, 0, -1]], F32)
SET_SPP = 3  # the spp at which the sets' conditions are asserted (samples 0..2, NoNEE and NEE, COSINE)


def _frozen(a):
    a.setflags(write=False)
    return a


def point_set(wpt, oracle, name):
    """(rays_fixtures scene, records (n, 6) f32) of scene `name`:
     - surface points: the hits of the scene's probe rays, o + d * t with the
       hit's normal (the oracle's trace_rays and shape normals);
     - free-space probes: the scene's camera position under the six axis normals,
       and a point far above the scene looking up (its paths leave the scene);
     - invalid records, normals far from unit length, and MIXED_NORMAL at a
       surface point."""
    def make():
        sc = rf.scene(wpt, oracle, name)
        mats = wpt.interface.DebugScene(sc.scene_id, sc.mesh).materials()
        rays = sc.probe_rays()
        pl = rfr.expected_planes(oracle, sc.ref, mats, rays)
        hit = pl["kind"] != 0
        assert hit.sum() >= 8, (name, int(hit.sum()))
        pos = (rays[hit, :3] + rays[hit, 3:] * pl["t"][hit, None]).astype(F32)
        surf = np.concatenate([pos, pl["normal"][hit]], axis=1)
        cam = np.asarray(sc.cam[:3], F32)
        free = np.concatenate([np.tile(cam, (6, 1)), FREE_NORMALS], axis=1)
        away = np.array([[0, 1000, 0, 0, 1, 0]], F32)
        far = np.array([tuple(surf[0, :3]) + tuple(F32(c) for c in n) for n in FAR_NORMALS + (MIXED_NORMAL,)], F32)
        mixed = np.array([tuple(p[:3]) + MIXED_NORMAL for p in surf[1:4]], F32)
        recs = np.concatenate([surf, free, away, INVALID_RECORDS[[0, 6, 8]], far, mixed]).astype(F32)
        return sc, _frozen(np.ascontiguousarray(recs))
    return rfr.once(("point_set", name), make)


def expected(wpt, ref, recs, keys, sample, spp, rtype, dist, depth=DEPTH, light_debug=0, threads=4):
    """The definition's identity on the oracle: (rgb (n, 3) f32, status (n,) u8,
    {'paths', 'rays', 'shadow_rays'}, per-sample validity (spp, n) bool)."""
    recs = np.ascontiguousarray(recs, F32).reshape(-1, 6)
    n = len(recs)
    k = np.arange(n, dtype=np.uint32) if keys is None else np.asarray(keys, np.uint32)
    rgb = np.zeros((n, 3), F32)
    counts = {"paths": 0, "rays": 0, "shadow_rays": 0}
    traced = np.zeros((spp, n), bool)
    for j in range(spp):
        rays = wpt.interface.point_rays(recs, k, SEED, sample + j, dist)
        c, st, stats = ref.radiance_rays(rays, k, sample + j, 1, rtype, depth, SEED, light_debug, threads)
        rgb = (rgb + c).astype(F32)
        traced[j] = st.astype(bool)
        counts["paths"] += int(st.sum())
        # the oracle's "rays" holds extension and shadow rays together
        counts["rays"] += stats["rays"] - stats["shadow_rays"]
        counts["shadow_rays"] += stats["shadow_rays"]
    return rgb, valid(recs), counts, traced


def set_expected(wpt, oracle, name, rtype, dist, sample=0, spp=SET_SPP, depth=DEPTH, light_debug=0):
    def make():
        sc, recs = point_set(wpt, oracle, name)
        out = expected(wpt, sc.ref, recs, None, sample, spp, rtype, dist, depth, light_debug)
        return tuple(_frozen(a) if isinstance(a, np.ndarray) else a for a in out)
    return rfr.once(("set_expected", name, rtype, dist, sample, spp, depth, light_debug), make)


bits = rf.bits
