"""Adversarial meshes and ray sets for the traversal and shadow kernels.

A plain helper module (no pytest hooks): tests/test_adversarial_cpu.py
asserts on the oracle alone that these constructions produce the conditions
they are built for (exact ties, NaN slab products, deep stacks, ...), and
tests/test_gpu_adversarial.py sends the same rays through the device.

Meshes are for scene 2: store_mesh takes mesh coordinates and the scene puts
them at world = 0.5 * mesh + (0, 0, 5) (wasm_interface.rs:300-311). The
sheets use dyadic coordinates, so their world coordinates are exact and every
triangle of one sheet has the same normal (0, k, 0) and the same n.v0: a hit
anywhere on a sheet has the same t bit for bit, whichever triangle reports
it. Everything is deterministic (np.random.default_rng with fixed seeds), at
most 4,096 triangles per mesh and 4,000 rays per set.
"""
import ctypes

import numpy as np

F32 = np.float32
K_EPSILON = F32(0.0002)      # math/mod.rs:11
# kLdsSlots in wpt_render.hip (WPT_LDS_SLOTS, default 9): traversal stack
# entries kept in LDS; deeper entries go to the global spill area
LDS_SLOTS = 9
MAX_TRIS, MAX_RAYS = 4096, 4000
Q = 64.0                     # origins are rounded to multiples of 1 / Q (dyadic: aimed rays are exact)


def world(mesh):
    """(n, 3, 3) world vertices of a mesh, in the scene's own f32 operations."""
    v = np.asarray(mesh, F32).reshape(-1, 3, 3)
    return (v * F32(0.5) + np.array([0.0, 0.0, 5.0], F32)).astype(F32)


# ---- meshes -----------------------------------------------------------------
def _grid(n, c, a0, b0, step, axes, flip):
    """n x n quads in the plane `axes[2]` = c; (a, b) run along axes[0], axes[1]."""
    out = np.empty((n, n, 2, 3, 3), np.float64)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    a, b = a0 + i * step, b0 + j * step

    def pt(aa, bb):
        p = np.empty(aa.shape + (3,))
        p[..., axes[0]], p[..., axes[1]], p[..., axes[2]] = aa, bb, c
        return p
    p00, p01, p11, p10 = pt(a, b), pt(a, b + step), pt(a + step, b + step), pt(a + step, b)
    for k, tri in enumerate(((p00, p01, p11), (p00, p11, p10))):
        t = (tri[0], tri[2], tri[1]) if flip else tri
        for m in range(3):
            out[:, :, k, m] = t[m]
    return out.reshape(-1).astype(F32)


def grid_y(n, y, x0, z0, step, flip=False):
    """An n x n quad sheet in the plane y (mesh coordinates), two triangles per
    quad, all with the normal (0, step^2, 0) (flip: (0, -step^2, 0))."""
    return _grid(n, y, x0, z0, step, (0, 2, 1), flip)


def grid_xy(n, z, x0, y0, step, flip=False):
    """The same sheet in the plane z; normal (0, 0, -+step^2)."""
    return _grid(n, z, x0, y0, step, (0, 1, 2), flip)


def mesh_a():
    """16 x 16 sheet at world y = 0.5, x in [-1, 1], z in [5, 7]."""
    return grid_y(16, 1.0, -2.0, 0.0, 0.25)


def mesh_b():
    """8 x 8 sheet coplanar with the floor plane (world y = -1, mesh y = -2)."""
    return grid_y(8, -2.0, -2.0, 0.0, 0.5)


def mesh_b_wall():
    """8 x 8 sheet coplanar with the back plane (world z = 13, mesh z = 16)."""
    return grid_xy(8, 16.0, -2.0, 0.0, 0.5)


def mesh_b_ulp():
    """Two floor sheets one f32 step above and below mesh y = -2 (side by side)."""
    up, dn = np.nextafter(F32(-2.0), F32(0.0)), np.nextafter(F32(-2.0), F32(-4.0))
    return np.concatenate([grid_y(8, float(up), -4.0, 0.0, 0.5), grid_y(8, float(dn), 0.0, 0.0, 0.5)])


def mesh_c():
    """Two coincident sheets of opposite winding and a third shifted by half a cell."""
    return np.concatenate([grid_y(8, 1.0, -2.0, 0.0, 0.5), grid_y(8, 1.0, -2.0, 0.0, 0.5, flip=True),
                           grid_y(8, 1.0, -1.75, 0.25, 0.5)])


def mesh_d(levels=2):
    """A closed mesh with shared edges and vertices: an octahedron subdivided
    `levels` times, the new vertices pushed onto the sphere (not coplanar).
    Centre mesh (0, 2, 3), radius 2: world centre (0, 1, 6.5), radius 1."""
    ax = np.eye(3)
    tris = []
    for sx in (1, -1):
        for sy in (1, -1):
            for sz in (1, -1):
                t = [sx * ax[0], sy * ax[1], sz * ax[2]]
                tris.append(t if sx * sy * sz > 0 else t[::-1])
    tris = np.array(tris)
    for _ in range(levels):
        a, b, c = tris[:, 0], tris[:, 1], tris[:, 2]
        ab, bc, ca = ((a + b) / 2, (b + c) / 2, (c + a) / 2)
        ab, bc, ca = (m / np.linalg.norm(m, axis=1, keepdims=True) for m in (ab, bc, ca))
        tris = np.concatenate([np.stack(t, axis=1) for t in ((a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca))])
    return (tris * 2.0 + np.array([0.0, 2.0, 3.0])).reshape(-1).astype(F32)


def mesh_e(wpt):
    """A 500-triangle cloud plus degenerate triangles (collinear, all three
    vertices equal, two equal) and triangles with NaN vertices."""
    v = wpt.scenes.triangle_cloud(500, seed=0xE5E).reshape(-1, 3, 3).copy()
    rng = np.random.default_rng(0xE)
    c = rng.uniform([-2.0, -2.0, 0.5], [2.0, 2.0, 4.5], (30, 3)).astype(F32)
    e = rng.uniform(-0.5, 0.5, (30, 3)).astype(F32)
    deg = np.stack([c, c + e, c + F32(2.0) * e], axis=1)   # collinear
    deg[10:20, 1] = deg[10:20, 0]
    deg[10:20, 2] = deg[10:20, 0]                         # a point
    deg[20:, 2] = deg[20:, 1]                             # two vertices equal
    nan = v[rng.choice(500, 24, replace=False)].copy()
    nan[:12] = np.nan                                     # whole triangles
    nan[12:, rng.integers(0, 3), :] = np.nan              # one vertex each
    nan[:3, :, 0] = -F32(np.nan)                          # negative NaN bits
    return np.concatenate([v, deg, nan]).reshape(-1).astype(F32)


def mesh_f(n=4096):
    """Overlap: large triangles with vertices uniform over the mesh box
    [-3, 3] x [-1.5, 5] x [-3, 3], so every node box nearly fills the root's."""
    rng = np.random.default_rng(0xF)
    return rng.uniform([-3.0, -1.5, -3.0], [3.0, 5.0, 3.0], (n, 3, 3)).astype(F32).reshape(-1)


F_WORLD_BOX = np.array([-1.5, -0.75, 3.5, 1.5, 2.5, 6.5], F32)
# the inside set starts in the central half of that box (in each axis): an
# origin there lies inside nearly every node box, so both children are hit
F_INSIDE_BOX = np.array([-0.75, 0.0625, 4.25, 0.75, 1.6875, 5.75], F32)


def mesh_g():
    """Shadow: a sheet coplanar with the light quad (world y = 7, x in [-1, 1],
    z in [0, 2]) over its x >= 0 half, a sheet under the light at world y = 3
    (x in [-1.5, 0.5]) and a sheet on the floor."""
    return np.concatenate([grid_y(8, 14.0, 0.0, -10.0, 0.5), grid_y(8, 6.0, -3.0, -10.0, 0.5),
                           grid_y(8, -2.0, -4.0, -10.0, 1.0)])


def mesh_ba():
    """The floor sheet and, beside it, sheet A (moved to world x in [1, 3]): the render fixture."""
    return np.concatenate([mesh_b(), grid_y(16, 1.0, 2.0, 0.0, 0.25)])


def scene2_meshes(wpt):
    """name -> mesh (f32, 9 per triangle)."""
    m = {"A": mesh_a(), "B": mesh_b(), "Bwall": mesh_b_wall(), "Bulp": mesh_b_ulp(), "C": mesh_c(), "D": mesh_d(),
         "E": mesh_e(wpt), "F": mesh_f(), "G": mesh_g(), "BA": mesh_ba()}
    assert all(v.size // 9 <= MAX_TRIS for v in m.values())
    return m


TIE_MESHES = ("A", "B", "Bwall", "C")      # exact ties by construction
F64_MESHES = ("A", "B", "C", "D", "F")     # compared with the f64 brute force
F64_EXCLUDED_SETS = ("on_plane", "on_surface")


# ---- ray sets ---------------------------------------------------------------
def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _rays(o, d):
    return np.concatenate([np.asarray(o, F32), np.asarray(d, F32)], axis=1).astype(F32)


def _finite_tris(mesh):
    w = world(mesh)
    return w[np.all(np.isfinite(w), axis=(1, 2))]


def _normals(w):
    """f64 unit normals; a degenerate triangle gets +y."""
    n = np.cross(w[:, 1].astype(np.float64) - w[:, 0], w[:, 2].astype(np.float64) - w[:, 0])
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    return np.where(ln > 1e-12, n / np.maximum(ln, 1e-300), np.array([0.0, 1.0, 0.0]))


def _aimed(rng, tgt, nrm, limit):
    """Rays at `tgt` from origins 0.5-4 along +-nrm (alternating: above and
    mirrored below, where a scene plane is not in the way) plus sideways
    noise, rounded to 1/Q; every fourth is
    perpendicular (no noise). Half keep the exact difference as direction
    (t = 1 where the coordinates are dyadic), half are normalised."""
    if len(tgt) > limit:
        pick = np.sort(rng.choice(len(tgt), limit, replace=False))
        tgt, nrm = tgt[pick], nrm[pick]
    n = len(tgt)
    k = np.arange(n)
    off = nrm * (rng.uniform(0.5, 4.0, (n, 1)) * np.where(k % 2, -1.0, 1.0)[:, None])
    off += np.where((k % 4 == 3)[:, None], 0.0, rng.normal(size=(n, 3)) * 0.7)
    # an origin behind the floor (y = -1) or the back plane (z = 13) of scene 2 whose target lies clearly in
    # front of it would only see that plane: such a ray comes from the other side instead
    o = tgt.astype(np.float64) + off
    blocked = ((o[:, 1] < -1.0) & (tgt[:, 1] > -0.999)) | ((o[:, 2] > 13.0) & (tgt[:, 2] < 12.999))
    off[blocked] = -off[blocked]
    o = (np.round((tgt.astype(np.float64) + off) * Q) / Q).astype(F32)
    d = (tgt.astype(F32) - o).astype(F32)
    dn = _unit(d).astype(F32)
    d[k % 8 >= 4] = dn[k % 8 >= 4]
    return _rays(o, d)


def vertex_rays(mesh, seed=1, limit=1000):
    w = _finite_tris(mesh)
    n = np.repeat(_normals(w), 3, axis=0)
    v, first = np.unique(w.reshape(-1, 3), axis=0, return_index=True)
    return _aimed(np.random.default_rng(seed), v, n[first], limit)


def edge_rays(mesh, seed=2, limit=1000):
    w = _finite_tris(mesh)
    mid = ((w + np.roll(w, -1, axis=1)) * F32(0.5)).astype(F32).reshape(-1, 3)
    n = np.repeat(_normals(w), 3, axis=0)
    m, first = np.unique(mid, axis=0, return_index=True)
    return _aimed(np.random.default_rng(seed), m, n[first], limit)


def interior_rays(mesh, seed=3, limit=600):
    rng = np.random.default_rng(seed)
    w = _finite_tris(mesh)
    pick = rng.integers(0, len(w), limit)
    b = rng.dirichlet([1.0, 1.0, 1.0], limit)
    p = np.einsum("nk,nkc->nc", b, w[pick].astype(np.float64)).astype(F32)
    return _aimed(rng, p, _normals(w)[pick], limit)


def on_plane_rays(nodes, seed=4, limit=600):
    """Origins with one coordinate exactly on a BVH2 node's bound and a +-0
    direction component on that axis: (bound - o) * (1 / d) = 0 * inf = NaN in
    the slab test. `nodes`: (n, 8) u32 rows (six f32 bounds, left_first, count)."""
    rng = np.random.default_rng(seed)
    box = nodes[:, :6].copy().view(F32)
    pick = rng.integers(0, len(box), limit)
    k = np.arange(limit)
    b = box[pick]
    o = rng.uniform(b[:, :3] - 0.25, b[:, 3:] + 0.25).astype(F32)
    inside = k % 3 != 2                    # two of three start inside the node's box
    o[inside] = rng.uniform(b[inside, :3], b[inside, 3:]).astype(F32)
    d = _unit(rng.normal(size=(limit, 3))).astype(F32)
    ax = k % 3
    o[k, ax] = b[k, ax + 3 * ((k // 3) % 2)]
    d[k, ax] = np.where(k % 2, F32(-0.0), F32(0.0))
    return _rays(o, d), pick, ax


def on_surface_rays(mesh, seed=5, limit=150):
    """Origins exactly on triangle vertices and on triangle planes (centroids),
    heading into, out of and within the plane; then the same origins moved by
    +-kEpsilon along the normal."""
    rng = np.random.default_rng(seed)
    w = _finite_tris(mesh)
    pick = rng.integers(0, len(w), limit)
    t, n = w[pick], _normals(w)[pick]
    cen = ((t[:, 0] + t[:, 1] + t[:, 2]) / F32(3.0)).astype(F32)
    k = np.arange(limit)
    o = np.where((k % 2 == 0)[:, None], t[:, 0], cen).astype(F32)
    edge = (t[:, 1] - t[:, 0]).astype(np.float64)
    edge = np.where(np.linalg.norm(edge, axis=1, keepdims=True) > 0, edge, np.array([1.0, 0.0, 0.0]))
    noise = rng.normal(size=(limit, 3)) * 0.4
    out = []
    for dirs in (-n + noise, n + noise, edge, -n, n):
        out.append(_rays(o, _unit(dirs)))
    for s in (1.0, -1.0):
        oo = (o + (s * float(K_EPSILON)) * n).astype(F32)
        out.append(_rays(oo, _unit(-s * n + noise)))
        out.append(_rays(oo, _unit(edge)))
    return np.concatenate(out)


def degenerate_rays(mesh, seed=6, limit=120):
    """Denormal direction components, unnormalised directions (length 1e-3 and
    1e3), origins 1e6 away, two zero components; all aimed at the mesh."""
    rng = np.random.default_rng(seed)
    base = interior_rays(mesh, seed, limit)
    o, d = base[:, :3].astype(np.float64), _unit(base[:, 3:])
    out = []
    for comp in range(3):                       # one denormal component
        dd = d.copy()
        dd[:, comp] = np.where(np.arange(limit) % 2, 1e-40, -3e-42)
        out.append(_rays(o, dd))
    out.append(_rays(o, d * 1e-3))
    out.append(_rays(o, d * 1e3))
    tgt = o + d * np.linalg.norm(base[:, 3:], axis=1, keepdims=True)
    far = tgt - d * 1e6
    out.append(_rays(far, d))
    for comp in range(3):                       # two zero components: axis rays through the targets
        dd = np.zeros((limit, 3))
        sgn = np.where(np.arange(limit) % 2, 1.0, -1.0)
        dd[:, comp] = sgn
        oo = tgt.copy()
        oo[:, comp] -= sgn * rng.uniform(0.5, 4.0, limit)
        out.append(_rays(oo, dd))
    return np.concatenate(out)


def inside_rays(box, seed=7, limit=2000):
    """Origins inside a world box, random directions."""
    rng = np.random.default_rng(seed)
    o = rng.uniform(box[:3], box[3:], (limit, 3))
    return _rays(o, _unit(rng.normal(size=(limit, 3))))


def scene2_sets(name, mesh, nodes):
    """name -> (n, 6) f32 rays for one scene-2 fixture."""
    s = {"vertices": vertex_rays(mesh), "edges": edge_rays(mesh), "interior": interior_rays(mesh),
         "on_plane": on_plane_rays(nodes)[0], "on_surface": on_surface_rays(mesh),
         "degenerate": degenerate_rays(mesh)}
    if name == "F":
        s["inside"] = inside_rays(F_INSIDE_BOX)
    assert all(len(r) <= MAX_RAYS for r in s.values())
    return s


# ---- shape sets for scenes 0, 100, 101 --------------------------------------
KIND_TRI, KIND_PLANE, KIND_SPHERE, KIND_AARECT, KIND_TORUS = 0, 1, 2, 3, 4


def _perp(u):
    a = np.where(np.abs(u[:, :1]) < 0.9, np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0]))
    return _unit(np.cross(u, a))


def sphere_rays(shapes, seed=8, per=3):
    """(rays, labels): closest approach r (1 +- k 2^-23), origin at the centre,
    origin on the surface heading in / out / tangent, through the centre from
    1e3 away."""
    rng = np.random.default_rng(seed)
    rays, lab = [], []
    for s in shapes[shapes[:, 12] == KIND_SPHERE]:
        c, r = s[:3].astype(np.float64), float(s[3])
        u = _unit(rng.normal(size=(per, 3)))
        w = _perp(u)
        for k in (0, 1, 2, 8, 64):
            for sg in ((1,) if k == 0 else (1, -1)):
                b = r * (1.0 + sg * k * 2.0 ** -23)
                o = c + 5.0 * u + b * w
                rays.append(_rays(o, -u))
                lab += [f"graze{sg * k:+d}"] * per
        rays.append(_rays(np.tile(c, (per, 1)), u))
        lab += ["centre"] * per
        surf = c + r * u
        for nm, dd in (("surf_in", -u + 0.3 * w), ("surf_out", u + 0.3 * w), ("surf_tangent", w)):
            rays.append(_rays(surf, _unit(dd)))
            lab += [nm] * per
        rays.append(_rays(c + 1e3 * u, -u))
        lab += ["far"] * per
    return np.concatenate(rays), np.array(lab)


def aarect_rays(shapes, seed=9, per=2):
    """(rays, labels): aimed at corners, edge midpoints and face centres; origins
    on faces with in-face directions; origins inside."""
    rng = np.random.default_rng(seed)
    rays, lab = [], []
    for s in shapes[shapes[:, 12] == KIND_AARECT]:
        lo, hi = s[[0, 2, 4]].astype(np.float64), s[[1, 3, 5]].astype(np.float64)
        mid = (lo + hi) / 2
        g = np.array([[(lo[0], mid[0], hi[0])[i], (lo[1], mid[1], hi[1])[j], (lo[2], mid[2], hi[2])[k]]
                      for i in range(3) for j in range(3) for k in range(3) if (i, j, k) != (1, 1, 1)])
        nm = np.array([("face", "edge", "corner")[sum(x != 1 for x in (i, j, k)) - 1]
                       for i in range(3) for j in range(3) for k in range(3) if (i, j, k) != (1, 1, 1)])
        for _ in range(per):
            out = _unit(g - mid + rng.normal(size=g.shape) * 0.05)
            o = np.round((g + out * rng.uniform(0.5, 3.0, (len(g), 1))) * Q) / Q
            d = g.astype(F32) - o.astype(F32)
            rays.append(_rays(o, d))
            lab += list(nm)
        for ax in range(3):                    # on a face, direction in the face
            for side in (lo, hi):
                o = rng.uniform(lo, hi, (per, 3))
                o[:, ax] = side[ax]
                d = _unit(rng.normal(size=(per, 3)))
                d[:, ax] = 0.0
                rays.append(_rays(o, d))
                lab += ["in_face"] * per
        rays.append(_rays(rng.uniform(lo, hi, (3 * per, 3)), _unit(rng.normal(size=(3 * per, 3)))))
        lab += ["inside"] * (3 * per)
    return np.concatenate(rays), np.array(lab)


def torus_rays(shapes, seed=10, tori=6, per=8):
    """(rays, labels) for tori with the y axis: along the axis (through the
    hole and down onto the tube), in the equatorial plane through the centre,
    tangent to the outer and inner equators and to the top circle, origins
    inside the tube and at the centre, origins 1e3 away. Labels starting with
    "tangent" mark the ill-conditioned ones."""
    rng = np.random.default_rng(seed)
    rays, lab = [], []
    tt = shapes[shapes[:, 12] == KIND_TORUS]
    for s in tt[:: max(1, len(tt) // tori)][:tori]:
        c, R, r = s[:3].astype(np.float64), float(s[3]), float(s[4])
        phi = rng.uniform(0, 2 * np.pi, per)
        rad = np.stack([np.cos(phi), np.zeros(per), np.sin(phi)], axis=1)
        tan = np.stack([-np.sin(phi), np.zeros(per), np.cos(phi)], axis=1)
        up = np.tile([0.0, 1.0, 0.0], (per, 1))
        add = lambda nm, o, d: (rays.append(_rays(o, d)), lab.extend([nm] * len(o)))  # noqa: E731
        add("axis_hole", c + 5.0 * up, -up)
        add("axis_tube", c + R * rad + 5.0 * up, -up)
        add("equator", c + 5.0 * rad, -rad)
        add("tangent_outer", c + (R + r) * rad - 4.0 * tan, tan)
        add("tangent_inner", c + (R - r) * rad - 4.0 * tan, tan)
        add("tangent_top", c + R * rad + r * up - 4.0 * tan, tan)
        add("in_tube", c + R * rad + 0.3 * r * _unit(rng.normal(size=(per, 3))), _unit(rng.normal(size=(per, 3))))
        add("centre", np.tile(c, (per, 1)), _unit(rad + 0.1 * rng.normal(size=(per, 3))))
        aim = c + R * rad + 0.5 * r * _unit(rng.normal(size=(per, 3)))
        far = _unit(rng.normal(size=(per, 3)) + 2.0 * up)
        add("far", aim + 1e3 * far, -far)
    return np.concatenate(rays), np.array(lab)


def shape_sets(scene_id, shapes):
    """name -> (rays, labels) built from a scene's shape records."""
    s = {}
    if scene_id == 101:
        s["sphere"] = sphere_rays(shapes)
    if scene_id in (0, 100):
        s["aarect"] = aarect_rays(shapes)
    if scene_id == 0:
        s["torus"] = torus_rays(shapes)
    assert all(len(r) <= MAX_RAYS for r, _ in s.values())
    return s


# ---- shadow segments for mesh G ---------------------------------------------
Q_CLASSES = ("vertex", "diagonal", "edge_in_sheet", "interior")
P_CLASSES = ("sheet3_vertex", "floor", "light_plane", "above", "random")


def shadow_set(shapes, seed=12, per=50):
    """(pq (n, 6), light ids, q class, p class) on the G scene: every q class
    with every p class. The light quad is lc1 (-1, 7, 0), lc2 (1, 7, 0), lc3
    (1, 7, 2), lc4 (-1, 7, 2), cut along lc1-lc3; q lies on the light named in
    `light ids`. Zero-length segments (p = q) are left out: their direction is
    0 / 0 in the reference."""
    rng = np.random.default_rng(seed)
    lights = np.nonzero(shapes[:, 13] == 1.0)[0].astype(np.int32)
    lv = shapes[lights, :9].reshape(-1, 3, 3)
    lc1, lc2, lc3 = np.array([-1.0, 7.0, 0.0]), np.array([1.0, 7.0, 0.0]), np.array([1.0, 7.0, 2.0])
    has_lc2 = np.array([np.any(np.all(t == lc2.astype(F32), axis=1)) for t in lv])
    l_a = int(lights[has_lc2][0])          # (lc3, lc2, lc1): the x >= z half, under the coplanar sheet's edge
    sheet3 = np.unique(world(grid_y(8, 6.0, -3.0, -10.0, 0.5)).reshape(-1, 3), axis=0)
    pq, li, qc, pc = [], [], [], []
    for qn in Q_CLASSES:
        for pn in P_CLASSES:
            k = np.arange(per)
            lk = lights[k % len(lights)]
            if qn == "vertex":
                q = lv[k % len(lights), k % 3].astype(np.float64)
            elif qn == "diagonal":
                s = np.round(rng.uniform(0, 1, (per, 1)) * 32) / 32
                q = lc1 + s * (lc3 - lc1)
            elif qn == "edge_in_sheet":     # lc2-lc3 (x = 1) lies inside the coplanar sheet (x in [0, 2])
                s = np.round(rng.uniform(0, 1, (per, 1)) * 32) / 32
                q = lc2 + s * (lc3 - lc2)
                lk = np.full(per, l_a, np.int32)
            else:
                t = lv[k % len(lights)].astype(np.float64)
                b = rng.dirichlet([1.0, 1.0, 1.0], per)
                q = np.einsum("nk,nkc->nc", b, t)
            if pn == "sheet3_vertex":
                p = sheet3[rng.integers(0, len(sheet3), per)].astype(np.float64)
            elif pn == "floor":
                p = np.stack([rng.uniform(-2, 2, per), np.full(per, -1.0), rng.uniform(0, 4, per)], axis=1)
            elif pn == "light_plane":
                p = np.stack([rng.uniform(-3, 3, per), np.full(per, 7.0), rng.uniform(-1, 3, per)], axis=1)
            elif pn == "above":
                p = np.stack([rng.uniform(-2, 2, per), rng.uniform(7.5, 10, per), rng.uniform(-1, 3, per)], axis=1)
            else:
                p = rng.uniform([-3.0, -0.9, -1.0], [3.0, 9.0, 4.0], (per, 3))
            seg = np.concatenate([p, q], axis=1).astype(F32)
            keep = np.any(seg[:, :3] != seg[:, 3:], axis=1)
            pq.append(seg[keep])
            li.append(lk[keep])
            qc += [qn] * int(keep.sum())
            pc += [pn] * int(keep.sum())
    return np.concatenate(pq), np.concatenate(li).astype(np.int32), np.array(qc), np.array(pc)


# ---- tools ------------------------------------------------------------------
def brute_hits(sc, rays, lib=None):
    """(n rays, n shapes) f32: every shape's own t for every ray through the
    oracle's per-shape trace (oracle_shape_trace), +inf where it misses. No
    BVH, no ordering, no culling: none of the code under test."""
    import pyoracle
    L = lib if lib is not None else pyoracle.lib()
    fn = L.oracle_shape_trace
    fn.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    fn.restype = ctypes.c_int
    shapes = np.ascontiguousarray(sc.shapes(), F32)
    r = np.ascontiguousarray(rays, F32).reshape(-1, 6)
    kinds = [int(k) for k in shapes[:, 12]]
    out = np.full((len(r), len(shapes)), np.inf, F32)
    t = np.zeros(1, F32)
    nrm = np.zeros(3, F32)
    tp, npn, g0, r0 = t.ctypes.data, nrm.ctypes.data, shapes.ctypes.data, r.ctypes.data
    for i in range(len(r)):
        ra = r0 + 24 * i
        row = out[i]
        for j, kind in enumerate(kinds):
            if fn(kind, g0 + 64 * j, ra, tp, npn):
                row[j] = t[0]
    return out


def _slabs(box, o, inv):
    with np.errstate(invalid="ignore", over="ignore"):
        t1 = ((box[:, :3] - o) * inv).astype(F32)
        t2 = ((box[:, 3:] - o) * inv).astype(F32)
    return t1, t2


def aabb_hit_np(box, o, inv):
    """AABB::hit (aabb.rs:132-164) in numpy f32 for (n, 6) boxes and (n, 3)
    rays: (hit, entry). np.fmin / np.fmax drop a NaN operand as f32::min / max do."""
    t1, t2 = _slabs(box, o, inv)
    lo, hi = np.fmin(t1, t2), np.fmax(t1, t2)
    tmin = np.fmax(np.fmax(lo[:, 0], lo[:, 1]), lo[:, 2])
    tmax = np.fmin(np.fmin(hi[:, 0], hi[:, 1]), hi[:, 2])
    with np.errstate(invalid="ignore"):
        hit = ~(tmin > tmax) & ((tmin >= 0) | (tmax >= 0))
        h = np.where(tmin >= 0, tmin, F32(0.0)).astype(F32)
    return hit, h


def first_descent_pending(nodes, o, d, max_dis=None):
    """Per ray: the number of levels on the reference's first root-to-leaf
    descent (scene.rs:191-288) at which both child boxes are hit before
    `max_dis` (the plane hit that seeds the search, default +inf). Nothing is
    popped before the first leaf is reached, so this is a lower bound of the
    ray's peak stack depth in the BVH2 machine."""
    o = np.asarray(o, F32).reshape(-1, 3)
    d = np.asarray(d, F32).reshape(-1, 3)
    n = len(o)
    md = np.full(n, np.inf, F32) if max_dis is None else np.asarray(max_dis, F32)
    with np.errstate(divide="ignore"):
        inv = (F32(1.0) / d).astype(F32)
    box = nodes[:, :6].copy().view(F32)
    lf, cnt = nodes[:, 6].astype(np.int64), nodes[:, 7]
    hit, h = aabb_hit_np(np.tile(box[0], (n, 1)), o, inv)
    live = hit & (h < md)
    cur = np.zeros(n, np.int64)
    pending = np.zeros(n, np.int64)
    while True:
        live &= cnt[cur] == 0
        if not live.any():
            return pending
        i = np.nonzero(live)[0]
        li = lf[cur[i]]
        hl, dl = aabb_hit_np(box[li], o[i], inv[i])
        hr, dr = aabb_hit_np(box[li + 1], o[i], inv[i])
        hl &= dl < md[i]
        hr &= dr < md[i]
        pending[i] += hl & hr
        left = hl & (~hr | (dl < dr))          # ties go right (scene.rs:244)
        cur[i] = np.where(left, li, li + 1)
        live[i] = hl | hr


# ---- independent f64 closest hit --------------------------------------------
# Each helper returns (possible, sure[, self]) per ray for one shape or one
# kind: the f64 t of a hit the reference's f32 arithmetic may report, and of a
# hit it certainly reports (+inf: none). Between the two lies the band in which
# f32 rounding decides; `sure` holds the largest t the reference may compute.
TRI_SLACK = 0.1 * 0.0002     # triangle.rs:41-45: an edge function may be this far below 0
U32 = 2.0 ** -24             # f32 unit roundoff
FLT_MAX = float(np.finfo(F32).max)


def _f64_plane(loc, n, o, d):
    """t = (loc - o).n / d.n, t > 0. sure: t plus the numerator's f32 error bound (as _f64_triangles)."""
    t = ((loc - o) @ n) / (d @ n)
    t = np.where(np.isfinite(t) & (t > 0), t, np.inf)
    return t, t + 2.0 ** -21 * (np.abs(n) @ np.abs(loc) + np.abs(o) @ np.abs(n)) / np.abs(d @ n)


def _f64_sphere(c, rad, o, d, t_oracle):
    """Analytic roots. Ambiguous in f32, hence possible but not sure: a graze
    (the discriminant b^2 - a c, formed from terms of size b^2 + a |oc|^2 with
    2^-22 of relative error or so, within 2^-17 of that size of 0: no root, or
    two within sqrt(2 g) / a of -b / a) and a root within 1e-5 of the origin (on
    the surface: its sign is rounding). There the oracle's own t is taken if it
    lies in that window (`self`: such a ray is not a check of t)."""
    oc = o - c
    a = np.einsum("ij,ij->i", d, d)
    b = np.einsum("ij,ij->i", oc, d)
    oc2 = np.einsum("ij,ij->i", oc, oc)
    disc = b * b - a * (oc2 - rad * rad)
    sq = np.sqrt(np.maximum(disc, 0))
    t0, t1 = (-b - sq) / a, (-b + sq) / a
    t = np.where(disc >= 0, np.where(t0 > 0, t0, np.where(t1 > 0, t1, np.inf)), np.inf)
    g = 2.0 ** -17 * (b * b + a * oc2)
    graze = np.abs(disc) <= g
    zero = (disc >= 0) & ((np.abs(t0) < 1e-5) | (np.abs(t1) < 1e-5))
    near = (graze & (np.abs(t_oracle + b / a) <= np.sqrt(2 * g) / a)) | \
           (zero & (np.minimum(np.abs(t_oracle - t0), np.abs(t_oracle - t1)) <= 1e-5))
    alt = np.where(np.abs(t_oracle - t1) < np.abs(t_oracle - t0), t1, t0)      # the root nearest the oracle's t
    real = zero & ~graze & (alt > 1e-5)
    amb = graze | zero
    poss = np.where(amb, np.where(real, alt, np.where(near, t_oracle, np.inf)), t)
    return poss, np.where(amb, np.inf, t), amb & ~real & near


def _f64_aarect(lo, hi, o, d):
    """Slabs; tmin if > 0, else tmax if > 0 (aa_rect.rs). Grazing an edge or a
    corner, starting on a face or running within a face is possible, not sure."""
    ta, tb = (lo - o) / d, (hi - o) / d
    par = d == 0
    inside = (o >= lo) & (o <= hi)
    # a direction component of 0: the slab is all of the line (origin within it) or none of it
    lo_t = np.where(par, np.where(inside, -np.inf, np.inf), np.minimum(ta, tb))
    hi_t = np.where(par, np.where(inside, np.inf, -np.inf), np.maximum(ta, tb))
    tn, tx = lo_t.max(axis=1), hi_t.min(axis=1)
    t = np.where(tn < tx, np.where(tn > 0, tn, np.where(tx > 0, tx, np.inf)), np.inf)
    edge = (np.abs(tx - tn) <= 1e-5 * np.maximum(1.0, np.abs(tn))) | (np.abs(tn) < 1e-5) | \
           (np.abs(tx) < 1e-5) | np.any(par & ((o == lo) | (o == hi)), axis=1)
    return np.where(edge & ~np.isfinite(t), np.where(tn > 0, tn, np.inf), t), np.where(edge, np.inf, t)


class _Tris:
    """The scene's triangles, prepared once."""

    def __init__(self, v):
        self.v = v
        nn = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
        nlen = np.linalg.norm(nn, axis=1)
        self.good = np.isfinite(nlen) & (nlen > 0)
        self.nh = nn / np.where(self.good, nlen, 1.0)[:, None]
        self.edges = np.stack([v[:, 1] - v[:, 0], v[:, 2] - v[:, 1], v[:, 0] - v[:, 2]], axis=1)   # (T, 3, 3)
        self.emax = np.linalg.norm(self.edges, axis=2).max(axis=1)
        self.vmax = np.abs(v).max(axis=(1, 2))


def _f64_triangles(T, o, d):
    """Moeller-Trumbore with the reference's edge slack as part of the shape
    (n^ . (edge x (p - v)) >= -0.1 EPSILON, triangle.rs:41-45): (m, T) arrays.
    The edge functions are evaluated in f32 by the reference, with an error of
    at most band = 2^-22 |edge| (|o| + |t d| + |v|) (three products and two sums
    of such magnitudes, doubled): within the band of the slack either verdict
    is right. t itself: the f32 numerator n.v0 - n.o is off by up to t_err =
    2^-21 sum |n_i| (|v0_i| + |o_i|) / |n.d|, so a plane that close to the
    origin may be behind it for the reference (t <= 0: no hit)."""
    nh, v = T.nh, T.v
    nd = d @ nh.T
    t = (np.einsum("tc,tc->t", nh, v[:, 0])[None, :] - o @ nh.T) / nd
    p = o[:, None, :] + t[:, :, None] * d[:, None, :]                     # (m, T, 3)
    emin = np.full(t.shape, np.inf)
    for k in range(3):
        emin = np.minimum(emin, np.einsum("tc,mtc->mt", nh, np.cross(T.edges[None, :, k, :], p - v[None, :, k, :])))
    reach = np.abs(o).max(axis=1)[:, None] + np.abs(t) * np.abs(d).max(axis=1)[:, None] + T.vmax[None, :]
    band = 2.0 ** -22 * T.emax[None, :] * reach
    valid = T.good[None, :] & np.isfinite(t) & (t > 0) & (nd != 0)
    t_err = 2.0 ** -21 * (np.einsum("tc,tc->t", np.abs(nh), np.abs(v[:, 0]))[None, :] + np.abs(o) @ np.abs(nh).T) / np.abs(nd)
    return (np.where(valid & (emin >= -TRI_SLACK - band), t, np.inf),
            np.where(valid & (emin >= -TRI_SLACK + band) & (t > t_err), t + t_err, np.inf))


def _forward_units(sh, kinds, wid, o, d, t64):
    """The f32 forward-error unit of a plane's or triangle's t = n.(v0 - o) / n.d:
    U32 (sum |n_i| (|v0_i| + |o_i|) + t sum |n_i d_i|) / |n.d|, the size of one
    rounding of the numerator's and the denominator's terms carried to t. For
    other shapes U32 t. |t - t64| in these units is `fwd`."""
    v0 = sh[wid, :3]
    nw = np.where((kinds[wid] == KIND_PLANE)[:, None], sh[wid, 3:6],
                  np.cross(sh[wid, 3:6] - sh[wid, :3], sh[wid, 6:9] - sh[wid, :3]))
    flat = (kinds[wid] == KIND_TRI) | (kinds[wid] == KIND_PLANE)
    with np.errstate(all="ignore"):
        an = np.abs(nw)
        unit = U32 * (np.einsum("ij,ij->i", an, np.abs(v0) + np.abs(o)) + t64 * np.einsum("ij,ij->i", an, np.abs(d))) \
            / np.abs(np.einsum("ij,ij->i", nw, d))
    return np.where(flat & np.isfinite(unit), unit, U32 * t64)


def f64_check(shapes, rays, t_o, id_o, tol, forward=None, chunk=128):
    """The oracle's (t, id) against an f64 brute force written from the geometry
    (the helpers above). Per ray, (ok, rel, fwd, self):
      * ok: the oracle's id is a possible hit of that shape; no sure hit is
        certainly closer (below t (1 - tol) even at the largest t the f32
        arithmetic may give it); an oracle miss has no sure hit at all; and t is
        within the bound: rel <= tol, or, if `forward` is given, fwd <= forward;
      * rel = |t - t64[id]| / t64[id], plain (0 for a miss);
      * fwd = |t - t64[id]| in the units of _forward_units;
      * self: t64 was taken from the oracle's own t (_f64_sphere), so rel is 0
        by construction and the ray checks the id and the window only.
    An f32 t that overflowed to +inf (a plane met through a denormal direction
    component) stands for any f64 t above the f32 range."""
    sh = np.asarray(shapes, np.float64)
    kinds = sh[:, 12].astype(int)
    r = np.asarray(rays, F32).astype(np.float64).reshape(-1, 6)
    n = len(r)
    ok, rel, fwd, selfref = np.zeros(n, bool), np.zeros(n), np.zeros(n), np.zeros(n, bool)
    tri = np.nonzero(kinds == KIND_TRI)[0]
    T = _Tris(sh[tri, :9].reshape(-1, 3, 3))
    for c0 in range(0, n, chunk):
        o, d = r[c0: c0 + chunk, :3], r[c0: c0 + chunk, 3:]
        m = len(o)
        tt = t_o[c0: c0 + m].astype(np.float64)
        ids = id_o[c0: c0 + m]
        sure = np.full((m, len(sh)), np.inf)
        poss = np.full((m, len(sh)), np.inf)
        own = np.zeros((m, len(sh)), bool)
        with np.errstate(all="ignore"):
            for j in np.nonzero(kinds == KIND_PLANE)[0]:
                poss[:, j], sure[:, j] = _f64_plane(sh[j, :3], sh[j, 3:6], o, d)
            for j in np.nonzero(kinds == KIND_SPHERE)[0]:
                poss[:, j], sure[:, j], own[:, j] = _f64_sphere(sh[j, :3], sh[j, 3], o, d, tt)
            for j in np.nonzero(kinds == KIND_AARECT)[0]:
                poss[:, j], sure[:, j] = _f64_aarect(sh[j, [0, 2, 4]], sh[j, [1, 3, 5]], o, d)
            poss[:, tri], sure[:, tri] = _f64_triangles(T, o, d)
        smin = sure.min(axis=1)
        miss = ids < 0
        ok[c0: c0 + m][miss] = ~np.isfinite(smin[miss])
        h = np.nonzero(~miss)[0]
        t64 = poss[h, ids[h]]
        selfref[c0 + h] = own[h, ids[h]]
        over = np.isinf(tt[h]) & (t64 > FLT_MAX) & np.isfinite(t64)
        with np.errstate(invalid="ignore"):
            err = np.where(over, 0.0, np.abs(tt[h] - t64))
            rl = err / t64
            fw = err / _forward_units(sh, kinds, ids[h], o[h], d[h], t64)
        rl = np.where(np.isfinite(rl), rl, np.inf)
        fw = np.where(np.isfinite(fw), fw, np.inf)
        rel[c0 + h], fwd[c0 + h] = rl, fw
        closer = smin[h] < np.where(np.isinf(tt[h]), FLT_MAX, tt[h] * (1 - tol))
        within = rl <= tol if forward is None else fw <= forward
        ok[c0 + h] = np.isfinite(t64) & within & ~closer
    return ok, rel, fwd, selfref
