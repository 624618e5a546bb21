"""Fixtures of the PNEE light-sampler suites (test_pnee_cpu.py,
test_gpu_pnee.py): deterministic builders, no I/O.

A photon list is (light u32 (n,), location f32 (n, 3), intensity f32 (n,)) in
insertion order. Point sets and RNG states are built per tree from its own
frozen arrays (child, cum of wpt_photon_build / wpt_photon_tree), through a
numpy f32 restatement of the octree descent (`descend`, `plan`) that the CPU
suite checks against the oracle's leaf query.
"""
import functools

import numpy as np

F = np.float32
SIZE = F(1024.0)
MAX_IN_CELL = 1024
HALF = F(0.5)
INV32 = F(1.0) / F(4294967296.0)  # rng.rs:19-21: 1.0 / (0xFFFFFFFF as f32)


# ---------------------------------------------------------------------------
# Photon lists
# ---------------------------------------------------------------------------
def _ball(rng, n, centre, radius):
    """n points within `radius` of `centre` (f32), none beyond it in any axis."""
    d = rng.uniform(-1.0, 1.0, (n, 3))
    return (np.asarray(centre, np.float64) + d * radius).astype(F)


def _cluster(rng, centre, radius, num_lights, n=1100, lights=None):
    loc = _ball(rng, n, centre, radius)
    if lights is None:
        lights = rng.choice(num_lights, size=min(num_lights, 3), replace=False)
    p = rng.dirichlet(np.ones(len(lights)))
    li = rng.choice(lights, size=n, p=p).astype(np.uint32)
    return li, loc, rng.uniform(0.1, 2.0, n).astype(F)


def _background(rng, n, num_lights):
    return (rng.integers(0, num_lights, n).astype(np.uint32), rng.uniform(-1000.0, 1000.0, (n, 3)).astype(F),
            rng.uniform(0.1, 2.0, n).astype(F))


def _join(parts):
    return (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]),
            np.concatenate([p[2] for p in parts]))


def octants():
    """1025 photons, one split of the root. Octant c (bit 2 x, bit 1 y, bit 0
    z high) holds 128 photons of which 14 * (c + 1) are of light 1, so the
    eight CDFs differ along every axis by far more than rounding."""
    rng = np.random.default_rng(0x0C7A)
    li, loc = [], []
    for c in range(8):
        n = 128 + (1 if c == 0 else 0)
        sign = np.array([1.0 if c & 4 else -1.0, 1.0 if c & 2 else -1.0, 1.0 if c & 1 else -1.0])
        loc.append((rng.uniform(100.0, 900.0, (n, 3)) * sign).astype(F))
        l = np.zeros(n, np.uint32)
        l[: 14 * (c + 1)] = 1
        li.append(rng.permutation(l))
    order = rng.permutation(1025)
    return np.concatenate(li)[order], np.concatenate(loc)[order], np.ones(1025, F)


# cluster radius 2^-k -> leaves at depth about 10 + k (cells of side 2^(11-d))
DEEP_K = (9, 10, 11, 12, 14, 17, 21, 22)


def deep():
    """Clusters of 1100 photons in balls of radius 2^-k: around small
    coordinates (k up to 22: leaves below depth 30) and around coordinates
    near 1000 (k up to 12; the f32 spacing there is 2^-14). Each ball touches,
    from below, a plane whose coordinate is a power of two in one axis, so the
    leaves under that plane have a far face where v + size rounds up."""
    rng = np.random.default_rng(0xDEE9)
    parts = [_background(rng, 1500, 2)]
    for i, k in enumerate(DEEP_K):
        r = 2.0 ** -k
        c = [0.3 + 0.01 * i, -0.3 - 0.02 * i, 0.3 + 0.03 * i]
        c[i % 3] = (0.25, 0.5, 0.125)[i % 3] - r
        parts.append(_cluster(rng, c, r, 2))
    for i, k in enumerate(DEEP_K[:4]):
        r = 2.0 ** -k
        c = [1000.3 - 3.0 * i, -1000.7 + 5.0 * i, 900.1 + 7.0 * i]
        c[(i + 1) % 3] = 512.0 - r
        parts.append(_cluster(rng, c, r, 2))
    return _join(parts)


COLLAPSED_AT = (0.3, -7.25, 100.1)


def collapsed():
    """1100 identical photons: the split chain runs to the depth-120 guard
    and the cell bounds collapse to single f32 values on the way."""
    rng = np.random.default_rng(0xC011)
    n = 1100
    loc = np.tile(np.asarray(COLLAPSED_AT, F), (n, 1))
    li = (np.arange(n) % 3 == 0).astype(np.uint32)
    return _join([_background(rng, 600, 2), (li, loc, rng.uniform(0.1, 2.0, n).astype(F))])


def walls():
    """Clusters against the root box's faces, edges and one corner (their
    leaves' neighbour indices clamp at 0 and at `last`), and a few photons
    outside +-1024, which the reference inserts."""
    rng = np.random.default_rng(0x3A11)
    parts = [_background(rng, 1200, 2)]
    r = 0.125
    e = 1024.0 - r
    for c in ([e, 3.0, -200.0], [-e, 700.0, 11.0], [5.0, e, 60.0], [-300.0, -e, 5.0], [40.0, -9.0, e], [7.0, 100.0, -e],
              [e, e, 300.0], [-e, 20.0, -e], [-e, -e, -e], [e, -e, e]):
        li, loc, it = _cluster(rng, c, r, 2)
        parts.append((li, np.clip(loc, -SIZE, SIZE), it))
    out = np.array([[1500.0, 3.0, 4.0], [-2000.0, 1.0, 1.0], [1.0e6, -1.0e6, 5.0], [0.0, 1024.5, 0.0],
                    [3.0, 4.0, -1025.0], [1e30, 1e30, 1e30]], F)
    parts.append((np.array([0, 1, 0, 1, 1, 0], np.uint32), out, np.ones(6, F)))
    return _join(parts)


def wide():
    """72 tight clusters (radius 2^-10, leaves near depth 20), half of them
    in the part of the box the stock scenes occupy, half scattered over the
    whole box (fewer shared ancestors): more than 6144 nodes, so a
    session reads the tree from global memory (view 0) while every leaf still
    has a corner-table row."""
    rng = np.random.default_rng(0x31DE)
    parts = [_background(rng, 1000, 2)]
    for i in range(72):
        span = 12.0 if i % 2 == 0 else 900.0
        parts.append(_cluster(rng, rng.uniform(-span, span, 3), 2.0 ** -10, 2))
    return _join(parts)


def many_lights():
    """A list for scene 0's 108 lights: 24 clusters of three lights each."""
    rng = np.random.default_rng(0x0108)
    parts = [_background(rng, 3000, 108)]
    for i in range(24):
        parts.append(_cluster(rng, rng.uniform(-20.0, 20.0, 3), 2.0 ** -(i % 4), 108))
    return _join(parts)


def weights_mild():
    """Intensities 0, -0.0, denormals and small negative values among ones:
    every bin stays positive and finite."""
    rng = np.random.default_rng(0x3E16)
    parts = [_background(rng, 800, 2)]
    for i in range(4):
        parts.append(_cluster(rng, rng.uniform(-50.0, 50.0, 3), 0.5, 2))
    li, loc, it = _join(parts)
    vals = np.array([0.0, -0.0, 1e-40, 1.4e-45, -2.0 ** -10, 1.0, 1.0, 0.5], F)
    return li, loc, vals[rng.integers(0, len(vals), len(it))]


def weights_wild():
    """Intensities of 1e30 (bin sums overflow: CDFs turn inf / NaN), large
    negative values (negative bins, CDFs that are not monotone) and -1e30."""
    rng = np.random.default_rng(0x371D)
    parts = [_background(rng, 800, 2)]
    for i in range(4):
        parts.append(_cluster(rng, rng.uniform(-50.0, 50.0, 3), 0.5, 2))
    li, loc, it = _join(parts)
    vals = np.array([1e30, 1e30, -1e30, -3.0, 1.0, 0.0, 3e38, 1e-40], F)
    return li, loc, vals[rng.integers(0, len(vals), len(it))]


# name -> (light count, builder); the 2-light trees run on scene 100 sessions,
# the 108-light tree on a scene 0 session
TREES = {
    "octants": (2, octants), "deep": (2, deep), "collapsed": (2, collapsed), "walls": (2, walls), "wide": (2, wide),
    "many_lights": (108, many_lights), "weights_mild": (2, weights_mild), "weights_wild": (2, weights_wild),
}
# trees whose arithmetic leaves the finite, well-conditioned range
WILD_TREES = ("collapsed", "weights_wild")


# ---------------------------------------------------------------------------
# xorshift32 (rng.rs:40-47), forwards and backwards
# ---------------------------------------------------------------------------
def xs_step(s):
    x = np.asarray(s, np.uint32).copy()
    x ^= x << np.uint32(13)
    x ^= x >> np.uint32(17)
    x ^= x << np.uint32(5)
    return x


def xs_unstep(s):
    x = np.asarray(s, np.uint32).copy()
    x ^= x << np.uint32(5); x ^= x << np.uint32(10); x ^= x << np.uint32(20)   # undo x ^= x << 5
    x ^= x >> np.uint32(17)                                                      # undo x ^= x >> 17
    x ^= x << np.uint32(13); x ^= x << np.uint32(26)                           # undo x ^= x << 13
    return x


def draws(states, k=4):
    """The first k draws of Rng::next from each state: (k, n) f32."""
    out, s = [], np.asarray(states, np.uint32)
    for _ in range(k):
        s = xs_step(s)
        out.append(s.astype(F) * INV32)
    return np.stack(out)


def state_before(u, k):
    """The state whose k-th output word is u (u != 0)."""
    s = np.asarray(u, np.uint32)
    for _ in range(k):
        s = xs_unstep(s)
    return s


def word_of(x):
    """The u32 word whose draw is exactly the f32 x, and whether one exists
    (x in (0, 1] with x * 2^32 an integer; 1.0 is drawn from 0xFFFFFFFF)."""
    x = np.asarray(x, F)
    with np.errstate(invalid="ignore", over="ignore"):
        y = x.astype(np.float64) * 4294967296.0
        ok = np.isfinite(y) & (y >= 1.0) & (y <= 4294967296.0) & (y == np.floor(y))
        u = np.where(ok, np.minimum(np.where(ok, y, 1.0), 4294967295.0), 1.0).astype(np.uint32)
    return u, ok


# ---------------------------------------------------------------------------
# The octree descent in numpy f32 (child(): photon_tree.rs:234-256)
# ---------------------------------------------------------------------------
def descend(child, pts, max_depth=None):
    """find_leaf (max_depth None) / find_node_cdf (depth limit per point):
    (node, depth, bounds (n, 6) = mins then maxes)."""
    pts = np.asarray(pts, F).reshape(-1, 3)
    n = len(pts)
    node = np.zeros(n, np.int64)
    depth = np.zeros(n, np.int32)
    b = np.tile(np.array([-SIZE] * 3 + [SIZE] * 3, F), (n, 1))
    lim = np.full(n, 1 << 30, np.int32) if max_depth is None else np.asarray(max_depth, np.int32)
    bits = np.array([4, 2, 1])
    with np.errstate(invalid="ignore", over="ignore"):
        while True:
            idx = np.nonzero((child[node] != 0) & (depth < lim))[0]
            if len(idx) == 0:
                break
            lo, hi = b[idx, :3], b[idx, 3:]
            c = HALF * (lo + hi)
            lt = pts[idx] < c
            b[idx, :3] = np.where(lt, lo, c)
            b[idx, 3:] = np.where(lt, c, hi)
            node[idx] = child[node[idx]].astype(np.int64) + np.where(lt, 0, bits).sum(axis=1)
            depth[idx] += 1
    return node, depth, b


def preorder(child):
    """Node ids in pre-order (node, then children 0..7) of a child array."""
    order, stack = [], [0]
    while stack:
        n = stack.pop()
        order.append(n)
        if child[n]:
            stack.extend(range(int(child[n]) + 7, int(child[n]) - 1, -1))
    return np.array(order)


class Plan:
    pass


def plan(child, pts):
    """What PhotonTree::sample (photon_tree.rs:80-159) derives from a point
    before it draws: leaf, depth, bounds, the per-axis weights and offsets, the
    8 cells of the mix (corner c: bit 2 x, bit 1 y, bit 0 z shifted), all in
    f32 as the reference computes them."""
    P = Plan()
    pts = np.asarray(pts, F).reshape(-1, 3)
    P.pts = pts
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        P.outside = np.any((pts < -SIZE) | (pts > SIZE), axis=1)
        P.leaf, P.depth, P.bounds = descend(child, pts)
        lo, hi = P.bounds[:, :3], P.bounds[:, 3:]
        size = hi - lo
        P.size = size
        P.high = pts > HALF * (lo + hi)
        left = (hi - (pts - size * HALF)) / size
        right = ((pts + size * HALF) - lo) / size
        P.w = np.where(P.high, left, right).astype(F)
        P.wadj = (F(1.0) - P.w).astype(F)
        P.off = np.where(P.high, F(1.0), F(-1.0)).astype(F)
        aj = (size * P.off).astype(F)
        P.shifted = (pts + aj).astype(F)
        P.corner = np.empty((len(pts), 8), np.int64)
        for c in range(8):
            sel = np.array([bool(c & 4), bool(c & 2), bool(c & 1)])
            q = np.where(sel, P.shifted, pts).astype(F)
            P.corner[:, c] = descend(child, q, P.depth)[0]
        # the neighbour index clamps: the adjacent cell lies outside the root box
        P.clamped = np.where(P.high, hi == SIZE, lo == -SIZE)
        # the shifted coordinate is not in the adjacent cell [hi, hi + size) or
        # [lo - size, lo) although that cell lies inside the root box
        in_adj = np.where(P.high, (P.shifted >= hi) & (P.shifted < hi + size),
                          (P.shifted >= lo - size) & (P.shifted < lo))
        P.escaped = ~in_adj & ~P.clamped & np.isfinite(pts)
    return P


def pick_node(P, d3):
    """The cell whose CDF is sampled, from the three self draws d3 (3, n)."""
    with np.errstate(invalid="ignore"):
        self_ = d3.T <= P.w
    pick = (~self_[:, 0]) * 4 + (~self_[:, 1]) * 2 + (~self_[:, 2]) * 1
    return P.corner[np.arange(len(pick)), pick], self_


# ---------------------------------------------------------------------------
# Point sets
# ---------------------------------------------------------------------------
def _ulp_up(x):
    return np.nextafter(np.asarray(x, F), F(np.inf))


def _ulp_dn(x):
    return np.nextafter(np.asarray(x, F), F(-np.inf))


def point_sets(child, photons, seed):
    """name -> (n, 3) f32 points for the tree `child` built from `photons`."""
    rng = np.random.default_rng(seed)
    loc = photons[1]
    sets = {}
    # random: half uniform in the root box and around photons, half in the same
    # leaves but drawn towards the faces (per axis the distance to the nearer
    # face is u^3 / 2 of the cell), so that "every axis samples the adjacent
    # cell", which a uniform point does with probability 1/64, is not rare
    base = np.concatenate([rng.uniform(-1024.0, 1024.0, (600, 3)).astype(F), _near(rng, loc, 1400)])
    _, _, b = descend(child, base)
    u = rng.uniform(0.0, 1.0, base.shape)
    q = np.where(rng.integers(0, 2, base.shape) == 1, 1.0 - 0.5 * u ** 3, 0.5 * u ** 3)
    biased = (b[:, :3].astype(np.float64) * (1.0 - q) + b[:, 3:].astype(np.float64) * q).astype(F)
    biased = np.clip(biased, b[:, :3], b[:, 3:])
    sets["random"] = np.concatenate([base, biased])
    # leaves reached by those points, each once, deepest first
    node, depth, b = descend(child, sets["random"])
    _, first = np.unique(node, return_index=True)
    first = first[np.argsort(-depth[first], kind="stable")][:600]
    if len(first) < 150:  # a tree of few leaves: each several times, with other random coordinates
        first = np.resize(first, 150)
    lb, ld = b[first], depth[first]
    lo, hi = lb[:, :3], lb[:, 3:]
    inner = lambda: (lo + (hi - lo) * rng.uniform(0.05, 0.95, lo.shape).astype(F)).astype(F)  # noqa: E731
    ctr = (HALF * (lo + hi)).astype(F)
    # centres: v > center is a tie in all three axes, or in one
    cs = [ctr]
    for a in range(3):
        p = inner()
        p[:, a] = ctr[:, a]
        cs.append(p)
    sets["centres"] = np.concatenate(cs)
    # faces: on a face, and one ulp either side
    fs, far = [], []
    for a in range(3):
        for face in (lo, hi):
            for step in (lambda x: x, _ulp_dn, _ulp_up):
                p = inner()
                p[:, a] = step(face[:, a])
                fs.append(p[:200])
        # one ulp inside the far face of the deepest leaves: v + size may round
        # past the adjacent cell
        for rep in range(3):
            p = inner()
            p[:, a] = _ulp_dn(hi[:, a])
            far.append(p)
            p = inner()
            p[:, a] = lo[:, a]
            far.append(p[:100])
    sets["faces"] = np.concatenate(fs)
    sets["far_face"] = np.concatenate(far)
    # the root box's faces: +-1024 exactly and one ulp outside; +-0.0
    edge = np.array([1024.0, -1024.0, _ulp_up(F(1024.0)), _ulp_dn(F(-1024.0)), _ulp_dn(F(1024.0)), _ulp_up(F(-1024.0))], F)
    p = rng.uniform(-1000.0, 1000.0, (216, 3)).astype(F)
    g = np.stack(np.meshgrid(edge, edge, edge, indexing="ij"), -1).reshape(-1, 3)
    root = [g]
    for a in range(3):
        q = p.copy()
        q[:, a] = edge[np.arange(216) % 6]
        root.append(q)
    sets["root_faces"] = np.concatenate(root)
    z = np.array([0.0, -0.0], F)
    g = np.stack(np.meshgrid(z, z, z, indexing="ij"), -1).reshape(-1, 3)
    q = rng.uniform(-1.0, 1.0, (96, 3)).astype(F)
    q[np.arange(96), np.arange(96) % 3] = z[(np.arange(96) // 3) % 2]
    sets["zeros"] = np.concatenate([g, q])
    # far outside, +-inf and NaN in one component (a plane met through a
    # denormal direction component has t = +inf and a NaN hit point)
    sp = rng.uniform(-900.0, 900.0, (120, 3)).astype(F)
    vals = np.array([np.inf, -np.inf, np.nan, 1e30, -1e30, 2048.0], F)
    sp[np.arange(120), np.arange(120) % 3] = vals[(np.arange(120) // 3) % 6]
    near = _near(rng, loc, 60)
    near[np.arange(60), np.arange(60) % 3] = F(np.nan)
    sets["special"] = np.concatenate([sp, near])
    return sets


def _near(rng, loc, n):
    """Points around photons: half of them a photon moved by up to 2^-6 ..
    2^-26 per axis, half a random point of the box spanned by a photon and the
    next one of the list (for a cluster's photons: within the cluster)."""
    i = rng.integers(0, len(loc) - 1, n)
    p = loc[i].astype(np.float64)
    r = 2.0 ** -rng.integers(6, 27, (n, 1))
    moved = p + rng.uniform(-1.0, 1.0, (n, 3)) * r
    between = p + (loc[i + 1].astype(np.float64) - p) * rng.uniform(0.0, 1.0, (n, 3))
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.where((np.arange(n) % 2 == 0)[:, None] | ~np.isfinite(between), moved, between)
    return np.clip(q, -1024.0, 1024.0).astype(F)


# point sets whose points sit on a comparison's tie or outside finite arithmetic
TIE_SETS = ("centres", "faces", "far_face", "root_faces", "zeros", "special")


# ---------------------------------------------------------------------------
# RNG states
# ---------------------------------------------------------------------------
def random_states(n, seed):
    s = np.random.default_rng(seed).integers(1, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    return s


def tie_states(child, cum, pts, seed):
    """class -> (points, states): states whose k-th draw is exactly 0 (state
    0: every draw), exactly 1.0, exactly the point's k-th weight, or exactly an
    entry of the CDF the fourth draw is searched in."""
    rng = np.random.default_rng(seed)
    pts = np.asarray(pts, F).reshape(-1, 3)
    P = plan(child, pts)
    ok = ~P.outside & np.all(np.isfinite(pts), axis=1)
    pts, idx = pts[ok], np.nonzero(ok)[0]
    out = {"zero": (pts[:200], np.zeros(min(200, len(pts)), np.uint32))}
    for k in (1, 2, 3, 4):
        u = (np.uint32(0xFFFFFF80) + rng.integers(0, 128, len(pts)).astype(np.uint32)).astype(np.uint32)
        out[f"one{k}"] = (pts[:200], state_before(u, k)[:200])
    for k in (1, 2, 3):
        u, good = word_of(P.w[idx, k - 1])
        out[f"weight{k}"] = (pts[good], state_before(u[good], k))
    # CDF entries: per candidate cell of the mix, the state whose fourth draw is
    # an entry of that cell's CDF; kept if its first three draws pick that cell
    L = cum.shape[1]
    got_p, got_s = [], []
    left = np.ones(len(pts), bool)
    for c in rng.permutation(8):
        node = P.corner[idx, c]
        j = rng.integers(1, L, len(pts))
        u, good = word_of(cum[node, j])
        s0 = state_before(u, 4)
        sampled, _ = pick_node(_sub(P, idx), draws(s0, 3))
        hit = good & left & (sampled == node)
        got_p.append(pts[hit])
        got_s.append(s0[hit])
        left &= ~hit
    out["cdf"] = (np.concatenate(got_p), np.concatenate(got_s))
    return out


def _sub(P, idx):
    Q = Plan()
    Q.w, Q.corner = P.w[idx], P.corner[idx]
    return Q


def tie_class_counts(child, cum, ties):
    """How many (point, state) pairs of each class of tie_states really are the
    tie they were built for, recomputed from the states."""
    counts = {}
    for name, (pts, st) in ties.items():
        P = plan(child, pts)
        d = draws(st, 4)
        if name == "zero":
            counts[name] = int(np.sum(np.all(d == 0.0, axis=0)))
        elif name.startswith("one"):
            counts[name] = int(np.sum(d[int(name[3:]) - 1] == 1.0))
        elif name.startswith("weight"):
            k = int(name[6:]) - 1
            counts[name] = int(np.sum(d[k] == P.w[:, k]))
        else:
            node, _ = pick_node(P, d[:3])
            counts[name] = int(np.sum(np.any(cum[node, 1:] == d[3][:, None], axis=1)))
    return counts


# ---------------------------------------------------------------------------
# Built once per tree and shared, read-only, by both suites
# ---------------------------------------------------------------------------
SCENE_OF_LIGHTS = {2: 100, 108: 0}


@functools.lru_cache(maxsize=None)
def tree(name):
    """The photon list `name`, its frozen arrays from the host builder
    (wpt_photon_build), its point sets and tie states."""
    import wpt_loader
    itf = wpt_loader.load().interface
    L, build = TREES[name]
    T = Plan()
    T.name, T.L, T.photons = name, L, build()
    T.child, T.cum, T.corners = itf.photon_build(L, T.photons)
    T.sets = point_sets(T.child, T.photons, seed=0x5E75)
    T.ties = tie_states(T.child, T.cum, T.sets["random"], seed=0x71E5)
    for a in (T.child, T.cum, T.corners, *T.photons, *T.sets.values()):
        a.setflags(write=False)
    return T


@functools.lru_cache(maxsize=None)
def _oracle_scene(num_lights):
    import pyoracle
    o = pyoracle.OracleScene(SCENE_OF_LIGHTS[num_lights])
    assert o.num_lights == num_lights
    return o


def oracle_with(T):
    """The oracle scene of the tree's light count, holding the tree's list."""
    o = _oracle_scene(T.L)
    o.set_photons(T.photons)
    return o
