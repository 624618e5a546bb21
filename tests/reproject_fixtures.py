"""Frames and a numpy restatement for the reprojection of a kept frame
(wpt_reproject, wpt_reproject_planes, wpt_reproject_host).

A plain helper module (no pytest hooks): tests/test_reproject_cpu.py holds
wpt_reproject_host against numpy_reproject below, tests/test_gpu_reproject.py
holds the device against wpt_reproject_host on the same frames. numpy_reproject
is written from the definition, independent of the C++: every
operation is one numpy f32 operation on whole planes, in the order the
definition gives; the cosines and sines of the history's camera come from the
oracle (oracle_cosf / oracle_sinf), as first_hit_fixtures.numpy_primary_rays
takes them. It also says why each pixel and each tap was rejected.

The planes are synthetic: the primary rays (wpt_primary_rays) of two cameras
against a floor, a back wall with an emissive panel and a box in front of it,
intersected in numpy. They need not be exact hits: they are inputs. On top of
them sit the edits that put a value on each decision of the definition. Frames
are made once per process and shared; nothing returned here is modified.
"""
import numpy as np

F32 = np.float32
KEEP, NEAREST, SAME_SHAPE = 1, 2, 4  # WPT_REPROJECT_*
FLAGS = (0, NEAREST, SAME_SHAPE, NEAREST | SAME_SHAPE)
SEED = 0xBABABEBE
COS_MIN, EPS_Z, MAX_LEN = F32(0.9), F32(0.05), 64
CPU_VIEWPORTS = ((1, 1), (3, 2), (17, 16), (37, 5), (33, 33), (64, 48))
GPU_VIEWPORTS = CPU_VIEWPORTS + ((130, 70),)  # more than one block each way, a ragged last block
# the history's camera, then the current one
CAM_A = (0.0, 1.5, -4.0, 0.0, 0.0)
PAIRS = {
    "identical": (CAM_A, CAM_A),
    "sideways": (CAM_A, (0.4, 1.5, -4.0, 0.0, 0.0)),
    "dolly": (CAM_A, (0.0, 1.5, -3.2, 0.0, 0.0)),
    "rot_y+": (CAM_A, (0.0, 1.5, -4.0, 0.0, 0.1)),
    "rot_y-": (CAM_A, (0.0, 1.5, -4.0, 0.0, -0.1)),
    "rot_x_move": (CAM_A, (0.2, 1.6, -3.9, 0.05, 0.0)),
    "half_turn": (CAM_A, (0.0, 1.5, -4.0, 0.0, 3.14159274)),  # looks away: every hit is behind the history's camera
}
# why a pixel passed through (0: it was merged)
PIX_MERGED, PIX_MISS, PIX_SUM, PIX_BEHIND, PIX_WINDOW, PIX_NO_TAP = range(6)
# why a tap was skipped (0: accepted; -1: never looked at), in the definition's order
TAP_OK, TAP_OUTSIDE, TAP_EMPTY, TAP_KIND, TAP_SHAPE, TAP_NORMAL, TAP_DEPTH, TAP_WEIGHT, TAP_MEAN = range(9)


def trig(oracle, pcam):
    """make_view's cos / sin of the history's rot_x, rot_y: (cx, sx, cy, sy)."""
    L = oracle.lib()
    rx, ry = float(F32(pcam[3])), float(F32(pcam[4]))
    return F32(L.oracle_cosf(rx)), F32(L.oracle_sinf(rx)), F32(L.oracle_cosf(ry)), F32(L.oracle_sinf(ry))


def project(tr, w, h, cam, pcam, dirs, t):
    """World point and previous view: (u, v, te, in front, inside the window)."""
    cx, sx, cy, sy = tr
    dirs, t = np.asarray(dirs, F32), np.asarray(t, F32)
    fw, fh = F32(w), F32(h)
    ar = fw / fh
    with np.errstate(all="ignore"):
        d = [(F32(cam[k]) + t * dirs[..., k]) - F32(pcam[k]) for k in range(3)]
        te = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        v1x, v1y, v1z = cy * d[0] - sy * d[2], d[1], sy * d[0] + cy * d[2]
        v2x, v2y, v2z = v1x, cx * v1y + sx * v1z, (-sx) * v1y + cx * v1z
        front = v2z > F32(0.0)
        k = F32(0.8) / v2z
        u = ((v2x * k) / ar + F32(0.5)) * fw - F32(0.5)
        v = (F32(0.5) - v2y * k) * fh - F32(0.5)
        inwin = (u > F32(-1.0)) & (u < fw) & (v > F32(-1.0)) & (v < fh)
    assert u.dtype == F32 and te.dtype == F32
    return u, v, te, front, inwin


def numpy_reproject(tr, cam, cur, pcam, hist, cos_min, eps_z, max_len, flags):
    """The definition in numpy f32: (acc (H, W, 3), cnt, len, info). info: 'pix'
    (H, W) the PIX_* reason, 'tap' (H, W, taps) the TAP_* reason, and per tap
    'dot', 'dz', 'lim' (the two sides of the normal and depth tests), 'u', 'v'."""
    acc, cnt, dirs, t, ids, n, kind = cur
    hacc, hcnt, ht, hid, hn, hkind = hist
    acc, n, hacc, hn, ht = (np.asarray(a, F32) for a in (acc, n, hacc, hn, ht))
    h, w = cnt.shape
    one, zero = F32(1.0), F32(0.0)
    cos_min, eps_z = F32(cos_min), F32(eps_z)
    with np.errstate(all="ignore"):
        u, v, te, front, inwin = project(tr, w, h, cam, pcam, dirs, t)
        pix = np.zeros((h, w), np.int8)
        live = np.ones((h, w), bool)
        for why, cond in ((PIX_MISS, kind == 0), (PIX_SUM, ~np.isfinite(acc).all(-1)), (PIX_BEHIND, ~front),
                          (PIX_WINDOW, ~inwin)):
            pix[live & cond] = why
            live &= ~cond
        us, vs = np.where(live, u, zero), np.where(live, v, zero)  # the guard in front of the conversions
        if flags & NEAREST:
            taps = [(np.floor(us + F32(0.5)).astype(np.int64), np.floor(vs + F32(0.5)).astype(np.int64),
                     np.ones((h, w), F32))]
        else:
            x0, y0 = np.floor(us), np.floor(vs)
            fx, fy = us - x0, vs - y0
            gx, gy = one - fx, one - fy
            ix, iy = x0.astype(np.int64), y0.astype(np.int64)
            taps = [(ix, iy, gx * gy), (ix + 1, iy, fx * gy), (ix, iy + 1, gx * fy), (ix + 1, iy + 1, fx * fy)]
        hmean = hacc / hcnt.astype(F32)[..., None]
        s3 = np.zeros((h, w, 3), F32)
        sw = np.zeros((h, w), F32)
        lmin = np.full((h, w), 0xFFFFFFFF, np.uint32)
        info = {k: np.zeros((h, w, len(taps)), F32) for k in ("dot", "dz", "lim")}
        tap = np.full((h, w, len(taps)), -1, np.int8)
        for j, (qx, qy, wt) in enumerate(taps):
            inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
            cy_, cx_ = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
            nq = hn[cy_, cx_]
            dot = (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2]
            dz = np.abs(ht[cy_, cx_] - te)
            lim = eps_z * te
            cq = hmean[cy_, cx_]
            why = np.zeros((h, w), np.int8)
            for code, bad in ((TAP_MEAN, ~np.isfinite(cq).all(-1)), (TAP_WEIGHT, ~(wt > zero)), (TAP_DEPTH, ~(dz <= lim)),
                              (TAP_NORMAL, ~(dot >= cos_min)),
                              (TAP_SHAPE, (hid[cy_, cx_] != ids) if flags & SAME_SHAPE else np.zeros((h, w), bool)),
                              (TAP_KIND, hkind[cy_, cx_] != kind), (TAP_EMPTY, hcnt[cy_, cx_] == 0),
                              (TAP_OUTSIDE, ~inside)):
                why[bad] = code  # the last one written is the first in the definition's order
            tap[..., j] = np.where(live, why, -1)
            use = live & (why == TAP_OK)
            s3 = np.where(use[..., None], s3 + wt[..., None] * cq, s3)
            sw = np.where(use, sw + wt, sw)
            lmin = np.where(use, np.minimum(lmin, hcnt[cy_, cx_]), lmin)
            info["dot"][..., j], info["dz"][..., j], info["lim"][..., j] = dot, dz, lim
        got = live & (sw > zero)
        pix[live & ~got] = PIX_NO_TAP
        hm = s3 / sw[..., None]
        room = np.uint32(0xFFFFFFFF) - cnt
        ln = np.minimum(np.minimum(lmin, np.uint32(max_len)), room)
        ln = np.where(got, ln, 0).astype(np.uint32)
        merged = acc + hm * ln.astype(F32)[..., None]
        acc_out = np.where(got[..., None], merged, acc).astype(F32)
        cnt_out = (cnt + ln).astype(np.uint32)
    info.update(pix=pix, tap=tap, u=u, v=v, te=te)
    return acc_out, cnt_out, ln, info


# ---------------------------------------------------------------------------
# The synthetic scene
# ---------------------------------------------------------------------------
WALL_Z, WALL_TOP = 5.0, 5.0
BOX = ((-0.8, 0.0, 1.0), (0.6, 1.4, 2.2))
ID_FLOOR, ID_WALL, ID_PANEL, ID_BOX = 0, 1, 2, 3


def planes(rays):
    """(t, id, normal, kind) of rays (n, 6) against the scene, in float64 cut to f32."""
    o, d = rays[:, :3].astype(np.float64), rays[:, 3:].astype(np.float64)
    n = len(rays)
    t = np.full(n, np.inf)
    ids = np.full(n, -1, np.int32)
    nor = np.zeros((n, 3))
    with np.errstate(all="ignore"):
        tf = -o[:, 1] / d[:, 1]
        ok = (tf > 1e-4) & np.isfinite(tf)
        t[ok], ids[ok] = tf[ok], ID_FLOOR
        nor[ok] = (0, 1, 0)
        tw = (WALL_Z - o[:, 2]) / d[:, 2]
        yw, xw = o[:, 1] + tw * d[:, 1], o[:, 0] + tw * d[:, 0]
        ok = (tw > 1e-4) & (tw < t) & (yw <= WALL_TOP) & (yw >= 0)
        t[ok] = tw[ok]
        nor[ok] = (0, 0, -1)
        ids[ok] = np.where((np.abs(xw[ok] - 1.5) < 0.6) & (np.abs(yw[ok] - 2.5) < 0.5), ID_PANEL, ID_WALL)
        lo, hi = np.array(BOX[0]), np.array(BOX[1])
        t0, t1 = (lo - o) / d, (hi - o) / d
        near, far = np.minimum(t0, t1), np.maximum(t0, t1)
        tn, tx = near.max(1), far.min(1)
        ok = (tn < tx) & (tn > 1e-4) & (tn < t)
        axis = near.argmax(1)
        bn = np.zeros((n, 3))
        bn[np.arange(n), axis] = -np.sign(d[np.arange(n), axis])
        t[ok], ids[ok] = tn[ok], ID_BOX
        nor[ok] = bn[ok]
    kind = np.where(ids < 0, 0, np.where(ids == ID_PANEL, 2, 1)).astype(np.uint8)
    return t.astype(F32), ids, nor.astype(F32), kind


def _frame_of(wpt, w, h, cam, sample, rng, spp):
    rays = wpt.interface.primary_rays(w, h, cam, SEED, sample)
    t, ids, nor, kind = planes(rays)
    tone = np.array([[0.05, 0.05, 0.08], [0.4, 0.3, 0.2], [0.2, 0.5, 0.3], [6.0, 6.0, 5.0], [0.6, 0.1, 0.1]], F32)[ids + 1]
    mean = (tone * (F32(1.0) + (rng.standard_normal((w * h, 3)) * 0.3).astype(F32))).astype(F32)
    cnt = rng.integers(spp[0], spp[1], w * h).astype(np.uint32)
    acc = (mean * cnt.astype(F32)[:, None]).astype(F32)
    return [acc.reshape(h, w, 3), cnt.reshape(h, w), rays[:, 3:].reshape(h, w, 3).copy(), t.reshape(h, w),
            ids.reshape(h, w), nor.reshape(h, w, 3), kind.reshape(h, w)]


def _pick(rng, mask, share):
    """A random `share` of the pixels in mask, as a mask."""
    return mask & (rng.random(mask.shape) < share)


def _solve_edge(tr, w, h, cam, pcam, point, lo, hi, rng, tries=200000):
    """(dir, t) whose point cam + t * dir, near `point`, projects to lo <= u <= hi
    (both f32): a random search over the last bits of dir.x, dir.z and t; None
    if none is found. Not every value is reachable: u = x * fw - 0.5 with x on a
    2^-24 grid gives -1 exactly where 0.5 / fw lies on that grid (fw = 64)."""
    base = (np.asarray(point, np.float64) - np.asarray(cam[:3], np.float64)).astype(F32)
    dirs = np.repeat(base[None], tries, 0)
    dirs[:, 0] += (rng.random(tries) * 8e-6 - 4e-6).astype(F32)
    dirs[:, 2] += (rng.random(tries) * 8e-6 - 4e-6).astype(F32)
    ts = (F32(1.0) + (rng.random(tries) * 8e-6 - 4e-6).astype(F32)).astype(F32)
    u, v, _, front, _ = project(tr, w, h, cam, pcam, dirs, ts)
    hit = np.nonzero((u >= F32(lo)) & (u <= F32(hi)) & front & (v > -1) & (v < h))[0]
    return (dirs[hit[0]], ts[hit[0]]) if len(hit) else None


def build(wpt, oracle, w, h, pair, edits=True):
    """(cam, cur, pcam, hist, marks) of one viewport and camera pair: cur = [acc,
    cnt, dir, t, id, normal, kind] under the current camera, hist = [acc, cnt, t,
    id, normal, kind] under the history's; with `edits`, the values that sit on
    the decisions (marks: name -> what was placed, for the tests that look for
    them)."""
    pcam, cam = PAIRS[pair]
    rng = np.random.default_rng(w * 1009 + h * 31 + sorted(PAIRS).index(pair))
    cur = _frame_of(wpt, w, h, cam, 0, rng, (1, 9))
    hf = _frame_of(wpt, w, h, pcam, 7, rng, (8, 200))
    hist = [hf[0], hf[1], hf[3], hf[4], hf[5], hf[6]]
    marks = {}
    if not edits or w * h < 150:
        return cam, cur, pcam, hist, marks
    tr = trig(oracle, pcam)
    acc, cnt, dirs, t, ids, nor, kind = cur
    hacc, hcnt, ht, hid, hn, hkind = hist
    # exact edges first, on the unedited frame: they need its taps
    _, _, _, info = numpy_reproject(tr, cam, cur, pcam, hist, COS_MIN, EPS_Z, MAX_LEN, NEAREST)
    us, vs = info["u"], info["v"]
    ok = np.argwhere(info["tap"][..., 0] == TAP_OK)
    floor_ok = [p for p in ok if ids[tuple(p)] == ID_FLOOR][:6]
    for k, p in enumerate(floor_ok):  # n_p = (0, 1, 0): the dot is hn.y, exactly
        q = (int(np.floor(vs[tuple(p)] + F32(0.5))), int(np.floor(us[tuple(p)] + F32(0.5))))
        c = COS_MIN if k % 2 == 0 else np.nextafter(COS_MIN, F32(0))
        hn[q] = (np.sqrt(F32(1) - c * c), c, 0)
    marks["cos_edge"] = len(floor_ok)
    placed = 0
    for p in ok[::3]:
        p = tuple(p)
        te = info["te"][p]
        e = EPS_Z * te
        far = F32(te + e)
        if F32(far - te) == e and placed < 6 and ids[p] != ID_FLOOR:  # te + e is exact: |ht - te| == eps_z * te
            q = (int(np.floor(vs[p] + F32(0.5))), int(np.floor(us[p] + F32(0.5))))
            ht[q] = far if placed % 2 == 0 else np.nextafter(far, F32(np.inf))
            placed += 1
    marks["depth_edge"] = placed
    # the sprinkled edits
    hit = kind != 0
    t[_pick(rng, hit, 0.01)] = np.nan
    t[_pick(rng, hit, 0.01)] = np.inf
    t[_pick(rng, hit, 0.01)] = F32(1e-41)
    acc[_pick(rng, hit, 0.01), 1] = np.nan
    acc[_pick(rng, hit, 0.01), 2] = -np.inf
    m = _pick(rng, hit, 0.03)
    cnt[m] = (0xFFFFFFFF - rng.integers(0, MAX_LEN + 8, int(m.sum()))).astype(np.uint32)
    hh = hkind != 0
    hcnt[_pick(rng, hh, 0.02)] = 0
    hcnt[_pick(rng, hh, 0.01)] = (1 << 24) + 5
    hcnt[_pick(rng, hh, 0.01)] = 1 << 31
    hacc[_pick(rng, hh, 0.01), 0] = np.inf
    hacc[_pick(rng, hh, 0.01), 2] = np.nan
    m = _pick(rng, hh, 0.01)
    hcnt[m] = 1
    hacc[m] = F32(2.0) ** 100
    m = _pick(rng, hh, 0.02)
    hkind[m] = 3 - hkind[m]
    m = _pick(rng, hh, 0.02)
    hn[m] = -hn[m]
    hid[_pick(rng, hh, 0.02)] = 17
    # points that project onto the window's edges, in the first pixels (the history's rot_x is 0)
    fwd = np.array([np.sin(float(pcam[4])), 0.0, np.cos(float(pcam[4]))])
    right = np.array([fwd[2], 0.0, -fwd[0]])
    slot = 0
    above = np.nextafter(F32(-1.0), F32(0))
    # an integer u: fx = 0 and two taps of weight 0; not every integer is reachable either
    edges = [("u=-1", F32(-1.0), F32(-1.0)), ("u>-1", above, F32(-0.99999)), ("u=fw", F32(w), F32(w))]
    edges += [("u=int", F32(k), F32(k)) for k in range(3, min(w - 2, 14))]
    for name, lo, hi in edges:
        if name in marks:
            continue
        off = ((float(lo) + 0.5) / w - 0.5) * (w / h) / 0.8  # x / z in the history's view
        found = _solve_edge(tr, w, h, cam, pcam, np.asarray(pcam[:3]) + fwd + off * right, lo, hi, rng)
        if found is None:
            continue
        p = (0, slot)
        dirs[p], t[p] = found
        acc[p], cnt[p] = (0.5, 0.5, 0.5), 1
        kind[p], ids[p], nor[p] = 1, ID_FLOOR, (0, 1, 0)
        marks[name] = p
        slot += 1
    return cam, cur, pcam, hist, marks


_BUILT = {}


def shared(wpt, oracle, w, h, pair, edits=True):
    k = (w, h, pair, edits)
    if k not in _BUILT:
        cam, cur, pcam, hist, marks = build(wpt, oracle, w, h, pair, edits)
        for a in cur + hist:
            a.setflags(write=False)
        _BUILT[k] = (cam, tuple(cur), pcam, tuple(hist), marks)
    return _BUILT[k]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8 if a.dtype == np.uint8 else np.uint32)


def same(got, want, what):
    """acc, cnt and len bit for bit."""
    for name, g, r in zip(("acc", "cnt", "len"), got, want):
        g, r = bits(g).reshape(-1), bits(r).reshape(-1)
        bad = np.nonzero(g != r)[0]
        assert g.shape == r.shape and len(bad) == 0, (what, name, len(bad), bad[:8], g[bad[:8]], r[bad[:8]])


def bounded_error(a, truth):
    """The mean over pixels and channels of |a - truth| / (|truth| + 0.01)."""
    a, truth = np.asarray(a, np.float64), np.asarray(truth, np.float64)
    return float(np.mean(np.abs(a - truth) / (np.abs(truth) + 0.01)))
