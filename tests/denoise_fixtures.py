"""Frames and a numpy restatement for the a-trous filter (wpt_denoise,
wpt_denoise_planes, wpt_denoise_host).

A plain helper module (no pytest hooks): tests/test_denoise_cpu.py holds
wpt_denoise_host against numpy_denoise below, tests/test_gpu_denoise.py holds
the device against wpt_denoise_host on the same frames. numpy_denoise is written
from the definition, independent of the C++: every operation is
one numpy f32 operation on whole planes, in the order the definition gives.
Frames are made once per process and shared; nothing returned here is modified.
"""
import numpy as np

F32 = np.float32
ALBEDO = 1  # WPT_DENOISE_ALBEDO
# render_target.rs:21-27, as written there
GAUSS5 = (1.0, 4.0, 6.0, 4.0, 1.0,
          4.0, 16.0, 24.0, 16.0, 4.0,
          6.0, 24.0, 36.0, 24.0, 6.0,
          4.0, 16.0, 24.0, 16.0, 4.0,
          1.0, 4.0, 6.0, 4.0, 1.0)
# (W, H): below the stencil, ragged, one column past a 16 x 16 tile, a viewport
# narrower than the halo, one pixel past two tiles each way
CPU_VIEWPORTS = ((1, 1), (3, 2), (5, 5), (17, 16), (37, 5), (33, 33))
# the step-16 halo of 32 pixels crosses two neighbour tiles each way at 130 x 70
GPU_VIEWPORTS = ((1, 1), (17, 16), (37, 5), (33, 33), (130, 70), (64, 48))
SIGMA_C, SIGMA_Z = F32(1.0), F32(0.1)


def numpy_denoise(acc, cnt, t, normal, albedo, kind, iterations, sigma_c, sigma_z, flags):
    """The definition in numpy f32: (rgb (H, W, 3), valid (H, W) u8, rgba (H, W, 4) u8)."""
    acc, t, normal, albedo = (np.asarray(a, F32) for a in (acc, t, normal, albedo))
    h, w = cnt.shape
    one, zero = F32(1.0), F32(0.0)
    with np.errstate(all="ignore"):
        m = acc / cnt.astype(F32)[..., None]
        ap = np.ones((h, w, 3), F32)
        c = m.copy()
        if flags & ALBEDO:
            dif = kind == 1
            a = np.where(albedo > zero, albedo, one)
            ap[dif] = a[dif]
            c[dif] = m[dif] / a[dif]
        valid = (cnt > 0) & np.isfinite(c).all(axis=-1)
        c[~valid] = zero
        surf = kind != 0
        sig = F32(sigma_c)
        for i in range(iterations):
            step = 1 << i
            s2 = sig * sig
            zden = (F32(sigma_z) * t) * F32(step)
            s3 = np.zeros((h, w, 3), F32)
            sw = np.zeros((h, w), F32)
            for vy in range(5):
                for vx in range(5):
                    ys, xs = np.arange(h) + (vy - 2) * step, np.arange(w) + (vx - 2) * step
                    inside = ((ys >= 0) & (ys < h))[:, None] & ((xs >= 0) & (xs < w))[None, :]
                    iy, ix = np.clip(ys, 0, h - 1)[:, None], np.clip(xs, 0, w - 1)[None, :]
                    cq = c[iy, ix]
                    if vy == 2 and vx == 2:
                        wt = np.full((h, w), 36.0, F32)
                        use = inside
                    else:
                        use = inside & valid[iy, ix] & (kind[iy, ix] == kind)
                        dc = c - cq
                        l = (dc[..., 0] * dc[..., 0] + dc[..., 1] * dc[..., 1]) + dc[..., 2] * dc[..., 2]
                        wt = F32(GAUSS5[vy * 5 + vx]) * (one / (one + l / s2))
                        nq = normal[iy, ix]
                        d = np.fmax((normal[..., 0] * nq[..., 0] + normal[..., 1] * nq[..., 1])
                                    + normal[..., 2] * nq[..., 2], zero)
                        for _ in range(5):
                            d = d * d
                        ws = wt * d
                        dz = np.abs(t - t[iy, ix])
                        r = dz / zden
                        ws = ws * (one / (one + r * r))
                        wt = np.where(surf, ws, wt)
                    use = use & (wt > zero)
                    s3 = np.where(use[..., None], s3 + wt[..., None] * cq, s3)
                    sw = np.where(use, sw + wt, sw)
            c = np.where(valid[..., None], s3 / sw[..., None], zero).astype(F32)
            sig = sig * F32(0.5)
        out = np.where(valid[..., None], c * ap, zero).astype(F32)
        rgba = np.empty((h, w, 4), np.uint8)
        rgba[..., :3] = (np.fmin(np.fmax(out, zero), one) * F32(255.0)).astype(np.uint8)
        rgba[..., 3] = 255
    return out, valid.astype(np.uint8), rgba


def planes(w, h, seed=1):
    """Guide planes of a w x h frame: vertical bands of misses, emitters and
    diffuse surfaces whose normal and depth change at band seams and, inside the
    diffuse bands, from pixel to pixel by a little; some albedo components are 0,
    one diffuse row has denormal depths."""
    rng = np.random.default_rng(seed * 7919 + w * 131 + h)
    x = np.arange(w)[None, :].repeat(h, 0)
    y = np.arange(h)[:, None].repeat(w, 1)
    band = (x // 5 + y // 11) % 4
    kind = np.array([1, 1, 2, 0], np.uint8)[band]
    base = np.array([[0, 0, 1], [0.6, 0, 0.8], [0, 1, 0], [0, 0, 0]], F32)[band]
    n = base + (rng.standard_normal((h, w, 3)) * 0.02).astype(F32)
    n = (n / np.maximum(np.sqrt((n * n).sum(-1, keepdims=True)), F32(1e-20))).astype(F32)
    n[kind == 0] = 0
    t = (F32(2.0) + band.astype(F32) + F32(0.05) * x.astype(F32) + (rng.random((h, w)) * 0.01).astype(F32)).astype(F32)
    t[(y % 7 == 3) & (kind == 1)] = F32(1e-41)  # denormal depths: sigma_z * t underflows to 0 at small sigma_z
    t[kind == 0] = np.inf
    alb = (F32(0.05) + rng.random((h, w, 3)) * 0.9).astype(F32)
    alb[(x + y) % 9 == 0, 1] = 0  # a component of 0 reads as 1
    alb[kind == 0] = 0
    return t, n, alb, kind


def frame(w, h, seed=1, wide=True):
    """(acc, cnt, t, normal, albedo, kind) of a w x h frame: noisy band colours;
    with `wide`, also means from denormals up to 2^100, pixels without samples and
    pixels whose sum is NaN or infinite."""
    t, n, alb, kind = planes(w, h, seed)
    rng = np.random.default_rng(seed * 104729 + w * 17 + h)
    x = np.arange(w)[None, :].repeat(h, 0)
    y = np.arange(h)[:, None].repeat(w, 1)
    tone = np.array([0.2, 0.7, 3.0, 0.05], F32)[(x // 5 + y // 11) % 4]
    mean = (tone[..., None] * (F32(1.0) + (rng.standard_normal((h, w, 3)) * 0.3).astype(F32))).astype(F32)
    cnt = rng.integers(1, 17, (h, w)).astype(np.uint32)
    if wide:
        pick = rng.random((h, w))
        expo = rng.integers(-149, 101, (h, w))
        scale = np.ldexp(F32(1.0), expo).astype(F32)
        mean = np.where((pick < 0.15)[..., None], (mean / np.maximum(tone[..., None], F32(0.05))) * scale[..., None],
                        mean).astype(F32)
        mean = np.clip(mean, -F32(2.0) ** 100, F32(2.0) ** 100).astype(F32)
        cnt[(pick > 0.90) & (pick < 0.93)] = 0
    acc = (mean * cnt.astype(F32)[..., None]).astype(F32)
    if wide:
        acc[(pick > 0.93) & (pick < 0.95), 0] = np.nan
        acc[(pick > 0.95) & (pick < 0.97), 2] = np.inf
        acc[(pick > 0.97) & (pick < 0.98), 1] = -np.inf
    return acc, cnt, t, n, alb, kind


_FRAMES = {}


def shared_frame(w, h, seed=1, wide=True):
    k = (w, h, seed, wide)
    if k not in _FRAMES:
        f = frame(w, h, seed, wide)
        for a in f:
            a.setflags(write=False)
        _FRAMES[k] = f
    return _FRAMES[k]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8 if a.dtype == np.uint8 else np.uint32)


def same(got, want, what):
    """All three outputs bit for bit."""
    for name, g, r in zip(("rgb", "valid", "rgba"), got, want):
        g, r = bits(g).reshape(-1), bits(r).reshape(-1)
        bad = np.nonzero(g != r)[0]
        assert g.shape == r.shape and len(bad) == 0, (what, name, len(bad), bad[:8], g[bad[:8]], r[bad[:8]])


def rel_l2(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(a - ref) / np.linalg.norm(ref))
