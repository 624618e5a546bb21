"""Planes and a numpy restatement for the guided upsampler (wpt_upsample,
wpt_upsample_planes, wpt_upsample_host).

A plain helper module (no pytest hooks): tests/test_upsample_cpu.py holds
wpt_upsample_host against numpy_upsample below, tests/test_gpu_upsample.py holds
the device against wpt_upsample_host on the same planes. numpy_upsample is
written from the definition, independent of the C++: the coarse
stage is denoise_fixtures' restatement of the filter's passes, the fine stage
one numpy f32 operation per step on whole planes, in the order the definition
gives. Cases are made once per process and shared; nothing returned here is
modified.
"""
import numpy as np

import denoise_fixtures as dfx

F32 = dfx.F32
# coarse (W, H): a single pixel, a row, a column, half a tile, ragged, wider than
# the fine tile at every scale, the session tests' viewport
VIEWPORTS = ((1, 1), (1, 5), (5, 1), (8, 8), (9, 7), (37, 5), (64, 48))
SCALES = (2, 3, 4)
SIGMA_C, SIGMA_Z = dfx.SIGMA_C, dfx.SIGMA_Z
# at this sigma_z the denormal depths make sigma_z * T underflow to 0: r = 0 / 0
SMALL_SIGMA_Z = F32(1e-5)
BACKGROUND = np.array([0.25, -0.0, 3.0e-41], F32)  # its bits must come through: a -0 and a denormal
# exact unit normals; ORTH[i] has dot exactly 0 with NORMALS[i]
NORMALS = np.array([[0, 0, 1], [0.6, 0, 0.8], [0, 1, 0], [1, 0, 0]], F32)
ORTH = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 1, 0]], F32)


def coarse_stage(acc, cnt, t, normal, albedo, kind, iterations, sigma_c, sigma_z):
    """Step 1: dn_pack with the albedo flag on, then the passes. The pack is
    restated here; the passes are denoise_fixtures.numpy_denoise's, entered with
    the packed value as a 1-sample mean and no flag, so that its own pack and
    unpack are the identity. -> (c' (H, W, 3), valid (H, W) bool)."""
    acc, albedo = np.asarray(acc, F32), np.asarray(albedo, F32)
    one, zero = F32(1.0), F32(0.0)
    with np.errstate(all="ignore"):
        c = (acc / cnt.astype(F32)[..., None]).astype(F32)
        dif = kind == 1
        a = np.where(albedo > zero, albedo, one)
        c[dif] = c[dif] / a[dif]
        valid = (cnt > 0) & np.isfinite(c).all(axis=-1)
        c[~valid] = zero
    out, v, _ = dfx.numpy_denoise(c, valid.astype(np.uint32), t, normal, albedo, kind, iterations, sigma_c, sigma_z, 0)
    assert np.array_equal(v.astype(bool), valid)
    return out, valid


def _axis(n_fine, s):
    a = 2 * np.arange(n_fine, dtype=np.int64) + 1 - s
    i0 = a // (2 * s)  # floor
    m = a - 2 * s * i0
    assert np.all((m >= 0) & (m < 2 * s))
    return i0, (m.astype(F32) / F32(2 * s)).astype(F32)


def numpy_upsample(scale, coarse, fine, background, iterations, sigma_c, sigma_z):
    """The definition in numpy f32: (rgb (sH, sW, 3), valid (sH, sW) u8, rgba (sH, sW, 4) u8)."""
    acc, cnt, t, normal, albedo, kind = coarse
    T, N, Al, K = (np.asarray(p) for p in fine)
    h, w = cnt.shape
    fh, fw = scale * h, scale * w
    one, zero = F32(1.0), F32(0.0)
    cq_all, ok_all = coarse_stage(acc, cnt, t, normal, albedo, kind, iterations, sigma_c, sigma_z)
    ok_all = ok_all & (kind == 1)
    x0, fx = _axis(fw, scale)
    y0, fy = _axis(fh, scale)
    gx, gy = one - fx, one - fy
    with np.errstate(all="ignore"):
        zden = F32(sigma_z) * T

        def tier(taps):
            s3 = np.zeros((fh, fw, 3), F32)
            sw = np.zeros((fh, fw), F32)
            for dx, dy, wb in taps:
                qx, qy = x0 + dx, y0 + dy
                inside = ((qy >= 0) & (qy < h))[:, None] & ((qx >= 0) & (qx < w))[None, :]
                iy, ix = np.clip(qy, 0, h - 1)[:, None], np.clip(qx, 0, w - 1)[None, :]
                nq = normal[iy, ix]
                d = np.fmax((N[..., 0] * nq[..., 0] + N[..., 1] * nq[..., 1]) + N[..., 2] * nq[..., 2], zero)
                for _ in range(5):
                    d = d * d
                r = np.abs(T - t[iy, ix]) / zden
                wt = (wb * d) * (one / (one + r * r))
                use = inside & ok_all[iy, ix] & (wt > zero)
                s3 = np.where(use[..., None], s3 + wt[..., None] * cq_all[iy, ix], s3)
                sw = np.where(use, sw + wt, sw)
            return s3, sw

        near = tier([(0, 0, gy[:, None] * gx[None, :]), (1, 0, gy[:, None] * fx[None, :]),
                     (0, 1, fy[:, None] * gx[None, :]), (1, 1, fy[:, None] * fx[None, :])])
        wide = tier([(dx, dy, np.ones((fh, fw), F32)) for dy in range(-1, 3) for dx in range(-1, 3)])
        ap = np.where(Al > zero, Al, one)
        out = np.zeros((fh, fw, 3), F32)
        valid = np.zeros((fh, fw), np.uint8)
        for level, (s3, sw) in ((2, wide), (1, near)):  # the four taps win where they pass
            hit = sw > zero
            out = np.where(hit[..., None], (s3 / sw[..., None]) * ap, out).astype(F32)
            valid = np.where(hit, level, valid).astype(np.uint8)
        out = np.where((K == 0)[..., None], np.asarray(background, F32), out)
        out = np.where((K != 0)[..., None] & (K != 1)[..., None], Al, out).astype(F32)
        valid[K != 1] = 1
        rgba = np.empty((fh, fw, 4), np.uint8)
        rgba[..., :3] = (np.fmin(np.fmax(out, zero), one) * F32(255.0)).astype(np.uint8)
        rgba[..., 3] = 255
    return out, valid, rgba


def case(w, h, s, seed=1):
    """(coarse, fine) planes of a w x h frame and its s w x s h guides.

    Coarse: denoise_fixtures' sums and counts (means from denormals to 2^100,
    pixels without samples, NaN and infinite sums) under guide planes of exact
    normals in bands of all three kinds, with rows of denormal depth and albedo
    components of 0. Fine: the coarse guides repeated, a third of the depths
    exactly the coarse ones (r = 0), the others off by up to 1 %, and on random
    pixels: the opposite normal, a normal with dot exactly 0, a depth 100 times
    as large, another kind, an albedo component of 0. From 8 x 7 up: a 2 x 2
    hole of coarse pixels without samples inside a flat diffuse patch (fine
    pixels between them find their four taps failing and the 4 x 4 block not).
    The last fine pixel is diffuse with a normal facing away from every coarse
    one: nothing passes."""
    rng = np.random.default_rng(seed * 7919 + w * 131 + h * 17 + s)
    acc, cnt = (a.copy() for a in dfx.shared_frame(w, h)[:2])
    x = np.arange(w)[None, :].repeat(h, 0)
    y = np.arange(h)[:, None].repeat(w, 1)
    band = (x // 3 + y // 4) % 5
    kind = np.array([1, 1, 0, 2, 1], np.uint8)[band]
    nsel = np.array([0, 1, 3, 2, 0])[band]
    t = (F32(2.0) + band.astype(F32) + F32(0.05) * x.astype(F32) + (rng.random((h, w)) * 0.01).astype(F32)).astype(F32)
    t[(y % 7 == 3) & (kind == 1)] = F32(1e-41)
    alb = (F32(0.05) + rng.random((h, w, 3)) * 0.9).astype(F32)
    alb[(x + y) % 9 == 0, 1] = 0
    hole = w >= 8 and h >= 7
    if hole:
        kind[1:5, 1:5], nsel[1:5, 1:5], t[1:5, 1:5] = 1, 0, F32(3.0)
        alb[1:5, 1:5] = F32(0.5)
        acc[1:5, 1:5] = (rng.random((4, 4, 3)) * 4).astype(F32)
        cnt[1:5, 1:5] = 4
        cnt[2:4, 2:4] = 0
    n = NORMALS[nsel].copy()
    n[kind == 0] = 0
    t[kind == 0] = np.inf
    alb[kind == 0] = 0

    fh, fw = s * h, s * w
    up = lambda a: a.repeat(s, 0).repeat(s, 1)
    K, sel, T = up(kind).copy(), up(nsel), up(t).copy()
    off = rng.random((fh, fw))
    T = np.where(off < 1 / 3, T, T * (F32(1.0) + (F32(0.03) * (off - 0.66)).astype(F32))).astype(F32)
    N = NORMALS[sel].copy()
    Al = (F32(0.05) + rng.random((fh, fw, 3)) * 0.9).astype(F32)
    pick = rng.random((fh, fw))
    N[pick < 0.04] = -N[pick < 0.04]
    o = (pick >= 0.04) & (pick < 0.08)
    N[o] = ORTH[sel[o]]
    T[(pick >= 0.08) & (pick < 0.11)] *= F32(100.0)
    K = np.where((pick >= 0.11) & (pick < 0.15), (K + 1) % 3, K).astype(np.uint8)
    Al[(pick >= 0.15) & (pick < 0.19), 2] = 0
    if hole:
        a, b = s, 5 * s
        K[a:b, a:b], N[a:b, a:b], T[a:b, a:b], Al[a:b, a:b] = 1, NORMALS[0], F32(3.0), F32(0.5)
    K[-1, -1], N[-1, -1], T[-1, -1], Al[-1, -1] = 1, (0, -1, 0), F32(3.0), F32(0.5)
    if fw > 1:  # a frame of one coarse pixel still has the three kinds
        K[0, 1] = 0
        K[-1, 0] = 2
    # what a kind implies for the other planes (k_first_hit's conventions)
    was_miss = (up(kind) == 0) & (K != 0)
    N[was_miss], T[was_miss] = NORMALS[0], F32(3.0)
    N[K == 0], T[K == 0], Al[K == 0] = 0, np.inf, 0
    Al[K == 2] = (F32(3.0) + rng.random((int((K == 2).sum()), 3)) * 5).astype(F32)
    return (acc, cnt, t, n, alb, kind), (T, N, Al, K)


_CASES = {}


def shared_case(w, h, s, seed=1):
    k = (w, h, s, seed)
    if k not in _CASES:
        c = case(w, h, s, seed)
        for part in c:
            for a in part:
                a.setflags(write=False)
        _CASES[k] = c
    return _CASES[k]


def replicate(mean, s):
    """The s x s replication of a coarse frame: the baseline an upsampler has to beat."""
    return np.asarray(mean).repeat(s, 0).repeat(s, 1)


def rel_l2_pair(img, ref):
    """(relative L2 on clamp(., 0, 1), relative L2 unclamped)."""
    return dfx.rel_l2(np.clip(img, 0, 1), np.clip(ref, 0, 1)), dfx.rel_l2(img, ref)


bits, same = dfx.bits, dfx.same
