"""wpt_denoise_host, the host restatement of the a-trous filter, against the
numpy restatement of tests/denoise_fixtures.py (written from the definition,
DESIGN.md §2) bit for bit, and the properties the definition promises exactly.
No GPU: tests/test_gpu_denoise.py then holds the kernels against
wpt_denoise_host.
"""
import ctypes

import numpy as np
import pytest

import denoise_fixtures as fx

F32 = fx.F32


@pytest.fixture(scope="module")
def itf(wpt):
    return wpt.interface


def _host(itf, f, it, flags, sc=fx.SIGMA_C, sz=fx.SIGMA_Z):
    return itf.denoise_host(*f, iterations=it, sigma_c=float(sc), sigma_z=float(sz), flags=flags)


@pytest.mark.parametrize("vp", fx.CPU_VIEWPORTS, ids=lambda v: f"{v[0]}x{v[1]}")
def test_host_against_numpy(itf, vp):
    """Every viewport, 1..5 iterations, both flag values, two sigma pairs; means
    from denormals up to 2^100, pixels without samples, NaN and infinite sums."""
    f = fx.shared_frame(*vp)
    assert np.isinf(f[0]).any() or vp[0] * vp[1] < 30
    for it in range(1, 6):
        for flags in (0, fx.ALBEDO):
            for sc, sz in ((fx.SIGMA_C, fx.SIGMA_Z), (F32(0.37), F32(1e-5))):
                got = _host(itf, f, it, flags, sc, sz)
                want = fx.numpy_denoise(*f, it, sc, sz, flags)
                fx.same(got, want, (vp, it, flags, float(sc)))


def test_frames_hold_their_conditions():
    """The 33 x 33 frame has what the comparison is meant to cover."""
    acc, cnt, t, n, alb, kind = fx.shared_frame(33, 33)
    with np.errstate(all="ignore"):
        m = np.abs(acc / cnt.astype(F32)[..., None])
    fin = m[np.isfinite(m)]
    assert (cnt == 0).any() and np.isnan(acc).any() and np.isinf(acc).any()
    assert fin.max() > 2.0 ** 90 and fin.max() <= 2.0 ** 100 and (fin[fin > 0].min() < 2.0 ** -126)
    assert set(np.unique(kind)) == {0, 1, 2}
    assert ((alb == 0) & (kind == 1)[..., None]).any()
    assert ((t < 1e-38) & (kind == 1)).any()
    # at sigma_z 1e-5 the denominator of r underflows to 0 on the denormal depths
    assert ((F32(1e-5) * t[(t < 1e-38)]) == 0).all()


def _uniform(w, h, value=0.5, kind=1):
    acc = np.full((h, w, 3), value * 4, F32)
    cnt = np.full((h, w), 4, np.uint32)
    t = np.full((h, w), 3.0, F32)
    n = np.zeros((h, w, 3), F32)
    n[..., 2] = 1
    alb = np.full((h, w, 3), 0.5, F32)
    return [acc, cnt, t, n, alb, np.full((h, w), kind, np.uint8)]


def test_uniform_frame_is_a_fixed_point(itf):
    for flags in (0, fx.ALBEDO):
        rgb, valid, rgba = _host(itf, _uniform(17, 12), 5, flags)
        assert np.all(rgb == F32(0.5)) and np.all(valid == 1)
        assert np.all(rgba[..., :3] == 127) and np.all(rgba[..., 3] == 255)


@pytest.mark.parametrize("edge", ["normal", "kind"])
def test_nothing_crosses_an_edge(itf, edge):
    """Left of column 8 the output bits do not depend on the colours right of it,
    across a normal edge with dot 0 and across a kind edge."""
    w, h = 17, 12
    rng = np.random.default_rng(5)
    outs = []
    for trial in range(2):
        f = _uniform(w, h)
        f[0] = (rng.random((h, w, 3)) * 4).astype(F32)
        if trial:
            f[0][:, 8:] = (rng.random((h, w - 8, 3)) * 400).astype(F32)
        else:
            left = f[0][:, :8].copy()
        f[0][:, :8] = left
        if edge == "normal":
            f[3][:, 8:] = (1, 0, 0)
        else:
            f[5][:, 8:] = 2
        outs.append(_host(itf, f, 3, 0))
    assert not np.array_equal(outs[0][0][:, 8:], outs[1][0][:, 8:])
    fx.same([o[:, :8] for o in outs[0]], [o[:, :8] for o in outs[1]], edge)
    # and something does cross where there is no edge
    f = _uniform(w, h)
    f[0] = (rng.random((h, w, 3)) * 4).astype(F32)
    a = _host(itf, f, 3, 0)[0]
    f[0] = f[0].copy()
    f[0][:, 8:] += F32(0.25)
    assert not np.array_equal(a[:, :8], _host(itf, f, 3, 0)[0][:, :8])


@pytest.mark.parametrize("bad", ["cnt0", "nan", "inf"])
def test_invalid_pixels(itf, bad):
    """A pixel without samples, or with a NaN or infinite mean: valid 0, +0 out,
    and its neighbours do not see what it holds."""
    w, h = 9, 7
    rng = np.random.default_rng(11)
    base = _uniform(w, h)
    base[0] = (rng.random((h, w, 3)) * 4).astype(F32)
    outs = []
    for fill in (1.0, 1e30):
        f = [a.copy() for a in base]
        f[0][3, 4] = fill
        if bad == "cnt0":
            f[1][3, 4] = 0
        elif bad == "nan":
            f[0][3, 4, 1] = np.nan
        else:
            f[0][3, 4, 2] = -np.inf
        outs.append(_host(itf, f, 3, fx.ALBEDO))
    rgb, valid, rgba = outs[0]
    assert valid[3, 4] == 0 and valid.sum() == w * h - 1
    assert np.all(fx.bits(rgb[3, 4]) == 0) and tuple(rgba[3, 4]) == (0, 0, 0, 255)
    fx.same(outs[0], outs[1], bad)
    # it is not a tap: the frame with that pixel's weight gone differs from the frame where it is valid
    f = [a.copy() for a in base]
    assert not np.array_equal(_host(itf, f, 3, fx.ALBEDO)[0][3, 3], rgb[3, 3])


def test_denormal_depth_stays_finite(itf):
    """sigma_z * t_p underflows to 0 and dz is 0: r = 0 / 0 is dropped by w > 0."""
    f = _uniform(9, 7)
    f[2][:] = F32(1e-42)
    f[0] = (np.random.default_rng(3).random((7, 9, 3)) * 4).astype(F32)
    sz = F32(1e-5)
    assert F32(sz * f[2][0, 0]) == 0
    rgb, valid, _ = _host(itf, f, 3, 0, sz=sz)
    assert np.all(np.isfinite(rgb)) and np.all(valid == 1)
    # every neighbour was dropped: the centre alone, 36 c / 36
    with np.errstate(all="ignore"):
        m = f[0] / F32(4)
    assert np.array_equal(fx.bits(rgb), fx.bits((F32(36) * m) / F32(36)))
    fx.same((rgb, valid, _), fx.numpy_denoise(*f, 3, fx.SIGMA_C, sz, 0), "denormal t")


def test_albedo_flag(itf):
    w, h = 9, 7
    f = _uniform(w, h)
    f[0] = (np.random.default_rng(2).random((h, w, 3)) * 4).astype(F32)
    f[4][2, 2] = (0.0, 0.25, 0.0)      # components of 0 use a' = 1
    f[4][4, 4] = (1e-38, 0.5, 0.5)     # m / a' overflows: invalid
    f[0][4, 4] = 4e3
    f[4][5, 5] = (-1.0, np.nan, 0.5)   # not > 0: a' = 1
    f[5][1, 1] = 2                     # an emitter keeps a' = 1 whatever its albedo plane holds
    rgb, valid, rgba = _host(itf, f, 1, fx.ALBEDO)
    fx.same((rgb, valid, rgba), fx.numpy_denoise(*f, 1, fx.SIGMA_C, fx.SIGMA_Z, fx.ALBEDO), "albedo")
    assert valid[4, 4] == 0 and np.all(fx.bits(rgb[4, 4]) == 0) and valid.sum() == w * h - 1
    assert np.all(np.isfinite(rgb))
    # without the flag the albedo plane is never read
    g = [a.copy() for a in f]
    g[4][:] = np.nan
    fx.same(_host(itf, f, 3, 0), _host(itf, g, 3, 0), "no flag")
    assert _host(itf, f, 3, 0)[1][4, 4] == 1
    # a frame that is albedo times a constant comes back as that, to rounding
    u = _uniform(w, h)
    u[4] = (0.1 + np.random.default_rng(4).random((h, w, 3)) * 0.8).astype(F32)
    u[0] = (u[4] * F32(2.0) * F32(4)).astype(F32)
    out = _host(itf, u, 3, fx.ALBEDO)[0]
    assert np.allclose(out, u[4] * 2, rtol=1e-6, atol=0)
    assert not np.allclose(_host(itf, u, 3, 0)[0], u[4] * 2, rtol=1e-3, atol=0)


def test_rgba_quantisation(itf):
    """(min(max(v, 0), 1) * 255) as u8, truncated; alpha 255."""
    vals = np.array([-1.0, -0.0, 0.0, 1e-40, 0.00391, 0.00393, 0.5, 0.99999, 1.0, 1.0000001, 7.0, 3e37,
                     254.0 / 255, 254.9 / 255, 1 / 255, 128 / 255], F32)
    w, h = len(vals), 1
    f = _uniform(w, h, kind=0)
    f[0] = (np.stack([vals, vals[::-1], vals], -1)[None] * F32(4)).astype(F32)
    f[5] = (np.arange(w) % 3).astype(np.uint8)[None]  # no two pixels 1 or 2 apart share a kind: nothing is mixed
    rgb, valid, rgba = _host(itf, f, 1, 0)
    with np.errstate(all="ignore"):
        m = f[0] / F32(4)
        want = (np.fmin(np.fmax((F32(36) * m) / F32(36), F32(0)), F32(1)) * F32(255)).astype(np.uint8)
    assert np.array_equal(rgba[..., :3], want) and np.all(rgba[..., 3] == 255)
    assert want.min() == 0 and want.max() == 255 and 254 in want and 127 in want


def test_argument_errors(wpt, itf):
    L = wpt.lib()
    INVALID = -4
    f = [np.ascontiguousarray(a) for a in _uniform(5, 4)]
    out = [np.zeros((4, 5, 3), F32), np.zeros((4, 5), np.uint8), np.zeros((4, 5, 4), np.uint8)]
    ptr = [a.ctypes.data for a in f]
    optr = [a.ctypes.data for a in out]

    def call(w=5, h=4, p=ptr, it=3, sc=1.0, sz=0.1, flags=0, o=optr):
        return L.wpt_denoise_host(w, h, *p, it, ctypes.c_float(sc), ctypes.c_float(sz), flags, *o)

    assert call() == 0
    assert call(o=[None, None, None]) == 0 and call(o=[None, optr[1], None]) == 0
    for it in (0, 6, 0xFFFFFFFF):
        assert call(it=it) == INVALID
    for s in (0.0, -1.0, float("inf"), float("nan"), -0.0):
        assert call(sc=s) == INVALID and call(sz=s) == INVALID
    for flags in (2, 3, 0x80000000):
        assert call(flags=flags) == INVALID
    for k in range(6):
        assert call(p=ptr[:k] + [None] + ptr[k + 1:]) == INVALID
    assert call(w=0) == INVALID and call(h=0) == INVALID and call(w=65536, h=65536) == INVALID
    with pytest.raises(itf.WptError):
        itf.denoise_host(*f, iterations=0)
