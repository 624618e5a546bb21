"""wpt_reproject_host, the host restatement of the reprojection of a kept frame,
against the numpy restatement of tests/reproject_fixtures.py (written from the
definition) bit for bit, the conditions the fixture is built for,
and the properties the definition promises exactly. No GPU:
tests/test_gpu_reproject.py then holds the kernel against wpt_reproject_host.
"""
import ctypes

import numpy as np
import pytest

import reproject_fixtures as fx

F32 = fx.F32
NOT_HALF = [p for p in fx.PAIRS if p != "half_turn"]


@pytest.fixture(scope="module")
def itf(wpt):
    return wpt.interface


def _host(itf, f, flags=0, cos_min=fx.COS_MIN, eps_z=fx.EPS_Z, max_len=fx.MAX_LEN):
    cam, cur, pcam, hist, _ = f
    return itf.reproject_host(cam, cur, pcam, hist, float(cos_min), float(eps_z), max_len, flags)


def _numpy(oracle, f, flags=0, cos_min=fx.COS_MIN, eps_z=fx.EPS_Z, max_len=fx.MAX_LEN):
    cam, cur, pcam, hist, _ = f
    return fx.numpy_reproject(fx.trig(oracle, pcam), cam, cur, pcam, hist, cos_min, eps_z, max_len, flags)


@pytest.mark.parametrize("vp", fx.CPU_VIEWPORTS, ids=lambda v: f"{v[0]}x{v[1]}")
def test_host_against_numpy(wpt, oracle, itf, vp):
    """Every viewport, camera pair and flag combination, at the defaults and at
    max_len 1 and 2^24 with other thresholds; the frames carry the edits."""
    for pair in fx.PAIRS:
        f = fx.shared(wpt, oracle, *vp, pair)
        for flags in fx.FLAGS:
            for kw in (dict(), dict(max_len=1, cos_min=F32(-1.0), eps_z=F32(0.0)),
                       dict(max_len=1 << 24, cos_min=F32(1.0), eps_z=F32(0.5))):
                got = _host(itf, f, flags, **kw)
                want = _numpy(oracle, f, flags, **kw)
                fx.same(got, want[:3], (vp, pair, flags, kw))
                assert np.all(got[2] <= kw.get("max_len", fx.MAX_LEN))
                assert np.array_equal(got[1] - f[1][1], got[2])  # cnt_out - cnt == len, no wrap


def test_every_reject_reason_occurs(wpt, oracle):
    """On the numpy model alone: every reason a pixel passes through and every
    reason a tap is skipped occurs on the 64 x 48 frames, and so do the values
    placed exactly on the thresholds."""
    pix, tap = set(), set()
    on_cos = on_depth = 0
    for pair in fx.PAIRS:
        f = fx.shared(wpt, oracle, 64, 48, pair)
        for flags in fx.FLAGS:
            info = _numpy(oracle, f, flags)[3]
            pix |= set(np.unique(info["pix"]))
            tap |= set(np.unique(info["tap"]))
            ok = info["tap"] == fx.TAP_OK
            on_cos += int((ok & (info["dot"] == fx.COS_MIN)).sum())
            on_depth += int((ok & (info["dz"] == info["lim"])).sum())
    assert pix == set(range(6)), pix
    assert tap == set(range(-1, 9)), tap
    assert on_cos > 0 and on_depth > 0
    # the edits are in the frame
    cam, cur, pcam, hist, marks = fx.shared(wpt, oracle, 64, 48, "sideways")
    acc, cnt, _, t, *_ = cur
    hacc, hcnt = hist[:2]
    assert np.isnan(t).any() and np.isinf(t).any() and ((t > 0) & (t < 1e-38)).any()
    assert np.isnan(acc).any() and np.isinf(acc).any()
    assert (cnt > 0xFFFFFFFF - fx.MAX_LEN).any()
    assert (hcnt == 0).any() and (hcnt > 1 << 24).any()
    with np.errstate(all="ignore"):
        m = hacc / hcnt.astype(F32)[..., None]
    assert (~np.isfinite(m)).any() and (m == F32(2.0) ** 100).any() and np.abs(m[np.isfinite(m)]).max() <= 2.0 ** 100


def test_window_edges(wpt, oracle):
    """The placed points project to u = -1 (rejected), just above -1 (kept in
    the window: its left taps are outside), fw (rejected) and an integer (two
    taps of weight 0)."""
    f = fx.shared(wpt, oracle, 64, 48, "rot_y+")
    marks = f[4]
    assert {"u=-1", "u>-1", "u=fw", "u=int"} <= set(marks), marks
    info = _numpy(oracle, f, 0)[3]
    u = info["u"]
    assert u[marks["u=-1"]] == F32(-1.0) and info["pix"][marks["u=-1"]] == fx.PIX_WINDOW
    assert u[marks["u=fw"]] == F32(64.0) and info["pix"][marks["u=fw"]] == fx.PIX_WINDOW
    p = marks["u>-1"]
    assert F32(-1.0) < u[p] < F32(-0.99999) and info["pix"][p] != fx.PIX_WINDOW
    assert info["tap"][p][0] == fx.TAP_OUTSIDE and info["tap"][p][2] == fx.TAP_OUTSIDE
    p = marks["u=int"]
    assert u[p] == np.floor(u[p]) and info["tap"][p][1] != fx.TAP_OK and info["tap"][p][3] != fx.TAP_OK
    # the smaller viewports hold the edges they can reach
    for vp in ((17, 16), (37, 5), (33, 33)):
        assert "u=fw" in fx.shared(wpt, oracle, *vp, "rot_y+")[4]


@pytest.mark.parametrize("vp", [v for v in fx.CPU_VIEWPORTS if v[0] >= 17], ids=lambda v: f"{v[0]}x{v[1]}")
def test_frames_keep_a_history(wpt, oracle, vp):
    """A condition of the fixture: every camera pair but the half turn keeps a
    history on at least a quarter of its hit pixels, with one tap and with four."""
    for pair in NOT_HALF:
        f = fx.shared(wpt, oracle, *vp, pair)
        hits = int((f[1][6] != 0).sum())
        for flags in (0, fx.NEAREST):
            ln = _numpy(oracle, f, flags)[2]
            assert (ln > 0).sum() >= 0.25 * hits, (vp, pair, flags, int((ln > 0).sum()), hits)


def _centre_frame(wpt, oracle, w, h):
    """Camera A twice, rays through the pixel centres, the current planes equal
    to the history's."""
    cam, cur, pcam, hist, _ = fx.build(wpt, oracle, w, h, "identical", edits=False)
    x, y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    d = np.stack([((x + 0.5) / w - 0.5) * (w / h), 0.5 - (y + 0.5) / h, np.full((h, w), 0.8)], -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    rays = np.concatenate([np.broadcast_to(np.asarray(cam[:3]), (h, w, 3)), d], -1).reshape(-1, 6).astype(F32)
    t, ids, nor, kind = (a.reshape(h, w, -1).squeeze(-1) if a.ndim == 1 else a.reshape(h, w, 3) for a in fx.planes(rays))
    cur = [cur[0], cur[1], rays[:, 3:].reshape(h, w, 3), t, ids, nor, kind]
    hist = [hist[0], hist[1], t, ids, nor, kind]
    return cam, cur, pcam, hist, {}


def test_same_camera_nearest_is_the_own_pixel(wpt, oracle, itf):
    w, h = 33, 33
    f = _centre_frame(wpt, oracle, w, h)
    acc, cnt, ln = _host(itf, f, fx.NEAREST)
    cur, hist = f[1], f[3]
    kept = ln > 0
    assert np.array_equal(kept, cur[6] != 0) and kept.sum() > 0.7 * w * h
    L = np.minimum(hist[1], fx.MAX_LEN).astype(F32)
    want = cur[0] + (hist[0] / hist[1].astype(F32)[..., None]) * L[..., None]
    assert np.array_equal(fx.bits(acc)[kept], fx.bits(want.astype(F32))[kept])
    assert np.array_equal(fx.bits(acc)[~kept], fx.bits(cur[0])[~kept])
    assert np.array_equal(ln[kept], np.minimum(hist[1], fx.MAX_LEN)[kept]) and np.array_equal(cnt, cur[1] + ln)
    fx.same((acc, cnt, ln), _numpy(oracle, f, fx.NEAREST)[:3], "centres")
    fx.same(_host(itf, f, 0), _numpy(oracle, f, 0)[:3], "centres, bilinear")


@pytest.mark.parametrize("what", ["half_turn", "empty_history", "all_misses"])
def test_pass_through(wpt, oracle, itf, what):
    """Bit for bit the input, NaN sums included."""
    cam, cur, pcam, hist, _ = fx.shared(wpt, oracle, 33, 33, "half_turn" if what == "half_turn" else "sideways")
    cur, hist = list(cur), list(hist)
    assert np.isnan(cur[0]).any()
    if what == "empty_history":
        hist[1] = np.zeros_like(hist[1])
    elif what == "all_misses":
        cur[6] = np.zeros_like(cur[6])
    for flags in fx.FLAGS:
        acc, cnt, ln = _host(itf, (cam, cur, pcam, hist, {}), flags)
        assert np.array_equal(fx.bits(acc), fx.bits(cur[0])) and np.array_equal(cnt, cur[1]) and not ln.any()


def test_same_shape_flag(wpt, oracle, itf):
    """Without the flag the id planes are never read; with it a tap of another
    shape is skipped."""
    cam, cur, pcam, hist, _ = f = fx.shared(wpt, oracle, 33, 33, "sideways")
    hist2 = list(hist)
    hist2[3] = np.full_like(hist[3], 99)
    fx.same(_host(itf, f, 0), _host(itf, (cam, cur, pcam, hist2, {}), 0), "ids unread")
    assert not _host(itf, (cam, cur, pcam, hist2, {}), fx.SAME_SHAPE)[2].any()
    a, b = _host(itf, f, fx.NEAREST)[2], _host(itf, f, fx.NEAREST | fx.SAME_SHAPE)[2]
    assert np.all((b > 0) <= (a > 0)) and (b > 0).sum() < (a > 0).sum()


def test_argument_errors(wpt, oracle, itf):
    L = wpt.lib()
    INVALID = -4
    cam, cur, pcam, hist, _ = fx.shared(wpt, oracle, 3, 2, "sideways")
    ins = [np.asarray(cam[:3], F32)] + [np.ascontiguousarray(a) for a in cur] + [np.asarray(pcam, F32)] + \
          [np.ascontiguousarray(a) for a in hist]
    ptr = [a.ctypes.data for a in ins]
    out = [np.zeros((2, 3, 3), F32), np.zeros((2, 3), np.uint32), np.zeros((2, 3), np.uint32)]
    optr = [a.ctypes.data for a in out]

    def call(w=3, h=2, p=ptr, cos_min=0.9, eps_z=0.05, max_len=64, flags=0, o=optr):
        return L.wpt_reproject_host(w, h, *p, ctypes.c_float(cos_min), ctypes.c_float(eps_z), max_len, flags, *o)

    assert call() == 0
    assert call(o=[None, None, None]) == 0 and call(o=[None, optr[1], None]) == 0
    assert call(cos_min=-1.0) == 0 and call(cos_min=1.0) == 0 and call(eps_z=0.0) == 0
    assert call(max_len=1) == 0 and call(max_len=1 << 24) == 0
    for c in (-1.0000001, 1.0000001, float("inf"), float("nan")):
        assert call(cos_min=c) == INVALID
    for e in (-1e-9, float("inf"), float("nan")):
        assert call(eps_z=e) == INVALID
    for m in (0, (1 << 24) + 1, 0xFFFFFFFF):
        assert call(max_len=m) == INVALID
    for flags in (fx.KEEP, fx.KEEP | fx.NEAREST, 8, 0x80000000):
        assert call(flags=flags) == INVALID
    for k in range(len(ptr)):
        assert call(p=ptr[:k] + [None] + ptr[k + 1:]) == INVALID
    assert call(w=0) == INVALID and call(h=0) == INVALID and call(w=65536, h=65536) == INVALID
    with pytest.raises(itf.WptError):
        itf.reproject_host(cam, cur, pcam, hist, max_len=0)
    # the session calls need a session
    assert L.wpt_reproject(0, ctypes.c_float(0.9), ctypes.c_float(0.05), 64, 0, *optr) == -1
    assert L.wpt_history_drop() == -1
    assert L.wpt_denoise_merged(3, ctypes.c_float(1.0), ctypes.c_float(0.1), 0, None, None, None) == -1
    assert L.wpt_reproject_planes(3, 2, *ptr, ctypes.c_float(0.9), ctypes.c_float(0.05), 64, 0, *optr) == -1
    assert itf.REPROJECT_DEFAULTS == {"cos_min": 0.9, "eps_z": 0.05, "max_len": 64, "flags": 0}
    assert itf.OPTIONS["history"] == 46
