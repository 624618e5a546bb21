"""wpt_first_hit_rays and wpt_denoise_rays without a GPU: the entry points and
their binding, the fixture's fisheye frame, the conditions the ray sets of
tests/test_gpu_rayframe.py are built for (asserted on the oracle alone), and
the quality condition of the filtered fisheye frame on the oracle's frames
through wpt_denoise_host.
"""
import inspect
import os
import re

import numpy as np
import pytest

import rayframe_fixtures as rx
import rays_adversarial as ra
import rays_fixtures as rf

NOT_INIT = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "wpt.h")).read()


def _declared(name):
    """The parameter types of `name` as include/wpt.h declares it."""
    m = re.search(r"\bint " + name + r"\(([^)]*)\);", _header())
    assert m, name
    out = []
    for p in m.group(1).split(","):
        p = " ".join(p.split())
        out.append("p" if "*" in p else p.rsplit(" ", 1)[0])
    return out


# ---------------------------------------------------------------------------
# The entry points and the binding
# ---------------------------------------------------------------------------
def test_calls_need_a_session(wpt):
    L = wpt.lib()
    rays = np.zeros((4, 6), np.float32)
    rays[:, 5] = 1
    t = np.full(4, 7.25, np.float32)
    rgb = np.full((2, 2, 3), 7.25, np.float32)
    assert L.wpt_first_hit_rays(4, rays.ctypes.data, 0, t.ctypes.data, None, None, None, None, None, None) == NOT_INIT
    assert L.wpt_denoise_rays(2, 2, rays.ctypes.data, None, 0, 1, 1, 3, 1.0, 0.1, 0, 0, rgb.ctypes.data, None, None, None,
                              None) == NOT_INIT
    assert np.all(t == np.float32(7.25)) and np.all(rgb == np.float32(7.25))
    assert b"init" in L.wpt_last_error()


@pytest.mark.parametrize("name", ["wpt_first_hit_rays", "wpt_denoise_rays"])
def test_binding_matches_the_header(wpt, name):
    import ctypes

    assert name in wpt._lib.header_symbols() and name in wpt._lib.EXPORTED
    res, args = wpt._lib._SIGS[name]
    ctype = {"p": ctypes.c_void_p, "size_t": ctypes.c_size_t, "uint32_t": ctypes.c_uint32, "float": ctypes.c_float}
    assert res is ctypes.c_int
    assert args == [ctype[p] for p in _declared(name)], (args, _declared(name))


def test_flag_and_defaults(wpt):
    itf = wpt.interface
    m = re.search(r"#define WPT_RAYS_DEVICE (\d+)u", _header())
    assert m and int(m.group(1)) == itf.RAYS_DEVICE
    sig = inspect.signature(itf.denoise_rays).parameters
    assert list(sig)[:7] == ["rays", "width", "height", "keys", "sample", "spp", "type"]
    assert (sig["keys"].default, sig["sample"].default, sig["spp"].default, sig["type"].default) == (None, 0, 1, 1)
    for k in ("iterations", "sigma_c", "sigma_z", "flags"):
        assert sig[k].default == itf.DENOISE_DEFAULTS[k]
    assert sig["device"].default is False
    fsig = inspect.signature(itf.first_hit_rays).parameters
    assert list(fsig) == ["rays", "planes", "device"] and fsig["device"].default is False
    assert set(fsig["planes"].default) == set(rx.PLANES) == set(itf.FIRST_HIT_RAYS_PLANES)
    # the planes' positions are the declaration's output order
    decl = re.search(r"int wpt_first_hit_rays\(([^)]*)\);", _header()).group(1)
    names = [p.split()[-1].lstrip("*") for p in decl.split(",")][3:]
    assert names == ["t", "id", "visits", "normal3", "albedo3", "kind", "status"]
    assert [n.rstrip("3") for n in names] == sorted(itf.FIRST_HIT_RAYS_PLANES, key=lambda k: itf.FIRST_HIT_RAYS_PLANES[k][0])


# ---------------------------------------------------------------------------
# The fisheye frame
# ---------------------------------------------------------------------------
def test_fisheye(wpt):
    for o in rx.FISH_ORIGINS:
        rays = rx.fisheye(o)
        assert rays.shape == (rx.FISH_W * rx.FISH_H, 6) and rays.dtype == np.float32
        status = wpt.interface.rays_valid(rays)
        assert int((status == 0).sum()) == rx.FISH_INVALID
        assert np.array_equal(status, rf.valid(rays))
        assert np.array_equal(rays[:, :3], np.tile(np.asarray(o, np.float32), (len(rays), 1)))
        d = rays[status == 1, 3:].astype(np.float64)
        assert np.all(np.abs(np.sqrt((d * d).sum(1)) - 1) < 1e-6) and np.all(d[:, 2] > -1e-6)
    # the centre looks along +z, the frame is mirror symmetric in x
    c = rx.fisheye()[(rx.FISH_H // 2) * rx.FISH_W + rx.FISH_W // 2, 3:]
    assert c[2] > 0.99


# ---------------------------------------------------------------------------
# The ray sets produce their conditions (oracle alone)
# ---------------------------------------------------------------------------
def _kinds(planes):
    return set(np.unique(planes["kind"][planes["status"] == 1]).tolist())


@pytest.mark.parametrize("name", ra.MESHES)
def test_mesh_sets_hold_every_kind(wpt, oracle, name):
    _, _, rays, want = rx.mesh_planes(wpt, oracle, name)
    assert len(rays) <= ra.MAX_SET_RAYS
    assert _kinds(want) == {0, 1, 2}, (name, _kinds(want))
    hit = want["id"] >= 0
    assert np.all(np.isposinf(want["t"][~hit]))
    assert np.all(want["visits"][want["status"] == 0] == 0)
    if name == "F":
        print("mesh F visits", int(want["visits"].min()), int(want["visits"].max()))
        assert int(want["visits"].max()) > rx.LDS_SLOTS


@pytest.mark.parametrize("scene_id", list(ra.SHAPE_SCENES))
def test_shape_sets_hold_every_kind(wpt, oracle, scene_id):
    _, sets = rx.shape_planes(wpt, oracle, scene_id)
    kinds = set()
    for _, want in sets.values():
        kinds |= _kinds(want)
    assert kinds == {0, 1, 2}, (scene_id, kinds)


def test_scaled_sets(wpt, oracle):
    for name in ra.SCALED_MESHES:
        _, _, scaled = rx.scaled_planes(wpt, oracle, name)
        assert set(scaled) == set(ra.SCALES)
        for s in ra.EXACT_SCALES:
            assert (scaled[s][1]["id"] >= 0).any(), (name, s)


def test_box_rays_and_their_invalid_variants(wpt, oracle):
    _, rays, want = rx.box_rays(wpt, oracle)
    assert len(rays) == 1025 and want["status"].all()
    assert _kinds({k: v[:rx.WAVE] for k, v in want.items()}) == {0, 1, 2}
    where = [0, 63, 64, 127]
    bad = rx.with_invalid(rays, where)
    st = rf.valid(bad)
    assert not st[where].any() and int(st.sum()) == len(rays) - len(where)
    m = rx.masked(want, where)
    assert np.all(m["id"][where] == -1) and np.all(np.isposinf(m["t"][where])) and np.all(m["visits"][where] == 0)
    keep = np.ones(len(rays), bool)
    keep[where] = False
    for k in want:
        assert np.array_equal(rx.bits(m[k][keep]), rx.bits(want[k][keep]))


# ---------------------------------------------------------------------------
# The filter helps the fisheye frame
# ---------------------------------------------------------------------------
def test_the_filter_helps_the_fisheye_frame(wpt, oracle):
    """The oracle's 4-spp NEE frames at the three origins through
    wpt_denoise_host (3 passes, sigma_c 1.0, sigma_z 0.1, flags 0) against its
    1,024-spp frames: the filtered error is below half the raw one."""
    print("origin | raw 4 spp | filtered | ratio")
    for o in rx.FISH_ORIGINS:
        raw, fil, same_valid = rx.fisheye_row(wpt, oracle, o)
        print(f"{o} | {raw:.4f} | {fil:.4f} | {fil / raw:.3f}")
        assert same_valid
        assert fil < rx.HELP_RATIO * raw, (o, raw, fil)
