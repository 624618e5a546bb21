"""wpt_first_hit's host side: wpt_primary_rays makes, bit for bit, the primary
rays the oracle's integrator traces; the cases of tests/first_hit_fixtures.py
produce the conditions they are built for (on the oracle alone); and the ABI
answers without a session. tests/test_gpu_first_hit.py runs the same cases on
the device."""
import numpy as np
import pytest

import adversarial as adv
import first_hit_fixtures as fx


def _vps(c):
    return [(vp, s) for vp in c.viewports for s in fx.SAMPLES]


@pytest.mark.parametrize("name", fx.CASES)
def test_host_rays_equal_numpy_restatement(wpt, oracle, name):
    """wpt_primary_rays == the numpy f32 restatement of tracer.rs:178-191,
    every pixel, both samples, bit for bit."""
    c = fx.case(wpt, oracle, name)
    for vp, s in _vps(c):
        got = c.rays(vp, s)
        want = fx.numpy_primary_rays(oracle, vp[0], vp[1], c.cam, fx.SEED, s)
        assert got.shape == want.shape
        bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))[0]
        assert len(bad) == 0, (name, vp, s, len(bad), bad[:5], got[bad[:5]], want[bad[:5]])


@pytest.mark.parametrize("name", fx.CASES)
def test_host_rays_are_the_oracles_own(wpt, oracle, name):
    """Per pixel, the oracle's depth-1 NoNEE path (one Scene::trace of the
    integrator's own primary ray): its node_visits equal trace_rays' of the
    host ray, and its radiance is the emissive intensity exactly where the
    traced id is a light, and the (black) background elsewhere."""
    c = fx.case(wpt, oracle, name)
    light = c.emissive()
    mats = c.dbg.materials()
    for vp, s in _vps(c):
        w, h = vp
        _, ids, visits = c.hits(vp, s)
        acc = np.zeros((h, w, 3), np.float32)
        got_v = np.empty(w * h, np.uint64)
        for p in range(w * h):
            x, y = p % w, p // w
            _, st = c.ref.render(w, h, c.cam, 0, 0, max_depth=1, seed=fx.SEED, s0=s, spp=1,
                                 region=(x, y, x + 1, y + 1), acc=acc)
            assert st["rays"] == 1 and st["shadow_rays"] == 0
            got_v[p] = st["node_visits"]
        assert np.array_equal(got_v, visits.astype(np.uint64)), (name, vp, s)
        want = np.zeros((w * h, 3), np.float32)
        lit = (ids >= 0) & light[np.maximum(ids, 0)]
        want[lit] = mats[ids[lit], :3]
        assert np.all((want[lit] != 0).any(axis=1))  # a light emits something
        assert np.array_equal(acc.reshape(-1, 3).view(np.uint32), want.view(np.uint32)), (name, vp, s)


def _classes(c, vp, s):
    t, ids, visits = c.hits(vp, s)
    light = c.emissive()
    hit = ids >= 0
    return {"miss": int((~hit).sum()), "plane": int((hit & (ids < c.ref.num_inf)).sum()),
            "finite": int((ids >= c.ref.num_inf).sum()), "light": int((hit & light[np.maximum(ids, 0)]).sum()),
            "v0": int((visits == 0).sum()), "v1": int((visits == 1).sum()), "v1000": int((visits > 1000).sum()),
            "n": len(ids), "inf_t": int(np.isposinf(t).sum())}


# what each case is built for: classes with at least one pixel (fixtures' table)
WANTED = {
    "default": ("plane", "finite"),
    "up": ("miss", "light", "plane"),
    "deep": ("finite", "v1000"),
    "E": ("plane", "finite"),
    "C": ("finite",),
    "museum": ("miss", "light", "finite", "v1"),
    "box": ("plane",),
    "spheres": ("v0", "finite"),
    "ragged": ("plane",),
}


@pytest.mark.parametrize("name", fx.CASES)
def test_cases_hold_their_conditions(wpt, oracle, name):
    c = fx.case(wpt, oracle, name)
    for vp, s in _vps(c):
        k = _classes(c, vp, s)
        assert k["inf_t"] == k["miss"]
        if vp == (1, 1):
            continue  # one pixel: covers the ragged tile only
        for cls in WANTED[name]:
            assert k[cls] >= 1, (name, vp, s, cls, k)
        if name == "deep":
            assert k["finite"] == k["n"]  # every pixel hits the mesh
        if name == "spheres":
            assert k["v0"] == k["n"] and c.ref.bvh_kind != 2  # no BVH: no visits
        if name == "box":
            assert c.ref.num_inf == 5
    if name == "deep":
        # the first descent alone defers more entries than the LDS slots hold
        r = c.rays((fx.W, fx.H), 0)
        pend = adv.first_descent_pending(c.ref.nodes(), r[:, :3], r[:, 3:])
        assert pend.max() > adv.LDS_SLOTS, pend.max()
    if name == "C":
        # coincident sheets: some ray's closest t is reported by two triangles, bit for bit
        r = c.rays((fx.W, fx.H), 0)
        t, ids, _ = c.hits((fx.W, fx.H), 0)
        pick = np.nonzero(ids >= c.ref.num_inf)[0][:150]
        every = adv.brute_hits(c.ref, r[pick])
        ties = (every.view(np.uint32) == t[pick].view(np.uint32)[:, None]).sum(axis=1)
        assert (ties >= 2).any()
    if name == "E":
        v = np.asarray(c.mesh, np.float32).reshape(-1, 9)
        assert np.isnan(v).any()
    if name == "ragged":
        assert all(w % 8 and h % 8 for w, h in c.viewports)


def test_first_hit_without_a_session(wpt):
    L = wpt.lib()
    t = np.zeros(4, np.float32)
    assert L.wpt_first_hit(0, None, t.ctypes.data, None, None, None, None, None) == wpt.interface.ERR_NOT_INIT
    assert L.wpt_last_error() == b"init not called"
    assert L.wpt_first_hit(0, None, None, None, None, None, None, None) == wpt.interface.ERR_NOT_INIT
    with pytest.raises(wpt.interface.WptError):
        wpt.interface.first_hit()


def test_primary_rays_arguments(wpt):
    itf = wpt.interface
    cam = np.zeros(5, np.float32)
    out = np.zeros(6, np.float32)
    L = wpt.lib()
    assert L.wpt_primary_rays(0, 1, cam.ctypes.data, 1, 0, out.ctypes.data) == itf.ERR_INVALID_ARG
    assert L.wpt_primary_rays(1, 1, None, 1, 0, out.ctypes.data) == itf.ERR_INVALID_ARG
    assert L.wpt_primary_rays(1, 1, cam.ctypes.data, 1, 0, None) == itf.ERR_INVALID_ARG
    r = itf.primary_rays(3, 2, (1.0, 2.0, 3.0, 0.0, 0.0), seed=5, sample=9)
    assert r.shape == (6, 6) and np.array_equal(r[:, :3], np.tile(np.float32([1, 2, 3]), (6, 1)))
    assert np.allclose(np.linalg.norm(r[:, 3:], axis=1), 1.0, atol=1e-6)
