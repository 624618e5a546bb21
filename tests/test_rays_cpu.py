"""The ray query (wpt_radiance_rays) without a GPU: the call's behaviour without
a session, the binding and the header constant, the validity rule on the host,
and the conditions tests/rays_fixtures.py is built for, on the oracle alone
(tests/test_gpu_rays.py then compares the device with the same expectations).
"""
import os
import re

import numpy as np

import rays_fixtures as rf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOT_INIT = -1


def test_no_session_is_not_init_and_writes_nothing(wpt):
    """WPT_ERR_NOT_INIT for valid and for invalid arguments alike."""
    L = wpt.lib()
    rays = np.tile(np.array([0, 1, -3.5, 0, 0, 1], np.float32), (5, 1))
    keys = np.arange(5, dtype=np.uint32)
    rgb = np.full((5, 3), 7.25, np.float32)
    status = np.full(5, 9, np.uint8)
    r, k, o, s = rays.ctypes.data, keys.ctypes.data, rgb.ctypes.data, status.ctypes.data
    calls = (
        (5, r, k, 0, 1, 1, 0, o, s), (5, r, None, 3, 2, 0, 0, o, None), (0, None, None, 0, 1, 1, 0, None, None),
        (5, None, None, 0, 1, 1, 0, o, s), (5, r, k, 0, 0, 1, 0, o, s), (5, r, k, 0, 1, 3, 0, o, s),
        (5, r, k, 0, 1, 1, 2, o, s), (5, r, k, 0xFFFFFFFF, 2, 1, 0, o, s), (1 << 32, r, k, 0, 1, 1, 0, o, s),
    )
    for c in calls:
        assert L.wpt_radiance_rays(*c) == NOT_INIT, c
    assert np.all(rgb == np.float32(7.25)) and np.all(status == 9)
    itf = wpt.interface
    try:
        itf.radiance_rays(rays)
    except itf.WptError as e:
        assert e.code == itf.ERR_NOT_INIT
    else:
        raise AssertionError("radiance_rays without a session did not raise")


def test_binding_and_header_constant(wpt):
    itf = wpt.interface
    assert callable(itf.radiance_rays) and itf.RAYS_DEVICE == 1
    text = open(os.path.join(ROOT, "include", "wpt.h")).read()
    m = re.search(r"#define\s+WPT_RAYS_DEVICE\s+(\d+)u?\b", text)
    assert m and int(m.group(1)) == itf.RAYS_DEVICE
    assert re.search(r"int\s+wpt_radiance_rays\(size_t n, const float\* rays6, const uint32_t\* keys, uint32_t sample, "
                     r"uint32_t spp,\s*uint32_t type, uint32_t flags, float\* rgb3, uint8_t\* status\);", text)
    assert hasattr(wpt.lib(), "wpt_radiance_rays")


def test_validity_rule(wpt):
    """The host's rule (the function the kernels call) on NaN, +-inf, -0
    directions, denormals and three zeros, against the table and its numpy twin."""
    rays = np.array([v[0] for v in rf.VALIDITY], np.float32)
    want = np.array([v[1] for v in rf.VALIDITY], np.uint8)
    assert 0 < want.sum() < len(want)
    got = wpt.interface.rays_valid(rays)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert np.array_equal(rf.valid(rays), want)
    # the frames' and the probes' rays are all valid
    assert wpt.interface.rays_valid(np.zeros((0, 6), np.float32)).shape == (0,)


def test_probes_produce_their_conditions(wpt, oracle):
    """Among each scene's 80 one-pixel paths (types 0 and 1) some are zero and
    some are not; over the scenes at least one probe hits an emitter first and
    at least one misses; every probe ray is valid."""
    emitter_first = misses = 0
    for name in rf.SCENES:
        sc = rf.scene(wpt, oracle, name)
        rays = sc.probe_rays()
        assert rays.shape == (rf.PROBES, 6) and rf.valid(rays).all()
        assert len(np.unique(rays[:, :3], axis=0)) == rf.PROBES  # the origins differ
        nz = sum(int((sc.probe_expect(t)[0] != 0).any(axis=1).sum()) for t in (0, 1))
        assert 0 < nz < 2 * rf.PROBES, (name, nz)
        # a depth-1 NoNEE path is one Scene::trace: non-zero iff an emitter is hit first
        emitter_first += int((sc.probe_expect(0, 1)[0] != 0).any(axis=1).sum())
        misses += int((sc.ref.trace_rays(rays)[1] < 0).sum())
    assert emitter_first > 0 and misses > 0


def test_frames_produce_their_conditions(wpt, oracle):
    """The anchor frames are not black, the three render types differ, and the
    frame's rays at sample 0 and 7 differ (the jitter)."""
    for name in rf.SCENES:
        sc = rf.scene(wpt, oracle, name)
        vp = (17, 16)
        a0, r0 = sc.frame(vp, 0, 0)
        a1, r1 = sc.frame(vp, 1, 0)
        assert (a1 != 0).any() and r1 > r0 > 0, name
        assert (rf.bits(a0) != rf.bits(a1)).any(), name
        assert (rf.bits(sc.rays(vp, 0)) != rf.bits(sc.rays(vp, 7))).any()
    for name in rf.PNEE_SCENES:
        sc = rf.scene(wpt, oracle, name)
        assert (rf.bits(sc.frame((17, 16), 2, 0)[0]) != rf.bits(sc.frame((17, 16), 1, 0)[0])).any(), name


def test_keys_select_the_stream(wpt, oracle):
    """What makes two rays of equal geometry and different keys differ somewhere
    in tests/test_gpu_rays.py's list: the streams of the keys it uses (0 .. 256,
    and those shifted by 1000) all differ, and a box path's value depends on its
    stream (every diffuse hit draws from it): the same pixels on another
    sample's streams give another frame. The oracle's own ray query holds the
    geometry and changes the key directly: tests/test_rays_oracle_cpu.py::test_keys
    (one ray under 300 keys gives more than 100 distinct answers), and
    tests/test_gpu_rays_adversarial.py compares the device's keyed answers with it."""
    L = oracle.lib()
    seeds = {L.oracle_path_seed(rf.SEED, k, 0) for k in list(range(257)) + list(range(1000, 1257))}
    assert len(seeds) == 514
    sc = rf.scene(wpt, oracle, "box")
    assert (rf.bits(sc.frame((17, 16), 1, 0)[0]) != rf.bits(sc.frame((17, 16), 1, 7)[0])).any()
