"""The point query on the device (wpt_radiance_points, wpt_points.h).

The expected value of every comparison is the definition's identity: a point's
sum is the sequential f32 sum over its samples of the ray query (spp = 1) along
wpt_point_rays' rays, answered by the oracle (OracleScene.radiance_rays) or, for
the large case, by wpt_radiance_rays on the device. Status bytes and the rises of
wpt_stats' paths, rays and shadow rays are compared too. Every comparison is bit
for bit.
"""
import numpy as np
import pytest

import pnee_fixtures as pf
import points_fixtures as px
import rays_fixtures as rf
import reproject_fixtures as rx

pytestmark = pytest.mark.gpu

INVALID = -4
SEED = px.SEED
DEPTH = px.DEPTH
DEFAULT_BATCH = 1 << 27
TOP = (1 << 32) - 300  # the last 300 sample indices


@pytest.fixture
def itf(wpt):
    i = wpt.interface
    yield i
    try:
        i.shutdown()
    except i.WptError:
        pass
    i.set_option("defaults", 0)


def _start(itf, sc, vp=(8, 8), settings=(0, 1, 0, 0), depth=DEPTH, batch=0, cam=None, photons=False, debug=0):
    itf.init(vp[0], vp[1], sc.scene_id, *(cam or sc.cam))
    if sc.mesh is not None:
        assert itf.store_mesh(1, sc.mesh)
    if settings is not None:
        itf.update_settings(*settings, debug)
    itf.set_render_options(depth, SEED, batch)
    if photons:
        itf.install_photons(pf.octants())


def _same(got, want, what):
    bad = np.any(px.bits(got) != px.bits(want), axis=1)
    assert not bad.any(), (what, "differs on", int(bad.sum()), "of", len(bad), "records, first", int(np.argmax(bad)),
                           got[np.argmax(bad)], want[np.argmax(bad)])


def _query(itf, *a, **kw):
    """(rgb, status, the rises of wpt_stats' paths, rays and shadow rays)."""
    s0 = itf.stats()
    rgb, status = itf.radiance_points(*a, **kw)
    s1 = itf.stats()
    return rgb, status, {k: s1[k] - s0[k] for k in ("paths", "rays", "shadow_rays")}


def _check(got, want, what):
    rgb, status, counts = got
    w_rgb, w_status, w_counts = want[:3]
    assert np.array_equal(status, w_status), what
    _same(rgb, w_rgb, what)
    assert counts == w_counts, (what, counts, w_counts)


# ---------------------------------------------------------------------------
# 1. Against the oracle
# ---------------------------------------------------------------------------
# (render type, depth cap, spp, first sample, light debug): every type, the depth
# caps 0 (Russian roulette only), 1 and 4, spp 1, 3, 64 and 300, samples 0, 7 and
# the last 300, the light-debug view
# (grouped by the session they need: depth cap and debug view)
COMBOS = [(0, 4, 1, 0, 0), (1, 4, 3, 7, 0), (2, 4, 3, 0, 0),
          (1, 1, 64, TOP, 0), (0, 1, 3, 0, 0), (2, 1, 64, 7, 0),
          (1, 0, 300, TOP, 0), (0, 0, 3, 7, 0),
          (1, 4, 3, 0, 1), (0, 4, 64, 7, 1), (2, 4, 1, TOP + 299, 1)]


@pytest.mark.parametrize("dist", [px.COSINE, px.SPHERE], ids=["cosine", "sphere"])
@pytest.mark.parametrize("name", list(rf.SCENES))
def test_against_oracle(wpt, oracle, itf, name, dist):
    sc, recs = px.point_set(wpt, oracle, name)
    pnee = name in rf.PNEE_SCENES
    state = None
    seen_nonzero = False
    for rtype, depth, spp, sample, debug in COMBOS:
        if rtype == 2 and not pnee:
            continue
        if state != (depth, debug):
            if state is not None:
                itf.shutdown()
            _start(itf, sc, depth=depth, photons=pnee, debug=debug)
            state = (depth, debug)
        want = px.set_expected(wpt, oracle, name, rtype, dist, sample, spp, depth, debug)
        got = _query(itf, recs, None, sample, spp, rtype, dist)
        _check(got, want, (name, dist, rtype, depth, spp, sample, debug))
        seen_nonzero |= bool((got[0] != 0).any())
        assert np.all(px.bits(got[0][got[1] == 0]) == 0)
    assert seen_nonzero


# ---------------------------------------------------------------------------
# 2. Sizes: the wave, the block, invalid records and invalid samples
# ---------------------------------------------------------------------------
def _size_records(wpt, oracle, variant):
    """257 records of the box set's surface points. spp1: invalid records at
    lanes 0 and 63 of the first wave and the whole third wave (records 128..191).
    spp3: records 85..170 invalid, which are all of positions 256..511 (the second
    block) at spp 3, and records 0..21, all of the first wave. mixed: MIXED_NORMAL
    records (valid and invalid samples in turn) at records 0, 1 and 200, so that at
    spp 130 their samples cross wave and block boundaries."""
    _, base = px.point_set(wpt, oracle, "box")
    ok = base[px.valid(base).astype(bool)][:40]
    recs = np.ascontiguousarray(np.tile(ok, (7, 1))[:257])
    if variant == "spp1":
        recs = px.rfr.with_invalid(recs, [0, 63] + list(range(128, 192)))
    elif variant == "spp3":
        recs = px.rfr.with_invalid(recs, list(range(0, 22)) + list(range(85, 171)))
    else:
        for i in (0, 1, 200):
            recs[i, 3:] = px.MIXED_NORMAL
    return recs


@pytest.mark.parametrize("variant,spp", [("spp1", 1), ("spp3", 3), ("mixed", 130)])
def test_sizes(wpt, oracle, itf, variant, spp):
    sc = rf.scene(wpt, oracle, "box")
    recs = _size_records(wpt, oracle, variant)
    rgb, status, _, traced = px.expected(wpt, sc.ref, recs, None, 5, spp, 1, px.COSINE)
    if variant == "mixed":
        # valid and invalid samples on both sides of the first wave boundary (position 64 of record 0)
        t0 = traced[:, 0]
        assert t0[:64].any() and not t0[:64].all() and t0[64:].any() and not t0[64:].all()
        assert (t0[:-1] != t0[1:]).sum() >= 8 and (traced[:, 200][:-1] != traced[:, 200][1:]).any()
    _start(itf, sc)
    for n in (257, 256, 255, 65, 64, 63, 1):
        got = _query(itf, recs[:n], None, 5, spp, 1, px.COSINE)
        assert np.array_equal(got[1], status[:n]), (variant, n)
        _same(got[0], rgb[:n], (variant, n))
        assert got[2]["paths"] == int(traced[:, :n].sum()), (variant, n)
    assert (rgb != 0).any()
    s0 = itf.stats()
    r0, st0 = itf.radiance_points(recs[:0])
    assert r0.shape == (0, 3) and st0.shape == (0,) and itf.stats() == s0
    # status may be NULL
    out = np.empty((257, 3), np.float32)
    assert wpt.lib().wpt_radiance_points(257, recs.ctypes.data, None, 5, spp, 1, 0, 0, out.ctypes.data, None) == 0
    _same(out, rgb, "status NULL")


# ---------------------------------------------------------------------------
# 3. Straddles: a block and a batch that start inside a record's samples
# ---------------------------------------------------------------------------
def _straddle_case(wpt, oracle, name, spp):
    sc, recs = px.point_set(wpt, oracle, name)
    if spp == 300:
        # six records: surface points, an invalid record, a far normal and a mixed one
        ok = np.nonzero(px.valid(recs))[0]
        recs = np.ascontiguousarray(recs[[ok[0], ok[1], len(recs) - 10, ok[2], len(recs) - 6, len(recs) - 1]])
    return sc, recs


@pytest.mark.parametrize("spp", [3, 300])
def test_straddles_batches_and_lanes(wpt, oracle, itf, spp):
    sc, recs = _straddle_case(wpt, oracle, "box", spp)
    keys = (np.arange(len(recs), dtype=np.uint32) * 7 + 3).astype(np.uint32)
    want = px.expected(wpt, sc.ref, recs, keys, 2, spp, 1, px.COSINE)
    assert (want[0] != 0).any() and not want[3].all() and (want[1] == 0).any()
    _start(itf, sc, batch=DEFAULT_BATCH)
    _check(_query(itf, recs, keys, 2, spp, 1, px.COSINE), want, ("default", spp))
    for batch in (64, 100, 257):
        itf.set_render_options(DEPTH, SEED, batch)
        for lanes in range(1, 9):
            itf.set_lanes(lanes)
            _check(_query(itf, recs, keys, 2, spp, 1, px.COSINE), want, ("batch", batch, "lanes", lanes, spp))


@pytest.mark.parametrize("spp", [3, 300])
def test_straddles_launch_settings(wpt, oracle, itf, spp):
    """Scene 2 (planes and a mesh: its depth-capped batches presolve): every
    presolve, drop-miss, shadow-presolve and fused setting, both traversals; both
    generators are reached."""
    sc, recs = _straddle_case(wpt, oracle, "cloud", spp)
    want = px.expected(wpt, sc.ref, recs, None, 1, spp, 1, px.SPHERE)
    _start(itf, sc, batch=100)
    for trav in (0, 1):
        itf.set_option("traversal", trav)
        itf.set_option("traversal_sh", trav)
        assert itf.get_option("scene_traversal") == trav
        for m in range(16):
            opts = {"presolve": m & 1, "drop_miss": (m >> 1) & 1, "presolve_shadow": (m >> 2) & 1, "fused": (m >> 3) & 1}
            for k, v in opts.items():
                itf.set_option(k, v)
            p0 = itf.stats()["presolved_rays"]
            _check(_query(itf, recs, None, 1, spp, 1, px.SPHERE), want, (trav, opts, spp))
            assert (itf.stats()["presolved_rays"] > p0) == bool(opts["presolve"]), (trav, opts)


# ---------------------------------------------------------------------------
# 4. The identity on the device
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dist", [px.COSINE, px.SPHERE], ids=["cosine", "sphere"])
def test_identity_with_the_ray_query(wpt, oracle, itf, dist):
    sc, recs = px.point_set(wpt, oracle, "box")
    _start(itf, sc)
    keys = np.arange(1000, 1000 + len(recs), dtype=np.uint32)
    for k in (None, keys):
        kk = np.arange(len(recs), dtype=np.uint32) if k is None else k
        for rtype, sample, spp in ((1, 0, 5), (0, TOP, 300)):
            parts = [itf.radiance_rays(itf.point_rays(recs, kk, SEED, sample + j, dist), kk, sample + j, 1, rtype)[0]
                     for j in range(spp)]
            got, status = itf.radiance_points(recs, k, sample, spp, rtype, dist)
            _same(got, rf.seq_sum(parts), (dist, rtype, sample, spp, k is None))
            assert np.array_equal(status, px.valid(recs))


@pytest.mark.parametrize("pointers", ["host", "device"])
def test_chunk_boundary(wpt, oracle, itf, pointers):
    """2^21 + 257 records at spp 1 on scene 100: the second chunk's records keep
    their keys (explicit ones, and with keys NULL their index in the call)."""
    import torch

    sc, base = px.point_set(wpt, oracle, "box")
    n = (1 << 21) + 257
    recs = np.ascontiguousarray(np.tile(base, (n // len(base) + 1, 1))[:n])
    rng = np.random.default_rng(0x706F696E)
    keys = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    _start(itf, sc)
    dev = torch.device("cuda", torch.cuda.current_device())
    for k in (None, keys):
        kk = np.arange(n, dtype=np.uint32) if k is None else k
        rays = itf.point_rays(recs, kk, SEED, 3, px.COSINE)
        if pointers == "device":
            d_k = None if k is None else torch.from_numpy(k.view(np.int32)).to(dev)
            want, w_st = itf.radiance_rays(torch.from_numpy(rays).to(dev), torch.from_numpy(kk.view(np.int32)).to(dev),
                                           3, 1, 1, device=True)
            s0 = itf.stats()
            got, st = itf.radiance_points(torch.from_numpy(recs).to(dev), d_k, 3, 1, 1, px.COSINE, device=True)
            s1 = itf.stats()
            assert got.device == want.device and st.dtype == torch.uint8
            got, st, want, w_st = got.cpu().numpy(), st.cpu().numpy(), want.cpu().numpy(), w_st.cpu().numpy()
        else:
            want, w_st = itf.radiance_rays(rays, kk, 3, 1, 1)
            s0 = itf.stats()
            got, st = itf.radiance_points(recs, k, 3, 1, 1, px.COSINE)
            s1 = itf.stats()
        assert np.array_equal(st, px.valid(recs))
        _same(got, want, (pointers, k is None))
        assert s1["paths"] - s0["paths"] == int(w_st.sum())
        tail = slice(1 << 21, n)
        assert (got[tail] != 0).any()
        # the tail under the keys of a chunk of its own would differ
        other = itf.radiance_points(recs[tail], None, 3, 1, 1, px.COSINE)[0]
        if k is None:
            assert (px.bits(other) != px.bits(got[tail])).any()


# ---------------------------------------------------------------------------
# 5. The session is not touched
# ---------------------------------------------------------------------------
def _session_state(itf, vp):
    acc, cnt = itf.read_radiance(*vp)
    return acc, cnt, itf.results(0, *vp), itf.results(1, *vp)


def _states_equal(a, b, what):
    for x, y, part in zip(a, b, ("radiance", "counts", "results(0)", "results(1)", "more", "more", "more", "more")):
        x, y = (px.bits(x), px.bits(y)) if x.dtype == np.float32 else (x, y)
        assert np.array_equal(x, y), (what, part)


def test_random_halves_continue_against_the_oracle(wpt, oracle, itf):
    """Two random halves, a cut mid-round, point queries of both distributions,
    then more samples: counts and radiance are the oracle's session in the same
    schedule, as if no query had happened."""
    sc, recs = px.point_set(wpt, oracle, "box")
    vp = (16, 16)
    a, b = 300, 3000
    _start(itf, sc, vp, settings=(0, 1, 0, 0))
    itf.compute(a)
    mid = _session_state(itf, vp)
    assert mid[1].min() < mid[1].max()  # a round is cut
    for dist in (px.COSINE, px.SPHERE):
        rgb, status = itf.radiance_points(recs, None, 1, 3, 1, dist)
        assert (rgb != 0).any() and not status.all()
    _states_equal(_session_state(itf, vp), mid, "right after the queries")
    itf.compute(b)
    acc, cnt = itf.read_radiance(*vp)
    ref = sc.ref.adaptive(vp[0], vp[1], sc.cam, (0, 1), (0, 0), DEPTH, SEED)
    ref.compute(a)
    ref.compute(b)
    acc_r, cnt_r, _ = ref.read()
    assert np.array_equal(cnt, cnt_r)
    assert np.array_equal(px.bits(acc), px.bits(acc_r))


def test_init_default_session_continues_as_its_twin(wpt, oracle, itf):
    """The init-default session (NEE random + PNEE adaptive, the sample stock,
    installed photons), a cut in the adaptive half's first round, with a kept
    history and a planned map: queries or none, then the map is traced and more
    is computed; the frame, the options and the guide planes' consumers (wpt_denoise,
    wpt_reproject) give the same as the twin that made no query."""
    sc, recs = px.point_set(wpt, oracle, "box")
    vp = (16, 16)
    npx = vp[0] * vp[1]
    states = []
    for query in (True, False):
        _start(itf, sc, vp, settings=None, photons=True)
        itf.compute(300)
        mid = _session_state(itf, vp)
        assert mid[1].min() < mid[1].max()
        if query:
            for t, dist in ((1, px.COSINE), (2, px.SPHERE)):
                rgb, status = itf.radiance_points(recs, None, 1, 3, t, dist)
                assert (rgb != 0).any()
            _states_equal(_session_state(itf, vp), mid, "right after the queries")
        itf.compute(3000)
        assert itf.stats()["stock_consumed"] > 0
        states.append(_session_state(itf, vp))
        itf.shutdown()
    _states_equal(states[0], states[1], "init default")
    cam_a, cam_b = rx.PAIRS["sideways"]
    frames = []
    for query in (True, False):
        _start(itf, sc, vp, settings=(1, 1, 0, 0), cam=cam_a)
        itf.compute(4 * npx)
        itf.reproject(0, flags=rx.KEEP)
        itf.update_camera(*cam_b)
        itf.compute(npx)
        before = itf.denoise(0) + itf.reproject(0) + itf.denoise_merged()
        count, (T, _) = itf.sample_map(0, target=6, max_per_pixel=6)
        assert T > 0
        opts = {k: itf.get_option(k) for k in ("history", "map_mode")}
        assert opts == {"history": 1, "map_mode": 0}
        if query:
            itf.radiance_points(recs, None, 0, 2, 1, px.COSINE)
            assert opts == {k: itf.get_option(k) for k in ("history", "map_mode")}
        # the planes the last reproject left on the device, then the guide planes' consumers anew
        after = itf.denoise_merged()
        after = itf.denoise(0) + itf.reproject(0) + after
        for x, y in zip(after, before):
            assert np.array_equal(px.rfr.bits(x), px.rfr.bits(y))
        itf.compute_map(None)
        assert itf.get_option("map_mode") == 1
        if query:
            itf.radiance_points(recs, None, 0, 2, 0, px.SPHERE)
            assert itf.get_option("map_mode") == 1 and itf.get_option("history") == 1
        frames.append(itf.read_radiance(*vp) + (itf.reproject(0)[2],) + itf.denoise(0))
        assert np.array_equal(frames[-1][1], 1 + count)
        itf.shutdown()
    for x, y in zip(frames[0], frames[1]):
        assert np.array_equal(px.rfr.bits(x), px.rfr.bits(y))


# ---------------------------------------------------------------------------
# 6. The argument errors
# ---------------------------------------------------------------------------
def test_argument_errors(wpt, oracle, itf):
    sc, base = px.point_set(wpt, oracle, "box")
    _start(itf, sc)
    L = wpt.lib()
    recs = np.ascontiguousarray(base[:20])
    keys = np.arange(20, dtype=np.uint32)
    rgb = np.full((20, 3), 7.25, np.float32)
    status = np.full(20, 9, np.uint8)
    r, k, o, s = recs.ctypes.data, keys.ctypes.data, rgb.ctypes.data, status.ctypes.data
    s0 = itf.stats()
    for c in ((20, None, k, 0, 1, 1, 0, 0, o, s), (20, r, k, 0, 1, 1, 0, 0, None, s), (20, r, k, 0, 0, 1, 0, 0, o, s),
              (20, r, k, 0, 1, 3, 0, 0, o, s), (20, r, k, 0, 1, 1, 2, 0, o, s), (20, r, k, 0, 1, 1, 0xFFFFFFFF, 0, o, s),
              (20, r, k, 0, 1, 1, 0, 2, o, s), (20, r, k, 0, 1, 1, 1, 0x80000000, o, s),
              (20, r, k, 0xFFFFFFFF, 2, 1, 0, 0, o, s), (20, r, k, 2, 0xFFFFFFFF, 1, 0, 0, o, s),
              (1 << 32, r, k, 0, 1, 1, 0, 0, o, s), (0, None, None, 0, 0, 1, 0, 0, None, None)):
        assert L.wpt_radiance_points(*c) == INVALID, c
        assert len(L.wpt_last_error()) > 0
    assert np.all(rgb == np.float32(7.25)) and np.all(status == 9)
    assert itf.stats() == s0
    # the largest sample index, and a degenerate call
    assert L.wpt_radiance_points(20, r, k, 0xFFFFFFFE, 2, 1, 1, 0, o, s) == 0
    assert np.array_equal(status, px.valid(recs))
    assert L.wpt_radiance_points(0, None, None, 0, 1, 1, 0, 0, None, None) == 0
