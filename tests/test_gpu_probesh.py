"""The SH projection of a point's gathers on the device (wpt_probe_sh, wpt_sh.h).

The expected value of every comparison is the definition: a record's coefficient
k is the sequential f32 sum over its traced samples of Y_k(w_j) * c_j, with c_j
the oracle's ray query (OracleScene.radiance_rays, spp = 1) along wpt_point_rays'
ray (o_j, w_j) and Y_k the numpy-f32 restatement of the basis
(probesh_fixtures.expected). Status bytes and the rises of wpt_stats' paths, rays
and shadow rays are compared too. Every comparison is bit for bit.
"""
import numpy as np
import pytest

import pnee_fixtures as pf
import points_fixtures as px
import probesh_fixtures as ps
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


def _start(itf, sc, vp=(8, 8), settings=(0, 1, 0, 0), depth=DEPTH, batch=0, cam=None, photons=False):
    itf.init(vp[0], vp[1], sc.scene_id, *(cam or sc.cam))
    if sc.mesh is not None:
        assert itf.store_mesh(1, sc.mesh)
    if settings is not None:
        itf.update_settings(*settings, 0)
    itf.set_render_options(depth, SEED, batch)
    if photons:
        itf.install_photons(pf.octants())


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.any(ps.bits(got).reshape(len(got), -1) != ps.bits(want).reshape(len(want), -1), axis=1)
    assert not bad.any(), (what, "differs on", int(bad.sum()), "of", len(bad), "records, first", int(np.argmax(bad)),
                           got[np.argmax(bad)], want[np.argmax(bad)])


def _query(itf, *a, **kw):
    """(sh, status, the rises of wpt_stats' paths, rays and shadow rays)."""
    s0 = itf.stats()
    sh, status = itf.probe_sh(*a, **kw)
    s1 = itf.stats()
    return sh, status, {k: s1[k] - s0[k] for k in ("paths", "rays", "shadow_rays")}


def _check(got, want, what):
    sh, status, counts = got
    w_sh, w_status, w_counts = want[:3]
    assert np.array_equal(status, w_status), what
    _same(sh, w_sh, what)
    assert counts == w_counts, (what, counts, w_counts)


# ---------------------------------------------------------------------------
# 1. Against the oracle
# ---------------------------------------------------------------------------
# (render type, depth cap, spp, first sample, order): NoNEE, NEE and PNEE (with an
# installed photon list, once), the depth caps 0 (Russian roulette only), 1 and 4,
# spp 1, 3, 64 and 300, samples 0, 7 and the last 300, every order
# (grouped by the session they need: the depth cap)
COMBOS = [(0, 4, 1, 0, 2), (1, 4, 3, 7, 2), (2, 4, 3, 0, 2), (1, 4, 3, 7, 1), (1, 4, 3, 7, 0),
          (1, 1, 64, TOP, 2), (0, 1, 3, 0, 1),
          (1, 0, 300, TOP, 2), (0, 0, 3, 7, 0)]


@pytest.mark.parametrize("dist", [px.COSINE, px.SPHERE], ids=["cosine", "sphere"])
@pytest.mark.parametrize("name", list(rf.SCENES))
def test_against_oracle(wpt, oracle, itf, name, dist):
    sc, recs = px.point_set(wpt, oracle, name)
    pnee = name == "box"  # PNEE with an installed photon list: once
    state = None
    seen_nonzero = False
    by_order = {}
    for rtype, depth, spp, sample, order in COMBOS:
        if rtype == 2 and not pnee:
            continue
        if state != depth:
            if state is not None:
                itf.shutdown()
            _start(itf, sc, depth=depth, photons=pnee)
            state = depth
        want = ps.set_expected(wpt, oracle, name, rtype, dist, sample, spp, depth, 0, order)
        got = _query(itf, recs, None, sample, spp, rtype, dist, order)
        _check(got, want, (name, dist, rtype, depth, spp, sample, order))
        assert got[0].shape == (len(recs), ps.ncoef(order), 3)
        seen_nonzero |= bool((got[0] != 0).any())
        # an invalid record's row is all +0
        assert np.all(ps.bits(got[0][got[1] == 0]) == 0)
        if (rtype, depth, spp, sample) == (1, 4, 3, 7):
            by_order[order] = got[0]
    assert seen_nonzero
    # the prefix property: a lower order's coefficients lead a higher order's
    assert sorted(by_order) == [0, 1, 2]
    _same(by_order[0], by_order[2][:, :1], (name, dist, "prefix 0 of 2"))
    _same(by_order[1], by_order[2][:, :4], (name, dist, "prefix 1 of 2"))


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
    sh, status, _, traced = ps.expected(wpt, sc.ref, recs, None, 5, spp, 1, px.COSINE)
    if variant == "mixed":
        # valid and invalid samples on both sides of the first wave boundary (position 64 of record 0)
        t0 = traced[:, 0]
        assert t0[:64].any() and not t0[:64].all() and t0[64:].any() and not t0[64:].all()
        assert (t0[:-1] != t0[1:]).sum() >= 8 and (traced[:, 200][:-1] != traced[:, 200][1:]).any()
    assert np.isfinite(sh).all()
    _start(itf, sc)
    for n in (257, 256, 255, 65, 64, 63, 1):
        got = _query(itf, recs[:n], None, 5, spp, 1, px.COSINE)
        assert np.array_equal(got[1], status[:n]), (variant, n)
        _same(got[0], sh[:n], (variant, n))
        assert got[2]["paths"] == int(traced[:, :n].sum()), (variant, n)
    assert (sh != 0).any()
    s0 = itf.stats()
    r0, st0 = itf.probe_sh(recs[:0])
    assert r0.shape == (0, 9, 3) and st0.shape == (0,) and itf.stats() == s0
    # status may be NULL
    out = np.empty((257, 9, 3), np.float32)
    assert wpt.lib().wpt_probe_sh(257, recs.ctypes.data, None, 5, spp, 1, 0, 2, 0, out.ctypes.data, None) == 0
    _same(out, sh, "status NULL")


# ---------------------------------------------------------------------------
# 3. Straddles: a lane, a block and a batch that start inside a record's samples
#    (the run then starts with sums already in the target)
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
    want = ps.expected(wpt, sc.ref, recs, keys, 2, spp, 1, px.COSINE)
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
    want = ps.expected(wpt, sc.ref, recs, None, 1, spp, 1, px.SPHERE)
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
# 4. Keys
# ---------------------------------------------------------------------------
def test_edge_and_random_keys(wpt, oracle, itf):
    sc, recs = px.point_set(wpt, oracle, "box")
    rng = np.random.default_rng(0x53484B)
    keys = rng.integers(0, 1 << 32, len(recs), dtype=np.uint64).astype(np.uint32)
    keys[:6] = (0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF)
    _start(itf, sc)
    for sample, spp in ((0, 3), ((1 << 32) - 3, 3)):  # the second: samples ending at 2^32 - 1
        want = ps.expected(wpt, sc.ref, recs, keys, sample, spp, 1, px.SPHERE)
        _check(_query(itf, recs, keys, sample, spp, 1, px.SPHERE), want, ("keys", sample))
    # keys NULL is the record's index
    a = itf.probe_sh(recs, None, 0, 3, 1, px.SPHERE)[0]
    b = itf.probe_sh(recs, np.arange(len(recs), dtype=np.uint32), 0, 3, 1, px.SPHERE)[0]
    _same(a, b, "keys NULL")


# ---------------------------------------------------------------------------
# 5. Agreement with wpt_radiance_points
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dist", [px.COSINE, px.SPHERE], ids=["cosine", "sphere"])
def test_agrees_with_radiance_points(wpt, oracle, itf, dist):
    """Status and counts equal wpt_radiance_points' for the same arguments, and
    coefficient 0 / C0 is its sum to (spp + 2) * 2^-23 relative: the terms are
    non-negative, and each side rounds once per product and per addition."""
    sc, recs = px.point_set(wpt, oracle, "box")
    _start(itf, sc)
    for rtype, sample, spp in ((1, 0, 5), (0, TOP, 300), (1, 3, 64)):
        s0 = itf.stats()
        rgb, st_p = itf.radiance_points(recs, None, sample, spp, rtype, dist)
        s1 = itf.stats()
        sh, st, counts = _query(itf, recs, None, sample, spp, rtype, dist, 2)
        assert np.array_equal(st, st_p)
        assert counts == {k: s1[k] - s0[k] for k in counts}, (dist, rtype, sample, spp)
        est = sh[:, 0, :].astype(np.float64) / float(ps.C0)
        ref = rgb.astype(np.float64)
        assert (ref >= 0).all() and (ref > 0).any()
        bound = (spp + 2) * 2.0 ** -23 * ref
        print(dist, rtype, spp, "worst |c0 / C0 - sum| / bound", float(np.max(np.abs(est - ref)[ref > 0] / bound[ref > 0])))
        assert np.all(np.abs(est - ref) <= bound), (dist, rtype, sample, spp)


# ---------------------------------------------------------------------------
# 6. The chunk boundary
# ---------------------------------------------------------------------------
def test_chunk_boundary(wpt, oracle, itf):
    """WPT_SH_CHUNK + 257 records at spp 1 on scene 100 through host and device
    pointers: the same bits; the records about the boundary and a seeded subset of
    512 agree with the oracle, so the second chunk's records keep their keys
    (explicit ones, and with keys NULL their index in the call)."""
    import torch

    sc, base = px.point_set(wpt, oracle, "box")
    chunk = itf.SH_CHUNK
    n = chunk + 257
    recs = np.ascontiguousarray(np.tile(base, (n // len(base) + 1, 1))[:n])
    rng = np.random.default_rng(0x53484348)
    keys = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    pick = np.unique(np.concatenate([np.arange(chunk - 4, chunk + 4), [0, n - 1], rng.choice(n, 512, replace=False)]))
    _start(itf, sc)
    dev = torch.device("cuda", torch.cuda.current_device())
    d_recs = torch.from_numpy(recs).to(dev)
    for k in (None, keys):
        kk = np.arange(n, dtype=np.uint32) if k is None else k
        s0 = itf.stats()
        got, st = itf.probe_sh(recs, k, 3, 1, 1, px.COSINE, 2)
        s1 = itf.stats()
        d_k = None if k is None else torch.from_numpy(k.view(np.int32)).to(dev)
        d_got, d_st = itf.probe_sh(d_recs, d_k, 3, 1, 1, px.COSINE, 2, device=True)
        s2 = itf.stats()
        assert d_got.device == d_recs.device and d_st.dtype == torch.uint8 and tuple(d_got.shape) == (n, 9, 3)
        assert all(s2[c] - s1[c] == s1[c] - s0[c] > 0 for c in ("paths", "rays", "shadow_rays"))
        _same(d_got.cpu().numpy(), got, ("device against host", k is None))
        assert np.array_equal(d_st.cpu().numpy(), st) and np.array_equal(st, px.valid(recs))
        want = ps.expected(wpt, sc.ref, recs[pick], kk[pick], 3, 1, 1, px.COSINE)
        _same(got[pick], want[0], ("chunk boundary", k is None))
        assert (got[chunk:] != 0).any() and (got[:chunk] != 0).any()
        if k is None:
            # the tail under the keys of a call of its own would differ
            other = itf.probe_sh(recs[chunk:], None, 3, 1, 1, px.COSINE, 2)[0]
            assert (ps.bits(other) != ps.bits(got[chunk:])).any()


# ---------------------------------------------------------------------------
# 7. The session is not touched
# ---------------------------------------------------------------------------
def _session_state(itf, vp):
    acc, cnt = itf.read_radiance(*vp)
    return acc, cnt, itf.results(0, *vp), itf.results(1, *vp)


def _states_equal(a, b, what):
    for x, y, part in zip(a, b, ("radiance", "counts", "results(0)", "results(1)")):
        x, y = (px.bits(x), px.bits(y)) if x.dtype == np.float32 else (x, y)
        assert np.array_equal(x, y), (what, part)


def test_random_halves_continue_against_the_oracle(wpt, oracle, itf):
    """Two random halves, a cut mid-round, SH queries of both distributions, then
    more samples: counts and radiance are the oracle's session in the same
    schedule, as if no query had happened."""
    sc, recs = px.point_set(wpt, oracle, "box")
    vp = (16, 16)
    a, b = 300, 3000
    _start(itf, sc, vp, settings=(0, 1, 0, 0))
    itf.compute(a)
    mid = _session_state(itf, vp)
    assert mid[1].min() < mid[1].max()  # a round is cut
    for dist in (px.COSINE, px.SPHERE):
        sh, status = itf.probe_sh(recs, None, 1, 3, 1, dist)
        assert (sh != 0).any() and not status.all()
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
    installed photons), a cut in the adaptive half's first round; then a session
    with a kept history and a planned map: SH queries or none, then the map is
    traced and more is computed; frame, counts, options and the guide planes'
    consumers give the same as the twin that made no query."""
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
                sh, status = itf.probe_sh(recs, None, 1, 3, t, dist)
                assert (sh != 0).any()
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
            itf.probe_sh(recs, None, 0, 2, 1, px.COSINE)
            assert opts == {k: itf.get_option(k) for k in ("history", "map_mode")}
        after = itf.denoise_merged()
        after = itf.denoise(0) + itf.reproject(0) + after
        for x, y in zip(after, before):
            assert np.array_equal(px.rfr.bits(x), px.rfr.bits(y))
        itf.compute_map(None)
        assert itf.get_option("map_mode") == 1
        if query:
            itf.probe_sh(recs, None, 0, 2, 0, px.SPHERE)
            assert itf.get_option("map_mode") == 1 and itf.get_option("history") == 1
        frames.append(itf.read_radiance(*vp) + (itf.reproject(0)[2],) + itf.denoise(0))
        assert np.array_equal(frames[-1][1], 1 + count)
        itf.shutdown()
    for x, y in zip(frames[0], frames[1]):
        assert np.array_equal(px.rfr.bits(x), px.rfr.bits(y))


# ---------------------------------------------------------------------------
# 8. The argument errors
# ---------------------------------------------------------------------------
def test_argument_errors(wpt, oracle, itf):
    sc, base = px.point_set(wpt, oracle, "box")
    _start(itf, sc)
    L = wpt.lib()
    recs = np.ascontiguousarray(base[:20])
    keys = np.arange(20, dtype=np.uint32)
    sh = np.full((20, 9, 3), 7.25, np.float32)
    status = np.full(20, 9, np.uint8)
    r, k, o, s = recs.ctypes.data, keys.ctypes.data, sh.ctypes.data, status.ctypes.data
    s0 = itf.stats()
    # (n, points6, keys, sample, spp, type, dist, order, flags, sh, status)
    for c in ((20, None, k, 0, 1, 1, 0, 2, 0, o, s), (20, r, k, 0, 1, 1, 0, 2, 0, None, s), (20, r, k, 0, 0, 1, 0, 2, 0, o, s),
              (20, r, k, 0, 1, 3, 0, 2, 0, o, s), (20, r, k, 0, 1, 1, 2, 2, 0, o, s), (20, r, k, 0, 1, 1, 0xFFFFFFFF, 2, 0, o, s),
              (20, r, k, 0, 1, 1, 0, 3, 0, o, s), (20, r, k, 0, 1, 1, 0, 0xFFFFFFFF, 0, o, s),
              (20, r, k, 0, 1, 1, 0, 2, 2, o, s), (20, r, k, 0, 1, 1, 1, 2, 0x80000000, o, s),
              (20, r, k, 0xFFFFFFFF, 2, 1, 0, 2, 0, o, s), (20, r, k, 2, 0xFFFFFFFF, 1, 0, 2, 0, o, s),
              (1 << 32, r, k, 0, 1, 1, 0, 2, 0, o, s), (0, None, None, 0, 0, 1, 0, 2, 0, None, None),
              (0, None, None, 0, 1, 1, 0, 3, 0, None, None)):
        assert L.wpt_probe_sh(*c) == INVALID, c
        assert len(L.wpt_last_error()) > 0
    assert np.all(sh == np.float32(7.25)) and np.all(status == 9)
    assert itf.stats() == s0
    # the largest sample index, and a degenerate call
    assert L.wpt_probe_sh(20, r, k, 0xFFFFFFFE, 2, 1, 1, 2, 0, o, s) == 0
    assert np.array_equal(status, px.valid(recs))
    assert L.wpt_probe_sh(0, None, None, 0, 1, 1, 0, 2, 0, None, None) == 0
