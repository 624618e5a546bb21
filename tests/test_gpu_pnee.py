"""PNEE light sampler on the device: photon_sample (wpt_render.hip) through
the wpt_photon_sample hook and through whole frames, against the oracle
holding the same photon list, bit for bit, on the trees, point sets and RNG
states of pnee_fixtures.py (their conditions: test_pnee_cpu.py).

A NaN pdf (a NaN hit point, a collapsed cell, an overflowed CDF) compares equal
to a NaN pdf: IEEE 754 leaves the sign and payload of an invalid operation's
result to the implementation, and the host's differ from the device's.
"""
import functools

import numpy as np
import pytest

import pnee_fixtures as fx

pytestmark = pytest.mark.gpu

LDS_WORDS = 6144  # kOctLdsWords
SEED = 0xBABABEBE


def _views(T):
    """The views a tree fits, and the one a session's shade kernel uses."""
    nodes, words = T.child.size, T.child.size + T.cum.size
    fits = [0] + ([1] if nodes <= LDS_WORDS else []) + ([2] if words <= LDS_WORDS else [])
    return fits, fits[-1]


@functools.lru_cache(maxsize=None)
def _cases(name):
    """Every point set under random states, and every tie class: one batch per
    tree, (points, states, [(label, slice)]) plus the oracle's answer."""
    T = fx.tree(name)
    pts, sts, labels, at = [], [], [], 0
    for k, (s, p) in enumerate(T.sets.items()):
        pts.append(p)
        sts.append(fx.random_states(len(p), seed=0x6B0 + k))
        labels.append((s, slice(at, at + len(p))))
        at += len(p)
    for cls, (p, st) in T.ties.items():
        pts.append(p)
        sts.append(st)
        labels.append(("tie:" + cls, slice(at, at + len(p))))
        at += len(p)
    pts, sts = np.concatenate(pts), np.concatenate(sts)
    ref = fx.oracle_with(T).photon_sample(pts, sts)
    return pts, sts, labels, ref


def _bits(pdf):
    b = pdf.view(np.uint32).copy()
    b[np.isnan(pdf)] = 0x7FC00000
    return b


def _assert_same(got, want, labels, what):
    for field, g, w in (("light", got[0], want[0]), ("pdf", _bits(got[1]), _bits(want[1])), ("state", got[2], want[2])):
        if np.array_equal(g, w):
            continue
        for label, sl in labels:
            bad = np.nonzero(g[sl] != w[sl])[0]
            assert len(bad) == 0, (f"{what}: {field} differs on {len(bad)} of {sl.stop - sl.start} points of set "
                                   f"{label}, first at {bad[0]}: {g[sl][bad[0]]} != {w[sl][bad[0]]}")


@pytest.fixture
def itf(wpt):
    i = wpt.interface
    yield i
    try:
        i.shutdown()
    except i.WptError:
        pass


def _start(itf, wpt, T, max_depth=4, lanes=None, w=32, h=24):
    scene = fx.SCENE_OF_LIGHTS[T.L]
    cam = wpt.scenes.scene_camera(scene)
    itf.init(w, h, scene, *cam)
    itf.update_settings(2, 2, 0, 0, 0)
    itf.set_render_options(max_depth, SEED, 0)
    if lanes is not None:
        itf.set_lanes(lanes)
    assert itf.get_option("oct_view") == -1
    itf.install_photons(T.photons)
    return cam


def _hook_parity(itf, wpt, name):
    T = fx.tree(name)
    _start(itf, wpt, T)
    fits, used = _views(T)
    assert itf.get_option("oct_view") == used
    # the installed tree is the host builder's, which the CPU suite holds against the oracle's
    child, cum, shot, stored = itf.photon_tree(T.L)
    assert np.array_equal(child, T.child) and np.array_equal(cum.view(np.uint32), T.cum.view(np.uint32))
    assert (shot, stored) == (0, len(T.photons[0]))
    pts, sts, labels, ref = _cases(name)
    for view in (0, 1, 2):
        if view not in fits:
            with pytest.raises(itf.WptError) as e:
                itf.photon_sample(pts[:4], sts[:4], view)
            assert e.value.code == itf.ERR_INVALID_ARG
            continue
        on = itf.photon_sample(pts, sts, view, table=True)
        off = itf.photon_sample(pts, sts, view, table=False)
        assert np.all(on[0] < T.L) and np.all(off[0] < T.L)
        _assert_same(on, ref, labels, f"{name} view {view} table on")
        _assert_same(off, ref, labels, f"{name} view {view} table off")
    return pts, sts, labels, fits


@pytest.mark.parametrize("name", [n for n in fx.TREES if n not in fx.WILD_TREES])
def test_hook_parity(wpt, itf, name):
    """Light, pdf bits and state out of the device's photon_sample equal the
    oracle's for every point set and state class of the tree, in every view
    the tree fits, with the corner table and without; every light is < the
    light count; a view the tree does not fit is WPT_ERR_INVALID_ARG."""
    _hook_parity(itf, wpt, name)


def test_hook_parity_collapsed(wpt, itf):
    """The split chain down to the depth-120 guard: cell sizes of 0, weights
    of NaN and inf. The reference would never return from building this tree."""
    _hook_parity(itf, wpt, "collapsed")


def test_hook_parity_overflowed_weights(wpt, itf):
    """Bin sums that overflow, CDFs of inf and NaN, negative bins. The
    reference would panic in its weight assertions or index out of bounds."""
    _hook_parity(itf, wpt, "weights_wild")


@pytest.mark.parametrize("name", list(fx.TREES))
def test_table_against_walks(wpt, itf, name):
    """The corner table changes nothing: with it and without it (oct_corners
    null: the lattice branch walks every neighbour) the results are identical,
    in every view."""
    T = fx.tree(name)
    _start(itf, wpt, T)
    pts, sts, labels, _ = _cases(name)
    for view in _views(T)[0]:
        on = itf.photon_sample(pts, sts, view, table=True)
        off = itf.photon_sample(pts, sts, view, table=False)
        _assert_same(on, off, labels, f"{name} view {view}: table on against off")


@pytest.mark.parametrize("lanes", [1, 4])
@pytest.mark.parametrize("max_depth", [4, 0])
@pytest.mark.parametrize("name", ["octants", "deep", "wide", "many_lights"])
def test_render_with_installed_tree(wpt, itf, name, max_depth, lanes):
    """PNEE frames of 32x24, 4 spp, with an installed tree, bit-exact against
    the oracle holding the same list: k_shade's three views (`octants` and
    `deep` 2, `many_lights` 1, `wide` 0; a scene 100 session's own tree, view
    1, is test_reset_shoots_own_tree_again's), depth cap 4 and uncapped (the
    finishing kernel reads the tree from global memory), 1 and 4 lanes."""
    W, H, spp = 32, 24, 4
    T = fx.tree(name)
    cam = _start(itf, wpt, T, max_depth, lanes, W, H)
    want_view = {"octants": 2, "deep": 2, "wide": 0, "many_lights": 1}[name]
    assert _views(T)[1] == want_view and itf.get_option("oct_view") == want_view
    itf.compute(W * H * spp)
    acc, cnt = itf.read_radiance(W, H)
    st = itf.stats()
    ref, rst = fx.oracle_with(T).render(W, H, cam, 2, 2, max_depth, SEED, 0, spp, threads=8)
    assert np.all(cnt == spp)
    assert st["photons"] == 0 and st["photon_rays"] == 0  # nothing was shot
    assert st["rays"] + st["shadow_rays"] == rst["rays"]
    exact = np.mean(np.all(acc.view(np.uint32) == ref.view(np.uint32), axis=2))
    print(f"{name} depth {max_depth} lanes {lanes}: bit-exact pixels {exact:.6f}")
    assert exact == 1.0


def test_reset_shoots_own_tree_again(wpt, itf, oracle):
    """What drops a shot tree drops an installed one: after update_scene the
    session shoots its own 300000 photons and renders the frame it renders
    today; a new frame seed does the same."""
    W, H, spp, depth = 32, 24, 4, 4
    T = fx.tree("octants")
    cam = _start(itf, wpt, T, depth, None, W, H)
    itf.compute(W * H * spp)
    installed, _ = itf.read_radiance(W, H)
    itf.update_scene(100)
    assert itf.get_option("oct_view") == -1
    itf.update_settings(2, 2, 0, 0, 0)
    itf.set_render_options(depth, SEED, 0)
    itf.compute(W * H * spp)
    acc, _ = itf.read_radiance(W, H)
    assert itf.stats()["photons"] == 300000
    assert itf.get_option("oct_view") == 1  # scene 100: 2089 nodes, 6267 words with the CDFs
    plain = oracle.OracleScene(100)
    ref, _ = plain.render(W, H, cam, 2, 2, depth, SEED, 0, spp, threads=8)
    assert np.array_equal(acc.view(np.uint32), ref.view(np.uint32))
    assert not np.array_equal(acc.view(np.uint32), installed.view(np.uint32))
    # a new frame seed
    itf.install_photons(T.photons)
    assert itf.get_option("oct_view") == 2
    itf.set_render_options(depth, SEED + 1, 0)
    assert itf.get_option("oct_view") == -1
    child, _, shot, stored = itf.photon_tree(2)
    assert stored == 300000 and shot > 0 and len(child) > 9


def test_install_errors(wpt, itf):
    i = itf
    with pytest.raises(i.WptError) as e:
        i.install_photons(fx.tree("octants").photons)
    assert e.value.code == i.ERR_NOT_INIT
    T = fx.tree("octants")
    _start(i, wpt, T)
    li = T.photons[0].copy()
    li[3] = 2  # scene 100 has lights 0 and 1
    with pytest.raises(i.WptError) as e:
        i.install_photons((li, T.photons[1], T.photons[2]))
    assert e.value.code == i.ERR_INVALID_ARG
    assert i.get_option("oct_view") == 2  # the tree installed before stays
    with pytest.raises(i.WptError) as e:
        i.set_option("oct_view", 0)
    assert e.value.code == i.ERR_INVALID_ARG
    with pytest.raises(i.WptError) as e:
        i.photon_sample(np.zeros((1, 3), np.float32), np.ones(1, np.uint32), 3)
    assert e.value.code == i.ERR_INVALID_ARG
