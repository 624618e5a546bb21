"""A viewport change on an adaptive session that holds a live sample-stock ring
(wpt_update_viewport, wasm_interface.rs:219-232): the counts are reallocated at
the new size before the partition is rebuilt, so the old ring must not be
touched through the old pixel list any more. The session then makes a new ring
(or reuses one of the same size) and renders the new viewport from scratch:
bit for bit the oracle's fresh session at that size. One rank, and two ranks
with WPT_OPT_STOCK_RANKS (each its own ring over its partition).
"""
import numpy as np
import pytest

from test_gpu_stock_multirank import BASE, _assert_union, _cfg, _oracle_session, _run_ranks

pytestmark = pytest.mark.gpu

TYPES, ADAPTIVE, DEPTH = (2, 1), (1, 1), 4
BEFORE = 48 * 32 * 6 + 17  # cuts a round: refills in flight, a round partly added


def _after(W, H):
    return (W * H * 6 + 5, 300, W * H * 5)


# a smaller viewport (the old pixel list indexes past the new counts), and one
# of the same pixel count (the ring is kept, its frontier reset)
@pytest.mark.parametrize("size", [(40, 24), (32, 48)])
def test_resize_with_live_ring_one_rank(wpt, oracle, cloud_small, size):
    itf = wpt.interface
    W, H = size
    cam = list(wpt.scenes.scene_camera(2))
    try:
        for k, v in BASE.items():
            itf.set_option(k, v)  # the defaults of the init below
        itf.init(48, 32, 2, *cam)
        itf.store_mesh(1, cloud_small)
        itf.update_settings(*TYPES, *ADAPTIVE, 0)
        itf.set_render_options(DEPTH, 0xBABABEBE, 0)
        itf.compute(BEFORE)
        assert itf.stats()["stock_consumed"] > 0 and itf.get_option("stock_ring_bytes") == 20 * 256 * 48 * 32
        itf.update_viewport(W, H)
        for n in _after(W, H):
            itf.compute(n)
        acc, cnt = itf.read_radiance(W, H)
        samp = itf.results(1, W, H)
        ring = itf.get_option("stock_ring_bytes")
    finally:
        try:
            itf.shutdown()
        except itf.WptError:
            pass
        itf.set_option("defaults", 0)
    ref = oracle.OracleScene(2, cloud_small).adaptive(W, H, cam, TYPES, ADAPTIVE, DEPTH)
    for n in _after(W, H):
        ref.compute(n)
    acc_r, cnt_r, samp_r = ref.read()
    assert ring == 20 * 256 * W * H
    assert cnt_r.max() > 8
    assert np.array_equal(cnt, cnt_r)
    assert np.array_equal(acc.view(np.uint32), acc_r.view(np.uint32))
    assert np.array_equal(samp, samp_r)


def test_shrink_with_live_rings_two_ranks(wpt, oracle, cloud_small):
    W, H = 40, 24  # 15 tiles of 8 px dealt 8 / 7
    steps = [("compute", BEFORE), ("snap",), ("viewport", W, H)] + [("compute", n) for n in _after(W, H)] + [("snap",)]
    cfg = _cfg(wpt, (48, 32), 8, 2, TYPES, ADAPTIVE, DEPTH, {}, steps)
    res = _run_ranks(2, cfg)
    ref0 = _oracle_session(oracle, cfg, cloud_small)
    ref0.compute(BEFORE)
    _assert_union(res, 0, cfg, ref0)
    ref = _oracle_session(oracle, dict(cfg, size=(W, H)), cloud_small)
    for n in _after(W, H):
        ref.compute(n)
    _assert_union(res, 1, cfg, ref)
    assert sorted(len(r[3][1]["px"]) for r in res) == [7 * 64, 8 * 64]
    for rank, _, _, snaps in res:
        assert snaps[0]["stats"]["stock_consumed"] > 0 and snaps[0]["ring"] == 20 * 256 * 768, rank
        assert snaps[1]["ring"] == 20 * 256 * len(snaps[1]["px"]), rank
        assert snaps[1]["stats"]["stock_consumed"] > 0, rank
