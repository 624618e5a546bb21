"""The counting variants of the traversal kernels, which the rest of the suite
leaves open: k_extend, k_shadow and k_trace are instantiated with and without
their work counters (wpt_set_counting), and a launcher that picked the wrong
one of the pair would still render the same frame.

On a triangle-only scene and on one with other shapes, for both traversals of
the extension rays and of the shadow rays (exact BVH2, BVH4 fast path) and for
fused and separate launches: the frame with counting on is the frame with it
off, bit for bit, with the same ray counts; the counters are above zero with
counting on wherever rays reached a traversal kernel, and zero with it off.

With WPT_OPT_FUSED 0 the batch runs separate k_extend / k_shadow launches only
when WPT_OPT_FUSED_BELOW does not claim it, so those cases set it to 0. The
fused form never runs the BVH4 fast path: with either traversal at 1 the
launches are separate whatever WPT_OPT_FUSED says.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, SPP, DEPTH = 40, 24, 2, 4
SEED = 0xBABABEBE
COUNTERS = ("ext_visits", "sh_visits")


def _session(itf, wpt, scene_id, mesh, opts, counting):
    for k, v in opts.items():
        itf.set_option(k, v)  # the defaults of the init below
    itf.init(W, H, scene_id, *wpt.scenes.scene_camera(scene_id))
    try:
        if mesh is not None:
            itf.store_mesh(1, mesh)
        itf.update_settings(1, 1, 0, 0, 0)
        itf.set_render_options(DEPTH, SEED, 0)
        itf.set_counting(counting)
        tri_only = itf.get_option("scene_tri_only")
        itf.compute(W * H * SPP)
        acc, cnt = itf.read_radiance(W, H)
        st = itf.stats()
    finally:
        itf.shutdown()
        itf.set_option("defaults", 0)
    return acc, cnt, st, tri_only


@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("trav_sh", [0, 1])
@pytest.mark.parametrize("trav", [0, 1])
@pytest.mark.parametrize("scene", ["triangles", "shapes"])
def test_counting_changes_no_bit_and_counts_only_when_on(wpt, cloud_small, scene, trav, trav_sh, fused):
    itf = wpt.interface
    scene_id, mesh, want_tri = (2, cloud_small, 1) if scene == "triangles" else (0, None, 0)
    opts = {"traversal": trav, "traversal_sh": trav_sh, "fused": fused}
    if not fused:
        opts["fused_below"] = 0
    on = _session(itf, wpt, scene_id, mesh, opts, 1)
    off = _session(itf, wpt, scene_id, mesh, opts, 0)
    assert on[3] == want_tri and off[3] == want_tri

    ext = on[2]["rays"] - on[2]["presolved_rays"]  # rays that reached k_extend / k_trace
    sh = on[2]["shadow_rays"] - on[2]["shadow_presolved_rays"]  # ... k_shadow / k_trace
    print(f"{scene} trav {trav}/{trav_sh} fused {fused}: rays {on[2]['rays']} ({ext} traversed), shadow rays "
          f"{on[2]['shadow_rays']} ({sh} traversed), counters on",
          {k: on[2][k] for k in COUNTERS}, "off", {k: off[2][k] for k in COUNTERS})
    assert np.array_equal(on[0].view(np.uint32), off[0].view(np.uint32))
    assert np.array_equal(on[1], off[1]) and np.all(on[1] == SPP)
    assert on[2]["rays"] == off[2]["rays"] and on[2]["shadow_rays"] == off[2]["shadow_rays"]
    assert ext > 0  # primary rays meet the scene's finite shapes
    assert on[2]["ext_visits"] > 0
    if sh > 0:
        assert on[2]["sh_visits"] > 0
    assert off[2]["ext_visits"] == 0 and off[2]["sh_visits"] == 0
