"""What the launch context decides, seen from outside: which launches of a
batch are timed, which lane and bounce each traversal launch carries in the
probe, and that the test hooks' launches (lane 0 alone) are never timed and
leave a batch's results alone. Profiling must not change a bit of the frame.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, DEPTH = 96, 64, 6
KERNELS = ("generate", "extend", "shade", "shadow", "accumulate", "trace")


def _hook_inputs(wpt, cloud):
    """A handful of rays into scene 2, and as many (p, q on a light) pairs."""
    rng = np.random.default_rng(2024)
    n = 37
    o = np.tile(np.array(wpt.scenes.scene_camera(2)[:3], np.float32), (n, 1))
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d[:, 1] = -np.abs(d[:, 1])
    d[:, 2] = np.abs(d[:, 2])
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
    rays = np.concatenate([o, d], axis=1).astype(np.float32)
    dbg = wpt.interface.DebugScene(2, cloud)
    li = dbg.lights().astype(np.int32)[rng.integers(0, dbg.num_lights, n)]
    q = dbg.shapes()[li, :9].reshape(n, 3, 3).mean(axis=1)
    p = rng.uniform([-2.0, -0.9, 3.0], [2.0, 3.0, 9.0], (n, 3))
    return rays, np.concatenate([p, q], axis=1).astype(np.float32), li


def _hooks(itf, inputs):
    rays, pq, li = inputs
    t, ids = itf.trace_rays(rays)
    return t.view(np.uint32).copy(), ids.copy(), itf.shadow_rays(pq, li)


def _launches(itf):
    kt = itf.kernel_times()
    return {k: kt[k]["launches"] for k in KERNELS}


def _session(itf, wpt, cloud, lanes, opts, profiling, inputs=None):
    itf.init(W, H, 2, *wpt.scenes.scene_camera(2))
    try:
        itf.store_mesh(1, cloud)
        itf.update_settings(1, 1, 0, 0, 0)
        itf.set_render_options(DEPTH, 0xBABABEBE, 0)
        for k, v in opts.items():
            itf.set_option(k, v)
        itf.set_option("probe", 4096)
        if lanes is not None:
            itf.set_lanes(lanes)
        itf.set_profiling(profiling)
        out = {}
        if inputs is not None:
            out["before"] = _hooks(itf, inputs)
            itf.probe_read()  # drop the hooks' records: the batch's alone below
        itf.clear_stats()
        itf.compute(W * H * 3)
        itf.sync()
        out["frame"] = itf.read_radiance(W, H)
        out["launches"] = _launches(itf)
        out["meta"] = itf.probe_read()[0]
        if inputs is not None:
            out["after"] = _hooks(itf, inputs)
            out["launches_after"] = _launches(itf)
            out["hook_meta"] = itf.probe_read()[0]
            # a timed hook launch would be counted with the next batch's
            itf.compute(W * H * 3)
            itf.sync()
            out["launches_again"] = _launches(itf)
    finally:
        itf.shutdown()
        itf.set_option("defaults", 0)
    return out


@pytest.mark.parametrize("lanes", [1, None])
@pytest.mark.parametrize("opts", [{"fused": 0, "fused_below": 0}, {"fused": 1}], ids=["unfused", "fused"])
def test_launch_counts_probe_rows_and_untimed_hooks(wpt, cloud_small, lanes, opts):
    itf = wpt.interface
    inputs = _hook_inputs(wpt, cloud_small)
    on = _session(itf, wpt, cloud_small, lanes, opts, 1, inputs)
    off = _session(itf, wpt, cloud_small, lanes, opts, 0)

    meta = on["meta"]
    lane_ids = sorted(set(meta[:, 1].tolist()))
    nl = len(lane_ids)
    print("lanes", lane_ids, "launches", on["launches"], "rows", np.bincount(meta[:, 0], minlength=6).tolist())
    assert nl >= 1 and (lanes != 1 or nl == 1)
    n = on["launches"]
    if opts["fused"]:
        want = dict(generate=nl, accumulate=nl, extend=nl, trace=(DEPTH - 1) * nl, shade=DEPTH * nl, shadow=nl)
    else:
        want = dict(generate=nl, accumulate=nl, extend=DEPTH * nl, shade=DEPTH * nl, shadow=DEPTH * nl, trace=0)
    assert n == want
    # the probe's rows number the traversal launches, kind by kind
    for kind, kernel in ((1, "extend"), (3, "shadow"), (5, "trace")):
        assert int((meta[:, 0] == kind).sum()) == n[kernel]
    # per lane the extension side (extend, trace) ran bounces 0 .. DEPTH-1, once each
    for l in lane_ids:
        ext = meta[(meta[:, 1] == l) & ((meta[:, 0] == 1) | (meta[:, 0] == 5))]
        assert sorted(ext[:, 2].tolist()) == list(range(DEPTH))

    # the hooks: not timed, and the same answers after the batch as before it
    assert on["launches_after"] == on["launches"]
    assert on["launches_again"] == {k: 2 * v for k, v in want.items()}
    assert all(np.array_equal(a, b) for a, b in zip(on["before"], on["after"]))
    assert (on["before"][1] >= 0).any() and sorted(on["hook_meta"][:, 0].tolist()) == [1, 3]

    # a session that is not profiled times nothing and renders the same bits
    assert all(v == 0 for v in off["launches"].values())
    assert np.array_equal(on["frame"][0].view(np.uint32), off["frame"][0].view(np.uint32))
    assert np.array_equal(on["frame"][1], off["frame"][1])
    assert np.array_equal(on["meta"][:, :3], off["meta"][:, :3])
