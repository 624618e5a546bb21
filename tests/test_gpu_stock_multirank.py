"""The sample stock on sessions with several ranks (WPT_OPT_STOCK_RANKS,
wpt_stock.h): every rank keeps a ring over its own partition, plans the same
global rounds as the others and adds its pixels' share of them from the ring.

The ranks share the box's one GPU (one process each, a gloo group, the
round-boundary exchange staged through host memory by multigpu.RoundExchange).
The yardstick is the oracle's adaptive session fed the same chunks, never
another run of the code under test: the union of the partitions equals its
frame bit for bit (counts, radiance as u32 bits) and every rank's sampling
view equals its view. Every case states all the stock options it runs with
and sets stock_ranks itself.
"""
import os
import socket
import sys
import time

import numpy as np
import pytest
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0xBABABEBE

# every async option, as tests/test_gpu_stock.py's BASE, and the rank switch
BASE = {"stock": 256, "stock_lanes": 2, "stock_ahead": 6, "stock_extra": 2, "stock_every": 2, "fill": 0,
        "async_prio": 0, "async_grid_pct": 0, "async_oneshot": 0, "stock_prefill": 1, "async_fused_below": 0,
        "stock_ranks": 1}
# the library's built-in stock settings (C5 runs with them)
PRODUCTION = {"stock": 1024, "stock_ahead": 40, "stock_extra": 8, "stock_every": 3, "async_grid_pct": 100,
              "async_fused_below": 1 << 26}
STOCK_COUNTERS = ("stock_traced", "stock_consumed", "stock_deficit", "stock_waits", "stock_rays", "stock_rays_used",
                  "stock_us")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, cfg, q):
    """One rank: cfg's session, then its steps: ("compute", n), ("option",
    name, value), ("camera", cam), ("viewport", W, H) and ("snap",), which
    records the rank's partition of the frame (its pixels at that moment), its
    sampling view, statistics and ring size."""
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import wpt_loader
        pkg = wpt_loader.load()
        from wasm_pathtracer_amd import multigpu
        itf = pkg.interface
        W, H = cfg["size"]
        for k, v in cfg["opts"].items():
            itf.set_option(k, v)  # the defaults of the init below
        itf.set_device(0)
        itf.init(W, H, cfg["scene"], *cfg["cam"])
        if cfg["scene"] == 2:
            itf.store_mesh(1, pkg.scenes.triangle_cloud(3000, seed=0x5EED))
        itf.update_settings(*cfg["types"], *cfg["adaptive"], 0)
        itf.set_render_options(cfg["depth"], SEED, 0)
        itf.set_partition(rank, world, cfg["tile"])
        ex = multigpu.RoundExchange(world, device="cuda")
        px0 = px = itf.partition_pixels()  # px0: the session's first partition
        calls, snaps = [], []
        for step in cfg["steps"]:
            if step[0] == "compute":
                itf.compute(step[1])
                st = itf.stats()
                calls.append((st["rays"], st["shadow_rays"], st["paths"]))
            elif step[0] == "option":
                itf.set_option(step[1], step[2])
            elif step[0] == "camera":
                itf.update_camera(*step[1])
            elif step[0] == "viewport":
                W, H = step[1], step[2]
                itf.update_viewport(W, H)  # the session keeps its rank: a new partition
                px = itf.partition_pixels()
            else:
                acc, cnt = itf.read_radiance(W, H)
                snaps.append({"size": (W, H), "px": px, "acc": acc.reshape(-1, 3)[px], "cnt": cnt.reshape(-1)[px],
                              "samp": itf.results(1, W, H),
                              "stats": itf.stats(), "ring": itf.get_option("stock_ring_bytes"), "ex": ex.calls})
        q.put((rank, px0, calls, snaps))
        ex.close()
        itf.shutdown()
    finally:
        dist.destroy_process_group()


def _run_ranks(world, cfg, timeout_s=240):
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    pc = mp.start_processes(_worker, args=(world, _free_port(), cfg, q), nprocs=world, join=False, start_method="spawn")
    deadline = time.time() + timeout_s
    res, done = [], False
    while len(res) < world:
        # taken as they come: the queue is a pipe, and a rank whose result does
        # not fit what is left of its buffer waits in put() until it is read
        while not q.empty():
            res.append(q.get())
        if done:
            break
        done = pc.join(timeout=0.1)
        if time.time() > deadline:
            for p in pc.processes:
                p.kill()
            raise TimeoutError("multi-rank workers did not finish")
    assert len(res) == world
    while not pc.join(timeout=0.1):
        if time.time() > deadline:
            for p in pc.processes:
                p.kill()
            raise TimeoutError("multi-rank workers did not finish")
    return sorted(res, key=lambda r: r[0])


def _cfg(wpt, size, tile, scene, types, adaptive, depth, opts, steps, cam=None):
    return {"size": size, "tile": tile, "scene": scene, "types": types, "adaptive": adaptive, "depth": depth,
            "opts": dict(BASE, **opts), "steps": steps, "cam": list(cam or wpt.scenes.scene_camera(scene))}


def _oracle_session(oracle, cfg, mesh):
    W, H = cfg["size"]
    scene = oracle.OracleScene(cfg["scene"], mesh if cfg["scene"] == 2 else None)
    return scene.adaptive(W, H, cfg["cam"], cfg["types"], cfg["adaptive"], cfg["depth"], SEED)


def _assert_union(res, snap, cfg, ref):
    """Snapshot `snap` of every rank against the oracle session `ref` (of the
    snapshot's viewport)."""
    W, H = res[0][3][snap]["size"]
    acc_r, cnt_r, samp_r = ref.read()
    acc = np.zeros((W * H, 3), np.float32)
    cnt = np.zeros(W * H, np.uint32)
    seen = np.zeros(W * H, np.int32)
    for rank, _, _, snaps in res:
        s = snaps[snap]
        px = s["px"]
        acc[px] = s["acc"]
        cnt[px] = s["cnt"]
        seen[px] += 1
        assert np.array_equal(s["samp"], samp_r), f"rank {rank}: sampling view differs"
    assert np.all(seen == 1)
    assert np.array_equal(cnt, cnt_r.reshape(-1))
    assert np.array_equal(acc.view(np.uint32), acc_r.reshape(-1, 3).view(np.uint32))
    return cnt_r


# 48 x 32: chunks that cut rounds mid-way, one below a half's 768 pixels
WRAP_CHUNKS = (48 * 32 * 20 + 11, 500, 48 * 32 * 25 + 7, 48 * 32 * 35 + 301)
WRAP_OPTS = {"stock": 64, "stock_ahead": 1, "stock_every": 1}


def test_ring_wrap_two_ranks(wpt, oracle, cloud_small):
    """The smallest ring, wrapped: some pixel takes more samples than it has
    slots. This case fails without the feature: a session with several ranks
    consumed nothing from the stock (and had no stock_ranks option)."""
    steps = [("compute", n) for n in WRAP_CHUNKS] + [("snap",)]
    cfg = _cfg(wpt, (48, 32), 8, 2, (2, 1), (1, 1), 4, WRAP_OPTS, steps)
    ref = _oracle_session(oracle, cfg, cloud_small)
    for n in WRAP_CHUNKS:
        ref.compute(n)
    assert ref.read()[1].max() > 64  # more samples than ring slots: the ring wrapped
    res = _run_ranks(2, cfg)
    _assert_union(res, 0, cfg, ref)
    paths = 0
    for rank, _, _, snaps in res:
        st = snaps[0]["stats"]
        assert st["stock_consumed"] > 0 and st["stock_traced"] >= st["stock_consumed"], (rank, st)
        paths += st["paths"]
    assert paths == sum(WRAP_CHUNKS)


def test_uneven_partitions_three_ranks_rr_only(wpt, oracle, cloud_small):
    """28 tiles dealt 10 / 9 / 9, the init defaults' layout (a random half
    beside the stocked one), no depth cap: k_finish and the async lanes in
    three processes on one card."""
    W, H = 56, 32
    chunks = (W * H * 6 + 13, 300, W * H * 9 + 5)
    steps = [("compute", n) for n in chunks] + [("snap",)]
    cfg = _cfg(wpt, (W, H), 8, 2, (1, 2), (0, 1), 0, {"stock": 256, "stock_lanes": 2, "stock_prefill": 1}, steps)
    ref = _oracle_session(oracle, cfg, cloud_small)
    for n in chunks:
        ref.compute(n)
    res = _run_ranks(3, cfg)
    assert sorted(len(px) for _, px, _, _ in res) == [9 * 64, 9 * 64, 10 * 64]
    cnt_r = _assert_union(res, 0, cfg, ref)
    assert cnt_r.max() > 8  # several adaptive rounds ran
    assert sum(snaps[0]["stats"]["paths"] for _, _, _, snaps in res) == sum(chunks)
    for rank, _, _, snaps in res:
        st = snaps[0]["stats"]
        assert st["stock_consumed"] > 0 and st["stock_traced"] >= st["stock_consumed"], (rank, st)


def test_rank_without_an_adaptive_pixel(wpt, oracle):
    """Tiles of 32 px on 64 x 32: rank 0 owns the left (random) half, rank 1
    the right (adaptive) one. Rank 0 stocks nothing and holds no ring, and
    still makes every exchange rank 1 makes."""
    W, H = 64, 32
    chunks = (W * H * 5 + 9, 700, W * H * 8 + 3)
    steps = [("compute", n) for n in chunks] + [("snap",)]
    cfg = _cfg(wpt, (W, H), 32, 101, (1, 1), (0, 1), 4, {}, steps)
    ref = _oracle_session(oracle, cfg, None)
    for n in chunks:
        ref.compute(n)
    res = _run_ranks(2, cfg)
    _assert_union(res, 0, cfg, ref)
    half = W // 2
    assert np.all(res[0][1] % W < half) and np.all(res[1][1] % W >= half)
    s0, s1 = res[0][3][0], res[1][3][0]
    assert all(s0["stats"][k] == 0 for k in STOCK_COUNTERS), s0["stats"]
    assert s0["ring"] == 0
    assert s1["stats"]["stock_consumed"] > 0 and s1["stats"]["stock_traced"] >= s1["stats"]["stock_consumed"]
    assert s1["ring"] > 0
    assert s0["ex"] == s1["ex"] > 0
    assert s0["stats"]["paths"] + s1["stats"]["paths"] == sum(chunks)


def test_off_switch_and_counts(wpt, oracle, cloud_small):
    """stock_ranks 0 and 1 on the wrap case's session (a smaller budget): the
    same frame, and after every compute call the same rays, shadow rays and
    paths summed over the ranks. Off: no stock counter moves. On: a rank's
    ring holds its own partition only."""
    chunks = (48 * 32 * 6 + 11, 500, 48 * 32 * 9 + 7)
    steps = [("compute", n) for n in chunks] + [("snap",)]
    ref = None
    sums = {}
    for ranks_on in (0, 1):
        cfg = _cfg(wpt, (48, 32), 8, 2, (2, 1), (1, 1), 4, dict(WRAP_OPTS, stock_ranks=ranks_on), steps)
        if ref is None:
            ref = _oracle_session(oracle, cfg, cloud_small)
            for n in chunks:
                ref.compute(n)
        res = _run_ranks(2, cfg)
        _assert_union(res, 0, cfg, ref)
        sums[ranks_on] = [tuple(sum(r[2][i][k] for r in res) for k in range(3)) for i in range(len(chunks))]
        largest = max(len(px) for _, px, _, _ in res)
        for rank, _, _, snaps in res:
            s = snaps[0]
            if ranks_on:
                assert s["stats"]["stock_consumed"] > 0
                assert 0 < s["ring"] <= 20 * WRAP_OPTS["stock"] * largest
            else:
                assert all(s["stats"][k] == 0 for k in STOCK_COUNTERS), (rank, s["stats"])
                assert s["ring"] == 0
    assert sums[0] == sums[1]
    assert [s[2] for s in sums[1]] == list(np.cumsum(chunks))


def test_drop_mid_round(wpt, oracle, cloud_small):
    """C5-like settings on two ranks. Between chunks that cut a round every
    rank changes the ring size: a new ring, the partly added round traced
    again as a deficit. Later a camera update resets the session; the oracle
    starts a fresh one with that camera."""
    W, H = 48, 32
    first = (W * H * 6 + 17, W * H * 5 + 3)
    second = (W * H * 5 + 29, 411)
    cam = list(wpt.scenes.scene_camera(2))
    cam2 = list(cam)
    cam2[0] += 0.05
    steps = [("compute", first[0]), ("option", "stock", 64), ("compute", first[1]), ("snap",), ("camera", cam2)]
    steps += [("compute", n) for n in second] + [("snap",)]
    cfg = _cfg(wpt, (W, H), 8, 2, (2, 2), (1, 1), 8, PRODUCTION, steps, cam=cam)
    res = _run_ranks(2, cfg)
    ref = _oracle_session(oracle, cfg, cloud_small)
    for n in first:
        ref.compute(n)
    _assert_union(res, 0, cfg, ref)
    ref2 = _oracle_session(oracle, dict(cfg, cam=cam2), cloud_small)
    for n in second:
        ref2.compute(n)
    _assert_union(res, 1, cfg, ref2)
    for rank, _, _, snaps in res:
        assert snaps[1]["stats"]["stock_consumed"] > 0, rank
        assert snaps[1]["ring"] == 20 * 64 * len(res[rank][1])
