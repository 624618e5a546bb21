"""The sample stock on two ranks sharing one GPU (WPT_OPT_STOCK_RANKS = 1; a gloo group, the exchange
staged through host memory): (a) C5's session at 1920x1080, compute(W*H*64) twice: per-rank stock
counters, ring bytes and exchanges; (b) the 64x48 parity session of bench.py's secondary block over
two ranks, the union of the partitions against the oracle's session.

    python tools/stock_ranks_stats.py OUT.json

wrote profiles/stockranks/rehearsal_stats.json (the process group logs to stdout, so the JSON goes to
a file)."""
import json
import os
import socket
import sys
import time

import numpy as np
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
CHUNKS = (64 * 48 * 6, 64 * 48 * 5 + 17, 64 * 48 * 9)
KEYS = ("paths", "rays", "shadow_rays", "stock_traced", "stock_consumed", "stock_deficit", "stock_waits", "stock_rays",
        "stock_rays_used")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, W, H, chunks, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import wpt_loader
        pkg = wpt_loader.load()
        from wasm_pathtracer_amd import multigpu
        itf = pkg.interface
        itf.set_option("stock_ranks", 1)
        itf.set_device(0)
        itf.init(W, H, 2, *pkg.scenes.scene_camera(2))
        itf.store_mesh(1, pkg.scenes.triangle_cloud(100000))
        itf.update_settings(2, 2, 1, 1, 0)
        itf.set_render_options(8, 0xBABABEBE, 1 << 27)
        itf.set_partition(rank, world, 16)
        ex = multigpu.RoundExchange(world, device="cuda")
        t0 = time.perf_counter()
        for n in chunks:
            itf.compute(n)
        itf.sync()
        dt = time.perf_counter() - t0
        st = itf.stats()
        px = itf.partition_pixels()
        out = {"rank": rank, "npart": len(px), "ring_bytes": itf.get_option("stock_ring_bytes"),
               "stock_slots": itf.get_option("stock"), "exchanges": ex.calls, "seconds": round(dt, 3),
               **{k: int(st[k]) for k in KEYS}}
        if W * H <= 64 * 48:
            acc, cnt = itf.read_radiance(W, H)
            out["px"], out["acc"], out["cnt"] = px, acc.reshape(-1, 3)[px], cnt.reshape(-1)[px]
        q.put(out)
        ex.close()
        itf.shutdown()
    finally:
        dist.destroy_process_group()


def run(world, W, H, chunks, timeout_s=150):
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    pc = mp.start_processes(_worker, args=(world, _free_port(), W, H, chunks, q), nprocs=world, join=False,
                            start_method="spawn")
    deadline = time.time() + timeout_s
    res, done = [], False
    while len(res) < world:
        while not q.empty():
            res.append(q.get())
        if done:
            break
        done = pc.join(timeout=0.1)
        if time.time() > deadline:
            for p in pc.processes:
                p.kill()
            raise TimeoutError
    while not pc.join(timeout=0.1):
        if time.time() > deadline:
            for p in pc.processes:
                p.kill()
            raise TimeoutError
    return sorted(res, key=lambda r: r["rank"])


def main():
    big = run(2, 1920, 1080, (1920 * 1080 * 64, 1920 * 1080 * 64))
    small = run(2, 64, 48, CHUNKS)
    import pyoracle
    import wpt_loader
    pkg = wpt_loader.load()
    ref = pyoracle.OracleScene(2, pkg.scenes.triangle_cloud(100000)).adaptive(64, 48, pkg.scenes.scene_camera(2),
                                                                             (2, 2), (1, 1), 8)
    for n in CHUNKS:
        ref.compute(n, threads=8)
    acc_r, cnt_r, _ = ref.read()
    acc = np.zeros((64 * 48, 3), np.float32)
    cnt = np.zeros(64 * 48, np.uint32)
    for r in small:
        acc[r["px"]] = r.pop("acc")
        cnt[r.pop("px")] = r.pop("cnt")
    parity = {"bit_exact": bool(np.array_equal(acc.view(np.uint32), acc_r.reshape(-1, 3).view(np.uint32))),
              "counts_equal": bool(np.array_equal(cnt, cnt_r.reshape(-1))),
              "rel_l2": float(np.linalg.norm(acc - acc_r.reshape(-1, 3)) / np.linalg.norm(acc_r)),
              "check": f"two ranks at 64x48, compute{CHUNKS}, against the oracle's session"}
    with open(sys.argv[1], "w") as f:
        json.dump({"c5_1080p_two_ranks": big, "parity_64x48_two_ranks": {"ranks": small, "parity": parity}}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
