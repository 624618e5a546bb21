"""A point query against the route it replaces (profiles/points/README.md), one
JSON line.

The C3 scene, NEE, depth 8, one session. The points are the first hits of a
1024 x 1024 frame of the scene's camera with their normals (2^20 records; a
pixel that misses gives a probe at the camera looking up), SPP samples each:
  replaced      per sample s: wpt_point_rays on the host, wpt_radiance_rays over
                the 2^20 rays at spp = 1 (host pointers), the f32 sum on the host
  points_host   wpt_radiance_points, host pointers
  points_device wpt_radiance_points, device pointers
The three alternate REPS + 1 times (the first the warm-up); the wall time runs to
wpt_sync. All three give the same bits (asserted) and trace the same rays, so
milliseconds compare. Beside them the summed device time of the generate kernel
(wpt_kernel_times under wpt_set_profiling) of one point query and of one ray query
over the same number of positions.

Usage: python3 tools/points_time.py [--reps 3] [--spp 16]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W = H = 1024
SEED = 0xBABABEBE


def run(reps, spp):
    import numpy as np
    import torch
    import wpt_loader
    pkg = wpt_loader.load()
    itf = pkg.interface
    path = os.path.join(ROOT, "tests", "golden", "cloud_100k.npy")
    mesh = np.load(path, allow_pickle=False) if os.path.exists(path) else pkg.scenes.triangle_cloud(100000, seed=0x5EED)
    cam = pkg.scenes.scene_camera(2)
    itf.set_device(0)
    itf.init(W, H, 2, *cam)
    n = W * H
    try:
        itf.store_mesh(1, mesh)
        itf.update_settings(1, 1, 0, 0, 0)
        itf.set_render_options(8, SEED, 0)
        fh = itf.first_hit(0, planes=("dir", "t", "normal", "kind"))
        hit = fh["kind"].reshape(-1) != 0
        t = np.where(hit, fh["t"].reshape(-1), 0).astype(np.float32)
        pts = np.empty((n, 6), np.float32)
        pts[:, :3] = np.asarray(cam[:3], np.float32) + fh["dir"].reshape(-1, 3) * t[:, None]
        pts[:, 3:] = np.where(hit[:, None], fh["normal"].reshape(-1, 3), np.array([0, 1, 0], np.float32))
        dev = torch.device("cuda", 0)
        d_pts = torch.from_numpy(pts).to(dev)
        torch.cuda.synchronize()
        runs = {"replaced": [], "points_host": [], "points_device": []}
        bits = {}
        for rep in range(reps + 1):
            for name in runs:
                itf.sync()
                st0 = itf.stats()
                t0 = time.perf_counter()
                if name == "replaced":
                    rgb = np.zeros((n, 3), np.float32)
                    for s in range(spp):
                        rgb += itf.radiance_rays(itf.point_rays(pts, None, SEED, s, 0), None, s, 1, 1)[0]
                elif name == "points_host":
                    rgb = itf.radiance_points(pts, None, 0, spp, 1, 0)[0]
                else:
                    rgb = itf.radiance_points(d_pts, None, 0, spp, 1, 0, device=True)[0]
                itf.sync()
                ms = (time.perf_counter() - t0) * 1e3
                st = itf.stats()
                assert st["paths"] - st0["paths"] == spp * n
                bits[name] = (rgb.cpu().numpy() if name == "points_device" else rgb).view(np.uint32)
                if rep:
                    runs[name].append((round(ms, 2), st["rays"] + st["shadow_rays"] - st0["rays"] - st0["shadow_rays"]))
            assert np.array_equal(bits["replaced"], bits["points_host"])
            assert np.array_equal(bits["replaced"], bits["points_device"])
        out = {"points": n, "spp": spp, "paths": spp * n, "reps": reps, "hits": int(hit.sum()),
               "nonzero_sums": int((bits["replaced"] != 0).any(axis=1).sum())}
        for name, v in runs.items():
            ms = [a[0] for a in v]
            out[name] = {"wall_ms": ms, "median_ms": statistics.median(ms), "rays": v[0][1],
                         "mray_s": [round(a[1] / a[0] / 1e3, 1) for a in v]}
        # the generators' device time over the same positions
        d_rays = torch.from_numpy(itf.point_rays(pts, None, SEED, 0, 0)).to(dev)
        itf.set_profiling(True)
        for name, call in (("k_generate_points", lambda: itf.radiance_points(d_pts, None, 0, spp, 1, 0, device=True)),
                           ("k_generate_rays", lambda: itf.radiance_rays(d_rays, None, 0, spp, 1, device=True))):
            for opt, suffix in ((1, "_ps"), (0, "")):
                itf.set_option("presolve", opt)
                call()
                k0 = itf.kernel_times()["generate"]
                call()
                k1 = itf.kernel_times()["generate"]
                out[name + suffix] = {"ms": round(k1["ms"] - k0["ms"], 4), "launches": k1["launches"] - k0["launches"]}
        itf.set_profiling(False)
        print(json.dumps(out))
    finally:
        itf.shutdown()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--spp", type=int, default=16)
    args = ap.parse_args()
    run(args.reps, args.spp)


if __name__ == "__main__":
    main()
