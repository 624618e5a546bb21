"""Timings of the ray-frame calls (profiles/rayframe/README.md) on the C3 scene
at 1920x1080, one lane, the rays wpt_primary_rays makes for the scene's camera.

Default run: k_first_hit_rays over the rays (a wave = 64 consecutive rays of a
row) beside k_first_hit over the same pixels (a wave = an 8 x 8 tile): device
pointers, all planes, one warm-up of each, then REPS alternating repetitions.
Neither launch is in wpt_kernel_times, so the device times come from a kernel
trace of this run, without counters:
  rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python3 tools/rayframe_time.py
  python3 tools/rayframe_time.py --trace DIR/.../run_kernel_trace.csv
--wall: no trace; the wall time of wpt_denoise_rays (RGBA8 only, host rays, NEE,
1 spp) beside the same frame composed from the three host-side calls
(wpt_radiance_rays, wpt_first_hit_rays, wpt_denoise_planes), REPS alternating
repetitions after a warm-up of each, and whether the two frames are equal.
Usage: python3 tools/rayframe_time.py [--reps 5] [--wall] [--trace CSV]"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _summary(v):
    return {"ms": [round(x, 4) for x in v], "median_ms": round(statistics.median(v), 4),
            "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def from_trace(path):
    """Device ms per kernel from a rocprofv3 kernel trace of the default run
    (the first launch of each is its warm-up)."""
    rays, pix = [], []
    for row in csv.DictReader(open(path)):
        ms = (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e6
        if "k_first_hit_rays" in row["Kernel_Name"]:
            rays.append((int(row["Start_Timestamp"]), ms))
        elif "k_first_hit" in row["Kernel_Name"]:
            pix.append((int(row["Start_Timestamp"]), ms))
    rays = [m for _, m in sorted(rays)]
    pix = [m for _, m in sorted(pix)]
    return {"launches": {"k_first_hit_rays": len(rays), "k_first_hit": len(pix)},
            "k_first_hit_rays": _summary(rays[1:]), "k_first_hit": _summary(pix[1:])}


def _session(pkg, W, H):
    import numpy as np

    itf = pkg.interface
    path = os.path.join(ROOT, "tests", "golden", "cloud_100k.npy")
    mesh = np.load(path, allow_pickle=False) if os.path.exists(path) else pkg.scenes.triangle_cloud(100000, seed=0x5EED)
    cam = pkg.scenes.scene_camera(2)
    itf.set_device(0)
    itf.init(W, H, 2, *cam)
    itf.store_mesh(1, mesh)
    itf.update_settings(1, 1, 0, 0, 0)
    itf.set_render_options(8, 0xBABABEBE, 0)
    itf.set_lanes(1)
    return itf, itf.primary_rays(W, H, cam)


def kernels(pkg, reps):
    import numpy as np
    import torch

    W, H = 1920, 1080
    itf, rays = _session(pkg, W, H)
    try:
        dev = torch.device("cuda", torch.cuda.current_device())
        d_rays = torch.from_numpy(rays).to(dev)
        names = ("t", "id", "visits", "normal", "albedo", "kind", "status")
        a = itf.first_hit_rays(d_rays, device=True)  # warm-ups
        g = itf.first_hit(0)
        for k in names[:6]:
            want = g[k].reshape(-1).view(np.uint8 if k == "kind" else np.uint32)
            x = a[k].cpu().numpy().reshape(-1)
            assert np.array_equal(x.view(np.uint8 if k == "kind" else np.uint32), want), k
        for _ in range(reps):
            itf.first_hit_rays(d_rays, device=True)
            itf.first_hit(0)
        print(json.dumps({"W": W, "H": H, "reps": reps, "planes_equal": True,
                          "visits_mean": round(float(g["visits"].mean()), 2)}))
    finally:
        itf.shutdown()


def wall(pkg, reps):
    import numpy as np

    W, H = 1920, 1080
    itf, rays = _session(pkg, W, H)
    try:
        def fused():
            return itf.denoise_rays(rays, W, H, None, 0, 1, 1, outputs=("rgba",))["rgba"]

        def composed():
            raw, status = itf.radiance_rays(rays, None, 0, 1, 1)
            p = itf.first_hit_rays(rays, planes=("t", "normal", "albedo", "kind"))
            cnt = status.astype(np.uint32).reshape(H, W)
            return itf.denoise_planes(raw.reshape(H, W, 3), cnt, p["t"], p["normal"], p["albedo"], p["kind"])[2]

        same = bool(np.array_equal(fused(), composed()))  # warm-ups
        tf, tc = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            fused()
            tf.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            composed()
            tc.append((time.perf_counter() - t0) * 1e3)
        print(json.dumps({"W": W, "H": H, "reps": reps, "frames_equal": same, "denoise_rays_wall": _summary(tf),
                          "three_calls_wall": _summary(tc)}))
    finally:
        itf.shutdown()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trace", default="")
    ap.add_argument("--wall", action="store_true")
    args = ap.parse_args()
    if args.trace:
        print(json.dumps(from_trace(args.trace)))
        return
    import wpt_loader
    pkg = wpt_loader.load()
    if args.wall:
        wall(pkg, args.reps)
    else:
        kernels(pkg, args.reps)


if __name__ == "__main__":
    main()
