"""Throughput of a ray query (profiles/rayquery/README.md), one JSON line.

The C3 scene at 1920x1080, NEE, depth 8, one session. The rays are
wpt_primary_rays of sample 0, on the device (WPT_RAYS_DEVICE), spp = 4; beside
it wpt_compute(4 * npix) of the same session after a reset of the accumulation,
and the same query through host pointers (the 50 MB upload and the 25 MB of
results through the pinned block). The three alternate REPS + 1 times (the first
the warm-up); the wall time runs to wpt_sync. A query re-uses one ray for its 4
samples where a frame jitters, so the two trace different rays: the figure to
compare is Mray/s from the wpt_stats deltas, not milliseconds.

With --trace CSV: the device times of the generate and accumulate kernels from a
kernel trace of a run of its own:
  rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python3 tools/rays_time.py
  python3 tools/rays_time.py --trace DIR/.../run_kernel_trace.csv

Usage: python3 tools/rays_time.py [--reps 5] [--spp 4] [--trace CSV]"""
import argparse
import csv
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H = 1920, 1080
KERNELS = ("k_generate_rays_ps", "k_generate_rays", "k_generate_shade", "k_generate_ps", "k_rays_status", "k_rays_unpack",
           "k_accumulate_round", "k_accumulate")


def trace(path):
    rows = [r for r in csv.DictReader(open(path))]
    out = {}
    for r in rows:
        m = re.search(r"\b(k_\w+)", r["Kernel_Name"])  # the whole identifier: k_generate_rays is a prefix of k_generate_rays_ps
        if not m or m.group(1) not in KERNELS:
            continue
        out.setdefault(m.group(1), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    print(json.dumps({k: {"launches": len(v), "median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4),
                          "max_ms": round(max(v), 4)} for k, v in out.items()}))


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
    npx = W * H
    try:
        itf.store_mesh(1, mesh)
        itf.update_settings(1, 1, 0, 0, 0)
        itf.set_render_options(8, 0xBABABEBE, 0)
        rays = itf.primary_rays(W, H, cam, 0xBABABEBE, 0)
        d_rays = torch.from_numpy(rays).to(torch.device("cuda", 0))
        torch.cuda.synchronize()
        runs = {"compute": [], "query_device": [], "query_host": []}
        for rep in range(reps + 1):
            for name in runs:
                itf.update_camera(*cam)  # resets the accumulation
                itf.sync()
                st0 = itf.stats()
                t0 = time.perf_counter()
                if name == "compute":
                    itf.compute(spp * npx)
                elif name == "query_device":
                    itf.radiance_rays(d_rays, None, 0, spp, 1, device=True)
                else:
                    itf.radiance_rays(rays, None, 0, spp, 1)
                itf.sync()
                ms = (time.perf_counter() - t0) * 1e3
                st = itf.stats()
                assert st["paths"] - st0["paths"] == spp * npx
                if rep:
                    runs[name].append((round(ms, 2), st["rays"] + st["shadow_rays"] - st0["rays"] - st0["shadow_rays"],
                                       st["presolved_rays"] - st0["presolved_rays"],
                                       st["gen_shaded_rays"] - st0["gen_shaded_rays"]))
        out = {"W": W, "H": H, "spp": spp, "paths": spp * npx, "reps": reps}
        for name, v in runs.items():
            ms = [a[0] for a in v]
            out[name] = {"wall_ms": ms, "median_ms": statistics.median(ms), "rays": v[0][1], "presolved_rays": v[0][2],
                         "gen_shaded_rays": v[0][3], "mray_s": [round(a[1] / a[0] / 1e3, 1) for a in v]}
        print(json.dumps(out))
    finally:
        itf.shutdown()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--trace", default="")
    args = ap.parse_args()
    if args.trace:
        trace(args.trace)
    else:
        run(args.reps, args.spp)


if __name__ == "__main__":
    main()
