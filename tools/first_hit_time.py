"""Timing of wpt_first_hit beside the production closest-hit kernel over the
same rays (profiles/firsthit/README.md): the C3 scene at 1920x1080, one lane,
REPS times in one session, alternating: first_hit (every plane), then
wpt_primary_rays into wpt_trace_rays (k_extend). The hook's launches are not
in wpt_kernel_times, so both kernels' device times come from a kernel trace of
this run (the run itself prints the calls' wall times as one JSON line):
  rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python3 tools/first_hit_time.py
  python3 tools/first_hit_time.py --trace DIR/.../run_kernel_trace.csv
Usage: python3 tools/first_hit_time.py [--reps 5] [--trace CSV]"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def from_trace(path):
    """Device ms of the k_first_hit and k_extend launches in a rocprofv3 kernel
    trace (the first of each is the warm-up), their medians and the ratio."""
    ms = {"k_first_hit": [], "k_extend": []}
    for row in csv.DictReader(open(path)):
        for k in ms:
            if k in row["Kernel_Name"]:
                ms[k].append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e6)
    out = {k: {"launches": len(v), "ms": [round(x, 4) for x in v], "median_ms": round(statistics.median(v[1:]), 4)}
           for k, v in ms.items() if len(v) > 1}
    if len(out) == 2:
        out["ratio"] = round(out["k_first_hit"]["median_ms"] / out["k_extend"]["median_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trace", default="")
    args = ap.parse_args()
    if args.trace:
        print(json.dumps(from_trace(args.trace)))
        return
    import numpy as np
    import wpt_loader
    pkg = wpt_loader.load()
    itf = pkg.interface
    W, H = 1920, 1080
    path = os.path.join(ROOT, "tests", "golden", "cloud_100k.npy")
    mesh = np.load(path, allow_pickle=False) if os.path.exists(path) else pkg.scenes.triangle_cloud(100000, seed=0x5EED)
    cam = pkg.scenes.scene_camera(2)
    itf.set_device(0)
    itf.init(W, H, 2, *cam)
    try:
        itf.store_mesh(1, mesh)
        itf.update_settings(1, 1, 0, 0, 0)
        itf.set_render_options(8, 0xBABABEBE, 0)
        itf.set_lanes(1)
        rays = itf.primary_rays(W, H, cam)
        g = itf.first_hit(0)  # warm-up of both (buffers, code objects)
        t, ids = itf.trace_rays(rays)
        assert np.array_equal(g["t"].reshape(-1).view(np.uint32), t.view(np.uint32)) and np.array_equal(
            g["id"].reshape(-1), ids)
        fh_wall, ext_wall = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            itf.first_hit(0)
            fh_wall.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            itf.trace_rays(rays)
            ext_wall.append((time.perf_counter() - t0) * 1e3)
        v = g["visits"]
        print(json.dumps({"W": W, "H": H, "triangles": int(mesh.size // 9), "reps": args.reps,
                          "first_hit_call_wall_ms": [round(x, 3) for x in fh_wall],
                          "trace_rays_call_wall_ms": [round(x, 3) for x in ext_wall],
                          "visits_mean": round(float(v.mean()), 2), "visits_max": int(v.max()),
                          "hit_pixels": int((g["id"] >= 0).sum())}))
    finally:
        itf.shutdown()


if __name__ == "__main__":
    main()
