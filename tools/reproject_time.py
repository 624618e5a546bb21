"""Timing of wpt_reproject (profiles/reproject/README.md): the C3 scene at
1920x1080, one session. 4 spp at the scene's camera, kept; the camera is set
again to the same place (a camera pair with full overlap), 4 spp; then REPS + 1
calls (the first the warm-up) of reproject() with four taps and with NEAREST,
alternating, so that one kernel trace holds both; then the wall time of
reproject (len output only) + denoise_merged (RGBA8 output only) against
wpt_denoise with the RGBA8 output only, all at the default parameters.
k_reproject is not in wpt_kernel_times, so the device times come from a kernel
trace of this run:
  rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python3 tools/reproject_time.py
  python3 tools/reproject_time.py --trace DIR/.../run_kernel_trace.csv
In the trace the launches of k_reproject alternate four taps, NEAREST after the
keeping one (launch 0, pass-through); the wall-time calls at the end are four
taps. Usage: python3 tools/reproject_time.py [--reps 5] [--trace CSV]"""
import argparse
import csv
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H = 1920, 1080
# per pixel: the frame (16 + 4), dir, t, normal, kind (12 + 4 + 12 + 1) read; under full overlap each kept
# record once (4 + 16 + 16); the merged frame, counts and lengths written (16 + 4 + 4)
FLOOR_BYTES = 20 + 29 + 36 + 24


def from_trace(path, reps):
    rows = [r for r in csv.DictReader(open(path)) if "k_reproject" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    ms = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in rows]
    # launch 0 keeps (no history), 1 and 2 warm up, then reps pairs, then the wall-time calls
    pairs = ms[3:3 + 2 * reps]
    out = {"launches": len(ms), "keep_pass_through_ms": round(ms[0], 4)}
    for name, v in (("bilinear", pairs[0::2]), ("nearest", pairs[1::2]), ("bilinear_wall_calls", ms[3 + 2 * reps:])):
        if v:
            med = statistics.median(v)
            out[name] = {"launches": len(v), "median_ms": round(med, 4), "min_ms": round(min(v), 4),
                         "max_ms": round(max(v), 4),
                         "floor_GBps": round(FLOOR_BYTES * W * H / (med * 1e-3) / 1e9, 1)}
    if rows:
        out["vgpr"] = rows[0].get("VGPR_Count") or rows[0].get("Arch_VGPR_Count")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trace", default="")
    args = ap.parse_args()
    if args.trace:
        print(json.dumps(from_trace(args.trace, args.reps)))
        return
    import numpy as np
    import wpt_loader
    pkg = wpt_loader.load()
    itf = pkg.interface
    L = pkg.lib()
    path = os.path.join(ROOT, "tests", "golden", "cloud_100k.npy")
    mesh = np.load(path, allow_pickle=False) if os.path.exists(path) else pkg.scenes.triangle_cloud(100000, seed=0x5EED)
    cam = pkg.scenes.scene_camera(2)
    itf.set_device(0)
    itf.init(W, H, 2, *cam)
    try:
        itf.store_mesh(1, mesh)
        itf.update_settings(1, 1, 0, 0, 0)
        itf.set_render_options(8, 0xBABABEBE, 0)
        itf.compute(W * H * 4)
        itf.reproject(0, flags=itf.REPROJECT_KEEP)
        itf.update_camera(*cam)
        itf.compute(W * H * 4)
        walls = {0: [], itf.REPROJECT_NEAREST: []}
        shares = {}
        for rep in range(args.reps + 1):
            for flags in walls:
                t0 = time.perf_counter()
                out = itf.reproject(0, flags=flags)
                if rep:
                    walls[flags].append((time.perf_counter() - t0) * 1e3)
                shares[flags] = float((out[2] > 0).mean())
        d, r = itf.DENOISE_DEFAULTS, itf.REPROJECT_DEFAULTS
        f = ctypes.c_float
        rgba = np.empty((H, W, 4), np.uint8)
        ln = np.empty((H, W), np.uint32)
        both, alone = [], []
        for rep in range(args.reps + 1):
            t0 = time.perf_counter()
            rc = L.wpt_reproject(0, f(r["cos_min"]), f(r["eps_z"]), r["max_len"], 0, None, None, ln.ctypes.data)
            rc |= L.wpt_denoise_merged(d["iterations"], f(d["sigma_c"]), f(d["sigma_z"]), d["flags"], None, None,
                                       rgba.ctypes.data)
            t1 = time.perf_counter()
            rc |= L.wpt_denoise(0, d["iterations"], f(d["sigma_c"]), f(d["sigma_z"]), d["flags"], None, None,
                                rgba.ctypes.data)
            t2 = time.perf_counter()
            assert rc == 0
            if rep:
                both.append((t1 - t0) * 1e3)
                alone.append((t2 - t1) * 1e3)
        r3 = lambda v: [round(x, 3) for x in v]
        print(json.dumps({"W": W, "H": H, "triangles": int(mesh.size // 9), "reps": args.reps,
                          "reproject_all_outputs_wall_ms_bilinear": r3(walls[0]),
                          "reproject_all_outputs_wall_ms_nearest": r3(walls[itf.REPROJECT_NEAREST]),
                          "share_len_gt_0_bilinear": shares[0], "share_len_gt_0_nearest": shares[itf.REPROJECT_NEAREST],
                          "reproject_len_plus_denoise_merged_rgba_wall_ms": r3(both),
                          "denoise_rgba_only_wall_ms": r3(alone)}))
    finally:
        itf.shutdown()


if __name__ == "__main__":
    main()
