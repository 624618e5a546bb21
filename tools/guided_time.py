"""Measurements of guided sampling (profiles/guided/README.md), one JSON line each.

  cost   the C3 scene at 1920x1080, NEE, depth 8, one session: after a reset of
         the accumulation, wpt_compute(4 * npix) against a uniform map of 4 per
         pixel through wpt_compute_map (the caller's array, and the device map
         wpt_sample_map left), alternating, REPS + 1 times (the first the
         warm-up). Both trace samples 0 .. 3 of every pixel, so the rays are the
         same; the wall time runs to wpt_sync.
  plan   the same session with 4 spp: wall time of wpt_sample_map without
         outputs, with and without a budget, with and without WPT_MAP_MISS_ONCE
         (which adds k_first_hit). The kernels are not in wpt_kernel_times; their
         device times come from a kernel trace of this run:
           rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python3 tools/guided_time.py plan
           python3 tools/guided_time.py plan --trace DIR/.../run_kernel_trace.csv
  error  scene 100 at 64 x 48, NEE, depth 4: 16 spp at camera A, kept; camera B
         (reproject_fixtures' sideways pair), 1 spp; then 2 * npix more paths,
         uniform (wpt_compute) on one session and guided (sample_map with that
         budget and --target, default the smallest target whose needs use it up,
         + compute_map) on its twin; the merged frames' relative L2 error
         against 1024 spp at camera B, plain and on clamp(rgb, 0, 1).

Usage: python3 tools/guided_time.py cost|plan|error [--reps 5] [--trace CSV] [--target N]"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H = 1920, 1080
CAM_A, CAM_B = (0.0, 1.5, -4.0, 0.0, 0.0), (0.4, 1.5, -4.0, 0.0, 0.0)


def _c3(pkg, np):
    itf = pkg.interface
    path = os.path.join(ROOT, "tests", "golden", "cloud_100k.npy")
    mesh = np.load(path, allow_pickle=False) if os.path.exists(path) else pkg.scenes.triangle_cloud(100000, seed=0x5EED)
    cam = pkg.scenes.scene_camera(2)
    itf.set_device(0)
    itf.init(W, H, 2, *cam)
    itf.store_mesh(1, mesh)
    itf.update_settings(1, 1, 0, 0, 0)
    itf.set_render_options(8, 0xBABABEBE, 0)
    return cam


def cost(pkg, np, reps):
    itf = pkg.interface
    cam = _c3(pkg, np)
    npx = W * H
    four = np.full((H, W), 4, np.uint32)
    runs = {"compute": [], "map_array": [], "map_device": []}
    try:
        for rep in range(reps + 1):
            for name in runs:
                itf.update_camera(*cam)  # resets the accumulation (and map mode)
                if name == "map_device":
                    itf.sample_map(0, 4, 4)
                itf.sync()
                st0 = itf.stats()
                t0 = time.perf_counter()
                if name == "compute":
                    itf.compute(4 * npx)
                elif name == "map_array":
                    itf.compute_map(four)
                else:
                    itf.compute_map(None)
                itf.sync()
                ms = (time.perf_counter() - t0) * 1e3
                st = itf.stats()
                rays = st["rays"] + st["shadow_rays"] - st0["rays"] - st0["shadow_rays"]
                assert st["paths"] - st0["paths"] == 4 * npx
                if rep:
                    runs[name].append((round(ms, 2), rays))
        out = {"W": W, "H": H, "paths": 4 * npx, "reps": reps}
        for name, v in runs.items():
            ms = [a for a, _ in v]
            out[name] = {"wall_ms": ms, "median_ms": statistics.median(ms), "rays": v[0][1],
                         "mray_s": [round(r / a / 1e3, 1) for a, r in v]}
        print(json.dumps(out))
    finally:
        itf.shutdown()


def plan_trace(path):
    rows = [r for r in csv.DictReader(open(path))]
    out = {}
    for key in ("k_first_hit", "k_map_need", "k_scan64_local", "k_scan64_sums", "k_scan64_add", "k_map_deal"):
        ms = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in rows if key in r["Kernel_Name"]]
        if ms:
            out[key] = {"launches": len(ms), "median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
                        "max_ms": round(max(ms), 4)}
    print(json.dumps(out))


def plan(pkg, np, reps):
    itf = pkg.interface
    L = pkg.lib()
    _c3(pkg, np)
    npx = W * H
    try:
        itf.compute(4 * npx)
        walls = {}
        for rep in range(reps + 1):
            for name, budget, flags in (("no_budget", 0, 0), ("budget", 2 * npx, 0), ("miss_once", 0, itf.MAP_MISS_ONCE),
                                        ("miss_once_budget", 2 * npx, itf.MAP_MISS_ONCE)):
                t0 = time.perf_counter()
                rc = L.wpt_sample_map(0, 8, 8, budget, flags, None, None)
                ms = (time.perf_counter() - t0) * 1e3
                assert rc == 0
                if rep:
                    walls.setdefault(name, []).append(round(ms, 3))
        print(json.dumps({"W": W, "H": H, "reps": reps, "sample_map_no_outputs_wall_ms": walls}))
    finally:
        itf.shutdown()


def error(pkg, np, target0):
    itf = pkg.interface
    vw, vh, spp_a, truth_spp = 64, 48, 16, 1024
    npx = vw * vh
    budget = 2 * npx

    def start(cam):
        itf.init(vw, vh, 100, *cam)
        itf.update_settings(1, 1, 0, 0, 0)
        itf.set_render_options(4, 0xBABABEBE, 0)

    def rel(a, t):
        return float(np.linalg.norm(a - t) / np.linalg.norm(t))

    itf.set_device(0)
    start(CAM_B)
    itf.compute(truth_spp * npx)
    acc, cnt = itf.read_radiance(vw, vh)
    truth = acc / cnt[..., None].astype(np.float32)
    itf.shutdown()
    out = {"W": vw, "H": vh, "history_spp": spp_a, "first_spp": 1, "budget_paths": budget, "truth_spp": truth_spp}
    for name in ("uniform", "guided"):
        start(CAM_A)
        itf.compute(spp_a * npx)
        itf.reproject(0, flags=itf.REPROJECT_KEEP)
        itf.update_camera(*CAM_B)
        itf.compute(npx)
        if name == "uniform":
            itf.compute(budget)
        else:
            _, _, ln = itf.reproject(0)
            # target 0: the smallest target whose needs use up the budget (the thinnest pixels are filled first)
            for target in ([target0] if target0 else range(2, 1 << 16)):
                count, tot = itf.sample_map(0, target=target, max_per_pixel=target, budget=budget)
                if tot[0] >= budget:
                    break
            itf.compute_map(None)
            out["guided_map"] = {"target": target, "T": tot[0], "dealt": tot[1],
                                 "pixels_with_samples": int((count > 0).sum()),
                                 "max_count": int(count.max()), "pixels_without_history": int((ln == 0).sum())}
        raw, rcnt = itf.read_radiance(vw, vh)
        m_acc, m_cnt, _ = itf.reproject(0)
        itf.shutdown()
        merged = m_acc / m_cnt[..., None].astype(np.float32)
        rawm = raw / rcnt[..., None].astype(np.float32)
        out[name] = {"merged_rel_l2": round(rel(merged, truth), 4),
                     "merged_rel_l2_clamped": round(rel(np.clip(merged, 0, 1), np.clip(truth, 0, 1)), 4),
                     "raw_rel_l2": round(rel(rawm, truth), 4),
                     "raw_rel_l2_clamped": round(rel(np.clip(rawm, 0, 1), np.clip(truth, 0, 1)), 4),
                     "paths": int(rcnt.sum())}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("cost", "plan", "error"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trace", default="")
    ap.add_argument("--target", type=int, default=0, help="error: sample_map's target (0: the smallest that uses up the budget)")
    args = ap.parse_args()
    if args.what == "plan" and args.trace:
        plan_trace(args.trace)
        return
    import numpy as np
    import wpt_loader
    pkg = wpt_loader.load()
    if args.what == "cost":
        cost(pkg, np, args.reps)
    elif args.what == "plan":
        plan(pkg, np, args.reps)
    else:
        error(pkg, np, args.target)


if __name__ == "__main__":
    main()
