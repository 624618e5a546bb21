"""Timing of wpt_denoise (profiles/denoise/README.md): the C3 scene at
1920x1080, 4 spp, one session. REPS + 1 calls (the first the warm-up) with five
iterations, alternating WPT_OPT_DENOISE_LDS 7 (steps 1, 2, 4 through LDS) and 0
(every step direct), so that one kernel trace holds both variants of each step;
then the wall time of the call with the RGBA8 output only against the host
path (first_hit's guide planes + read_radiance + denoise_host), both at the
default parameters. The filter's launches are not in wpt_kernel_times, so the
device times come from a kernel trace of this run:
  rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python3 tools/denoise_time.py
  python3 tools/denoise_time.py --trace DIR/.../run_kernel_trace.csv
Usage: python3 tools/denoise_time.py [--reps 5] [--trace CSV]"""
import argparse
import csv
import ctypes
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H = 1920, 1080
FLOOR_BYTES = 48  # per pixel and iteration: A and B read once, A written once


def kernel_of(name):
    """'pack', 'unpack', 'atrous<STEP> lds|direct' or None from a (mangled or demangled) kernel name."""
    if "k_dn_pack" in name:
        return "pack"
    if "k_dn_unpack" in name:
        return "unpack"
    m = re.search(r"k_dn_atrous<(\d+), (true|false)>", name) or re.search(r"k_dn_atrousILi(\d+)ELb([01])E", name)
    if not m:
        return None
    return f"atrous<{m.group(1)}> " + ("lds" if m.group(2) in ("true", "1") else "direct")


def from_trace(path, warm):
    """Device ms per kernel in a rocprofv3 kernel trace: median and range of the
    launches after each kernel's first `warm`, and bytes/s against the floor."""
    ms = {}
    for row in csv.DictReader(open(path)):
        k = kernel_of(row["Kernel_Name"])
        if k:
            ms.setdefault(k, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e6)
    out = {}
    for k, v in sorted(ms.items()):
        v = v[warm:] or v
        med = statistics.median(v)
        out[k] = {"launches": len(v), "median_ms": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
        if k.startswith("atrous"):
            out[k]["floor_GBps"] = round(FLOOR_BYTES * W * H / (med * 1e-3) / 1e9, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trace", default="")
    ap.add_argument("--warm", type=int, default=1, help="launches of each kernel to drop from a trace")
    args = ap.parse_args()
    if args.trace:
        print(json.dumps(from_trace(args.trace, args.warm)))
        return
    import numpy as np
    import wpt_loader
    pkg = wpt_loader.load()
    itf = pkg.interface
    L = pkg.lib()
    path = os.path.join(ROOT, "tests", "golden", "cloud_100k.npy")
    mesh = np.load(path, allow_pickle=False) if os.path.exists(path) else pkg.scenes.triangle_cloud(100000, seed=0x5EED)
    itf.set_device(0)
    itf.init(W, H, 2, *pkg.scenes.scene_camera(2))
    try:
        itf.store_mesh(1, mesh)
        itf.update_settings(1, 1, 0, 0, 0)
        itf.set_render_options(8, 0xBABABEBE, 0)
        itf.compute(W * H * 4)
        lds_default = itf.get_option("denoise_lds")
        walls = {7: [], 0: []}
        outs = {}
        for rep in range(args.reps + 1):
            for lds in (7, 0):
                itf.set_option("denoise_lds", lds)
                t0 = time.perf_counter()
                outs[lds] = itf.denoise(0, iterations=5)
                if rep:
                    walls[lds].append((time.perf_counter() - t0) * 1e3)
        assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(outs[7], outs[0]))
        itf.set_option("denoise_lds", lds_default)
        d = itf.DENOISE_DEFAULTS
        rgba = np.empty((H, W, 4), np.uint8)
        call, host = [], []
        for rep in range(args.reps + 1):
            t0 = time.perf_counter()
            rc = L.wpt_denoise(0, d["iterations"], ctypes.c_float(d["sigma_c"]), ctypes.c_float(d["sigma_z"]), d["flags"],
                               None, None, rgba.ctypes.data)
            t1 = time.perf_counter()
            assert rc == 0
            g = itf.first_hit(0, planes=("t", "normal", "albedo", "kind"))
            acc, cnt = itf.read_radiance(W, H)
            t2 = time.perf_counter()
            ref = itf.denoise_host(acc, cnt, g["t"], g["normal"], g["albedo"], g["kind"])
            t3 = time.perf_counter()
            if rep:
                call.append((t1 - t0) * 1e3)
                host.append(((t2 - t1) * 1e3, (t3 - t2) * 1e3))
        assert np.array_equal(ref[2], rgba)
        r3 = lambda v: [round(x, 3) for x in v]
        print(json.dumps({"W": W, "H": H, "triangles": int(mesh.size // 9), "reps": args.reps, "denoise_lds": lds_default,
                          "denoise5_all_outputs_wall_ms_lds7": r3(walls[7]), "denoise5_all_outputs_wall_ms_lds0": r3(walls[0]),
                          "denoise_rgba_only_wall_ms": r3(call),
                          "host_first_hit_read_radiance_wall_ms": r3(h[0] for h in host),
                          "host_denoise_host_wall_ms": r3(h[1] for h in host),
                          "valid_pixels": int(outs[7][1].sum())}))
    finally:
        itf.shutdown()


if __name__ == "__main__":
    main()
