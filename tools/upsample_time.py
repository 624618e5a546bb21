"""Records of wpt_upsample (profiles/upsample/README.md).

time (default): the C3 scene at 1920x1080, 4 spp, one session. REPS + 1 calls
  each (the first the warm-up) of wpt_first_hit_scaled(2) with the kind plane
  alone and with the four guide planes, of wpt_upsample(2) with every output and
  with the RGBA8 output only (3 passes and none), then a native 3840x2160
  session of the same scene and wpt_denoise there with the RGBA8 output only.
  Wall times; the launches are not in wpt_kernel_times, so device times come
  from a kernel trace of this run:
    rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python3 tools/upsample_time.py
    python3 tools/upsample_time.py --trace DIR/.../run_kernel_trace.csv
budget: scene 100, NEE, depth 4. A coarse W x H session at 4N spp upsampled x2
  against a native 2W x 2H session at N spp, N = 1, 4, 16, both measured against
  the 1024-spp native frame: relative L2, clamped to [0, 1] and not.
Usage: python3 tools/upsample_time.py [time|budget] [--reps 5] [--trace CSV]"""
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
W, H, S = 1920, 1080, 2
# k_upsample per fine pixel: the guides read (t 4, normal 12, albedo 12, kind 1)
# and the outputs written (rgb 12, valid 1, rgba 4)
GUIDE_BYTES, OUT_BYTES = 29, {"all": 17, "rgba": 4}


def from_trace(path):
    """Device ms per kernel of a rocprofv3 kernel trace, launches in order."""
    ms = {}
    for row in csv.DictReader(open(path)):
        n = row["Kernel_Name"]
        for key in ("k_first_hit", "k_upsample", "k_dn_pack", "k_dn_atrous", "k_dn_unpack"):
            if key in n:
                ms.setdefault(key, []).append(round((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e6, 4))
    out = {k: {"launches": len(v), "median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "ms": v}
           for k, v in sorted(ms.items())}
    nf = S * W * S * H
    for which, b in OUT_BYTES.items():
        out[f"k_upsample_floor_MB_{which}"] = round((GUIDE_BYTES + b) * nf / 1e6, 1)
    return out


def _session(pkg, mesh, w, h, spp):
    itf = pkg.interface
    itf.init(w, h, 2, *pkg.scenes.scene_camera(2))
    itf.store_mesh(1, mesh)
    itf.update_settings(1, 1, 0, 0, 0)
    itf.set_render_options(8, 0xBABABEBE, 0)
    itf.compute(w * h * spp)


def run_time(pkg, reps):
    import numpy as np
    itf, L = pkg.interface, pkg.lib()
    f = ctypes.c_float
    path = os.path.join(ROOT, "tests", "golden", "cloud_100k.npy")
    mesh = np.load(path, allow_pickle=False) if os.path.exists(path) else pkg.scenes.triangle_cloud(100000, seed=0x5EED)
    d = itf.UPSAMPLE_DEFAULTS
    fw, fh = S * W, S * H
    rgb = np.empty((fh, fw, 3), np.float32)
    valid = np.empty((fh, fw), np.uint8)
    rgba = np.empty((fh, fw, 4), np.uint8)
    kind = np.empty((fh, fw), np.uint8)
    res = {"W": W, "H": H, "scale": S, "triangles": int(mesh.size // 9), "reps": reps}

    def timed(name, fn):
        ms = []
        for rep in range(reps + 1):
            t0 = time.perf_counter()
            assert fn() == 0, L.wpt_last_error()
            if rep:
                ms.append(round((time.perf_counter() - t0) * 1e3, 3))
        res[name] = ms

    itf.set_device(0)
    _session(pkg, mesh, W, H, 4)
    try:
        timed("first_hit_scaled2_kind_wall_ms",
              lambda: L.wpt_first_hit_scaled(S, 0, None, None, None, None, None, None, kind.ctypes.data))
        timed("first_hit_scaled2_guides_wall_ms", lambda: itf.first_hit_scaled(S, 0, planes=("t", "normal", "albedo", "kind")) and 0)
        for it in (d["iterations"], 0):
            timed(f"upsample2_it{it}_all_outputs_wall_ms",
                  lambda: L.wpt_upsample(S, 0, it, f(d["sigma_c"]), f(d["sigma_z"]), 0, rgb.ctypes.data, valid.ctypes.data,
                                         rgba.ctypes.data))
            timed(f"upsample2_it{it}_rgba_only_wall_ms",
                  lambda: L.wpt_upsample(S, 0, it, f(d["sigma_c"]), f(d["sigma_z"]), 0, None, None, rgba.ctypes.data))
        res["valid_0_1_2"] = [int((valid == v).sum()) for v in (0, 1, 2)]
        res["fine_kinds_0_1_2"] = [int((kind == v).sum()) for v in (0, 1, 2)]
    finally:
        itf.shutdown()
    _session(pkg, mesh, fw, fh, 1)
    try:
        dn = itf.DENOISE_DEFAULTS
        timed("native4k_denoise_rgba_only_wall_ms",
              lambda: L.wpt_denoise(0, dn["iterations"], f(dn["sigma_c"]), f(dn["sigma_z"]), dn["flags"], None, None,
                                    rgba.ctypes.data))
    finally:
        itf.shutdown()
    print(json.dumps(res))


def run_budget(pkg, w, h):
    import numpy as np
    itf = pkg.interface

    def frame(vp, spp, upsample=False):
        itf.init(vp[0], vp[1], 100, *pkg.scenes.scene_camera(100))
        try:
            itf.update_settings(1, 1, 0, 0, 0)
            itf.set_render_options(4, 0xBABABEBE, 0)
            itf.compute(vp[0] * vp[1] * spp)
            acc, cnt = itf.read_radiance(*vp)
            assert np.all(cnt == spp)
            ups = {it: itf.upsample(S, 0, iterations=it)[0] for it in (0, itf.UPSAMPLE_DEFAULTS["iterations"])} if upsample else {}
            return acc / np.float32(spp), ups
        finally:
            itf.shutdown()

    def err(img, ref):
        a, r = np.asarray(img, np.float64), np.asarray(ref, np.float64)
        l2 = lambda x, y: float(np.linalg.norm(x - y) / np.linalg.norm(y))
        return {"clamped": round(l2(np.clip(a, 0, 1), np.clip(r, 0, 1)), 4), "unclamped": round(l2(a, r), 4)}

    itf.set_device(0)
    fine = (S * w, S * h)
    ref, _ = frame(fine, 1024)
    rows = []
    for n in (1, 4, 16):
        native, _ = frame(fine, n)
        coarse, ups = frame((w, h), 4 * n, upsample=True)
        rows.append({"N": n, "native_N_spp": err(native, ref),
                     "coarse_4N_replicated": err(coarse.repeat(S, 0).repeat(S, 1), ref),
                     **{f"coarse_4N_upsampled_it{it}": err(u, ref) for it, u in ups.items()}})
    print(json.dumps({"scene": 100, "coarse": [w, h], "fine": list(fine), "reference_spp": 1024, "rows": rows}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="?", default="time", choices=("time", "budget"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trace", default="")
    ap.add_argument("--coarse", default="160x120")
    args = ap.parse_args()
    if args.trace:
        print(json.dumps(from_trace(args.trace)))
        return
    import wpt_loader
    pkg = wpt_loader.load()
    if args.what == "time":
        run_time(pkg, args.reps)
    else:
        run_budget(pkg, *(int(v) for v in args.coarse.split("x")))


if __name__ == "__main__":
    main()
