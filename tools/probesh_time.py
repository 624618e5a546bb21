"""An SH query against the route it replaces and against the plain point query
(profiles/probesh/README.md), one JSON line.

The C3 scene, NEE, depth 8, one session. The probes are a 32 x 32 x 32 lattice
(2^15 records) about the scene's camera position, normal (0, 1, 0),
WPT_POINTS_SPHERE, SPP samples each, order 2:
  replaced       per sample s: wpt_radiance_points at spp = 1 (host pointers),
                 wpt_point_rays on the host for the directions, wpt_sh_basis of
                 them and the f32 multiply-add in numpy
  probe_sh       wpt_probe_sh, device pointers
  points         wpt_radiance_points at the same spp, device pointers: the same
                 paths and rays, so the difference to probe_sh is the projection
The three alternate REPS + 1 times (the first the warm-up); the wall time runs to
wpt_sync. replaced and probe_sh give the same bits (asserted); all three trace
the same rays (asserted), so milliseconds compare. Beside them the summed device
time of the accumulation slot of wpt_kernel_times under wpt_set_profiling: for
probe_sh that is k_sh_dirs + k_accumulate_sh, for points k_accumulate_round.

Usage: python3 tools/probesh_time.py [--reps 3] [--spp 256]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
G = 32
SEED = 0xBABABEBE
SPHERE = 1


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
    itf.init(64, 64, 2, *cam)
    n = G * G * G
    try:
        itf.store_mesh(1, mesh)
        itf.update_settings(1, 1, 0, 0, 0)
        itf.set_render_options(8, SEED, 0)
        g = (np.arange(G, dtype=np.float32) + 0.5) / G - 0.5
        pts = np.empty((n, 6), np.float32)
        pts[:, :3] = np.asarray(cam[:3], np.float32) + np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
        pts[:, 3:] = np.array([0, 1, 0], np.float32)
        dev = torch.device("cuda", 0)
        d_pts = torch.from_numpy(pts).to(dev)
        torch.cuda.synchronize()
        runs = {"replaced": [], "probe_sh": [], "points": []}
        bits = {}
        for rep in range(reps + 1):
            for name in runs:
                itf.sync()
                st0 = itf.stats()
                t0 = time.perf_counter()
                if name == "replaced":
                    sh = np.zeros((n, 9, 3), np.float32)
                    for s in range(spp):
                        c = itf.radiance_points(pts, None, s, 1, 1, SPHERE)[0]
                        Y = itf.sh_basis(itf.point_rays(pts, None, SEED, s, SPHERE)[:, 3:], 2)
                        sh += Y[:, :, None] * c[:, None, :]
                elif name == "probe_sh":
                    sh = itf.probe_sh(d_pts, None, 0, spp, 1, SPHERE, 2, device=True)[0]
                else:
                    itf.radiance_points(d_pts, None, 0, spp, 1, SPHERE, device=True)
                itf.sync()
                ms = (time.perf_counter() - t0) * 1e3
                st = itf.stats()
                assert st["paths"] - st0["paths"] == spp * n
                if name != "points":
                    bits[name] = (sh.cpu().numpy() if name == "probe_sh" else sh).view(np.uint32)
                if rep:
                    runs[name].append((round(ms, 2), st["rays"] + st["shadow_rays"] - st0["rays"] - st0["shadow_rays"]))
            assert np.array_equal(bits["replaced"], bits["probe_sh"])
        out = {"probes": n, "spp": spp, "paths": spp * n, "order": 2, "reps": reps,
               "nonzero_rows": int((bits["probe_sh"] != 0).any(axis=(1, 2)).sum())}
        for name, v in runs.items():
            ms = [a[0] for a in v]
            assert v[0][1] == runs["probe_sh"][0][1]
            out[name] = {"wall_ms": ms, "median_ms": statistics.median(ms), "rays": v[0][1]}
        # the accumulation's device time over the same positions
        itf.set_profiling(True)
        for name, call in (("probe_sh", lambda: itf.probe_sh(d_pts, None, 0, spp, 1, SPHERE, 2, device=True)),
                           ("points", lambda: itf.radiance_points(d_pts, None, 0, spp, 1, SPHERE, device=True))):
            call()
            ms = []
            for _ in range(reps):
                k0 = itf.kernel_times()["accumulate"]
                call()
                k1 = itf.kernel_times()["accumulate"]
                ms.append(round(k1["ms"] - k0["ms"], 4))
                launches = k1["launches"] - k0["launches"]
            out["accumulate_" + name] = {"ms": ms, "launches": launches}
        itf.set_profiling(False)
        print(json.dumps(out))
    finally:
        itf.shutdown()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--spp", type=int, default=256)
    args = ap.parse_args()
    run(args.reps, args.spp)


if __name__ == "__main__":
    main()
